"""fqz5_filter_match (filter.hip) on synthetic device arrays: the per-record
sums of a block's bases and qualities, the rule over them and the compacted
selection.  No codec is involved.

Expected values come from fqz5_filter_host and, independently, from the rule
restated in plain Python (filter_ref).  The bases and the qualities are views
into larger buffers whose guard bytes would change a sum if they were read:
'N' and 'G' beside the bases (n, gc, and diff against any base next to them),
200 beside the qualities.  Guard words surround every output."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import filter_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x55555555
GUARD64 = 0x5555555555555555
PAD = 48                                                    # guard bytes on both sides
ALL = {"min_len": 2, "max_len": 5000, "max_n": 2, "min_mean_q": 21, "low_q": 10, "max_low_pct": 30,
       "gc_pct": (20, 70), "min_complexity_pct": 60}


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def T():
    return int(Z._load().fqz5_filter_tile())


def _records(rng, lens, alphabet=b"ACGTN", quals=range(2, 42)):
    quals = list(quals)
    return [(bytes(rng.choice(alphabet) for _ in range(n)), bytes(rng.choice(quals) for _ in range(n)))
            for n in lens]


def _cut(total: int, cuts) -> list[int]:
    edges = [0] + sorted(cuts) + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def _dev(blob: bytes, mis: int, guard: bytes):
    """The blob `mis` bytes past a 16-byte address, guard bytes around it:
    (the tensor, the blob's address)."""
    left = (guard * (PAD + 16))[:PAD + mis]
    t = torch.frombuffer(bytearray(left + blob + (guard * PAD)[:PAD]), dtype=torch.uint8).cuda()
    base = t.data_ptr()
    assert base % 16 == 0
    return t, base + PAD + mis


def _match(records, crit, pairs=False, invert=False, mis=(0, 0), seq=True, qual=True, sums=True,
           lens=None):
    """One fqz5_filter_match: (rc, the selected indices, failed, the sums)."""
    so = Z._load()
    lens = np.asarray([len(s) for s, _ in records] if lens is None else lens, np.uint32)
    n = len(lens)
    sblob = b"".join(s for s, _ in records)
    st, sp = _dev(sblob, mis[0], b"NG")
    qt, qp = _dev(b"".join(q for _, q in records), mis[1], b"\xc8")
    rec = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda")
    u32 = [torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda") for _ in range(4)]
    u64 = torch.full((n + 2,), GUARD64, dtype=torch.int64, device="cuda")
    arrs = [u32[0], u32[1], u32[2], u64, u32[3]]
    ds = Z._FilterSums(*(a.data_ptr() + a.element_size() for a in arrs))
    failed = np.zeros(9, np.uint64)
    failed[0] = failed[8] = GUARD64
    hit = C.c_uint64(12345)
    spec = Z.Filter(**crit).spec()
    lib.after_torch()
    rc = so.fqz5_filter_match(C.byref(spec), sp if seq else None, qp if qual else None, len(sblob),
                              lens.ctypes.data, n, int(pairs), int(invert), rec.data_ptr() + 4,
                              C.byref(hit), failed.ctypes.data + 8, C.byref(ds) if sums else None)
    torch.cuda.synchronize()
    assert failed[0] == failed[8] == GUARD64
    rec = rec.cpu().numpy().view(np.uint32)
    arrs = [a.cpu().numpy().view(np.uint64 if a.dtype == torch.int64 else np.uint32) for a in arrs]
    assert rec[0] == rec[-1] == GUARD
    for a in arrs:
        assert a[0] == a[-1] and int(a[0]) in (GUARD, GUARD64)
    if rc:
        assert (rec == GUARD).all() and not failed[1:8].any() and hit.value == 0
        return rc, None, None, None
    k = int(hit.value)
    assert (rec[1 + k:] == GUARD).all()                     # nothing past the selection
    if not sums:
        assert all(int(x) in (GUARD, GUARD64) for a in arrs for x in a)
    return rc, rec[1:1 + k].tolist(), failed[1:8].tolist(), [a[1:-1] for a in arrs]


def _both(records, crit, pairs=False, invert=False, mis=(0, 0), ref=False, what=None):
    """The GPU against the host restatement (ref: and against filter_ref)."""
    rc, sel, failed, sums = _match(records, crit, pairs, invert, mis)
    assert rc == 0, lib.last_error()
    seq = b"".join(s for s, _ in records)
    keep, hf, hs = Z._filter_host(Z.Filter(**crit), seq, b"".join(q for _, q in records),
                                  [len(s) for s, _ in records], pairs, invert)
    for k, name in enumerate(("n", "gc", "diff", "qsum", "lowq")):
        assert sums[k].dtype == hs[k].dtype
        bad = np.flatnonzero(sums[k] != hs[k])
        assert not len(bad), (what, name, bad[:5].tolist(), sums[k][bad[:5]], hs[k][bad[:5]])
    assert sel == np.flatnonzero(keep).tolist(), what        # ascending, n_hit exact
    assert failed == hf.tolist(), what
    if ref:
        ek, ef, _ = R.rule(records, crit, pairs, invert)
        assert sel == [i for i, k in enumerate(ek) if k] and failed == ef, what
        exp = [R.sums(r, crit.get("low_q")) for r in records]
        for k in range(5):
            assert sums[k].tolist() == [e[k + 1] for e in exp], (what, k)
    return sel, failed, sums


def test_record_ends_at_the_tile_edge(T):
    """Records ending at T - 1, T and T + 1, a short last tile; against the
    rule in plain Python as well."""
    rng = random.Random(3)
    for e in (T - 1, T, T + 1):
        cuts = sorted([7, 60, e - 40, e, e + 3, T + 90])
        records = _records(rng, _cut(T + 133, cuts), alphabet=b"ACGTNacgtn")
        for pairs in (False, True):
            sel, failed, _ = _both(records + ([(b"", b"")] if pairs else []), ALL, pairs, ref=True,
                                   what=e)
        assert sum(failed) > 0


def test_one_record_across_three_tiles(T):
    rng = random.Random(5)
    records = _records(rng, [2 * T + 77], quals=range(256))
    crit = dict(ALL, max_len=3 * T, max_n=T, min_mean_q=100)
    sel, failed, sums = _both(records, crit, mis=(3, 9), ref=True)
    assert sums[2][0] > T and sums[3][0] > 100 * 2 * T
    records = _records(rng, [5, 3 * T - 9, 4])
    _both(records, dict(ALL, max_len=3 * T, max_n=T))


def test_one_base_records():
    """5000 records of one base: more than 2048 records in a tile, the sums
    past the LDS ends go straight to the global cells."""
    rng = random.Random(7)
    records = _records(rng, [1] * 5000)
    crit = {"max_n": 0, "min_mean_q": 12, "gc_pct": (0, 0), "min_complexity_pct": 100}
    for pairs, mis in ((False, (0, 0)), (True, (5, 2))):
        sel, failed, sums = _both(records, crit, pairs, mis=mis, ref=not pairs)
        assert not sums[2].any() and 0 < len(sel) < 5000
    # two-base records: every diff has its neighbour in the record, none beyond
    records = _records(rng, [2] * 4200)
    sel, failed, sums = _both(records, {"min_complexity_pct": 100})
    assert set(sums[2].tolist()) == {0, 1}


def test_runs_of_empty_records(T):
    """Runs of empty records at the start, on the tile edge and at the end."""
    rng = random.Random(9)
    lens = [0] * 300 + _cut(T, [100, 900, T - 30]) + [0] * 310 + _cut(T // 2, [11, 500]) + [0] * 305
    records = _records(rng, lens)
    for crit in (ALL, dict(ALL, min_len=0), {"max_len": 0}):
        for pairs in (False, True):
            _both(records, crit, pairs, mis=(1, 0), ref=crit is ALL and not pairs)
    sel, failed, _ = _both(records, {"max_len": 0})
    assert len(sel) == 915
    # all records empty, no base at all
    empty = [(b"", b"")] * 70
    assert _both(empty, dict(ALL, min_len=0))[0] == list(range(70))
    assert _both(empty, ALL)[1] == [70, 0, 0, 0, 0, 0, 0]
    assert _both(empty, ALL, invert=True, pairs=True)[0] == list(range(70))


@pytest.mark.parametrize("edge", ["tile", "chunk"])
def test_neighbours_across_an_edge(T, edge):
    """Two different bases on both sides of T - 1 | T (of a 16-byte chunk
    edge): inside one record diff counts them, across a record boundary not."""
    total = T + 64
    q = bytes([30] * total)
    crit = {"min_complexity_pct": 0, "max_n": 0}
    for mis in (0, 5):                                      # (chunks are cut at 16-byte addresses)
        at = T if edge == "tile" else 7 * 16 - mis
        seq = bytearray(b"A" * total)
        seq[at:] = b"C" * (total - at)                      # the only change: at - 1 | at
        one = [(bytes(seq), q)]
        split = [(bytes(seq[:at]), q[:at]), (bytes(seq[at:]), q[at:])]
        assert _both(one, crit, mis=(mis, 0), ref=True)[2][2].tolist() == [1]
        assert _both(split, crit, mis=(mis, 0), ref=True)[2][2].tolist() == [0, 0]
    # the boundary one base before and after the edge: the change stays inside a record
    for cut in (at - 1, at + 1):
        recs = [(bytes(seq[:cut]), q[:cut]), (bytes(seq[cut:]), q[cut:])]
        assert sorted(_both(recs, crit, ref=True)[2][2].tolist()) == [0, 1]
    # an empty record exactly on the edge
    recs = [split[0], (b"", b""), split[1]]
    assert _both(recs, crit)[2][2].tolist() == [0, 0, 0]


@pytest.mark.parametrize("mis_seq", range(16))
def test_misaligned_views(T, mis_seq):
    """The bases at every misalignment, the qualities at another: nothing
    outside either view is read (the guard bytes would change the sums)."""
    rng = random.Random(40 + mis_seq)
    records = _records(rng, _cut(T + 41, [0, 3, 50, T - 2, T + 8]), alphabet=b"ACT")
    mis_q = (5 * mis_seq + 3) % 16
    sel, failed, sums = _both(records, ALL, mis=(mis_seq, mis_q), ref=mis_seq == 0)
    assert not sums[0].any()                                # no 'N' of the guard was counted
    _both(records[:3], ALL, mis=(mis_seq, mis_q))           # 50 bases: one partial chunk or two


def test_q_255(T):
    records = [(b"ACGT" * (T // 2), bytes([255] * (2 * T))), (b"AC", bytes([255, 254]))]
    sel, failed, sums = _both(records, {"min_mean_q": 255, "low_q": 255, "max_low_pct": 0},
                              mis=(0, 7), ref=True)
    assert sums[3].tolist() == [255 * 2 * T, 509] and sel == [0] and failed == [0, 0, 0, 1, 0, 0, 0]


def test_selections(T):
    """Everything, nothing, only the first record, only the last."""
    rng = random.Random(13)
    records = [(b"ACGTACGTAC", bytes([40] * 10))] + _records(rng, [50] * 700, alphabet=b"ACGT") + \
        [(b"AC" * 60, bytes([40] * 120))]
    n = len(records)
    assert sum(len(s) for s, _ in records) > 2 * T
    assert _both(records, {"min_len": 10}, ref=True)[0] == list(range(n))
    assert _both(records, {"min_len": 10}, invert=True)[0] == []
    assert _both(records, {"min_len": 121}, ref=True)[0] == []
    assert _both(records, {"max_len": 10})[0] == [0]
    assert _both(records, {"min_len": 120})[0] == [n - 1]
    assert _both(records, {"min_mean_q": 40})[0] == [0, n - 1]
    assert _both(records, {"max_len": 10}, invert=True)[0] == list(range(1, n))


def test_pairs_with_mates_in_different_tiles(T):
    """Mates of T bases (each a tile of its own), of T - 10 and of T + 10."""
    rng = random.Random(17)
    records = []
    for k, n in enumerate((T, T - 10, T + 10)):
        a, b = _records(rng, [n] * 2, alphabet=b"ACGT")
        if k == 1:
            b = (b"N" * 5 + b[0][5:], b[1])                 # the second mate alone fails
        records += [a, b]
    crit = {"max_n": 4, "min_complexity_pct": 40}
    assert _both(records, crit, pairs=True, ref=True)[0] == [0, 1, 4, 5]
    assert _both(records, crit, pairs=True, invert=True, ref=True)[0] == [2, 3]
    assert _both(records, crit)[0] == [0, 1, 2, 4, 5]


def test_streams_left_out_and_errors(T):
    rng = random.Random(19)
    records = _records(rng, [40, 3, 90, 0, 7])
    rc, sel, failed, sums = _match(records, {"min_len": 7, "max_len": 40}, seq=False, qual=False)
    assert rc == 0 and sel == [0, 4] and failed == [2, 1, 0, 0, 0, 0, 0]
    assert not any(s.any() for s in sums)                   # no stream: the sums are zeros
    rc, sel, failed, _ = _match(records, {"min_len": 7}, seq=False, qual=False, sums=False)
    assert rc == 0 and sel == [0, 2, 4]
    rc, sel, _, sums = _match(records, {"max_n": 40}, qual=False)      # bases alone
    assert rc == 0 and sel == [0, 1, 2, 3, 4] and not sums[3].any()
    assert sums[1].tolist() == [R.sums(r)[2] for r in records]
    rc, sel, _, _ = _match(records, {"max_n": 0}, qual=False, sums=False)
    assert rc == 0 and sel == [i for i, r in enumerate(records) if R.sums(r)[1] == 0]
    assert _match(records, {"min_mean_q": 1}, qual=False)[0] == -1
    assert "quality criterion without" in lib.last_error()
    assert _match(records, {"max_n": 1}, seq=False)[0] == -1
    assert "base criterion without" in lib.last_error()
    assert _match(records, {"min_len": 1}, pairs=True)[0] == -1 and "odd record count" in lib.last_error()
    for lens in ([40, 3, 90, 0, 6], [40, 3, 90, 0, 8], [40, 3, 90, 0], []):
        assert _match(records, ALL, lens=lens)[0] == -1 and "do not sum" in lib.last_error()
    assert _match([], ALL)[:3] == (0, [], [0] * 7)          # nrec = 0
