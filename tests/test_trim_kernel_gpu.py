"""fqz5_trim_cuts and fqz5_trim_gather (trim.hip) on synthetic device arrays:
per record the kept interval, the accounting, and the streams compacted to
the intervals.  No codec is involved.

Expected values come from fqz5_trim_host and, independently, from the rule
restated in plain Python (trim_ref).  The bases and the qualities are views
into larger buffers whose guard bytes would change a result if they were read:
'N' or the adapter's own bytes beside the bases, 0 and 200 beside the
qualities.  Guard words surround every output."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import trim_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x55555555
GUARD64 = 0x5555555555555555
PAD = 160                                                   # guard bytes on both sides (> an adapter)
AD = b"AGATCGGAAGAGC"
ALL = {"head": 2, "tail": 1, "q5": 15, "q3": 20, "adapters": [AD, b"CTGTCTCTTATA"],
       "min_overlap": 4, "max_err_pct": 10, "trim_n": True, "max_len": 3000}
NWORDS = 12 + 2 * Z.TRIM_ADAPTERS


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _records(rng, lens, alphabet=b"ACGTNacgtn", plant=True):
    """Records over the alphabet, qualities 2..41; every third with an adapter
    written in somewhere (cut off by the record's end where it does not fit),
    every other third with a low-quality tail."""
    out = []
    for i, L in enumerate(lens):
        s = bytearray(rng.choice(alphabet) for _ in range(L))
        q = bytearray(rng.randint(2, 41) for _ in range(L))
        if plant and i % 3 == 0 and L > 4:
            at = rng.randint(0, L - 4)
            s[at:at + len(AD)] = AD[:L - at]
        if plant and i % 3 == 1 and L:
            k = rng.randint(1, min(L, 90))
            q[L - k:] = bytes(rng.randint(2, 12) for _ in range(k))
        out.append((bytes(s), bytes(q)))
    return out


def _dev(blob: bytes, mis: int, left: bytes, right: bytes):
    """The blob `mis` bytes past a 16-byte address, guard bytes around it:
    (the tensor, the blob's address)."""
    lg = (left * (PAD + 16))[:PAD + mis]
    t = torch.frombuffer(bytearray(lg + blob + (right * PAD)[:PAD]), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + PAD + mis


def _cuts(records, spec, pairs=False, mis=(0, 0), seq=True, qual=True, lens=None, guard=b"N"):
    """One fqz5_trim_cuts and, where it succeeds, a fqz5_trim_gather of both
    streams: (rc, starts, new lengths, counts, compacted bases, compacted
    qualities)."""
    so = Z._load()
    lens = np.asarray([len(s) for s, _ in records] if lens is None else lens, np.uint32)
    n = len(lens)
    sblob, qblob = b"".join(s for s, _ in records), b"".join(q for _, q in records)
    st, sp = _dev(sblob, mis[0], guard, guard)
    qt, qp = _dev(qblob, mis[1], b"\x00", b"\xc8")
    start = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda")
    new = np.full(n + 2, GUARD, np.uint32)
    counts = np.zeros(NWORDS + 2, np.uint64)
    counts[0] = counts[-1] = GUARD64
    t, ad = Z.Trim(**spec).spec()
    lib.after_torch()
    rc = so.fqz5_trim_cuts(C.byref(t), C.byref(ad), sp if seq else None, qp if qual else None,
                           len(sblob), lens.ctypes.data, n, int(pairs), start.data_ptr() + 4,
                           new.ctypes.data + 4, counts.ctypes.data + 8)
    torch.cuda.synchronize()
    assert counts[0] == counts[-1] == GUARD64 and new[0] == new[-1] == GUARD
    hs = start.cpu().numpy().view(np.uint32)
    assert hs[0] == hs[-1] == GUARD
    if rc or not n:                                         # nothing is written
        assert (hs == GUARD).all() and (new == GUARD).all() and not counts[1:-1].any()
        return rc, None, None, None, None, None
    total = int(new[1:-1].astype(np.uint64).sum())
    out = []
    for src, blob in ((sp, sblob), (qp, qblob)):
        dt = torch.full((total + 2 * PAD,), 0x5A, dtype=torch.uint8, device="cuda")
        got = C.c_uint64(12345)
        lib.after_torch()
        grc = so.fqz5_trim_gather(src, len(blob), lens.ctypes.data, start.data_ptr() + 4,
                                  new.ctypes.data + 4, n, dt.data_ptr() + PAD, total, C.byref(got))
        torch.cuda.synchronize()
        assert grc == 0, lib.last_error()
        assert got.value == total
        d = dt.cpu().numpy()
        assert (d[:PAD] == 0x5A).all() and (d[PAD + total:] == 0x5A).all()
        out.append(d[PAD:PAD + total].tobytes())
    return rc, hs[1:-1], new[1:-1], counts[1:-1], out[0], out[1]


def _both(records, spec, pairs=False, mis=(0, 0), guard=b"N", what=None):
    """The GPU against the host restatement and against trim_ref."""
    rc, start, new, counts, seq, qual = _cuts(records, spec, pairs, mis, guard=guard)
    assert rc == 0, lib.last_error()
    hstart, hnew, hcounts, hseq, hqual = Z._trim_host(
        Z.Trim(**spec), b"".join(s for s, _ in records), b"".join(q for _, q in records),
        [len(s) for s, _ in records], pairs, compact=True)
    bad = np.flatnonzero((start != hstart) | (new != hnew))
    assert not len(bad), (what, bad[:5].tolist(), start[bad[:5]], hstart[bad[:5]], new[bad[:5]],
                          hnew[bad[:5]])
    assert counts.tolist() == hcounts.tolist(), what
    assert seq == hseq and qual == hqual, what
    want = R.trim(records, spec, pairs)
    assert start.tolist() == want.starts and new.tolist() == want.lengths, what
    assert seq == b"".join(s for s, _ in want.records), what
    assert qual == b"".join(q for _, q in want.records), what
    assert counts[:2].tolist() == [want.bases_in, want.bases_out], what
    assert counts[2:7].tolist() == want.trimmed and counts[7:12].tolist() == want.removed, what
    n_ad = len(want.adapter_hits)
    assert counts[12:12 + n_ad].tolist() == want.adapter_hits and not counts[12 + n_ad:].any(), what
    return want


LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]


@pytest.mark.parametrize("mis", [(0, 0), (1, 15), (15, 1)])
def test_lengths_at_the_wave_edges(mis):
    """Every step on records of 0 .. 4097 bases, three of each, as views at
    misalignments 0, 1 and 15; the guard bytes are 'N' (trim_n would walk on)
    and the adapter's own bytes (an adapter cut off by the end would match
    further)."""
    rng = random.Random(100 + mis[0])
    records = _records(rng, LENS * 3)
    for guard in (b"N", AD):
        want = _both(records, ALL, mis=mis, guard=guard, what=(mis, guard))
        assert all(0 < t < len(records) for t in want.trimmed)
    _both(records, dict(ALL, adapters2=[b"ACGTNacg"]), pairs=True, mis=mis)
    for step, spec in (("quality", {"q3": 20}), ("quality", {"q5": 25}),
                       ("adapter", {"adapters": [AD]}), ("trim_n", {"trim_n": True}),
                       ("clip", {"head": 64, "tail": 64}), ("crop", {"max_len": 64})):
        want = _both(records, spec, mis=mis, guard=AD if step == "adapter" else b"N", what=spec)
        assert 0 < want.trimmed[R.STEPS.index(step)] < len(records), spec


def test_runs_of_empty_records():
    rng = random.Random(9)
    lens = [0] * 300 + [100, 0, 0, 7, 64] + [0] * 310 + [11, 500] + [0] * 305
    records = _records(rng, lens)
    for pairs in (False, True):
        want = _both(records, ALL, pairs, mis=(1, 0))
        assert want.bases_out > 0
    empty = [(b"", b"")] * 70
    want = _both(empty, ALL)
    assert want.lengths == [0] * 70 and want.trimmed == [0] * 5


def _break_at(q, cutoff):
    """How many positions from the 3' end the scan reads before it breaks
    (len(q): it never does), by the rule."""
    total = 0
    for k, x in enumerate(reversed(q)):
        total += cutoff - x
        if total < 0:
            return k
    return len(q)


BIG = 20_000


@pytest.mark.parametrize("low,chunk", [(5, 0), (5000, 145), (10760, 312)])
def test_quality_break_in_a_long_record(low, chunk):
    """One 20 000-base record whose 3' scan breaks in its first, a middle and
    its last 64-chunk (312 of 313), and the mirror for the 5' end; the
    arg-max lies `low` positions in, chunks before the break."""
    rng = random.Random(low)
    s = bytes(rng.choice(b"ACGT") for _ in range(BIG))
    q = bytes([41] * (BIG - low) + [2] * low)
    assert _break_at(q, 20) // 64 == chunk and low // 64 <= chunk
    for mis in ((0, 0), (3, 9)):
        want = _both([(s, q)], {"q3": 20}, mis=mis)
        assert want.lengths == [BIG - low]
        want = _both([(s, q[::-1])], {"q5": 20}, mis=mis)
        assert want.starts == [low] and want.lengths == [BIG - low]
    # between other records, both ends at once
    other = _records(rng, [70, 0, 130])
    _both(other[:2] + [(s, q[::-1][:BIG // 2] + q[BIG // 2:])] + other[2:], {"q5": 20, "q3": 20},
          mis=(7, 2))


def test_all_qualities_below_the_cutoff():
    rng = random.Random(21)
    s = bytes(rng.choice(b"ACGT") for _ in range(BIG))
    q = bytes(rng.randint(0, 19) for _ in range(BIG))
    want = _both([(s, q)], {"q3": 20}, mis=(0, 5))
    assert want.lengths == [0] and want.removed[1] == BIG
    want = _both([(s, q)], {"q5": 20, "q3": 20})
    assert want.starts == [BIG] and want.lengths == [0]
    # q = 255 everywhere: the most negative terms, nothing trimmed
    want = _both([(s, bytes([255] * BIG))], {"q5": 93, "q3": 93})
    assert want.lengths == [BIG]
    # equal maxima in different chunks: the first in scan order stays
    q = bytearray([20] * BIG)
    q[BIG - 1], q[BIG - 500], q[BIG - 501] = 10, 30, 10
    want = _both([(s, bytes(q))], {"q3": 20})
    assert want.lengths == [BIG - 1]


@pytest.mark.parametrize("where", ["first", "middle", "last", "partial"])
def test_adapter_in_a_long_record(where):
    rng = random.Random(33)
    at = {"first": 0, "middle": 10_037, "last": BIG - len(AD), "partial": BIG - 4}[where]
    s = bytearray(rng.choice(b"ACGT") for _ in range(BIG))
    s[at:at + len(AD)] = AD[:BIG - at]
    q = bytes([30] * BIG)
    spec = {"adapters": [b"TTTTTTTTTTTTTTTTTTTT", AD], "min_overlap": 4}
    for mis in ((0, 0), (15, 1)):
        want = _both([(bytes(s), q)], spec, mis=mis, guard=AD, what=where)
        assert want.lengths == [at] and want.adapter_hits == [0, 1]
    other = _records(rng, [64, 1])
    want = _both(other + [(bytes(s), q)] + other[:1], spec, pairs=True, guard=AD)
    assert want.lengths[2] == at


def test_one_base_records():
    """3 000 records of one base: more records than a tile walk keeps ends for."""
    rng = random.Random(7)
    records = _records(rng, [1] * 3000, plant=False)
    for pairs, mis in ((False, (0, 0)), (True, (5, 2))):
        want = _both(records, {"q3": 20, "trim_n": True, "adapters": [b"A"], "min_overlap": 1,
                               "max_err_pct": 0}, pairs, mis=mis)
        assert all(0 < t < 3000 for t in want.trimmed[1:4])
    want = _both(records, {"head": 1})
    assert want.bases_out == 0


def test_streams_left_out_and_errors():
    rng = random.Random(19)
    records = _records(rng, [40, 3, 90, 0, 7])
    rc, start, new, counts, _, _ = _cuts(records, {"head": 3, "max_len": 30}, seq=False, qual=False)
    assert rc == 0 and new.tolist() == [30, 0, 30, 0, 4] and start.tolist() == [3, 3, 3, 0, 3]
    rc, start, new, _, _, _ = _cuts(records, {"trim_n": True}, qual=False)     # bases alone
    assert rc == 0 and new.tolist() == R.trim(records, {"trim_n": True}).lengths
    assert _cuts(records, {"q3": 20}, qual=False)[0] == -1
    assert "quality step without" in lib.last_error()
    assert _cuts(records, {"q5": 20, "head": 1}, qual=False)[0] == -1
    assert _cuts(records, {"trim_n": True}, seq=False)[0] == -1
    assert "base step without" in lib.last_error()
    assert _cuts(records, {"adapters": [AD]}, seq=False)[0] == -1
    assert _cuts(records, {"head": 1}, pairs=True)[0] == -1 and "odd record count" in lib.last_error()
    for lens in ([40, 3, 90, 0, 6], [40, 3, 90, 0, 8], [40, 3, 90, 0], []):
        assert _cuts(records, ALL, lens=lens)[0] == -1 and "do not sum" in lib.last_error()
    assert _cuts([], ALL)[0] == 0                           # nrec = 0: nothing written


def test_gather_refuses_what_it_cannot_do():
    so = Z._load()
    blob = b"ACGTACGTAC"
    t, p = _dev(blob, 0, b"N", b"N")
    lens, new = np.asarray([6, 4], np.uint32), np.asarray([3, 4], np.uint32)
    start = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    dst = torch.full((64,), 0x5A, dtype=torch.uint8, device="cuda")
    got = C.c_uint64(0)
    lib.after_torch()

    def gather(src, dstp, cap, lens=lens, new=new):
        rc = so.fqz5_trim_gather(src, len(blob), lens.ctypes.data, start.data_ptr(),
                                 new.ctypes.data, len(lens), dstp, cap, C.byref(got))
        torch.cuda.synchronize()
        return rc
    assert gather(p, p, 10) == -1 and "overlap" in lib.last_error()          # dst == src
    assert gather(p, p + 9, 7) == -1 and "overlap" in lib.last_error()
    assert gather(p, dst.data_ptr(), 6) == -1 and "too small" in lib.last_error()
    assert gather(p, dst.data_ptr(), 64, new=np.asarray([7, 4], np.uint32)) == -1
    assert "outside its record" in lib.last_error()
    assert gather(p, dst.data_ptr(), 64, lens=np.asarray([6, 5], np.uint32)) == -1
    assert "do not sum" in lib.last_error()
    assert t.cpu().numpy().tobytes()[PAD:PAD + 10] == blob and (dst.cpu().numpy() == 0x5A).all()
    assert gather(p, dst.data_ptr() + 8, 7) == 0 and got.value == 7
    d = dst.cpu().numpy()
    assert d[8:15].tobytes() == b"CGT" + b"GTAC" and (d[:8] == 0x5A).all() and (d[15:] == 0x5A).all()
