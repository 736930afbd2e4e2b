"""fqz5_stats_add / fqz5_stats_read (stats.hip) on synthetic device arrays:
the statistics of a block's bases and qualities (two device buffers, the
records' bytes one after the other).  No codec is involved.

Expected values come from the definitions restated with numpy
(stats_ref.rule); fqz5_stats_host, the host restatement, must say the same.
Guard bytes (0x55) surround every output and must stay untouched."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import stats_ref as R

pytestmark = pytest.mark.gpu
GUARD64 = 0x5555555555555555


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def T():
    return int(Z._load().fqz5_stats_tile())


def _records(rng, lens, alphabet=b"ACGTN", quals=range(2, 42), qual=True):
    quals = list(quals)
    return [(bytes(rng.choice(alphabet) for _ in range(n)),
             bytes(rng.choice(quals) for _ in range(n)) if qual else None) for n in lens]


def _cut(total: int, cuts) -> list[int]:
    """Record lengths of `total` bases cut at `cuts` (ascending; repeats give
    empty records)."""
    edges = [0] + sorted(cuts) + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def _dev(blob: bytes, pad: int):
    return torch.frombuffer(bytearray(b"\x01" * pad + blob + b"\x01" * 7), dtype=torch.uint8).cuda()


def _add(acc, records, pads=(0, 0), per_record=True, lens=None):
    """One fqz5_stats_add of the records: (rc, record_qsum, record_gc).  pads:
    how many bytes into their buffers the bases and the qualities start."""
    seq = b"".join(s for s, _ in records)
    has_q = bool(records) and records[0][1] is not None
    lens = np.asarray([len(s) for s, _ in records] if lens is None else lens, np.uint32)
    n = len(lens)
    sd = _dev(seq, pads[0])
    qd = _dev(b"".join(q for _, q in records), pads[1]) if has_q else None
    qs = torch.full((n + 2,), GUARD64, dtype=torch.int64, device="cuda")
    gc = torch.full((n + 2,), 0x55555555, dtype=torch.int32, device="cuda")
    lib.after_torch()
    rc = acc.add(sd.data_ptr() + pads[0], qd.data_ptr() + pads[1] if has_q else None, len(seq),
                 lens, qs.data_ptr() + 8 if per_record else None,
                 gc.data_ptr() + 4 if per_record else None)
    assert sd[:pads[0]].eq(1).all() and sd[pads[0] + len(seq):].eq(1).all()   # (inputs as they were)
    qs, gc = qs.cpu().numpy().view(np.uint64), gc.cpu().numpy().view(np.uint32)
    assert qs[0] == qs[-1] == GUARD64 and gc[0] == gc[-1] == 0x55555555
    if not per_record or rc:
        assert (qs == GUARD64).all() and (gc == 0x55555555).all()      # nothing was written
        return rc, None, None
    return rc, qs[1:-1], gc[1:-1]


def _read(acc) -> dict:
    """fqz5_stats_read between guard words."""
    so = Z._load()
    w = int(so.fqz5_stats_words(acc.cycles, acc.mates))
    out = np.full(w + 4, GUARD64, np.uint64)
    assert so.fqz5_stats_read(acc.p, out.ctypes.data + 16, w) == 0, lib.last_error()
    assert (out[:2] == GUARD64).all() and (out[-2:] == GUARD64).all()
    assert so.fqz5_stats_read(acc.p, out.ctypes.data + 16, w - 1) == -1
    return Z._stats_unpack(out[2:-2], acc.cycles, acc.mates)


def _host(records, cycles, mates):
    seq = b"".join(s for s, _ in records)
    qual = b"".join(q for _, q in records) if records and records[0][1] is not None else None
    flat, _, _ = Z._stats_host(seq, qual, [len(s) for s, _ in records], cycles, mates)
    return Z._stats_unpack(flat, cycles, mates)


def _both(records, cycles, mates=1, pads=(0, 0), what=None):
    """The GPU against the rule and against the host restatement."""
    exp = R.rule(records, cycles, mates)
    with Z._StatsAcc(cycles, mates) as acc:
        rc, qs, gc = _add(acc, records, pads)
        assert rc == 0, lib.last_error()
        got = _read(acc)
    R.same(got, exp, what)
    R.same(_host(records, cycles, mates), exp, what)
    assert (qs == exp["record_qsum"]).all() and (gc == exp["record_gc"]).all(), what
    return got


@pytest.mark.parametrize("pads", [(0, 0), (0, 3), (3, 0), (3, 3)])
def test_total_sizes(T, pads):
    """0, 1, T - 1, T, T + 1 and 3T + 5 bases in a handful of records; the two
    arrays misaligned independently."""
    rng = random.Random(5 + 7 * pads[0] + pads[1])
    for total in (0, 1, T - 1, T, T + 1, 3 * T + 5):
        cuts = sorted(rng.randrange(total + 1) for _ in range(4)) + [total]    # (the last is empty)
        records = _records(rng, _cut(total, cuts))
        got = _both(records, 100, pads=pads, what=total)
        assert int(got["bases"][0]) == total and int(got["records"][0]) == 6
        _both(records, 100, mates=2, pads=pads, what=total)


@pytest.mark.parametrize("mis_seq", range(16))
def test_misaligned_views(T, mis_seq):
    """The bases at every misalignment, the qualities at another: T + 5 bases
    cut into records at T - 1, T and T + 1, cycles 64, so the long record's
    chunks past the cycle window are skipped without a load at every
    alignment of the chunk grid.  Against fqz5_stats_host."""
    rng = random.Random(60 + mis_seq)
    records = _records(rng, _cut(T + 5, [T - 1, T, T + 1]), alphabet=b"ACGTNacgt", quals=range(256))
    got = _both(records, 64, pads=(mis_seq, (5 * mis_seq + 3) % 16), what=mis_seq)
    R.same(got, _host(records, 64, 1), mis_seq)
    assert int(got["cycle_base"].sum()) == 64 + 1 + 1 + 4


@pytest.mark.parametrize("cycles", ["1", "64", "65", "2T"])
def test_one_record_across_tiles(T, cycles):
    """One record of 3T + 5 bases: its sums cross three tile edges."""
    cycles = 2 * T if cycles == "2T" else int(cycles)
    rng = random.Random(19)
    records = _records(rng, [3 * T + 5], alphabet=b"ACGTNacgt", quals=range(256))
    for pads in ((0, 0), (3, 1)):
        got = _both(records, cycles, pads=pads)
        assert int(got["cycle_qual"].sum()) == cycles and int(got["read_qual"].sum()) == 1


def test_short_records_and_runs_of_empty_ones(T):
    """Records of 1 to 4 bases filling 2T bases (more records than a lane has
    bytes), with runs of 300 and more empty records at the start, across the
    tile edge and at the end."""
    rng = random.Random(23)
    lens, tot = [0] * 300, 0
    while tot < 2 * T:
        n = min(rng.randint(1, 4), 2 * T - tot, T - tot if tot < T else 4)
        lens.append(n)
        tot += n
        if tot == T:
            lens += [0] * 310
    lens += [0] * 305
    assert sum(lens) == 2 * T and lens.count(0) == 915 and len(lens) > 2 * T // 4 + 915
    at = np.cumsum(lens)
    assert (at == T).sum() == 311                          # the run sits on the edge
    records = _records(rng, lens)
    for mates, pads in ((1, (0, 0)), (1, (3, 2)), (2, (1, 0))):
        if mates == 2 and len(records) % 2:
            records = records + [(b"", b"")]
        got = _both(records, 3, mates, pads)
        assert int(got["empty"].sum()) >= 915
    _both(records, 1024, 1)
    # one base per record: as many records as bases in every tile
    _both(_records(rng, [1] * (T + 50)), 2, 2, (0, 1))


def test_the_cap_row(T):
    """A record of exactly `cycles` bases, then one of cycles + 1: the last
    row counts both, position `cycles` only the whole-file tables."""
    for cycles in (5, 64, T):
        records = [(b"A" * cycles, bytes([7] * cycles)), (b"C" * cycles + b"T", bytes([9] * cycles + [40]))]
        got = _both(records, cycles)
        assert got["cycle_base"][0, -1].tolist() == [1, 1, 0, 0, 0, 0]
        assert got["cycle_qual"][0, -1, 7] == got["cycle_qual"][0, -1, 9] == 1
        assert int(got["cycle_qual"].sum()) == 2 * cycles and not got["cycle_qual"][0, :, 40].any()
        assert got["qual_counts"][0, 40] == 1 and got["base_counts"][0, ord("T")] == 1
        assert int(got["cycle_base"][0, :, 3].sum()) == 0


def test_one_hot_cell():
    """70 000 records of 4 bases, all 'A' with one quality: every cycle_qual
    cell in use takes 70 000 adds (more than 2^16), qual_counts 280 000."""
    n = 70_000
    records = [(b"AAAA", b"\x25\x25\x25\x25")] * n
    with Z._StatsAcc(8, 1) as acc:
        rc, qs, gc = _add(acc, records, (1, 2))
        assert rc == 0, lib.last_error()
        got = _read(acc)
    exp = {k: np.zeros_like(v) for k, v in R.rule([], 8, 1).items()}
    exp["records"][0] = exp["qual_records"][0] = n
    exp["bases"][0] = 4 * n
    exp["base_counts"][0, ord("A")] = exp["qual_counts"][0, 0x25] = 4 * n
    exp["read_qual"][0, 0x25] = exp["read_gc"][0, 0] = n
    exp["cycle_base"][0, :4, 0] = exp["cycle_qual"][0, :4, 0x25] = n
    R.same(got, exp)
    R.same(_host(records, 8, 1), exp)
    assert (qs == 4 * 0x25).all() and not gc.any()


def test_all_byte_values_and_bin_edges():
    """All 256 values in both streams; lower case folded in cycle_base and
    kept in base_counts; records whose per-read bins sit on an edge."""
    rng = random.Random(29)
    records = [(bytes(range(256)), bytes(range(255, -1, -1))),
               (b"GAT", bytes([10, 10, 9])), (b"c" + b"A" * 199, bytes([1] * 199 + [0])),
               (b"GC", bytes([255, 255])), (b"gcat", bytes([0, 0, 0, 3]))]
    records += _records(rng, [300, 0, 77], alphabet=bytes(range(256)), quals=range(256))
    got = _both(records, 256, pads=(2, 3))
    exp = R.rule(records[1:5], 8)
    assert np.flatnonzero(exp["read_gc"][0]).tolist() == [0, 33, 50, 100]
    assert np.flatnonzero(exp["read_qual"][0]).tolist() == [0, 9, 255]
    assert got["base_counts"][0, ord("a")] >= 2 and got["base_counts"][0, ord("A")] >= 200
    assert got["cycle_base"][0, ord("a"), 0] >= 1 and got["cycle_base"][0, ord("A"), 0] >= 1
    assert got["read_gc"][0, 33] >= 1 and got["read_gc"][0, 100] >= 1 and got["read_qual"][0, 255] >= 1


def test_two_mates(T):
    """Mates of different lengths and qualities; an odd count is refused."""
    rng = random.Random(31)
    records = []
    for _ in range(120):
        records += _records(rng, [rng.randint(90, 150)], quals=range(30, 41))
        records += _records(rng, [rng.randint(20, 60)], alphabet=b"ACGTacgt", quals=range(2, 20))
    assert sum(len(s) for s, _ in records) > 2 * T
    got = _both(records, 128, mates=2, pads=(3, 0))
    assert not got["qual_counts"][0, :30].any() and not got["qual_counts"][1, 20:].any()
    assert not got["cycle_base"][1, 60:].any() and got["cycle_base"][0, 89].sum() == 120
    R.same(_both(records, 128, mates=1), R.rule(records, 128, 1))
    with Z._StatsAcc(128, 2) as acc:
        rc, _, _ = _add(acc, records[:-1])
        assert rc == -1 and "odd record count" in lib.last_error()
        assert not any(v.any() for v in _read(acc).values())


def test_no_qualities_and_two_blocks(T):
    """d_qual NULL leaves the quality tables and qual_records as they were;
    two blocks into one accumulator are the sum of the two alone; per-record
    pointers of NULL write nothing else."""
    rng = random.Random(37)
    a = _records(rng, _cut(T + 100, [0, 50, 50, T - 1, T + 3]), quals=range(256))
    b = _records(rng, [40, 0, T + 9, 1], qual=False)
    c = _records(rng, [3, 70, 2 * T], alphabet=b"ACGTNacgtn*")
    ea, eb, ec = (R.rule(x, 90, 1) for x in (a, b, c))
    with Z._StatsAcc(90, 1) as acc:
        assert _add(acc, a, (1, 2))[0] == 0
        R.same(_read(acc), ea)
        rc, qs, gc = _add(acc, b, (3, 0))
        assert rc == 0 and not qs.any() and (gc == eb["record_gc"]).all()
        got = _read(acc)
        R.same(got, R.add(ea, eb))
        for k in ("qual_records", "qual_counts", "read_qual", "cycle_qual"):
            assert (got[k] == ea[k]).all()
        assert _add(acc, c, (0, 3), per_record=False)[0] == 0
        R.same(_read(acc), R.add(R.add(ea, eb), ec))
    R.same(_host(b, 90, 1), eb)


def test_limits():
    rng = random.Random(41)
    records = _records(rng, [16, 4, 19])
    with Z._StatsAcc(4, 1) as acc:
        assert _add(acc, [])[0] == 0                       # nrec = 0
        for lens in ([16, 4, 18], [16, 4, 20], [16, 4], []):
            rc, _, _ = _add(acc, records, lens=lens)
            assert rc == -1 and "do not sum" in lib.last_error()
        assert not any(v.any() for v in _read(acc).values())
        assert _add(acc, [(b"", b""), (b"", b"")])[0] == 0  # records without a base
        got = _read(acc)
        assert got["records"][0] == got["empty"][0] == got["qual_records"][0] == 2
        assert not got["base_counts"].any() and not got["read_gc"].any()
    so = Z._load()
    for cycles, mates in ((0, 1), (65537, 1), (4, 0), (4, 3)):
        assert not so.fqz5_stats_new(cycles, mates) and lib.last_error()
