"""fqz5_stats_host (stats.hip), the host restatement of the statistics
kernels' rule, against the definitions restated with numpy (stats_ref.rule)
on random arrays.  No GPU."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import stats_ref as R


def _records(rng, lens, qual=True, alphabet=None):
    out = []
    for n in lens:
        s = bytes(rng.choice(alphabet) if alphabet else rng.randrange(256) for _ in range(n))
        out.append((s, bytes(rng.randrange(256) for _ in range(n)) if qual else None))
    return out


def _host(records, cycles, mates, out=None, per_record=False):
    seq = b"".join(s for s, _ in records)
    qual = None if records and records[0][1] is None else b"".join(q for _, q in records)
    flat, qs, gc = Z._stats_host(seq, qual, [len(s) for s, _ in records], cycles, mates, out,
                                 per_record)
    return flat, Z._stats_unpack(flat, cycles, mates), qs, gc


def test_layout():
    so = Z._load()
    assert so.fqz5_stats_words(1024, 1) == 873 + 262 * 1024
    assert so.fqz5_stats_words(7, 2) == 2 * (873 + 262 * 7)
    assert so.fqz5_stats_tile() >= 256


@pytest.mark.parametrize("mates", [1, 2])
def test_all_byte_values_and_cycle_caps(mates):
    """All 256 byte values in both streams, lengths from 0 on, and cycles of
    1, of a record's length and of that length +- 1."""
    rng = random.Random(3 + mates)
    lens = [0, 1, 37, 0, 2, 300, 36, 38, 1, 0, 5, 37]
    records = _records(rng, lens)
    records[5] = (bytes(range(256)) + records[5][0][256:], bytes(range(255, -1, -1)) + records[5][1][256:])
    for cycles in (1, 36, 37, 38, 300, 301, 1024):
        _, got, qs, gc = _host(records, cycles, mates, per_record=True)
        exp = R.rule(records, cycles, mates)
        R.same(got, exp, cycles)
        assert (qs == exp["record_qsum"]).all() and (gc == exp["record_gc"]).all()
    exp = R.rule(records, 38, mates)
    assert int(exp["empty"].sum()) == 3 and int(exp["base_counts"].sum()) == sum(lens)
    # lower case is folded in cycle_base and kept in base_counts
    one = R.rule([(b"acgtnACGTN*", bytes(11))], 16)
    assert one["cycle_base"][0, :11].argmax(1).tolist() == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5]
    assert one["base_counts"][0, ord("a")] == one["base_counts"][0, ord("A")] == 1
    _, got, _, _ = _host([(b"acgtnACGTN*", bytes(11))], 16, 1)
    R.same(got, one)


def test_bin_edges():
    """floor(100 gc / L) and floor(sum q / L) on bin edges."""
    records = [(b"GAT", bytes([10, 10, 9])), (b"C" + b"A" * 199, bytes([1] * 199 + [0])),
               (b"GC", bytes([255, 255])), (b"gcAT", bytes([0, 0, 0, 3])), (b"", b"")]
    _, got, _, _ = _host(records, 8, 1)
    exp = R.rule(records, 8, 1)
    R.same(got, exp)
    assert [int(k) for k in np.flatnonzero(exp["read_gc"][0])] == [0, 33, 50, 100]
    assert [int(k) for k in np.flatnonzero(exp["read_qual"][0])] == [0, 9, 255]
    assert int(exp["read_gc"].sum()) == 4 == int(exp["read_qual"].sum())


@pytest.mark.parametrize("mates", [1, 2])
def test_no_qualities_and_two_adds(mates):
    rng = random.Random(11)
    a = _records(rng, [5, 0, 90, 17, 1, 64], alphabet=b"ACGTNacgtn")
    b = _records(rng, [33, 12, 0, 0], qual=False, alphabet=b"ACGT")
    flat, got, _, _ = _host(b, 64, mates)
    exp_b = R.rule(b, 64, mates)
    R.same(got, exp_b)
    for k in ("qual_records", "qual_counts", "read_qual", "cycle_qual"):
        assert not got[k].any()
    # a second block into the same table
    _, both, qs, gc = _host(a, 64, mates, out=flat, per_record=True)
    R.same(both, R.add(exp_b, R.rule(a, 64, mates)))
    assert both["qual_records"].sum() == 6 and both["records"].sum() == 10
    assert (qs == R.rule(a, 64, mates)["record_qsum"]).all()


def test_refused():
    rng = random.Random(13)
    records = _records(rng, [4, 5, 6])
    seq, qual = b"".join(s for s, _ in records), b"".join(q for _, q in records)
    for lens in ([4, 5, 7], [4, 5], [4, 5, 6, 1], []):
        with pytest.raises(lib.NativeError, match="do not sum"):
            Z._stats_host(seq, qual, lens, 8, 1)
    with pytest.raises(lib.NativeError, match="odd record count"):
        Z._stats_host(seq, qual, [4, 5, 6], 8, 2)
    out = np.zeros(int(Z._load().fqz5_stats_words(8, 1)), np.uint64)
    with pytest.raises(lib.NativeError, match="cycles"):
        Z._stats_host(seq, qual, [4, 5, 6], 0, 1, out=out)
    with pytest.raises(lib.NativeError, match="smaller than the tables"):
        Z._stats_host(seq, qual, [4, 5, 6], 9, 1, out=out)
    assert not out.any()                                   # nothing was added by a refused call
    Z._stats_host(seq, qual, [4, 5, 6], 8, 1, out=out)
    assert out[0] == 3 and out[1] == 15


def test_nx_and_merged_lengths():
    rng = random.Random(17)
    lens = [rng.choice([0, 1, 50, 50, 75, 1000, 12345]) for _ in range(200)]
    a = np.unique(np.asarray(lens[:120], np.uint32), return_counts=True)
    b = np.unique(np.asarray(lens[120:], np.uint32), return_counts=True)
    v, c = Z._merge_lengths((a[0], a[1].astype(np.uint64)), (b[0], b[1].astype(np.uint64)))
    ev, ec = np.unique(lens, return_counts=True)
    assert v.tolist() == ev.tolist() and c.tolist() == ec.tolist() and c.dtype == np.uint64
    st = Z.Stats(1, {}, [(v, c)], 0)
    for x in (0.001, 10, 50, 90, 99.999, 100):
        assert st.nx(x) == R.nx(lens, x), x
    assert st.nx(50) in (1000, 12345)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    assert Z.Stats(1, {}, [none], 0).nx(50) == 0
    # a 1 Gbase record stays two cells
    v, c = Z._merge_lengths(none, (np.asarray([10**9], np.uint32), np.asarray([3], np.uint64)))
    assert Z.Stats(1, {}, [(v, c)], 0).nx(50) == 10**9
