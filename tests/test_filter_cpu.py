"""fqz5_filter_host (filter.hip), the host restatement of the filter by read
metrics, and fqz5file.Filter's validation.  No GPU.

Expected values come from the rule restated in plain Python (filter_ref)."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import filter_ref as R


def _host(records, crit, pairs=False, invert=False, lens=None):
    seq = b"".join(s for s, _ in records)
    has_q = bool(records) and records[0][1] is not None
    qual = b"".join(q for _, q in records) if has_q else None
    return Z._filter_host(Z.Filter(**crit), seq, qual,
                          [len(s) for s, _ in records] if lens is None else lens, pairs, invert)


def _same(records, crit, pairs=False, invert=False):
    keep, failed, sums = _host(records, crit, pairs, invert)
    ek, ef, _ = R.rule(records, crit, pairs, invert)
    assert keep.tolist() == [int(k) for k in ek], crit
    assert failed.dtype == np.uint64 and failed.tolist() == ef, crit
    exp = [R.sums(r, crit.get("low_q")) for r in records]
    for k in range(5):
        assert sums[k].tolist() == [e[k + 1] for e in exp], (crit, k)
    return keep.tolist(), failed.tolist()


def _records(rng, lens, alphabet=b"ACGTN", quals=range(2, 42)):
    quals = list(quals)
    return [(bytes(rng.choice(alphabet) for _ in range(n)), bytes(rng.choice(quals) for _ in range(n)))
            for n in lens]


CRITERIA = [{"min_len": 20}, {"max_len": 60}, {"min_len": 20, "max_len": 60}, {"max_n": 3},
            {"min_mean_q": 22}, {"low_q": 20, "max_low_pct": 45}, {"gc_pct": (30, 50)},
            {"min_complexity_pct": 76},
            {"min_len": 10, "max_len": 90, "max_n": 8, "min_mean_q": 20, "low_q": 10,
             "max_low_pct": 30, "gc_pct": (25, 60), "min_complexity_pct": 70}]


@pytest.mark.parametrize("crit", CRITERIA, ids=lambda c: "+".join(c))
def test_host_against_the_rule(crit):
    rng = random.Random(11)
    records = _records(rng, [rng.randint(0, 100) for _ in range(300)], alphabet=b"ACGTNacgtn")
    for pairs in (False, True):
        for invert in (False, True):
            keep, failed = _same(records, crit, pairs, invert)
    assert 0 < sum(_same(records, crit)[0]) < 300          # (the case decides something)


def test_filter_validation():
    ok = Z.Filter(min_len=5, max_len=5, max_n=0, min_mean_q=0, low_q=0, max_low_pct=100,
                  gc_pct=(50, 50), min_complexity_pct=100)
    assert ok.spec().set == 0x7F and ok.keys() == (Z.S.SEC_SEQ, Z.S.SEC_QUAL)
    assert Z.Filter().spec().set == 0 and Z.Filter().keys() == ()
    assert Z.Filter(min_len=1, max_len=2).keys() == ()
    for base in ({"max_n": 1}, {"gc_pct": (0, 100)}, {"min_complexity_pct": 1}):
        assert Z.Filter(**base).keys() == (Z.S.SEC_SEQ,)
    for bad in ({"min_len": -1}, {"max_len": -1}, {"max_n": -1}, {"min_mean_q": -1},
                {"low_q": -1, "max_low_pct": 1}, {"low_q": 1, "max_low_pct": -1},
                {"gc_pct": (-1, 5)}, {"min_complexity_pct": -1},
                {"low_q": 1, "max_low_pct": 101}, {"gc_pct": (0, 101)}, {"gc_pct": (101, 101)},
                {"min_complexity_pct": 101}, {"gc_pct": (51, 50)}, {"low_q": 3},
                {"max_low_pct": 3}, {"min_len": 6, "max_len": 5}):
        with pytest.raises(ValueError, match="Filter"):
            Z.Filter(**bad)
    assert Z.FilterHits.REASONS == R.REASONS and len(R.REASONS) == 7


def test_equality_thresholds():
    """Each ratio criterion exactly on its threshold passes; one unit off fails."""
    on = (b"ACGTACGTAC", bytes([20] * 10))                 # qsum 200 = 20 * 10
    off = (b"ACGTACGTAC", bytes([20] * 9 + [19]))          # 199
    assert _same([on, off], {"min_mean_q": 20})[0] == [1, 0]
    # 3 of 10 below 15: 300 = 30 * 10; 4 of 10: 400 > 300
    on = (b"A" * 10, bytes([14] * 3 + [15] * 7))
    off = (b"A" * 10, bytes([14] * 4 + [15] * 6))
    assert _same([on, off], {"low_q": 15, "max_low_pct": 30})[0] == [1, 0]
    # gc 4 of 10 = 40 %: both edges
    rec = lambda gc: (b"G" * gc + b"A" * (10 - gc), bytes(10))
    assert _same([rec(3), rec(4), rec(5)], {"gc_pct": (40, 100)})[0] == [0, 1, 1]
    assert _same([rec(3), rec(4), rec(5)], {"gc_pct": (0, 40)})[0] == [1, 1, 0]
    assert _same([rec(3), rec(4), rec(5)], {"gc_pct": (40, 40)})[0] == [0, 1, 0]
    # L = 11: 10 neighbour pairs, 5 of them differ: 500 = 50 * 10; 4: 400 < 500
    on = (b"ACACAC" + b"C" * 5, bytes(11))
    off = (b"ACACA" + b"A" * 6, bytes(11))
    assert R.sums(on)[3] == 5 and R.sums(off)[3] == 4
    assert _same([on, off], {"min_complexity_pct": 50})[0] == [1, 0]
    # max_n and the lengths
    assert _same([(b"NnA", bytes(3)), (b"NnN", bytes(3))], {"max_n": 2})[0] == [1, 0]
    assert _same([(b"A" * k, bytes(k)) for k in (4, 5, 6, 7)],
                 {"min_len": 5, "max_len": 6})[0] == [0, 1, 1, 0]


def test_lengths_zero_and_one():
    """L = 0: every ratio criterion holds, the lengths alone decide.  L = 1:
    no neighbour, complexity holds at any percentage."""
    e, one = (b"", b""), (b"N", bytes([0]))
    ratio = {"max_n": 0, "min_mean_q": 40, "low_q": 50, "max_low_pct": 0, "gc_pct": (50, 60),
             "min_complexity_pct": 100}
    keep, failed = _same([e, one, e], ratio)
    assert keep == [1, 0, 1] and failed == [0, 0, 1, 0, 0, 0, 0]
    assert _same([e, one], dict(ratio, min_len=1))[0] == [0, 0]
    assert _same([e, one], {"max_len": 0})[0] == [1, 0]
    assert _same([e, one, (b"AA", bytes(2)), (b"AC", bytes(2))],
                 {"min_complexity_pct": 100})[0] == [1, 1, 0, 1]


def test_reason_is_the_lowest_index():
    bad = (b"NNNN", bytes([1] * 4))                        # fails 0, 2, 3, 4, 5, 6
    crit = {"min_len": 5, "max_len": 9, "max_n": 0, "min_mean_q": 9, "low_q": 5, "max_low_pct": 10,
            "gc_pct": (10, 90), "min_complexity_pct": 10}
    order = ["min_len", "max_n", "min_mean_q", "low_q", "gc_pct", "min_complexity_pct"]
    for k, name in enumerate(order):
        c = {a: b for a, b in crit.items() if a not in order[:k]}
        if "low_q" not in c:
            c.pop("max_low_pct", None)
        _, failed = _same([bad], c)
        assert failed == [int(i == R.REASONS.index(name)) for i in range(7)], name
    assert _same([(b"A" * 10, bytes(10))], {"max_len": 9, "min_mean_q": 1})[1] == [0, 1, 0, 0, 0, 0, 0]


def test_pairs_and_invert():
    good, short, nn = (b"ACGTAC", bytes([30] * 6)), (b"AC", bytes([30] * 2)), (b"ACNNNN", bytes([30] * 6))
    crit = {"min_len": 3, "max_n": 1}
    recs = [good, good, good, short, nn, good, nn, short, short, nn]
    keep, failed = _same(recs, crit, pairs=True)
    assert keep == [1, 1] + [0] * 8 and failed == [3, 0, 1, 0, 0, 0, 0]    # (pair 3: min(2, 0))
    keep, failed = _same(recs, crit, pairs=True, invert=True)
    assert keep == [0, 0] + [1] * 8 and failed == [3, 0, 1, 0, 0, 0, 0]
    assert _same(recs, crit)[0] == [1, 1, 1, 0, 0, 1, 0, 0, 0, 0]
    assert _same(recs, crit, invert=True)[0] == [0, 0, 0, 1, 1, 0, 1, 1, 1, 1]
    assert _same([], crit, pairs=True) == ([], [0] * 7)


def test_errors():
    good = (b"ACGTAC", bytes([30] * 6))
    with pytest.raises(lib.NativeError, match="odd record count"):
        _host([good] * 3, {"min_len": 1}, pairs=True)
    for lens in ([6, 5], [6, 7], [6], []):
        with pytest.raises(lib.NativeError, match="do not sum"):
            _host([good] * 2, {"min_len": 1}, lens=lens)
    with pytest.raises(lib.NativeError, match="quality criterion without"):
        _host([(b"ACGT", None)], {"min_mean_q": 1})
    with pytest.raises(lib.NativeError, match="base criterion without"):
        Z._filter_host(Z.Filter(max_n=1), None, None, [4])
    keep, failed, sums = Z._filter_host(Z.Filter(min_len=5), None, None, [4, 5])
    assert keep.tolist() == [0, 1] and failed.tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert not any(s.any() for s in sums)
