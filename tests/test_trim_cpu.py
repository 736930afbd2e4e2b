"""fqz5_trim_host (trim.hip's one-thread restatement, no GPU) against the rule
in plain Python (trim_ref), the Trim arguments' validation, and TrimHits'
constants.  Expected values never come from the code under test."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import trim_ref as R

AD1 = [b"AGATCGGAAGAGC", b"CTGTCTCTTATACACATCT"]
AD2 = [b"TTACGGCATTGAC"]
STEPS = {
    "clip": {"head": 5, "tail": 3},
    "quality": {"q5": 18, "q3": 20},
    "adapter": {"adapters": AD1, "min_overlap": 4, "max_err_pct": 12},
    "trim_n": {"trim_n": True},
    "crop": {"max_len": 100},
}
ALL = {k: v for d in STEPS.values() for k, v in d.items()}


def _planted(n=300, seed=11):
    """n records of length 0..200 over ACGTNacgtn, qualities 2..41; a third
    with an adapter (whole, or cut off by the record's end) written in, another
    third with a low-quality tail, every 50th empty."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = 0 if i % 50 == 7 else rng.randint(0, 200)
        s = bytearray(rng.choice(b"ACGTNacgtn") for _ in range(L))
        q = bytearray(rng.randint(2, 41) for _ in range(L))
        if i % 3 == 0 and L > 8:
            ad = rng.choice(AD1 + AD2)
            at = rng.randint(0, L - 4)
            s[at:at + len(ad)] = ad[:L - at]
        if i % 3 == 1 and L:
            k = rng.randint(1, min(L, 30))
            q[L - k:] = bytes(rng.randint(2, 12) for _ in range(k))
        out.append((bytes(s), bytes(q)))
    return out


RECORDS = _planted()


def _host(records, spec, pairs=False):
    seq = b"".join(s for s, _ in records)
    qual = b"".join(q for _, q in records)
    return Z._trim_host(Z.Trim(**spec), seq, qual, [len(s) for s, _ in records], pairs,
                        compact=True)


def _same(records, spec, pairs=False, what=None):
    want = R.trim(records, spec, pairs)
    start, new, counts, seq, qual = _host(records, spec, pairs)
    assert start.tolist() == want.starts and new.tolist() == want.lengths, what
    assert seq == b"".join(s for s, _ in want.records), what
    assert qual == b"".join(q for _, q in want.records), what
    n_ad = len(want.adapter_hits)
    assert counts[:2].tolist() == [want.bases_in, want.bases_out], what
    assert counts[2:7].tolist() == want.trimmed and counts[7:12].tolist() == want.removed, what
    assert counts[12:12 + n_ad].tolist() == want.adapter_hits and not counts[12 + n_ad:].any(), what
    return want


@pytest.mark.parametrize("step", list(STEPS))
def test_each_step_alone(step):
    k = R.STEPS.index(step)
    want = _same(RECORDS, STEPS[step], what=step)
    assert 0 < want.trimmed[k] < len(RECORDS), step         # some records, not all
    assert want.trimmed[k] == sum(want.trimmed) and want.removed[k] == want.bases_in - want.bases_out
    if step == "adapter":
        assert all(want.adapter_hits)
    if step == "quality":
        for spec in ({"q5": 18}, {"q3": 20}):
            one = _same(RECORDS, spec, what=spec)
            assert 0 < one.trimmed[1] < len(RECORDS)


@pytest.mark.parametrize("pairs", [False, True])
def test_all_steps_together(pairs):
    spec = dict(ALL, adapters2=AD2) if pairs else ALL
    want = _same(RECORDS, spec, pairs, what=pairs)
    assert all(0 < t < len(RECORDS) for t in want.trimmed)
    if pairs:                                               # mate 2's adapter counted in its own slot
        assert want.adapter_hits[2] > 0
        assert want.lengths != R.trim(RECORDS, spec).lengths
        alone = _same(RECORDS, ALL, True)                   # without adapters2 both mates share
        assert alone.lengths == R.trim(RECORDS, ALL).lengths


def _one(s, q, spec):
    """(start, length) of the one record by the host, checked against the rule."""
    want = _same([(s, bytes(q))], spec, what=(s, list(q), spec))
    return want.starts[0], want.lengths[0]


def test_quality_break_tie_and_crossing():
    # 3' end, cutoff 20, terms from the end: +10 (sum 10), -15 (sum -5: the
    # break), then +18 +18 would reach 31 > 10 but lies past the break
    q = [2, 2, 35, 10]
    assert _one(b"ACGT", q, {"q3": 20}) == (0, 3)
    # the same without the break: the larger, later maximum is taken
    assert _one(b"ACGT", [2, 2, 25, 10], {"q3": 20}) == (0, 0)
    # a tie in best: sums 5, 0, 5 from the end; the first maximum (larger i) stays
    assert _one(b"ACG", [15, 25, 15], {"q3": 20}) == (0, 2)
    assert _one(b"ACG", [15, 25, 15], {"q5": 20}) == (1, 2)
    # sum exactly 0 is no break: sums 10, 0, 15, then -5
    assert _one(b"ACGT", [10, 30, 5, 40], {"q5": 20}) == (3, 1)
    # both ends cross: everything is below both cutoffs
    assert _one(b"ACGTA", [5] * 5, {"q5": 20, "q3": 20}) == (5, 0)
    # each end is judged on what the clip left, not on what the other end left
    assert _one(b"ACGTAC", [5, 5, 41, 41, 5, 5], {"q5": 20, "q3": 20}) == (2, 2)
    assert _one(b"AACGTACC", [40, 5, 5, 41, 41, 5, 5, 40], {"q5": 20, "q3": 20, "head": 1, "tail": 1}) \
        == (3, 2)
    # cutoff 0 trims nothing, 93 with q 93 nothing either (the sum stays 0)
    assert _one(b"ACG", [0, 0, 0], {"q3": 0, "q5": 0}) == (0, 3)
    assert _one(b"ACG", [93, 93, 93], {"q3": 93}) == (0, 3)


def test_adapter_mismatches_and_overlap():
    ad = b"ACGTACGTACGTACGTACGT"                              # 20 bytes: 10 % allows 2
    read = b"T" * 10 + ad
    two = bytearray(read)
    two[12], two[25] = ord("T"), ord("A")
    three = bytearray(two)
    three[29] = ord("A")
    q = [30] * 30
    spec = {"adapters": [ad], "min_overlap": 3, "max_err_pct": 10}
    assert _one(read, q, spec) == (0, 10)
    assert _one(bytes(two), q, spec) == (0, 10)             # exactly at (10 * 20) / 100
    assert _one(bytes(three), q, spec)[1] > 10              # one over
    # an overlap of exactly min_overlap at the read's end, and one under
    spec = {"adapters": [b"GGGTTT"], "min_overlap": 3, "max_err_pct": 0}
    assert _one(b"ACACACGGG", [30] * 9, spec) == (0, 6)
    assert _one(b"ACACACAGG", [30] * 9, spec) == (0, 9)
    # integer division: 9 % of 11 bytes allows no mismatch, 10 % of 10 bytes one
    assert _one(b"CCAAAAAAAAAAT", [30] * 13, {"adapters": [b"AAAAAGAAAAA"], "max_err_pct": 9}) == (0, 13)
    assert _one(b"CCAAAAAAAAAAT", [30] * 13, {"adapters": [b"AAAAAGAAAA"], "max_err_pct": 10}) == (0, 2)
    # an adapter longer than the read, matching from its first base: an empty record
    assert _one(b"ACGTAC", [30] * 6, {"adapters": [b"ACGTACGTTTTT"]}) == (0, 0)
    # at p = a after a clip
    assert _one(b"TTACGTAC", [30] * 8, {"adapters": [b"ACGTAC"], "head": 2}) == (2, 0)
    # no case folding, no wildcard
    assert _one(b"TTTTacgtac", [30] * 10, {"adapters": [b"ACGTAC"]}) == (0, 10)
    assert _one(b"TTTTNNNNNN", [30] * 10, {"adapters": [b"ACGTAC"]}) == (0, 10)
    # two adapters at the same p: the lower index is counted
    s, q = b"TTTTACGTAC", bytes([30] * 10)
    for ads, hits in (([b"ACGTAC", b"ACGT"], [1, 0]), ([b"ACGT", b"ACGTAC"], [1, 0]),
                      ([b"GGGG", b"ACGT"], [0, 1]), ([b"CGTA", b"ACGT"], [0, 1])):
        want = _same([(s, q)], {"adapters": ads})
        assert want.adapter_hits == hits and want.lengths == [4]


def test_n_clip_and_crop_edges():
    assert _one(b"NNnnNN", [30] * 6, {"trim_n": True}) == (6, 0)      # all N
    assert _one(b"NnACNGTnN", [30] * 9, {"trim_n": True}) == (2, 5)
    assert _one(b"ACGTACGT", [30] * 8, {"head": 6, "tail": 5}) == (6, 0)   # head + tail > L
    assert _one(b"ACGTACGT", [30] * 8, {"head": 100}) == (8, 0)
    assert _one(b"ACGTACGT", [30] * 8, {"tail": 100}) == (0, 0)
    assert _one(b"ACGTACGT", [30] * 8, {"head": 0, "tail": 0}) == (0, 8)
    assert _one(b"ACGTACGT", [30] * 8, {"max_len": 0}) == (0, 0)
    assert _one(b"NACGTACGT", [30] * 9, {"max_len": 3, "trim_n": True}) == (1, 3)
    assert _one(b"ACGTACGT", [30] * 8, {"max_len": 1 << 70, "head": 1 << 70}) == (8, 0)
    assert _one(b"", [], ALL) == (0, 0)
    want = _same([(b"", b"")] * 5, ALL, pairs=False)
    assert want.trimmed == [0] * 5 and want.bases_in == 0
    assert _same([], ALL).lengths == []                     # nrec = 0


def test_streams_a_step_needs():
    lens = np.asarray([4, 2], np.uint32)
    assert Z._trim_host(Z.Trim(head=1, max_len=2), None, None, lens)[1].tolist() == [2, 1]
    assert Z._trim_host(Z.Trim(trim_n=True), b"NACGNN", None, lens)[1].tolist() == [3, 0]
    for trim, seq, qual, msg in ((Z.Trim(q3=20), b"ACGTAC", None, "quality step without"),
                                 (Z.Trim(trim_n=True), None, b"123456", "base step without"),
                                 (Z.Trim(adapters=[b"ACG"]), None, None, "base step without")):
        with pytest.raises(lib.NativeError, match=msg):
            Z._trim_host(trim, seq, qual, lens)
    with pytest.raises(lib.NativeError, match="do not sum"):
        Z._trim_host(Z.Trim(head=1), b"ACGTA", b"12345", lens)
    with pytest.raises(lib.NativeError, match="odd record count"):
        Z._trim_host(Z.Trim(head=1), b"ACG", b"123", [3], pairs=True)


def test_trim_validation():
    bad = [{"head": -1}, {"tail": -1}, {"q5": -1}, {"q3": -2}, {"max_len": -1},
           {"q5": 94}, {"q3": 94},
           {"adapters": [b"ACGT"], "max_err_pct": 101}, {"adapters": [b"ACGT"], "max_err_pct": -1},
           {"adapters": [b"ACGT"], "min_overlap": 0}, {"adapters": [b"ACGT"], "min_overlap": -3},
           {"adapters": [b""]}, {"adapters": []}, {"adapters": [b"A" * 129]},
           {"adapters": [b"ACGT"] * 17}, {"adapters": [b"ACGT"], "adapters2": [b"AC"] * 17},
           {"adapters2": [b"ACGT"]}, {"min_overlap": 5}, {"max_err_pct": 20},
           {"trim_n": True, "min_overlap": 4}]
    for kw in bad:
        with pytest.raises(ValueError):
            Z.Trim(**kw)
    with pytest.raises(TypeError):
        Z.Trim(head=1.5)
    t = Z.Trim(head=np.int64(2), q3=93, adapters=["ACGT", b"A" * 128] * 8, adapters2="GGG",
               max_err_pct=100, min_overlap=1)
    assert t.head == 2 and len(t.adapters) == 16 and t.adapters2 == [b"GGG"]
    spec, ad = t.spec()
    assert list(spec.n_adapters) == [16, 1] and list(ad.len[:17]) == [4, 128] * 8 + [3]
    N, B, Q = Z.S.SEC_NAME, Z.S.SEC_SEQ, Z.S.SEC_QUAL
    assert Z.Trim().keys() == () and Z.Trim(head=1, tail=2, max_len=9).keys() == ()
    assert Z.Trim(trim_n=True).keys() == (B,) and Z.Trim(adapters=[b"ACG"], head=1).keys() == (B,)
    assert Z.Trim(q5=3).keys() == (B, Q) and Z.Trim(q3=3, trim_n=True).keys() == (B, Q)
    assert N not in Z.Trim(**ALL).keys()
    assert Z.Trim().spec()[0].set == 0


def test_steps_are_the_references():
    assert Z.TrimHits.STEPS == R.STEPS
