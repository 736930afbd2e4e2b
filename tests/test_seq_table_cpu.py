"""The host side of lookup by sequence content: the pattern table and the
host restatement of the kernel's rule (fqz5_seqs_table_build /
fqz5_seqs_scan_host, seq_match.hip), the pattern list reader and the mapping
from the caller's patterns to internal queries and back
(fqz5file.read_pattern_list, _seq_queries, _seq_hits).  No GPU.

Expected values come from Python's `in` on the records' bytes: per record
the lowest i with queries[i] in it, per query whether any record holds it."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

NONE = 0xFFFFFFFF
FORMS = [(32, 0), (32, 1), (1, 0), (1, 1)]             # (tag_bits, anchor)
forms = pytest.mark.parametrize("tag_bits,anchor", FORMS)


def _rule(records, queries):
    hit = [next((i for i, q in enumerate(queries) if q in r), NONE) for r in records]
    seen = [int(any(q in r for r in records)) for q in queries]
    return hit, seen


def _scan(records, queries, tag_bits, anchor):
    """scan_host against the rule; returns (hit, seen)."""
    with Z._SeqTable(queries, tag_bits, anchor) as tab:
        assert tab.anchor == (anchor or min(12, min(len(q) for q in queries)))
        hit, seen = tab.scan_host(b"".join(records), [len(r) for r in records], len(queries))
    assert (hit.tolist(), seen.tolist()) == _rule(records, queries)
    return hit.tolist(), seen.tolist()


@forms
def test_one_pattern_start_end_whole(tag_bits, anchor):
    p = b"GATTACAGATTACA"
    records = [p + b"CCCCCC", b"CCCCCC" + p, p, b"CCCC" + p[:-1], p[1:] + b"CCCC", b"CC" + p + b"CC"]
    hit, seen = _scan(records, [p], tag_bits, anchor)
    assert hit == [0, 0, 0, NONE, NONE, 0] and seen == [1]


@forms
def test_never_across_two_records(tag_bits, anchor):
    p = b"ACGTTGCAAC"
    for cut in range(1, len(p)):
        records = [b"TTTT" + p[:cut], p[cut:] + b"GGGG"]
        assert p in b"".join(records)
        hit, seen = _scan(records, [p], tag_bits, anchor)
        assert hit == [NONE, NONE] and seen == [0]


@forms
def test_pattern_longer_than_every_record(tag_bits, anchor):
    records = [b"ACGTACGT", b"ACGTACGTAC", b"ACGT"]
    long = b"ACGTACGTACG"
    hit, seen = _scan(records, [long, b"GTAC"], tag_bits, anchor)
    assert hit == [1, 1, NONE] and seen == [0, 1]
    hit, seen = _scan(records, [long], tag_bits, anchor)
    assert hit == [NONE] * 3 and seen == [0]


@forms
def test_overlapping_occurrences(tag_bits, anchor):
    hit, seen = _scan([b"AAAAAA", b"AAA", b"AAAA", b"CAAAAC"], [b"AAAA"], tag_bits, anchor)
    assert hit == [0, NONE, 0, 0] and seen == [1]


@forms
def test_zero_length_records(tag_bits, anchor):
    p = b"TTGACA"
    records = [b"", b"", p, b"", b"GG" + p, b"", b"", p + b"GG", b"GGGG", b""]
    hit, seen = _scan(records, [p], tag_bits, anchor)
    assert hit == [NONE, NONE, 0, NONE, 0, NONE, NONE, 0, NONE, NONE]
    hit, _ = _scan([b"", b""], [p], tag_bits, anchor)
    assert hit == [NONE, NONE]


@forms
def test_shared_anchor_and_prefixes(tag_bits, anchor):
    a, c, g = b"ACGTACGTACGTA", b"ACGTACGTACGTC", b"ACGTACGTACGTG"
    records = [b"TT" + c + b"TT", b"TT" + a, g, b"ACGTACGTACGTT", a + c, c + a]
    hit, seen = _scan(records, [a, c, g], tag_bits, anchor)
    assert hit == [1, 0, 2, NONE, 0, 0] and seen == [1, 1, 1]
    # the later pattern first in the table's probe order as well
    hit, seen = _scan(records, [g, c, a], tag_bits, anchor)
    assert hit == [1, 2, 0, NONE, 1, 1]
    # one pattern a prefix of another: the longer listed first, and second
    short, long = b"GATTACA", b"GATTACAGATT"
    records = [b"C" + long + b"C", b"C" + short + b"C", b"GATTAC", long[:-1]]
    hit, seen = _scan(records, [long, short], tag_bits, anchor)
    assert hit == [0, 1, NONE, 1] and seen == [1, 1]
    hit, seen = _scan(records, [short, long], tag_bits, anchor)
    assert hit == [0, 0, NONE, 0] and seen == [1, 1]


@forms
def test_case_and_n_are_bytes(tag_bits, anchor):
    records = [b"TTACGTTT", b"TTacgtTT", b"TTACNTTT", b"TTAcGTTT"]
    hit, seen = _scan(records, [b"acgt", b"ACGT", b"ACNT", b"ANNT"], tag_bits, anchor)
    assert hit == [1, 0, 2, NONE] and seen == [1, 1, 1, 0]


@forms
def test_thousand_random_patterns(tag_bits, anchor):
    rng = random.Random(11)
    pats = set()
    while len(pats) < 1000:
        pats.add(bytes(rng.choice(b"ACGT") for _ in range(rng.randint(8, 40))))
    pats = sorted(pats)
    rng.shuffle(pats)
    records = [bytearray(rng.choice(b"ACGT") for _ in range(rng.randint(0, 120)))
               for _ in range(300)]
    for r in rng.sample(range(300), 200):                  # one planted occurrence each
        p = pats[rng.randrange(1000)]
        at = rng.randint(0, 60)
        records[r][at:at + len(p)] = p
    records = [bytes(r) for r in records]
    hit, seen = _scan(records, pats, tag_bits, anchor)
    assert sum(h != NONE for h in hit) >= 150 and sum(h == NONE for h in hit) >= 50
    assert 100 <= sum(seen) < 1000


@forms
def test_seen_behind_a_lower_pattern(tag_bits, anchor):
    """Pattern 1 occurs only in records that also hold pattern 0: no record
    reports it, yet it was seen; pattern 2 occurs nowhere."""
    p0, p1, p2 = b"AACCGGTT", b"TGCATGCA", b"GGGGCCCC"
    records = [p1 + b"A" + p0, b"CCCC", p0 + p1, p0]
    hit, seen = _scan(records, [p0, p1, p2], tag_bits, anchor)
    assert hit == [0, NONE, 0, 0] and seen == [1, 1, 0]
    given, qs, origin = Z._seq_queries([p0, p1, p2], False)
    h = Z._seq_hits(given, qs, origin, False, [0, 2, 3], [0, 0, 0], seen)
    assert h.missing == [p2] and h.query.tolist() == [0, 0, 0]


def test_refusals():
    for bad, what in (([b"AC", b"", b"GT"], "pattern 1 is empty"),
                      ([b"AC", b"GT", b"ACG", b"GT", b"AC"], "pattern 3 is a duplicate of pattern 1")):
        with pytest.raises(lib.NativeError, match=what):
            Z._SeqTable(bad)
    for bits in (0, 33):
        with pytest.raises(lib.NativeError, match="tag_bits"):
            Z._SeqTable([b"ACGT"], bits)
    with pytest.raises(lib.NativeError, match="anchor is longer than the shortest"):
        Z._SeqTable([b"ACGTACGT", b"ACG"], 32, 4)
    with Z._SeqTable([b"ACGTACGT", b"ACG"], 32, 3) as tab:
        assert tab.anchor == 3
    with Z._SeqTable([b"ACGTACGTACGTACGT", b"ACGTACGTACGTAAAA"]) as tab:
        assert tab.anchor == 12
    so = Z._load()
    assert not so.fqz5_seqs_table_build(b"", 0, 0, 32, 0) and "no pattern" in lib.last_error()
    assert not so.fqz5_seqs_table_build(b"a\0b", 3, 2, 32, 0) and "fewer terminated" in lib.last_error()
    long = b"A" * 65536 + b"\0"
    assert not so.fqz5_seqs_table_build(long, len(long), 1, 32, 0) and "longer than" in lib.last_error()
    tab = so.fqz5_seqs_table_build(long[1:], len(long) - 1, 1, 32, 0)       # 65535: taken
    assert tab and so.fqz5_seqs_table_anchor(tab) == 12
    so.fqz5_seqs_table_free(tab)
    assert so.fqz5_seqs_match_tile() >= 64
    # lens that do not sum to the bases
    with Z._SeqTable([b"ACGT"]) as tab:
        for lens in ([4, 3], [4, 5], []):
            with pytest.raises(lib.NativeError, match="do not sum"):
                tab.scan_host(b"ACGTACGT", lens, 1)
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="pattern 1 is empty"):
        Z.find_seqs(b"not a container", [b"ACGT", b""])
    with pytest.raises(ValueError, match="pattern 0 holds a NUL"):
        Z.find_seqs(b"not a container", [b"AC\0GT"])
    for bad in (b"ACGU", b"ACRT", b"AC-T", "ACGT "):
        with pytest.raises(ValueError, match="pattern 1 holds a byte without a complement"):
            Z.find_seqs(b"not a container", [b"ACGT", bad], revcomp=True)


def _rc(b: bytes) -> bytes:
    return bytes({65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97, 78: 78,
                  110: 110}[c] for c in reversed(b))


def test_revcomp_expansion_and_back():
    assert _rc(b"AACGNn") == b"nNCGTT" and _rc(b"acgt") == b"acgt"
    # a palindrome has no rc of its own; pattern 2 is the rc of pattern 1
    pats = [b"ACGT", "AAC", b"GTT", b"AAC", b"CCNa"]
    given, qs, origin = Z._seq_queries(pats, True)
    assert given == pats
    assert qs == [b"ACGT", b"AAC", b"GTT", b"CCNa", b"tNGG"]
    assert origin == [(0, False), (1, False), (1, True), (4, False), (4, True)]
    assert Z._seq_queries(pats, False)[1:] == ([b"ACGT", b"AAC", b"GTT", b"CCNa"],
                                               [(0, False), (1, False), (2, False), (4, False)])
    # records 5, 6 (a mate), 9 and 12 hold queries 2 (rc of "AAC"), none, 4 and 0
    seen = [1, 0, 1, 0, 1]
    h = Z._seq_hits(given, qs, origin, True, [5, 6, 9, 12], [2, NONE, 4, 0], seen)
    assert h.records.dtype == np.uint64 and h.records.tolist() == [5, 6, 9, 12]
    assert h.query.dtype == np.int64 and h.query.tolist() == [1, -1, 4, 0]
    assert h.reverse.dtype == bool and h.reverse.tolist() == [True, False, True, False]
    assert h.missing == []                   # "GTT" was seen, as the rc of "AAC" and itself
    h = Z._seq_hits(given, qs, origin, True, [], [], [0, 0, 0, 0, 0])
    assert h.missing == [b"ACGT", "AAC", b"GTT", b"CCNa"] and h.records.tolist() == []
    h = Z._seq_hits(given, qs, origin, True, [3], [3], [0, 0, 0, 1, 0])
    assert h.missing == [b"ACGT", "AAC", b"GTT"] and h.reverse.tolist() == [False]
    assert Z._seq_queries([], True) == ([], [], [])


def test_read_pattern_list(tmp_path):
    p = tmp_path / "patterns.txt"
    p.write_bytes(b"ACGT\r\n\r\nGATTACA\r\n\nacgtn\nTTTT")
    assert Z.read_pattern_list(str(p)) == [b"ACGT", b"GATTACA", b"acgtn", b"TTTT"]
    p.write_bytes(b">adapter 1\r\nAGATCGGAAG\r\nAGCACACGTC\r\n\r\n>primer\r\nGATTACA\r\n"
                  b">empty\r\n>last\nTT\n")
    assert Z.read_pattern_list(str(p)) == [b"AGATCGGAAGAGCACACGTC", b"GATTACA", b"TT"]
    p.write_bytes(b"")
    assert Z.read_pattern_list(str(p)) == []


def test_empty_list_touches_nothing():
    """An empty list returns before the file or the GPU is looked at."""
    for rc in (False, True):
        h = Z.find_seqs(b"not a container", [], revcomp=rc)
        assert h.records.tolist() == [] and h.query.tolist() == [] and h.reverse.tolist() == []
        assert h.missing == [] and h.written == 0
    assert Z.extract_seqs_bytes(b"not a container", []) == b""
