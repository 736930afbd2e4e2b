"""The query tables of lookup by read name and by sequence content
(fqz5_names_table_build, fqz5_seqs_table_build): every refusal of a builder
with its exact message, the anchor rule, fqz5_names_table_find and
fqz5_seqs_scan_host on patterns that share an anchor.  The builders and the
host probes never touch the GPU."""
import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

NONE = 0xFFFFFFFF
TABLES = [("names", "query", "queries"), ("seqs", "pattern", "patterns")]


def _blob(queries):
    return b"".join(q + b"\0" for q in queries)


def _build(kind, blob, nq, tag_bits=32, anchor=0):
    """The table's handle (freed here) as a truth value, or the error's text."""
    so = Z._load()
    extra = (anchor,) if kind == "seqs" else ()
    p = getattr(so, f"fqz5_{kind}_table_build")(blob, len(blob), nq, tag_bits, *extra)
    if not p:
        return lib.last_error()
    getattr(so, f"fqz5_{kind}_table_free")(p)
    return True


@pytest.mark.parametrize("kind,noun,nouns", TABLES)
def test_refusals_of_both_builders(kind, noun, nouns):
    who = f"{kind}_table_build"
    good = [b"ACGTACGTACGTA", b"TTTTGGGGCCCCAAAA"]
    assert _build(kind, _blob(good), 2) is True
    assert _build(kind, _blob(good), 2, tag_bits=1) is True
    for bits in (0, 33):
        assert _build(kind, _blob(good), 2, tag_bits=bits) == f"{who}: tag_bits not in 1..32"
    assert _build(kind, _blob(good)[:-1], 2) == f"{who}: fewer terminated {nouns} than nq"
    assert _build(kind, _blob(good), 3) == f"{who}: fewer terminated {nouns} than nq"
    assert _build(kind, _blob(good) + b"A", 2) == f"{who}: bytes after the last {noun}"
    assert _build(kind, _blob(good), 1) == f"{who}: bytes after the last {noun}"
    assert _build(kind, _blob([b""] + good), 3) == f"{who}: {noun} 0 is empty"
    assert _build(kind, _blob(good + [b"", b"GATTACA"]), 4) == f"{who}: {noun} 2 is empty"


@pytest.mark.parametrize("kind,noun,nouns", TABLES)
def test_a_duplicate_names_the_lowest_repeat_and_the_first_copy(kind, noun, nouns):
    who = f"{kind}_table_build"
    A, B = b"ACGTACGTACGTAA", b"ACGTACGTACGTAC"                   # (one anchor for both)
    assert _build(kind, _blob([A, B, A, B, A]), 5) == f"{who}: {noun} 2 is a duplicate of {noun} 0"
    assert _build(kind, _blob([B, A, A, B]), 4) == f"{who}: {noun} 2 is a duplicate of {noun} 1"
    assert _build(kind, _blob([A, A]), 2, tag_bits=1) == f"{who}: {noun} 1 is a duplicate of {noun} 0"
    # a prefix is no duplicate
    assert _build(kind, _blob([A, A + b"C", A[:-1]]), 3) is True


def test_seqs_duplicate_behind_a_longer_pattern_of_its_anchor():
    P = b"ACGTACGTACGTAA"
    for anchor in (0, 1, 14):
        assert _build("seqs", _blob([P, P + b"CCCC", P]), 3, anchor=anchor) == \
            "seqs_table_build: pattern 2 is a duplicate of pattern 0"
    assert _build("seqs", _blob([b"T" + P, P, P + b"CCCC", P + b"CCCG", P]), 5) == \
        "seqs_table_build: pattern 4 is a duplicate of pattern 1"
    assert _build("seqs", _blob([P, P + b"CCCC", P + b"CCCG"]), 3) is True


def test_seqs_only_refusals():
    who = "seqs_table_build"
    P = b"ACGTACGTACGTAA"
    assert _build("seqs", b"", 0) == f"{who}: no pattern"
    assert _build("names", b"", 0) is True
    for anchor in (-1, 65):
        assert _build("seqs", _blob([P]), 1, anchor=anchor) == f"{who}: anchor not in 0..64"
    assert _build("seqs", _blob([P, P[:5]]), 2, anchor=6) == \
        f"{who}: the anchor is longer than the shortest pattern"
    assert _build("seqs", _blob([P, P[:5]]), 2, anchor=5) is True
    assert _build("seqs", _blob([b"A" * 64]), 1, anchor=64) is True
    assert _build("seqs", _blob([P, b"C" * 65535]), 2) is True
    assert _build("seqs", _blob([P, b"C" * 65536]), 2) == \
        f"{who}: pattern 1 is longer than 65535 bytes"
    assert _build("names", _blob([P, b"C" * 65536]), 2) is True


@pytest.mark.parametrize("shortest,anchor", [(1, 1), (11, 11), (12, 12), (13, 12)])
def test_the_default_anchor(shortest, anchor):
    with Z._SeqTable([b"ACGT" * 5, b"G" * shortest, b"T" * 40]) as T:
        assert T.anchor == anchor
    with Z._SeqTable([b"ACGT" * 5, b"G" * shortest], anchor=1) as T:
        assert T.anchor == 1


@pytest.mark.parametrize("tag_bits", [32, 8, 1])
def test_names_table_find(tag_bits):
    names = [b"read1", b"read10", b"r", b"another/2"] + [b"n%d" % k for k in range(200)]
    with Z._NameTable(names, tag_bits) as T:
        for k, n in enumerate(names):
            assert T.find(n) == k
        for absent in (b"read", b"read12", b"read1 ", b"", b"R", b"another/", b"n200", b"n"):
            assert T.find(absent) == -1, absent
    with Z._NameTable([]) as T:
        assert T.find(b"read1") == -1


@pytest.mark.parametrize("tag_bits", [32, 1])
def test_scan_host_with_three_patterns_of_one_anchor(tag_bits):
    anchor = b"ACGTACGTACGT"
    X, Y, Zp = anchor + b"AA", anchor + b"AAC", anchor + b"GG"
    # X ends record 1 and Y would run into record 2; record 3 holds Y, so X too
    records = [b"TTTTTTTTTTTTTTTT", b"TT" + X, b"CGGTTTTT", b"", b"G" + Y + b"T", anchor + b"G"]
    with Z._SeqTable([Zp, Y, X], tag_bits) as T:
        assert T.anchor == 12
        hit, seen = T.scan_host(b"".join(records), [len(r) for r in records], 3)
    assert hit.tolist() == [NONE, 2, NONE, NONE, 1, NONE]
    assert seen.tolist() == [0, 1, 1]
    with Z._SeqTable([X, Y, Zp], tag_bits) as T:
        hit, seen = T.scan_host(b"".join(records), [len(r) for r in records], 3)
    assert hit.tolist() == [NONE, 0, NONE, NONE, 0, NONE]
    assert seen.tolist() == [1, 1, 0]
    assert hit.dtype == np.uint32
