"""The host side of lookup by read name: the query table
(fqz5_names_table_build / _find, name_match.hip), the name list reader and
the mapping from the caller's names to distinct queries and back
(fqz5file.read_name_list, _queries, _name_hits).  No GPU: the table is built
and probed on the host with the hash the kernel uses.

Expected values come from a Python dict of the queries."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

TAG_BITS = (32, 1)


def _random_names(n: int, seed: int) -> list[bytes]:
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(bytes(rng.choice(b"ACGT0123456789.:_/") for _ in range(rng.randint(1, 40))))
    return sorted(out)


def _check(queries: list[bytes], absent: list[bytes], tag_bits: int) -> None:
    want = {q: i for i, q in enumerate(queries)}
    assert not set(absent) & set(want)
    with Z._NameTable(queries, tag_bits) as tab:
        for q, i in want.items():
            assert tab.find(q) == i, (q, tag_bits)
        for k in absent:
            assert tab.find(k) == want.get(k, -1) == -1, (k, tag_bits)
        assert tab.find(b"") == -1


@pytest.mark.parametrize("tag_bits", TAG_BITS)
def test_one_query(tag_bits):
    _check([b"SRR1.1"], [b"SRR1.2", b"SRR1.", b"SRR1.11", b"S"], tag_bits)


@pytest.mark.parametrize("tag_bits", TAG_BITS)
def test_thousand_random_queries(tag_bits):
    names = _random_names(1500, 7)
    _check(names[:1000], names[1000:], tag_bits)


@pytest.mark.parametrize("tag_bits", TAG_BITS)
def test_prefixes_and_last_byte(tag_bits):
    # one query a prefix of another; queries that differ in their last byte only
    _check([b"read1", b"read10", b"read100", b"lane:7:A", b"lane:7:B", b"lane:7:C"],
           [b"read", b"read11", b"read1000", b"lane:7:", b"lane:7:D", b"lane:7:AA"], tag_bits)


def test_long_query():
    long = bytes(65 + k % 26 for k in range(20000))
    _check([long, long[:-1] + b"!"], [long[:-1], long + b"A"], 32)


@pytest.mark.parametrize("tag_bits", TAG_BITS)
def test_empty_and_duplicate_refused(tag_bits):
    with pytest.raises(lib.NativeError, match="query 1 is empty"):
        Z._NameTable([b"a", b"", b"b"], tag_bits)
    with pytest.raises(lib.NativeError, match="query 2 is a duplicate of query 0"):
        Z._NameTable([b"a", b"b", b"a"], tag_bits)
    so = Z._load()
    # the terminators are the builder's to find: fewer than nq, bytes after the last
    assert not so.fqz5_names_table_build(b"a\0b", 3, 2, 32) and "fewer terminated" in lib.last_error()
    assert not so.fqz5_names_table_build(b"a\0b\0c", 5, 2, 32) and "after the last" in lib.last_error()
    for bits in (0, 33):
        assert not so.fqz5_names_table_build(b"a\0", 2, 1, bits) and "tag_bits" in lib.last_error()
    assert so.fqz5_names_match_window() >= 64


def test_read_name_list(tmp_path):
    p = tmp_path / "names.txt"
    p.write_bytes(b"r1\r\n\r\n@r2 with comment\r\n\n  padded \nlast")
    assert Z.read_name_list(str(p)) == [b"r1", b"@r2 with comment", b"  padded ", b"last"]
    p.write_bytes(b"")
    assert Z.read_name_list(str(p)) == []


def test_names_to_queries_and_back():
    names = [b"b", "a", b"b", b"zz", "a", b"c"]
    given, qs, first = Z._queries(names)
    assert given == names and qs == [b"b", b"a", b"zz", b"c"] and first == [0, 1, 3, 5]
    # records 10, 11 (a mate), 40 and 41 carry queries 1 ("a"), none, 3 ("c") and 1
    h = Z._name_hits(given, first, [10, 11, 40, 41], [1, 0xFFFFFFFF, 3, 1])
    assert h.records.dtype == np.uint64 and h.records.tolist() == [10, 11, 40, 41]
    assert h.query.dtype == np.int64 and h.query.tolist() == [1, -1, 5, 1]
    assert h.missing == [b"b", b"zz"]
    h = Z._name_hits(given, first, [], [])
    assert h.records.tolist() == [] and h.query.tolist() == [] and h.missing == [b"b", "a", b"zz", b"c"]
    for bad in ([b"x", b""], ["", "y"]):
        with pytest.raises(ValueError, match="empty"):
            Z._queries(bad)
    assert Z._queries([]) == ([], [], [])


def test_empty_names_touch_nothing(tmp_path):
    """An empty list returns before the file or the GPU is looked at."""
    h = Z.find_names(b"not a container", [])
    assert h.records.tolist() == [] and h.query.tolist() == [] and h.missing == []
    assert Z.extract_names_bytes(b"not a container", []) == b""
