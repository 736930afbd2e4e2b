"""fqz5_names_match (name_match.hip) on synthetic name sections: which records
of a section (name [' ' comment] '\\0' per record, a device buffer) carry one
of the query names, compacted on the device.  No codec is involved.

Expected values come from a Python dict of the queries, looked up with each
record's key (the line up to the first ' ' or '\\t'; whole: the line)."""
import ctypes as C
import random
import re

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
ALPHA = b"ACGTNacgt0123456789.:_/-#@+=|"      # no ' ', '\t' or NUL


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _word(rng, lo: int, hi: int) -> bytes:
    return bytes(rng.choice(ALPHA) for _ in range(rng.randint(lo, hi)))


def _section(n: int, seed: int) -> list[bytes]:
    """n header lines: ids of 1..200 bytes; a quarter without a separator, the
    others with a comment after ' ' or '\\t'; one line empty, one with an
    empty name before its comment (where n leaves room)."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        ident = _word(rng, 1, 200)
        style = k % 4
        if style == 0:
            out.append(ident)
        elif style == 1:
            out.append(ident + b" " + _word(rng, 1, 30))
        elif style == 2:
            out.append(ident + b"\t" + _word(rng, 1, 30))
        else:
            out.append(ident + b" " + _word(rng, 1, 10) + b"\t" + _word(rng, 1, 10) + b" x")
    if n >= 2:
        out[n // 2] = b""
    if n >= 4:
        out[n // 2 + 1] = b" " + _word(rng, 5, 9)
    return out


def _key(line: bytes, whole: bool) -> bytes:
    return line if whole else re.split(b"[ \t]", line, maxsplit=1)[0]


def _expect(lines, queries, whole: bool, pairs: bool):
    """(record indices, query indices) by dict lookup."""
    want = {q: i for i, q in enumerate(queries)}
    assert len(want) == len(queries)
    hit = [want.get(_key(x, whole), NONE) for x in lines]
    n = len(lines)
    sel = [k for k in range(n)
           if hit[k] != NONE or (pairs and (k ^ 1) < n and hit[k ^ 1] != NONE)]
    return sel, [hit[k] for k in sel]


def _match(lines, queries, whole, pairs, tag_bits, pad: int = 0, nrec=None):
    """fqz5_names_match of the section: (rc, record indices, query indices).
    pad: the section starts that many bytes into its buffer."""
    so = Z._load()
    blob = b"".join(x + b"\0" for x in lines)
    n = len(lines) if nrec is None else nrec
    buf = torch.frombuffer(bytearray(b"\x01" * pad + blob + b"\x01" * 7), dtype=torch.uint8).cuda()
    out = torch.full((2, max(n, 1)), 0x55, dtype=torch.int32, device="cuda")
    cnt = C.c_uint64(12345)
    with Z._NameTable(queries, tag_bits) as tab:
        lib.after_torch()
        rc = so.fqz5_names_match(tab.p, buf.data_ptr() + pad, len(blob), n, int(whole), int(pairs),
                                 out[0].data_ptr(), out[1].data_ptr(), C.byref(cnt))
    if rc:
        return rc, None, None
    k = int(cnt.value)
    assert k <= n
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:, k:] == 0x55).all()                     # nothing written past the count
    return 0, got[0, :k].tolist(), got[1, :k].tolist()


def _both(lines, queries, whole, pairs, tag_bits, pad=0):
    exp = _expect(lines, queries, whole, pairs)
    rc, rec, qi = _match(lines, queries, whole, pairs, tag_bits, pad)
    assert rc == 0, lib.last_error()
    assert rec == sorted(rec) and len(set(rec)) == len(rec)
    assert (rec, qi) == exp
    return rec, qi


@pytest.mark.parametrize("tag_bits", [32, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_section_sizes_and_name_shapes(n, tag_bits):
    lines = _section(n, 100 + n)
    rng = random.Random(n)
    ids = [_key(x, False) for x in lines]
    queries = sorted({x for x in ids[::3] if x} | {ids[-1] or b"last"})
    absent = [_word(rng, 201, 230) for _ in range(5)]
    queries += absent
    rec, qi = _both(lines, queries, False, False, tag_bits, pad=n % 5)
    assert len(rec) >= (n + 2) // 3 - 2 and (n - 1 in rec or not ids[-1])
    assert not set(qi) & {queries.index(a) for a in absent}
    # pairs over the same section (129: an odd count, the last record has no mate)
    _both(lines, queries, False, True, tag_bits)


@pytest.mark.parametrize("tag_bits", [32, 1])
def test_negative_cases(tag_bits):
    """A query equal to a comment, a proper prefix of an id and an id plus
    one byte match nothing; with whole the full line matches and the bare id
    of a record with a comment does not."""
    rng = random.Random(5)
    lines = []
    for k in range(70):
        ident = b"read%d:" % k + _word(rng, 20, 40)
        lines.append(ident if k % 5 == 0 else ident + (b" " if k % 2 else b"\t") + _word(rng, 12, 20))
    ids = [_key(x, False) for x in lines]
    comment = lines[1][len(ids[1]) + 1:]
    neg = [comment, ids[2][:-1], ids[3] + b"A", ids[66][:-1], ids[67] + b"/1", lines[68]]
    assert lines[1] == ids[1] + b" " + comment and not set(neg) & set(ids)
    good = [ids[0], ids[1], ids[64], ids[69]]
    queries = neg + good
    rec, qi = _both(lines, queries, False, False, tag_bits)
    assert rec == [0, 1, 64, 69] and qi == [6, 7, 8, 9]
    # whole: the entire line is the key
    assert lines[0] == ids[0] and lines[6] != ids[6] and lines[11] != ids[11]
    queries = [lines[6], ids[11], lines[0], lines[64][:-1], comment]
    rec, qi = _both(lines, queries, True, False, tag_bits)
    assert rec == [0, 6] and qi == [2, 0]


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("tag_bits", [32, 1])
def test_staging_windows(tag_bits, whole):
    """A section of more than three staging windows, so keys straddle window
    edges; a key of two windows and three bytes that is a query, and one that
    differs from its query in the last byte."""
    win = Z._load().fqz5_names_match_window()
    rng = random.Random(9)
    lines = _section(300, 77)
    long_a = _word(rng, 2 * win + 3, 2 * win + 3)
    long_b = _word(rng, 2 * win + 3, 2 * win + 3)
    near_b = long_b[:-1] + (b"Y" if long_b[-1:] != b"Y" else b"Z")
    lines[70] = long_a
    lines[71] = near_b
    lines[130] = long_a if whole else long_a + b" again, with a comment"
    assert sum(len(x) + 1 for x in lines) > 3 * win + 2 * len(long_a)
    ids = [_key(x, whole) for x in lines]
    queries = sorted({x for x in ids[::2] if x}) + [long_b]
    assert long_a in queries and near_b not in queries
    rec, qi = _both(lines, queries, whole, False, tag_bits, pad=3)
    assert 70 in rec and 130 in rec and 71 not in rec
    assert queries.index(long_b) not in qi
    # the same bytes at a 16-byte aligned start
    _both(lines, queries, whole, False, tag_bits, pad=0)


@pytest.mark.parametrize("tag_bits", [32, 1])
def test_pairs(tag_bits):
    lines = [b"p%d/%d c" % (k // 2, 1 + k % 2) for k in range(7)]
    ids = [_key(x, False) for x in lines]
    # an odd record alone, both mates, and the last record of an odd-length section
    queries = [ids[6], ids[5], ids[3], ids[4]]
    rc, rec, qi = _match(lines, queries, False, True, tag_bits)
    assert rc == 0 and rec == [2, 3, 4, 5, 6] and qi == [NONE, 2, 3, 1, 0]
    assert (rec, qi) == _expect(lines, queries, False, True)
    rc, rec, qi = _match(lines, queries, False, False, tag_bits)
    assert rc == 0 and rec == [3, 4, 5, 6] and qi == [2, 3, 1, 0]
    # an even record alone takes its odd mate
    rc, rec, qi = _match(lines, [ids[0]], False, True, tag_bits)
    assert rc == 0 and rec == [0, 1] and qi == [0, NONE]


def test_limits():
    lines = [b"a 1", b"b", b"c 3"]
    rc, rec, qi = _match(lines, [b"b"], False, False, 32, nrec=0)
    assert rc == 0 and rec == [] and qi == []
    rc, _, _ = _match(lines, [b"b"], False, False, 32, nrec=4)
    assert rc == -1 and "fewer names" in lib.last_error()
    # no hit at all
    rc, rec, qi = _match(lines, [b"d", b"1", b"3"], False, False, 32)
    assert rc == 0 and rec == [] and qi == []
    # fewer records claimed than the section holds: the first ones are matched
    rc, rec, qi = _match(lines, [b"a", b"c"], False, False, 32, nrec=2)
    assert rc == 0 and rec == [0] and qi == [0]
