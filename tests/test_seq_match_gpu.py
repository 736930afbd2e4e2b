"""fqz5_seqs_match (seq_match.hip) on synthetic base arrays: which records of
a block's bases (the records' sequences one after the other, a device buffer)
hold one of the patterns, compacted on the device.  No codec is involved.

Expected values come from Python's `in` on each record's bytes (the lowest
pattern index that occurs in it; per pattern whether any record holds it);
fqz5_seqs_scan_host, the host restatement, must say the same."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
FORMS = [(32, 0), (32, 1), (1, 0), (1, 1)]             # (tag_bits, anchor)
forms = pytest.mark.parametrize("tag_bits,anchor", FORMS)


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def T():
    return int(Z._load().fqz5_seqs_match_tile())


def _bases(rng, n: int) -> bytearray:
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def _cut(blob: bytes, cuts) -> list[bytes]:
    """blob as records that end at `cuts` (ascending, repeats give empty ones)."""
    edges = [0] + list(cuts) + [len(blob)]
    return [bytes(blob[a:b]) for a, b in zip(edges, edges[1:])]


def _expect(records, queries, pairs: bool):
    hit = [next((i for i, q in enumerate(queries) if q in r), NONE) for r in records]
    n = len(records)
    sel = [k for k in range(n) if hit[k] != NONE or (pairs and (k ^ 1) < n and hit[k ^ 1] != NONE)]
    seen = [int(any(q in r for r in records)) for q in queries]
    return sel, [hit[k] for k in sel], seen


def _match(tab, records, nq, pairs=False, pad=0, seen=None, lens=None):
    """fqz5_seqs_match of the records: (rc, record indices, query indices,
    seen).  pad: the bases start that many bytes into their buffer."""
    so = Z._load()
    blob = b"".join(records)
    lens = np.asarray([len(r) for r in records] if lens is None else lens, np.uint32)
    n = len(lens)
    buf = torch.frombuffer(bytearray(b"\x01" * pad + blob + b"\x01" * 7), dtype=torch.uint8).cuda()
    out = torch.full((2, max(n, 1)), 0x55, dtype=torch.int32, device="cuda")
    if seen is None:
        seen = torch.zeros(nq + 3, dtype=torch.uint8, device="cuda")
        seen[nq:] = 0x55
    cnt = C.c_uint64(12345)
    lib.after_torch()
    rc = so.fqz5_seqs_match(tab.p, buf.data_ptr() + pad, len(blob), lens.ctypes.data, n, int(pairs),
                            out[0].data_ptr(), out[1].data_ptr(), C.byref(cnt), seen.data_ptr())
    if rc:
        return rc, None, None, None
    k = int(cnt.value)
    assert k <= n
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:, k:] == 0x55).all()                             # nothing written past the count
    sn = seen.cpu().numpy()
    assert (sn[nq:] == 0x55).all() and set(sn[:nq].tolist()) <= {0, 1}
    return 0, got[0, :k].tolist(), got[1, :k].tolist(), sn[:nq].tolist()


def _both(records, queries, tag_bits, anchor, pairs=False, pad=0):
    """The GPU against the rule and against the host restatement."""
    exp = _expect(records, queries, pairs)
    with Z._SeqTable(queries, tag_bits, anchor) as tab:
        rc, rec, qi, seen = _match(tab, records, len(queries), pairs, pad)
        assert rc == 0, lib.last_error()
        hh, hs = tab.scan_host(b"".join(records), [len(r) for r in records], len(queries))
    assert rec == sorted(rec) and len(set(rec)) == len(rec)
    assert (rec, qi, seen) == exp
    assert [hh[r] for r in rec] == qi and hs.tolist() == seen
    if not pairs:
        assert [r for r in range(len(records)) if hh[r] != NONE] == rec
    return rec, qi, seen


PATS = [b"GATTACAGATTACAGG", b"TTGACAGCTAGCTCAGTCCT", b"CCCCCCCCCCCCAAAA", b"GATTACAGATTACAGC"]


@forms
@pytest.mark.parametrize("pad", [0, 3])
def test_total_sizes(T, tag_bits, anchor, pad):
    """Arrays of 1, m - 1, m, T - 1, T, T + 1 and 3T + 5 bases in a handful of
    records, a pattern planted at the very start and the very end."""
    m = anchor or 12
    rng = random.Random(17 * pad + tag_bits + anchor)
    for total in (1, m - 1, m, T - 1, T, T + 1, 3 * T + 5):
        blob = _bases(rng, total)
        if total >= 40:
            blob[:16] = PATS[0]
            blob[-20:] = PATS[1]
        elif total == 12:
            blob[:] = b"ACGTTGCATGCA"
        cuts = sorted(rng.randrange(total) for _ in range(4)) if total else [0, 0]
        cuts = [c for c in cuts if not 0 < c < 16 and not total - 20 < c < total] + [total]
        records = _cut(blob, cuts)                         # (the last record is empty)
        queries = PATS + [b"ACGTTGCATGCA", b"ACGTTGCATGCAA"]
        rec, qi, seen = _both(records, queries, tag_bits, anchor, pad=pad)
        if total >= 40:
            assert 0 in qi and seen[0] == seen[1] == 1 and len(records) - 2 in rec
        if total == 12:
            assert qi == [4] and seen == [0, 0, 0, 0, 1, 0]
        # the whole array as one record
        _both([bytes(blob)], queries, tag_bits, anchor, pad=pad)


@forms
@pytest.mark.parametrize("pad", [0, 3])
def test_occurrences_across_tile_edges(T, tag_bits, anchor, pad):
    """One record of 3T + 5 bases; an occurrence starting at T - m, T - 1, T
    and 2T - ceil(len / 2), so the anchor and the pattern straddle an edge."""
    m = anchor or 12
    rng = random.Random(23)
    base = _bases(rng, 3 * T + 5)
    for p in PATS:
        assert p not in base
    for k, at in enumerate((T - m, T - 1, T, 2 * T - (len(PATS[1]) + 1) // 2)):
        blob = bytearray(base)
        blob[at:at + len(PATS[1])] = PATS[1]
        rec, qi, seen = _both([bytes(blob)], PATS, tag_bits, anchor, pad=pad)
        assert (rec, qi, seen) == ([0], [1], [0, 1, 0, 0]), at
        # a record ends where the occurrence starts: it lies in the second
        rec, qi, _ = _both(_cut(blob, [at]), PATS, tag_bits, anchor, pad=pad)
        assert (rec, qi) == ([1], [1]), at
        # ... and one ends inside it: it lies in neither
        rec, qi, seen = _both(_cut(blob, [at + 9]), PATS, tag_bits, anchor, pad=pad)
        assert (rec, seen) == ([], [0, 0, 0, 0]), at


@forms
def test_pattern_longer_than_a_tile(T, tag_bits, anchor):
    rng = random.Random(29)
    long = bytes(_bases(rng, T + 7))
    alts = [c for c in b"ACGT" if c != long[-1]]
    near, other = long[:-1] + bytes(alts[:1]), long[:-1] + bytes(alts[1:2])
    assert len({long, near, other}) == 3
    records = [bytes(_bases(rng, 50)), bytes(_bases(rng, 33)) + long + bytes(_bases(rng, 30)),
               near, bytes(_bases(rng, T - 100)), long[1:], long[:-1]]
    assert sum(len(r) for r in records) > 3 * T
    for pad in (0, 3):
        rec, qi, seen = _both(records, [other, long], tag_bits, anchor, pad=pad)
        assert (rec, qi, seen) == ([1], [1], [0, 1])
    rec, qi, seen = _both(records, [near, long], tag_bits, anchor)
    assert (rec, qi, seen) == ([1, 2], [1, 0], [1, 1])


@forms
@pytest.mark.parametrize("pad", [0, 3])
def test_four_hundred_short_records(tag_bits, anchor, pad):
    """400 records of 0..40 bases (about a quarter of them empty) and patterns
    of 8..20 bases cut from them, with others that occur nowhere."""
    rng = random.Random(31)
    records = [bytes(_bases(rng, rng.randint(1, 40) if rng.randrange(4) else 0)) for _ in range(400)]
    records[0] = records[399] = records[200] = b""
    pats = set()
    for r in rng.sample([r for r in records if len(r) >= 20], 40):
        n = rng.randint(8, 20)
        at = rng.randint(0, len(r) - n)
        pats.add(r[at:at + n])
    while len(pats) < 60:
        pats.add(bytes(_bases(rng, rng.randint(12, 24))))
    pats = sorted(pats)
    rng.shuffle(pats)
    rec, qi, seen = _both(records, pats, tag_bits, anchor, pad=pad)
    assert 40 <= len(rec) < 300 and 30 <= sum(seen) < 60
    _both(records, pats, tag_bits, anchor, pairs=True, pad=pad)


@forms
def test_never_across_two_records(T, tag_bits, anchor):
    p = PATS[1]
    rng = random.Random(37)
    for edge in (300, T, 2 * T - 3):          # the boundary within a tile, on an edge and by one
        for cut in (1, 9, len(p) - 1):
            blob = _bases(rng, 2 * T + 50)
            blob[edge - cut:edge - cut + len(p)] = p
            records = _cut(blob, [edge])
            assert p in blob and p not in records[0] and p not in records[1]
            rec, qi, seen = _both(records, [p], tag_bits, anchor)
            assert (rec, seen) == ([], [0])
            # with empty records at the boundary as well
            rec, qi, seen = _both(_cut(blob, [edge, edge, edge]), [p], tag_bits, anchor)
            assert (rec, seen) == ([], [0])


@forms
def test_pairs_on_an_odd_count(tag_bits, anchor):
    f = lambda k: b"TTTTTTTTTTTTTTT" + PATS[k] + b"TTT"
    plain = b"TTTTTTTTTTTTTTTTTTTTTTTTTTT"
    # record 3 alone of its pair, both mates of (4, 5), the last record without a mate
    records = [plain, plain, plain, f(2), f(3), f(1), f(0)]
    with Z._SeqTable(PATS, tag_bits, anchor) as tab:
        rc, rec, qi, _ = _match(tab, records, 4, pairs=True)
        assert rc == 0 and rec == [2, 3, 4, 5, 6] and qi == [NONE, 2, 3, 1, 0]
        rc, rec, qi, _ = _match(tab, records, 4, pairs=False)
        assert rc == 0 and rec == [3, 4, 5, 6] and qi == [2, 3, 1, 0]
        # an even record alone takes its odd mate
        rc, rec, qi, _ = _match(tab, [f(0), plain, plain], 4, pairs=True)
        assert rc == 0 and rec == [0, 1] and qi == [0, NONE]
    _both(records, PATS, tag_bits, anchor, pairs=True)


def test_seen_accumulates_over_calls():
    """d_seen is OR-ed: two calls into one buffer; a pattern that occurs only
    behind a lower one is seen as well."""
    seen = torch.zeros(7, dtype=torch.uint8, device="cuda")
    seen[4:] = 0x55
    with Z._SeqTable(PATS) as tab:
        rc, rec, qi, sn = _match(tab, [b"AA" + PATS[2] + b"AA", b"ACGT" * 9], 4, seen=seen)
        assert (rc, rec, qi, sn) == (0, [0], [2], [0, 0, 1, 0])
        rc, rec, qi, sn = _match(tab, [b"", PATS[3] + b"C" + PATS[0], b"ACGT" * 9], 4, seen=seen)
        assert (rc, rec, qi, sn) == (0, [1], [0], [1, 0, 1, 1])
        rc, rec, qi, sn = _match(tab, [b"ACGT" * 9], 4, seen=seen)
        assert (rc, rec, qi, sn) == (0, [], [], [1, 0, 1, 1])


def test_limits():
    with Z._SeqTable(PATS) as tab:
        rc, rec, qi, sn = _match(tab, [], 4)
        assert (rc, rec, qi, sn) == (0, [], [], [0, 0, 0, 0])
        records = [PATS[0], b"ACGT", PATS[1]]
        for lens in ([16, 4, 19], [16, 4, 21], [16, 4], []):
            rc, _, _, _ = _match(tab, records, 4, lens=lens)
            assert rc == -1 and "do not sum" in lib.last_error()
        # fewer bases than the anchor: nothing can match, nothing is launched
        rc, rec, qi, sn = _match(tab, [b"GATT", b"ACA"], 4)
        assert (rc, rec, qi, sn) == (0, [], [], [0, 0, 0, 0])
        rc, rec, qi, sn = _match(tab, records, 4)
        assert (rc, rec, qi, sn) == (0, [0, 2], [0, 1], [1, 1, 0, 0])
