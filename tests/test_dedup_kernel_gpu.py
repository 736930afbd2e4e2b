"""The duplicates kernels (dedup.hip) on synthetic device arrays: the unit keys
of a block's bases, the wait-free insert into the device table, the pick with
its compaction, and the levels.  No codec is involved.

Expected values come from the host entry points (fqz5_dedup_keys_host and the
host table) and, independently, from the rule in plain Python (dedup_ref).
The bases are a view into a larger buffer whose guard bytes would change a key
if they were read.  Guard words surround every output."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import dedup_ref as R

pytestmark = pytest.mark.gpu
GUARD = 0x55555555
GUARD64 = 0x5555555555555555
PAD = 48                                                    # guard bytes on both sides
KCAP = 2048                                                 # record_tile.hpp's ST_KCAP
M = R.M
MODES = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def T():
    t = int(Z._load().fqz5_filter_tile())
    assert t == 4096
    return t


def _seqs(rng, lens, alphabet=b"ACGTNacgt"):
    return [bytes(rng.choice(alphabet) for _ in range(n)) for n in lens]


def _cut(total: int, cuts) -> list[int]:
    edges = [0] + sorted(cuts) + [total]
    return [b - a for a, b in zip(edges, edges[1:])]


def _dev(blob: bytes, mis: int, guard: bytes = b"NG"):
    """The blob `mis` bytes past a 16-byte address, guard bytes around it:
    (the tensor, the blob's address)."""
    left = (guard * (PAD + 16))[:PAD + mis]
    t = torch.frombuffer(bytearray(left + blob + (guard * PAD)[:PAD]), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + PAD + mis


def _guarded(n: int, dtype):
    """n + 2 guard words on the device: (the tensor, the address of word 1)."""
    t = torch.full((n + 2,), GUARD64 if dtype == torch.int64 else GUARD, dtype=dtype, device="cuda")
    return t, t.data_ptr() + t.element_size()


def _back(t):
    a = t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint32)
    g = GUARD64 if t.dtype == torch.int64 else GUARD
    assert a[0] == g and a[-1] == g
    return a[1:-1]


def _keys(seqs, pairs=False, rc=False, mis=0, lens=None):
    """fqz5_dedup_keys: (rc, the keys as (lo, hi) tuples)."""
    so = Z._load()
    lens = np.asarray([len(s) for s in seqs] if lens is None else lens, np.uint32)
    units = len(lens) // (2 if pairs else 1)
    blob = b"".join(seqs)
    st, sp = _dev(blob, mis)
    kt, kp = _guarded(2 * units, torch.int64)
    lib.after_torch()
    ret = so.fqz5_dedup_keys(sp, len(blob), lens.ctypes.data, len(lens), int(pairs), int(rc), kp)
    torch.cuda.synchronize()
    k = _back(kt)
    if ret:
        assert (k == GUARD64).all()
        return ret, None
    return ret, [tuple(x) for x in k.reshape(-1, 2).tolist()]


def _keys_same(seqs, pairs=False, rc=False, mis=0, ref=False, what=None):
    """The GPU's keys against the host restatement (ref: and dedup_ref)."""
    ret, got = _keys(seqs, pairs, rc, mis)
    assert ret == 0, lib.last_error()
    host = Z._dedup_host(b"".join(seqs), [len(s) for s in seqs], pairs, rc)[0]
    exp = [tuple(x) for x in host.tolist()]
    bad = [u for u, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad and len(got) == len(exp), (what, pairs, rc, mis, bad[:5])
    if ref:
        assert got == R.keys(seqs, pairs, rc), (what, pairs, rc, mis)
    return got


# ---- keys ------------------------------------------------------------------
@pytest.mark.parametrize("pairs,rc", MODES)
def test_a_record_over_three_tiles(T, pairs, rc):
    """2 T + 37 bases in one record (reverse-complement keys included: the
    positions count from the record's far end, two tiles away)."""
    rng = random.Random(5)
    seqs = _seqs(rng, [5, 2 * T + 37, 4, 9])
    got = _keys_same(seqs, pairs, rc, mis=3, ref=True)
    assert len(set(got)) == len(got)
    if rc and not pairs:                                    # the other strand: the same key
        assert _keys_same([R.revcomp(s) for s in seqs], False, True, mis=11) == got


def test_records_that_end_on_a_tile_edge(T):
    rng = random.Random(7)
    for e in (T - 1, T, T + 1):
        seqs = _seqs(rng, _cut(2 * T + 133, [7, 60, e - 40, e, e + 3, 2 * T, 2 * T + 90]))
        for pairs, rc in MODES:
            _keys_same(seqs, pairs, rc, mis=e % 16, ref=(e == T), what=e)


def test_empty_records(T):
    """Runs of empty records at the start, on a tile edge and at the end; a
    block without a base."""
    rng = random.Random(9)
    lens = [0] * 300 + _cut(T, [100, 900, T - 30]) + [0] * 310 + _cut(T // 2, [11, 500]) + [0] * 305
    seqs = _seqs(rng, lens)
    empty = (R.mix(R.SEEDS[0]), R.mix(R.SEEDS[1]))
    for pairs, rc in MODES:
        got = _keys_same(seqs, pairs, rc, mis=1, ref=not pairs and not rc)
        if not pairs:
            assert got[0] == got[299] == got[304] == got[-1] == empty
    for pairs, rc in MODES:
        got = _keys_same([b""] * 70, pairs, rc, ref=True)
        assert len(set(got)) == 1 and len(got) == (35 if pairs else 70)
    assert _keys([])[0] == 0                                # nrec = 0


@pytest.mark.parametrize("pairs,rc", MODES)
def test_more_records_in_a_tile_than_lds_ends(pairs, rc):
    """ST_KCAP + 100 one-base records: the sums past the LDS cells go straight
    to the global cells."""
    rng = random.Random(11)
    seqs = _seqs(rng, [1] * (KCAP + 100), alphabet=b"ACGT")
    got = _keys_same(seqs, pairs, rc, mis=5, ref=True)
    assert len(set(got)) == (10 if pairs and rc else 16 if pairs else 2 if rc else 4)
    _keys_same(_seqs(rng, [2] * (KCAP + 40) + [0] * 9 + [3] * 7), pairs, rc)


@pytest.mark.parametrize("mis", range(16))
def test_misaligned_views(T, mis):
    """The bases at every misalignment: nothing outside the view is read (a
    guard byte would change a key)."""
    rng = random.Random(40 + mis)
    seqs = _seqs(rng, _cut(T + 41, [0, 3, 50, T - 2, T + 8]))
    for pairs, rc in ((False, False), (True, True), (False, True)):
        _keys_same(seqs, pairs, rc, mis=mis, ref=not pairs and not rc)
    _keys_same(seqs[:3], mis=mis, ref=True)                 # 50 bases: one partial chunk or two


def test_mates_of_which_one_is_empty():
    x = b"ACGTTGCAAC"
    seqs = [b"", x, x, b"", b"", b"", x, x]
    for rc in (False, True):
        got = _keys_same(seqs, True, rc, ref=True)
        assert len(set(got)) == (3 if rc else 4)            # (("", x) and (x, "") are swapped mates)


def test_key_errors():
    seqs = [b"ACG", b"T", b"GG"]
    assert _keys(seqs, pairs=True)[0] == -1 and "odd record count" in lib.last_error()
    for lens in ([3, 1, 1], [3, 1, 3], [3, 1]):
        assert _keys(seqs, lens=lens)[0] == -1 and "do not sum" in lib.last_error()


# ---- insert ----------------------------------------------------------------
def _insert(tab, keys, base=0):
    """fqz5_dedup_insert_keys of (lo, hi) pairs: (rc, the slots)."""
    so = Z._load()
    flat = np.asarray([w for k in keys for w in k], np.uint64)
    kt = torch.from_numpy(flat.view(np.int64).copy()).cuda()
    st, sp = _guarded(len(keys), torch.int32)
    lib.after_torch()
    ret = so.fqz5_dedup_insert_keys(tab.p, kt.data_ptr(), len(keys), base, sp)
    torch.cuda.synchronize()
    return ret, _back(st).tolist()


def _slot(tab, s):
    """(lo, hi, first, count) of slot s."""
    out = np.zeros(4, np.uint64)
    assert Z._load().fqz5_dedup_table_slot(tab.p, s, out.ctypes.data) == 0, lib.last_error()
    return tuple(out.tolist())


def _occupied(tab):
    n = int(Z._load().fqz5_dedup_table_slots(tab.p))
    return {s: x for s, x in ((s, _slot(tab, s)) for s in range(n)) if x[3]}


def test_keys_that_share_a_word():
    """Equal first words with different second words, and the reverse; zero
    and all-ones words are key words like any other."""
    keys = [(5, 1), (5, 2), (1, 5), (2, 5), (0, 7), (7, 0), (0, 0), (M, M), (M, 0), (0, M),
            (1 << 63, 0), (0, 1), (1, 0), (1, 1)]
    with Z._DedupTable(32) as tab:
        ret, slots = _insert(tab, keys, base=100)
        assert ret == 0, lib.last_error()
        assert len(set(slots)) == len(keys)
        for u, (k, s) in enumerate(zip(keys, slots)):
            assert _slot(tab, s) == (k[0], k[1], 100 + u, 1), k
        assert len(_occupied(tab)) == len(keys)
        ret, again = _insert(tab, keys[::-1], base=500)     # the same keys: the same slots
        assert ret == 0 and again == slots[::-1]
        for u, (k, s) in enumerate(zip(keys, slots)):
            assert _slot(tab, s) == (k[0], k[1], 100 + u, 2), k   # `first` from the first call
        lv = tab.levels()
        assert lv[2] == len(keys) and lv[R.LEVELS] == len(keys) and lv[R.LEVELS + 1] == 2


def test_equal_keys_in_one_wave():
    with Z._DedupTable(64) as tab:
        ret, slots = _insert(tab, [(0xABCDEF, 0x1234)] * 64, base=1000)
        assert ret == 0 and len(set(slots)) == 1
        assert _slot(tab, slots[0]) == (0xABCDEF, 0x1234, 1000, 64)
        assert len(_occupied(tab)) == 1


def test_a_table_filled_across_its_end():
    """8 slots, 8 keys whose home is slot 6: the probes wrap past the end; a
    ninth key is the "table full" error, an ordinary return of the bounded
    probe loop."""
    so = Z._load()
    with Z._DedupTable(4) as tab:
        assert so.fqz5_dedup_table_slots(tab.p) == 8
        keys = [(6 + 8 * j, j) for j in range(8)]
        ret, slots = _insert(tab, keys)
        assert ret == 0, lib.last_error()
        assert sorted(slots) == list(range(8))
        for u, (k, s) in enumerate(zip(keys, slots)):
            assert _slot(tab, s) == (k[0], k[1], u, 1)
        ret, slots = _insert(tab, [keys[3]], base=50)       # a key that is there still finds its slot
        assert ret == 0 and _slot(tab, slots[0]) == (keys[3][0], 3, 3, 2)
        ret, slots = _insert(tab, [(6 + 64, 99)], base=60)
        assert ret == -1 and "table full" in lib.last_error()
        assert slots == [0xFFFFFFFF]
        assert so.fqz5_dedup_table_reset(tab.p) == 0
        assert _occupied(tab) == {} and _slot(tab, 0) == (0, 0, M, 0)
        ret, slots = _insert(tab, [(6 + 64, 99)], base=60)
        assert ret == 0 and slots == [6]


def test_levels_cells():
    """Counts of 1, 2, 1023, 1024 and 1500."""
    keys = ([(11, 1)] + [(12, 2)] * 2 + [(13, 3)] * 1023 + [(14, 4)] * 1024 + [(15, 5)] * 1500)
    random.Random(3).shuffle(keys)
    with Z._DedupTable(8) as tab:
        ret, slots = _insert(tab, keys)
        assert ret == 0 and len(set(slots)) == 5
        lv = tab.levels()
    exp = [0] * R.LEVELS
    exp[1] = exp[2] = exp[1023] = 1
    exp[1024] = 2
    assert lv[:R.LEVELS].tolist() == exp and lv[R.LEVELS] == 5 and lv[R.LEVELS + 1] == 1500


# ---- match -----------------------------------------------------------------
def _match(tab, seqs, pairs=False, rc=False, invert=False, base=0, mis=0, first=True):
    """One fqz5_dedup_match: (rc, the selected indices, `first` per unit)."""
    so = Z._load()
    lens = np.asarray([len(s) for s in seqs], np.uint32)
    n = len(lens)
    units = n // (2 if pairs else 1)
    blob = b"".join(seqs)
    st, sp = _dev(blob, mis)
    rt, rp = _guarded(n, torch.int32)
    ft, fp = _guarded(units, torch.int64)
    hit = C.c_uint64(12345)
    lib.after_torch()
    ret = so.fqz5_dedup_match(tab.p, sp, len(blob), lens.ctypes.data, n, int(pairs), int(rc),
                              int(invert), base, rp, C.byref(hit), fp if first else None)
    torch.cuda.synchronize()
    rec, f = _back(rt), _back(ft)
    if ret:
        assert hit.value == 0 and (rec == GUARD).all()
        return ret, None, None
    k = int(hit.value)
    assert (rec[k:] == GUARD).all()                         # nothing past the selection
    if not first:
        assert (f == GUARD64).all()
    return ret, rec[:k].tolist(), f.tolist()


def _blocks_same(blocks, pairs=False, rc=False, invert=False):
    """Blocks matched in turn into one table against the host table and the
    exact dict over all of them."""
    flat = [s for b in blocks for s in b]
    assert R.distinct_keys(flat, pairs, rc)
    ek, ef, counts = R.dedup(flat, pairs, rc, invert)
    mates = 2 if pairs else 1
    out, at = [], 0
    with Z._DedupTable(len(flat) // mates) as tab, Z._DedupHostTable() as host:
        for j, b in enumerate(blocks):
            ret, sel, first = _match(tab, b, pairs, rc, invert, base=at // mates, mis=j % 16)
            assert ret == 0, lib.last_error()
            _, hk, hf = Z._dedup_host(b"".join(b), [len(s) for s in b], pairs, rc, invert, host,
                                      at // mates)
            assert sel == np.flatnonzero(np.repeat(hk, mates)).tolist(), j
            assert first == hf.tolist(), j
            assert sel == [r for r in range(len(b)) if ek[at + r]], j
            assert first == ef[at // mates:(at + len(b)) // mates], j
            out.append(sel)
            at += len(b)
        lv = tab.levels()
        assert lv.tolist() == host.levels().tolist()
    hist, distinct, top = R.levels(counts)
    assert lv[:R.LEVELS].tolist() == hist and lv[R.LEVELS] == distinct and lv[-1] == top
    return out


def test_duplicates_in_different_tiles_and_workgroups(T):
    """One sequence at records 3, 150 and 290 of a block of eight tiles (the
    insert's workgroups hold 256 units): the lowest is kept."""
    rng = random.Random(13)
    seqs = _seqs(rng, [rng.randint(90, 110) for _ in range(300)], alphabet=b"ACGT")
    seqs[150] = seqs[290] = seqs[3]
    seqs[299] = seqs[0]
    assert sum(len(s) for s in seqs) > 6 * T
    (sel,) = _blocks_same([seqs])
    assert sel == [r for r in range(300) if r not in (150, 290, 299)]
    (inv,) = _blocks_same([seqs], invert=True)
    assert inv == [150, 290, 299]
    with Z._DedupTable(300) as tab:                         # without the per-unit output
        assert _match(tab, seqs, first=False)[1] == sel


@pytest.mark.parametrize("pairs,rc", MODES)
def test_blocks_into_one_table(pairs, rc):
    """Duplicates within a block and across blocks, other strands and swapped
    mates among them; with pairs both mates are selected."""
    rng = random.Random(17)
    pool = _seqs(rng, [rng.randint(0, 70) for _ in range(120)])
    blocks = []
    for n in (260, 90, 2, 300):
        b = []
        for _ in range(n // 2):
            a, c = rng.choice(pool), rng.choice(pool[:12])
            x = rng.random()
            b += [c, a] if x < 0.3 else [R.revcomp(a), c] if x < 0.5 else [a, c]
        blocks.append(b)
    for invert in (False, True):
        out = _blocks_same(blocks, pairs, rc, invert)
        assert 0 < sum(map(len, out)) < sum(map(len, blocks))
        if pairs:
            assert all(s[0::2] == [r - 1 for r in s[1::2]] and all(r % 2 == 0 for r in s[0::2])
                       for s in out)


def test_match_errors():
    with Z._DedupTable(8) as tab:
        assert _match(tab, [b"ACG", b"T", b"GG"], pairs=True)[0] == -1
        assert "odd record count" in lib.last_error()
        assert _match(tab, [])[:2] == (0, [])               # nrec = 0
        assert _occupied(tab) == {}
