"""fqz5_dedup_keys_host and the host table (dedup.hip), the host restatement of
the duplicates rule.  No GPU.

Expected values come from the rule restated in plain Python (dedup_ref): the
keys bit for bit, the selection from an exact dict on the sequences.  Every
input is first checked to have different keys for different units."""
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import dedup_ref as R

MODES = [(False, False), (False, True), (True, False), (True, True)]


def _records(rng, n, lens=(0, 60), alphabet=b"ACGTNacgt", dup=0.4):
    """n records, about `dup` of them a copy of an earlier one, its reverse
    complement, or an earlier neighbour (so that pairs repeat, also swapped)."""
    out = []
    for _ in range(n):
        x = rng.random()
        if out and x < dup:
            s = rng.choice(out)
            out.append(R.revcomp(s) if x < dup / 3 else s)
        else:
            out.append(bytes(rng.choice(alphabet) for _ in range(rng.randint(*lens))))
    return out


def _host(seqs, pairs=False, rc=False, invert=False, table=None, first_unit=0, lens=None):
    return Z._dedup_host(b"".join(seqs), [len(s) for s in seqs] if lens is None else lens, pairs,
                         rc, invert, table, first_unit)


def _same(seqs, pairs, rc, invert=False):
    assert R.distinct_keys(seqs, pairs, rc)
    keys, keep, first = _host(seqs, pairs, rc, invert)
    assert keys.dtype == np.uint64 and [tuple(k) for k in keys.tolist()] == R.keys(seqs, pairs, rc)
    ek, ef, _ = R.dedup(seqs, pairs, rc, invert)
    mates = 2 if pairs else 1
    assert np.repeat(keep, mates).tolist() == [int(k) for k in ek]
    assert first.tolist() == ef
    return keep.tolist()


@pytest.mark.parametrize("pairs,rc", MODES)
def test_host_against_the_rule(pairs, rc):
    rng = random.Random(21)
    seqs = _records(rng, 400)
    if pairs:                                               # whole pairs repeated, some swapped
        for k in range(20):
            a = rng.randrange(0, 100) * 2
            seqs[200 + 10 * k:202 + 10 * k] = seqs[a:a + 2] if k % 2 else seqs[a:a + 2][::-1]
        assert len(seqs) == 400
    keep = _same(seqs, pairs, rc)
    assert 0 < sum(keep) < len(keep)                        # (the case decides something)
    inv = _same(seqs, pairs, rc, invert=True)
    assert [a + b for a, b in zip(keep, inv)] == [1] * len(keep)    # the exact complement
    if rc:
        assert sum(keep) < sum(_same(seqs, pairs, False))   # (the other strand merged something)


def test_first_across_blocks():
    """Three blocks into one table: `first` and the selection are those of the
    whole file."""
    rng = random.Random(23)
    seqs = _records(rng, 300, dup=0.5)
    ek, ef, counts = R.dedup(seqs)
    assert R.distinct_keys(seqs)
    with Z._DedupHostTable() as t:
        keep, first = [], []
        for a in (0, 100, 130):
            b = {0: 100, 100: 130, 130: 300}[a]
            _, k, f = _host(seqs[a:b], table=t, first_unit=a)
            keep += k.tolist()
            first += f.tolist()
        lv = t.levels()
    assert keep == [int(k) for k in ek] and first == ef
    assert any(f < 100 <= u for u, f in enumerate(ef))      # (a duplicate across blocks)
    hist, distinct, top = R.levels(counts)
    assert lv[:R.LEVELS].tolist() == hist and int(lv[R.LEVELS]) == distinct and int(lv[-1]) == top
    assert int(lv[:R.LEVELS].sum()) == distinct
    assert sum(c * int(x) for c, x in enumerate(lv[:R.LEVELS])) == len(seqs)


def test_levels_top_cell():
    seqs = [b"ACGT"] * 1500 + [b"AC"] * 1024 + [b"A"] * 1023 + [b"", b""] + [b"T"]
    with Z._DedupHostTable() as t:
        _, keep, _ = _host(seqs, table=t)
        lv = t.levels()
    assert int(keep.sum()) == 5
    assert lv[1] == 1 and lv[2] == 1 and lv[1023] == 1 and lv[1024] == 2
    assert lv[R.LEVELS] == 5 and lv[R.LEVELS + 1] == 1500


def test_empty_records_only():
    seqs = [b""] * 9
    for pairs in (False, True):
        keep = _same(seqs[:8] if pairs else seqs, pairs, False)
        assert keep == [1] + [0] * (len(keep) - 1)
    keys, _, _ = _host([b""])
    assert tuple(keys[0].tolist()) == (R.mix(R.SEEDS[0]), R.mix(R.SEEDS[1]))
    assert _host([])[0].shape == (0, 2)


def test_palindrome_and_strands():
    pal = b"ACGTACGT"
    assert R.revcomp(pal) == pal
    seqs = [pal, b"AACC", b"GGTT", pal, b"aacc", b"ggtt", b"AANCC", b"GGNTT"]
    assert _same(seqs, False, True) == [1, 1, 0, 0, 1, 0, 1, 0]
    assert _same(seqs, False, False) == [1, 1, 1, 0, 1, 1, 1, 1]
    keys, _, _ = _host([pal], rc=True)
    assert tuple(keys[0].tolist()) == (R.K(0, pal), R.K(1, pal))


def test_swapped_mates():
    a, b, c = b"ACGTTGCA", b"GGGTAC", b"TTAGC"
    seqs = [a, b, b, a, a, c, R.revcomp(a), R.revcomp(b), a, b]
    assert _same(seqs, True, True) == [1, 0, 1, 1, 0]       # (no base is complemented)
    assert _same(seqs, True, False) == [1, 1, 1, 1, 0]
    # the mates' seeds differ: (a, b) and (b, a) have different keys without revcomp
    k = R.keys(seqs, True)
    assert k[0] != k[1] and R.keys(seqs, True, True)[0] == R.keys(seqs, True, True)[1]


def test_case_is_kept():
    seqs = [b"ACGT", b"acgt", b"ACGt", b"ACGT"]
    assert _same(seqs, False, False) == [1, 1, 1, 0]
    assert _same(seqs, False, True) == [1, 1, 1, 0]


def test_argument_errors():
    seqs = [b"ACG", b"T", b"GG"]
    with pytest.raises(lib.NativeError, match="odd record count"):
        _host(seqs, pairs=True)
    for lens in ([3, 1, 1], [3, 1, 3], [3, 1]):
        with pytest.raises(lib.NativeError, match="do not sum"):
            _host(seqs, lens=lens)
    so = Z._load()
    assert so.fqz5_dedup_table_bytes(0) == 8 * 32 and so.fqz5_dedup_table_bytes(5) == 16 * 32
    assert so.fqz5_dedup_table_bytes(1 << 20) == (1 << 21) * 32
    assert so.fqz5_dedup_table_bytes((1 << 30) + 1) == 0    # more than 2^31 slots
    assert so.fqz5_dedup_host_add(None, None, 0, 0, 0, None, None) == -1
    assert "no table" in lib.last_error()
    assert so.fqz5_dedup_insert_keys(None, None, 0, 0, None) == -1 and "no table" in lib.last_error()
    out = np.zeros(R.LEVELS + 2, np.uint64)
    assert so.fqz5_dedup_levels(None, out.ctypes.data) == -1 and "no table" in lib.last_error()
