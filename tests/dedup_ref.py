"""The duplicates rule (include/fqz5_fastq.h, "Duplicates") restated in plain
Python ints, and an exact deduplication by a dict on the sequences themselves.
No test and no conftest: the dedup tests import it.

The key of a unit is what the library computes, bit for bit; the exact
deduplication never looks at a key.  distinct_keys() is the condition every
test input meets first: different units (as the dict tells them apart) have
different keys, so the library's selection must be the dict's."""
M = (1 << 64) - 1
SEEDS = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
LEVELS = 1025


def mix(x: int) -> int:
    x &= M
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M
    x ^= x >> 31
    return x


def K(s: int, seq: bytes) -> int:
    """K_s of one record."""
    k = mix(SEEDS[s] ^ len(seq))
    for i, c in enumerate(seq):
        k += mix(SEEDS[s] + (i << 8 | c))
    return k & M


def revcomp(seq: bytes) -> bytes:
    return bytes(seq).translate(COMP)[::-1]


def unit_key(unit, pairs: bool = False, rc: bool = False):
    """(first word, second word) of a unit: a record's bytes, with pairs the
    tuple of its mates' bytes."""
    if pairs:
        a, b = unit
        fwd = ((K(0, a) + K(2, b)) & M, (K(1, a) + K(3, b)) & M)
        return min(fwd, ((K(0, b) + K(2, a)) & M, (K(1, b) + K(3, a)) & M)) if rc else fwd
    fwd = (K(0, unit), K(1, unit))
    return min(fwd, (K(0, revcomp(unit)), K(1, revcomp(unit)))) if rc else fwd


def units_of(seqs, pairs: bool = False):
    seqs = [bytes(s) for s in seqs]
    if not pairs:
        return seqs
    assert len(seqs) % 2 == 0
    return list(zip(seqs[0::2], seqs[1::2]))


def canonical(unit, pairs: bool = False, rc: bool = False):
    """What the exact deduplication compares: the unit itself, with rc the
    smaller of it and its other strand (pairs: its mates swapped)."""
    if not rc:
        return unit
    return min(unit, (unit[1], unit[0])) if pairs else min(unit, revcomp(unit))


def keys(seqs, pairs: bool = False, rc: bool = False):
    return [unit_key(u, pairs, rc) for u in units_of(seqs, pairs)]


def distinct_keys(seqs, pairs: bool = False, rc: bool = False) -> bool:
    """Different units have different keys (the condition on a test input)."""
    seen = {}
    for u in units_of(seqs, pairs):
        c = canonical(u, pairs, rc)
        if seen.setdefault(unit_key(u, pairs, rc), c) != c:
            return False
    return len(set(seen.values())) == len(seen)


def dedup(seqs, pairs: bool = False, rc: bool = False, invert: bool = False):
    """Exact, by a dict on the sequences: (keep per record, per unit the
    number of the first unit equal to it, the count per distinct unit in order
    of first occurrence)."""
    first, count, firsts = {}, {}, []
    for u, unit in enumerate(units_of(seqs, pairs)):
        c = canonical(unit, pairs, rc)
        firsts.append(first.setdefault(c, u))
        count[c] = count.get(c, 0) + 1
    mates = 2 if pairs else 1
    keep = [(f == u) != invert for u, f in enumerate(firsts) for _ in range(mates)]
    return keep, firsts, list(count.values())


def levels(counts):
    """The histogram fqz5_dedup_levels gives: LEVELS cells, the keys, the
    largest count."""
    out = [0] * LEVELS
    for c in counts:
        out[min(c, LEVELS - 1)] += 1
    return out, len(counts), max(counts, default=0)
