"""The filter by read metrics restated in plain Python, for the tests of
fqz5_filter_host, fqz5_filter_match and fqz5file.filter_*.  Nothing here calls
the code under test.

A record is (sequence bytes, quality bytes already - 33 modulo 256, or None
for a record of a block without qualities).  Criteria are a dict with the
keyword names of fqz5file.Filter; one that is absent or None is off."""
REASONS = ("min_len", "max_len", "max_n", "min_mean_q", "low_q", "gc_pct", "min_complexity_pct")
NONE = 7


def sums(rec, low_q=None):
    """(L, n, gc, diff, qsum, lowq) of one record (Python ints)."""
    s, q = rec
    s = bytes(s)
    q = bytes(q) if q is not None else b""
    return (len(s), sum(c in b"Nn" for c in s), sum(c in b"GCgc" for c in s),
            sum(a != b for a, b in zip(s, s[1:])), sum(q),
            sum(x < low_q for x in q) if low_q is not None else 0)


def reason(rec, crit: dict) -> int:
    """The lowest criterion the record fails, NONE when it passes."""
    g = lambda k: crit.get(k)
    L, n, gc, diff, qsum, lowq = sums(rec, g("low_q"))
    if g("min_len") is not None and not L >= g("min_len"):
        return 0
    if g("max_len") is not None and not L <= g("max_len"):
        return 1
    if g("max_n") is not None and not n <= g("max_n"):
        return 2
    if g("min_mean_q") is not None and not qsum >= g("min_mean_q") * L:
        return 3
    if g("low_q") is not None and not 100 * lowq <= g("max_low_pct") * L:
        return 4
    if g("gc_pct") is not None and not g("gc_pct")[0] * L <= 100 * gc <= g("gc_pct")[1] * L:
        return 5
    if g("min_complexity_pct") is not None and \
            not 100 * diff >= g("min_complexity_pct") * max(L - 1, 0):
        return 6
    return NONE


def rule(records, crit: dict, pairs: bool = False, invert: bool = False):
    """(keep per record, failed[7] in units, the units seen)."""
    mates = 2 if pairs else 1
    assert len(records) % mates == 0
    why = [reason(r, crit) for r in records]
    keep, failed = [], [0] * 7
    for u in range(len(records) // mates):
        w = min(why[u * mates:(u + 1) * mates])
        if w != NONE:
            failed[w] += 1
        keep += [(w == NONE) != invert] * mates
    return keep, failed, len(records) // mates


def fastq_records(text: bytes):
    """4-line FASTQ text as (records, each record's four lines as one bytes)."""
    lines = text.split(b"\n")[:-1]
    recs = [(s, bytes((c - 33) & 255 for c in q)) for s, q in zip(lines[1::4], lines[3::4])]
    texts = [b"".join(x + b"\n" for x in lines[k:k + 4]) for k in range(0, len(lines), 4)]
    return recs, texts
