"""The statistics' definitions restated with numpy, for the tests of
fqz5_stats_host, fqz5_stats_add and fqz5file.stats.  Nothing here calls the
code under test.

A record is (sequence bytes, quality bytes already - 33 modulo 256, or None
for a record of a block without qualities)."""
import numpy as np

FIELDS = ("records", "bases", "qual_records", "empty", "base_counts", "qual_counts", "read_qual",
          "read_gc", "cycle_base", "cycle_qual")
CLASS = np.full(256, 5, np.int64)
for _k, _c in enumerate(b"ACGTN"):
    CLASS[_c] = CLASS[_c | 0x20] = _k
GC = np.zeros(256, np.int64)
GC[list(b"GCgc")] = 1


def rule(records, cycles: int, mates: int = 1) -> dict:
    """Every table over `cycles` positions (the caller's cap, untrimmed)."""
    t = {"records": np.zeros(mates, np.uint64), "bases": np.zeros(mates, np.uint64),
         "qual_records": np.zeros(mates, np.uint64), "empty": np.zeros(mates, np.uint64),
         "base_counts": np.zeros((mates, 256), np.uint64),
         "qual_counts": np.zeros((mates, 256), np.uint64),
         "read_qual": np.zeros((mates, 256), np.uint64),
         "read_gc": np.zeros((mates, 101), np.uint64),
         "cycle_base": np.zeros((mates, cycles, 6), np.uint64),
         "cycle_qual": np.zeros((mates, cycles, 256), np.uint64)}
    gcs, qsums = [], []
    for r, (s, q) in enumerate(records):
        m = r & 1 if mates == 2 else 0
        s = np.frombuffer(bytes(s), np.uint8).astype(np.int64)
        L = len(s)
        t["records"][m] += 1
        t["bases"][m] += L
        t["empty"][m] += L == 0
        t["base_counts"][m] += np.bincount(s, minlength=256).astype(np.uint64)
        c = min(L, cycles)
        np.add.at(t["cycle_base"][m], (np.arange(c), CLASS[s[:c]]), 1)
        gc = int(GC[s].sum())
        gcs.append(gc)
        if L:
            t["read_gc"][m, 100 * gc // L] += 1
        if q is None:
            qsums.append(0)
            continue
        q = np.frombuffer(bytes(q), np.uint8).astype(np.int64)
        assert len(q) == L
        t["qual_records"][m] += 1
        t["qual_counts"][m] += np.bincount(q, minlength=256).astype(np.uint64)
        np.add.at(t["cycle_qual"][m], (np.arange(c), q[:c]), 1)
        qsums.append(int(q.sum()))
        if L:
            t["read_qual"][m, int(q.sum()) // L] += 1
    t["record_gc"] = np.asarray(gcs, np.uint32)
    t["record_qsum"] = np.asarray(qsums, np.uint64)
    t["record_len"] = np.asarray([len(s) for s, _ in records], np.uint32)
    return t


def same(got: dict, exp: dict, what=None) -> None:
    for k in FIELDS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.dtype == np.uint64 and g.shape == e.shape, (what, k, g.dtype, g.shape, e.shape)
        assert (g == e).all(), (what, k, np.argwhere(g != e)[:5].tolist())


def add(a: dict, b: dict) -> dict:
    return {k: a[k] + b[k] for k in FIELDS}


def nx(lengths, x: float) -> int:
    """The Nx length from the record lengths themselves."""
    ls = np.sort(np.asarray(lengths, np.int64))[::-1]
    tot = int(ls.sum())
    if not tot:
        return 0
    cum = np.cumsum(ls)
    return int(ls[np.argmax(cum * 100 >= x * tot)])


def fastq_records(text: bytes):
    """4-line FASTQ text as records."""
    lines = text.split(b"\n")[:-1]
    return [(s, (np.frombuffer(q, np.uint8) - np.uint8(33)).tobytes())
            for s, q in zip(lines[1::4], lines[3::4])]
