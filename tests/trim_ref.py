"""The trim rule (include/fqz5_fastq.h, "Trim and clip") in plain Python loops
over (seq, qual) records, written from the rule's table and from nothing else:
what the tests of fqz5_trim_host, fqz5_trim_cuts / fqz5_trim_gather and
fqz5file.trim_* expect.  A record is (seq bytes, qual bytes) with qual the
quality line's bytes - 33 (None: no qualities); a spec is the keyword
arguments of fqz5file.Trim as a dict."""
STEPS = ("clip", "quality", "adapter", "trim_n", "crop")


def _as_list(x):
    if x is None:
        return []
    if isinstance(x, (bytes, str)):
        x = [x]
    return [a.encode() if isinstance(a, str) else bytes(a) for a in x]


def quality3(q, a0, b0, cutoff):
    total, best, stop = 0, 0, b0
    i = b0 - 1
    while i >= a0:
        total += cutoff - q[i]
        if total < 0:
            break
        if total > best:
            best, stop = total, i
        i -= 1
    return stop


def quality5(q, a0, b0, cutoff):
    total, best, start = 0, 0, a0
    i = a0
    while i < b0:
        total += cutoff - q[i]
        if total < 0:
            break
        if total > best:
            best, start = total, i + 1
        i += 1
    return start


def matches(s, p, b, adapter, min_overlap, max_err_pct):
    ov = min(len(adapter), b - p)
    if ov < min_overlap:
        return False
    wrong = 0
    for k in range(ov):
        if s[p + k] != adapter[k]:
            wrong += 1
    return wrong <= (max_err_pct * ov) // 100


def cut(record, spec, mate=0):
    """One record through the five steps: (a, b, the bases each step took off,
    the adapter that cut it as an index into adapters + adapters2, or None)."""
    s, q = record
    L = len(s)
    a, b = 0, L
    took, hit = [0] * 5, None
    head, tail = spec.get("head"), spec.get("tail")
    if head is not None or tail is not None:
        a = min(head or 0, L)
        b = max(a, L - min(tail or 0, L))
    took[0] = L - (b - a)
    n = b - a
    q5, q3 = spec.get("q5"), spec.get("q3")
    if q5 is not None or q3 is not None:
        a0, b0 = a, b
        start = quality5(q, a0, b0, q5) if q5 is not None else a0
        stop = quality3(q, a0, b0, q3) if q3 is not None else b0
        a, b = start, max(start, stop)
    took[1] = n - (b - a)
    n = b - a
    ad1, ad2 = _as_list(spec.get("adapters")), _as_list(spec.get("adapters2"))
    if ad1:
        mine, first = (ad2, len(ad1)) if mate and ad2 else (ad1, 0)
        min_overlap, pct = spec.get("min_overlap", 3), spec.get("max_err_pct", 10)
        p = a
        while hit is None and p <= b - min_overlap:
            for j, adapter in enumerate(mine):
                if matches(s, p, b, adapter, min_overlap, pct):
                    hit = first + j
                    break
            if hit is None:
                p += 1
        if hit is not None:
            b = p
    took[2] = n - (b - a)
    n = b - a
    if spec.get("trim_n"):
        while a < b and s[a] in b"Nn":
            a += 1
        while b > a and s[b - 1] in b"Nn":
            b -= 1
    took[3] = n - (b - a)
    n = b - a
    if spec.get("max_len") is not None:
        b = min(b, a + spec["max_len"])
    took[4] = n - (b - a)
    return a, b, took, hit


class Result:
    """records: the trimmed (seq, qual); starts, lengths per record; the
    counters of fqz5file.TrimHits."""


def trim(records, spec, pairs=False):
    r = Result()
    n_ad = len(_as_list(spec.get("adapters"))) + len(_as_list(spec.get("adapters2")))
    r.records, r.starts, r.lengths = [], [], []
    r.trimmed, r.removed, r.adapter_hits = [0] * 5, [0] * 5, [0] * n_ad
    r.bases_in = r.bases_out = 0
    for i, (s, q) in enumerate(records):
        a, b, took, hit = cut((s, q), spec, i & 1 if pairs else 0)
        r.records.append((s[a:b], None if q is None else q[a:b]))
        r.starts.append(a)
        r.lengths.append(b - a)
        r.bases_in += len(s)
        r.bases_out += b - a
        for k in range(5):
            r.removed[k] += took[k]
            r.trimmed[k] += took[k] > 0
        if hit is not None:
            r.adapter_hits[hit] += 1
    return r


def fastq_records(text: bytes):
    """(names, records) of 4-line FASTQ text, or of one-line-per-sequence
    FASTA text (qual None): a name is the header line without its first byte,
    qual the quality line's bytes - 33."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    names, records = [], []
    if text[:1] == b">":
        for k in range(0, len(lines), 2):
            names.append(lines[k][1:])
            records.append((lines[k + 1], None))
        return names, records
    assert len(lines) % 4 == 0
    for k in range(0, len(lines), 4):
        names.append(lines[k][1:])
        records.append((lines[k + 1], bytes(c - 33 for c in lines[k + 3])))
        assert len(records[-1][0]) == len(records[-1][1])
    return names, records


def text(names, records, keep=None, plus_name=False, with_qual=True) -> bytes:
    """The FASTQ (a record without qualities, or with_qual False: FASTA) text
    of the records keep[i] selects (all when None)."""
    out = []
    for i, (name, (s, q)) in enumerate(zip(names, records)):
        if keep is not None and not keep[i]:
            continue
        if q is None or not with_qual:
            out.append(b">" + name + b"\n" + s + b"\n")
        else:
            out.append(b"@" + name + b"\n" + s + b"\n+" + (name if plus_name else b"") + b"\n" +
                       bytes(c + 33 for c in q) + b"\n")
    return b"".join(out)
