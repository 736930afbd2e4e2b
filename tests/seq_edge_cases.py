"""Inputs at the edges of the sequence context model's kernels
(test_seq_edge_cases.py, test_seq_edges_gpu.py), with a plain restatement of
the context rule (fqzcomp5.c:1103-1105, :1176-1199, :1210-1219) and a census
that says what each input reaches.  Pure numpy, seeded; nothing here calls
the code under test.

The decoders forward a step's stores to the next steps' loads by hand
(seq_cm.hip: k_seq_dec's fn == fw, rv == fw, fn == rv; SEQ_LA_STEP's hf[] and
hr[] of the last three steps; the re-priming at a record's or run's end), and
those terms matter only where a context recurs within three bases:
homopolymers, short-period repeats, reverse-complement palindromes, and, in a
record's first k bases, whatever the two seeds make of the bases.  The model
pass (k_seq_model_runs) walks a context's events by a lane below 48 events and
by a wave from there, 64 per round, in tiles of `span` sorted events.

  walk(seq, lens, k, both)      the coded steps: (piece starts, fw, fn, rn)
  hazards(seq, lens, k, both)   per step inside a piece (same record, same
                                run): the seven forwarding terms, the pieces
                                of 1..4 bases, the ring position pieces end at
  model_runs(seq, lens, k, both)  per-context run lengths in the sorted keys,
                                invalid keys, and the tiles of the span that
                                launch_seq_model picks
Case.want holds the census minima a case is built for; they are conditions on
the input alone (test_seq_edge_cases.py asserts them from this file).
"""
import functools
from collections import Counter, namedtuple

import numpy as np

Case = namedtuple("Case", "name seq lens k both want")

SEQ_LONG = 48                    # events: a wave rather than a lane (seq_cm.hip)
SEQ_CTX_W = 2048                 # k_seq_ctx's window, bytes
RUN_LENGTHS = (47, 48, 49, 63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 1000)
TERMS = ("fn_fw", "rn_fw", "fn_rn", "fn_hf", "fn_hr", "rn_hf", "rn_hr")
ONE_STEP_TERMS = ("fn_fw", "rn_fw", "fn_rn")      # k_seq_dec's own three

_CLS = np.full(256, 2, np.uint8)
_CODE = np.full(256, 3, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CLS[_c], _CLS[_c | 0x20] = 0, 1
    _CODE[_c] = _CODE[_c | 0x20] = _i


def seeds(k):
    mask = (1 << (2 * k)) - 1
    return 0x007616C7 & mask, (0x2C6B62FF >> (32 - 2 * k)) & mask


def segments(lens, n):
    """Record starts as the reference sees them: it counts a record down in
    an int, so a record of length 0 is never seen to end (no later start).
    None: a start is due but the records are used up."""
    seg = [0]
    lens = [int(x) for x in lens] or [0]
    if n:
        pos, left, nxt = 0, lens[0], 1
        while 0 < left < 2 ** 31:
            b = pos + left
            if b >= n:
                break
            if nxt >= len(lens):
                return None
            seg.append(b)
            pos, left = b, lens[nxt]
            nxt += 1
    seg.append(n)
    return seg


def walk(seq, lens, k, both):
    """The coded base steps in stream order: (new_piece, fw, fn, rn) with fw
    the context that codes the base, fn the next one and rn the reverse
    context whose model counts the base that leaves it (-1: one strand).
    A piece is an unbroken stretch of one record and one class run; literal
    bytes code no step and leave the contexts alone."""
    a = np.frombuffer(bytes(seq), np.uint8)
    n = len(a)
    seg = segments(lens, n)
    assert seg is not None
    cls, code = _CLS[a].tolist(), _CODE[a].tolist()
    starts = set(seg[1:-1])
    mask, top = (1 << (2 * k)) - 1, 2 * k - 2
    f0, r0 = seeds(k)
    fw, rv, prev = f0, r0, -1
    out = []
    for p in range(n):
        rec = p in starts
        if rec:
            fw, rv = f0, r0
        c = cls[p]
        new = rec or c != prev
        prev = c
        if c == 2:
            continue
        b = code[p]
        fn = ((fw << 2) + b) & mask
        rn = (rv >> 2) + ((3 - b) << top) if both else -1
        out.append((new, fw, fn, rn))
        fw = fn
        if both:
            rv = rn
    return out


def hazards(seq, lens, k, both):
    """Counter of, per step: fn_fw, rn_fw, fn_rn; fn / rn found among the
    forward (hf) and reverse (hr) contexts stored one and two steps earlier in
    the same piece (fn_hf1, fn_hf2, ... and their sums fn_hf, fn_hr, rn_hf,
    rn_hr); and per piece: ("len", L) for L = 1..4 and ("ring", L % 3)."""
    h = Counter()
    hf, hr, plen = [], [], 0

    def close():
        if plen:
            if plen <= 4:
                h[("len", plen)] += 1
            h[("ring", plen % 3)] += 1
            h["pieces"] += 1

    for new, fw, fn, rn in walk(seq, lens, k, both):
        if new:
            close()
            hf, hr, plen = [], [], 0
        plen += 1
        h["steps"] += 1
        h["fn_fw"] += fn == fw
        for d, (x, y) in enumerate(zip(hf[::-1], hr[::-1]), 1):
            h["fn_hf%d" % d] += fn == x
            h["fn_hf"] += fn == x
            if both:
                h["fn_hr%d" % d] += fn == y
                h["fn_hr"] += fn == y
                h["rn_hf%d" % d] += rn == x
                h["rn_hf"] += rn == x
                h["rn_hr%d" % d] += rn == y
                h["rn_hr"] += rn == y
        if both:
            h["rn_fw"] += rn == fw
            h["fn_rn"] += fn == rn
        hf = (hf + [fw])[-2:]
        hr = (hr + [rn])[-2:]
    close()
    return h


def model_span(nkeys, k):
    """launch_seq_model's tile: about 256 runs of the mean length, 256..4096"""
    nctx = min(1 << (2 * k), nkeys)
    run = min((nkeys + nctx - 1) // nctx, 16)
    return 256 * max(run, 1)


def model_runs(seq, lens, k, both):
    """The model pass's view: k_seq_ctx's keys (fw per base and, both
    strands, rn; the invalid key for a literal byte), sorted."""
    a = np.frombuffer(bytes(seq), np.uint8)
    nkeys = len(a) * (2 if both else 1)
    inval = 1 << (2 * k)
    keys = np.full(nkeys, inval, np.int64)
    pos = np.flatnonzero(_CLS[a] < 2)
    st = walk(seq, lens, k, both)
    assert len(st) == len(pos)
    if both:
        keys[2 * pos] = [s[1] for s in st]
        keys[2 * pos + 1] = [s[3] for s in st]
    else:
        keys[pos] = [s[1] for s in st]
    keys.sort(kind="stable")
    nvalid = int(np.searchsorted(keys, inval))
    heads = np.flatnonzero(np.r_[True, keys[1:nvalid] != keys[:nvalid - 1]]) if nvalid else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], nvalid]
    out = {"nkeys": nkeys, "invalid": nkeys - nvalid, "runs": Counter((ends - heads).tolist()),
           "span": 0, "tiles": 0, "tiles_no_head": 0, "tiles_invalid_only": 0, "tiles_inside_run": 0,
           "runs_crossing": 0}
    if not nkeys:
        return out
    span = model_span(nkeys, k)
    ntile = (nkeys + span - 1) // span
    with_head = set((heads // span).tolist())
    out.update(span=span, tiles=ntile, tiles_no_head=ntile - len(with_head),
               tiles_invalid_only=sum(1 for t in range(ntile) if t * span >= nvalid),
               tiles_inside_run=sum(1 for t in range(ntile)
                                    if t not in with_head and t * span < nvalid),
               runs_crossing=int(np.sum(ends > (heads // span + 1) * span)))
    return out


# ---------------------------------------------------------------------------
MOTIFS = ("AT", "CG", "ACG", "AAT", "ACGT", "AATT")
CUTS = (1, 2, 3, 4, 7, 64, 65)
KB = [(k, b) for k in range(1, 14) for b in (0, 1)]     # every k of 1..13, both modes


def _rep(m, n):
    return (m * (n // len(m) + 1))[:n]


def _cut(s, c):
    return [c] * (len(s) // c) + ([len(s) % c] if len(s) % c else [])


def _rand(seed, n, alpha=b"ACGT"):
    return np.random.default_rng(seed).choice(np.frombuffer(alpha, np.uint8), n).tobytes()


def _exact(seq, k, both, c):
    """The shortest prefix of seq in which some context has exactly c events
    and is the first to reach c (one record)."""
    cnt = Counter()
    per = 2 if both else 1
    st = walk(seq, [len(seq)], k, both)
    for i, (_, fw, _, rn) in enumerate(st):
        hit = False
        for key in (fw, rn)[:per]:
            cnt[key] += 1
            hit |= cnt[key] == c
        if hit and c in cnt.values():
            return seq[:i + 1]
    raise AssertionError("no context reaches %d events" % c)


def record_reaching(k, term, steps=None):
    """A record (str) whose last base makes fn == rn ("fn_rn") or rn == fw
    ("rn_fw") at context size k, or None where no record can.

    Once k bases of a record are coded, rn is fn's reverse complement: an
    odd-length k-mer is never its own (the middle base would be its own
    complement), and rn == fw asks fw[1:], k - 1 bases, to be its own, which
    needs k odd.  So fn == rn at odd k and rn == fw at even k can occur only
    in a record's first k bases, where the contexts still hold seed bases.
    This solves base by base: position i of fn, rn and fw after j bases is a
    seed base or a base of the record (complemented in rn), and equal
    positions either fix a base, tie two bases, or compare two constants."""
    f0, r0 = seeds(k)
    sf = [(f0 >> (2 * (k - 1 - i))) & 3 for i in range(k)]
    sr = [(r0 >> (2 * (k - 1 - i))) & 3 for i in range(k)]
    for j in range(2 * k + 2 if steps is None else steps):
        # terms: (base index or None, constant or complement flag)
        fn = [(j + 1 - k + i, 0) if j + 1 - k + i >= 0 else (None, sf[j + 1 + i]) for i in range(k)]
        rn = [(j - i, 1) if j - i >= 0 else (None, sr[i - j - 1]) for i in range(k)]
        fw = [(j - k + i, 0) if j - k + i >= 0 else (None, sf[j + i]) for i in range(k)]
        eqs = list(zip(fn, rn)) if term == "fn_rn" else list(zip(rn, fw))
        val = _solve(eqs, j + 1)
        if val is not None:
            return "".join("ACGT"[v] for v in val)
    return None


def _solve(eqs, nvar):
    adj = [[] for _ in range(nvar)]
    fixed = {}
    for (a, ca), (b, cb) in eqs:
        if a is None and b is None:
            if ca != cb:
                return None
        elif a is None or b is None:
            v, c, const = (b, cb, ca) if a is None else (a, ca, cb)
            want = 3 - const if c else const
            if fixed.setdefault(v, want) != want:
                return None
        else:
            adj[a].append((b, ca != cb))
            adj[b].append((a, ca != cb))
    val = [None] * nvar
    for root in range(nvar):
        if val[root] is not None:
            continue
        for guess in range(4):
            seen = {root: guess}
            todo, ok = [root], True
            while todo and ok:
                x = todo.pop()
                ok = fixed.get(x, seen[x]) == seen[x]
                for y, flip in adj[x]:
                    w = 3 - seen[x] if flip else seen[x]
                    if y not in seen:
                        seen[y] = w
                        todo.append(y)
                    elif seen[y] != w:
                        ok = False
            if ok:
                break
        else:
            return None
        for x, v in seen.items():
            val[x] = v
    return val


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    names = set()

    def add(name, seq, lens, k, both, **want):
        assert name not in names, name
        names.add(name)
        out.append(Case(name, bytes(seq), [int(x) for x in lens], k, both, want))

    i = 0

    def kb():
        nonlocal i
        i += 1
        return KB[(i - 1) % len(KB)]

    # homopolymers and repeats, upper and lower case and with a class switch
    # off the motif's phase, whole and cut into records
    for m in ("A", "T") + MOTIFS:
        s = _rep(m, 601)
        for tag, t in (("uc", s), ("lc", s.lower()), ("sw", s[:301] + s[301:452].lower() + s[452:])):
            k, b = kb()
            # a context recurs after the motif's period: at once, one step
            # back, two steps back, or (period 4) outside the forwarding ring
            term = {1: "fn_fw", 2: "fn_hf1", 3: "fn_hf2", 4: "steps"}[len(m)]
            add(f"rep_{m}_{tag}_k{k}b{b}", t.encode(), [len(t)], k, b, hz={term: 250})
    for m in MOTIFS:
        for c in CUTS:
            k, b = kb()
            s = _rep(m, 5 * 65 + 3)
            add(f"cut_{m}_{c}_k{k}b{b}", s.encode(), _cut(s, c), k, b, hz={"pieces": len(_cut(s, c))})
    # every forwarding term of both decoders on purpose: all motifs in one
    # block, a record each and then cut, at the smallest look-ahead k (3: the
    # windows wrap the whole model), an even and an odd k above it, and the
    # one-step decoder's k = 1, 2
    def terms_want(k, b):
        w = {t: 50 for t in (TERMS if b else ("fn_fw", "fn_hf"))}
        w.pop("fn_rn" if k % 2 else "rn_fw", None)      # (record_reaching: no input has them)
        w.update({("len", L): 4 for L in (1, 2, 3, 4)})
        w.update({("ring", r): 4 for r in (0, 1, 2)})
        return {"hz": w}

    def terms_block(motifs, n):
        txt = [_rep(m, n) for m in motifs]
        return ("".join(txt) + "".join(t[:66] for t in txt),
                [n] * len(txt) + [c for t in txt for c in (1, 2, 3, 4, 7, 49)])

    blk, lens = terms_block(("A", "T", "C") + MOTIFS, 240)
    for k in (1, 2, 3, 4, 5, 12, 13):
        for b in (0, 1):
            add(f"terms_k{k}b{b}", blk.encode(), lens, k, b, **terms_want(k, b))
    # (fn == rn at odd k and rn == fw at even k: no record reaches them at
    # any k of 1..14, record_reaching; the seeds do not line up)
    # the one k = 14 case (1 GiB of counts): the same hazards, small
    blk, lens = terms_block(("A", "AT", "ACG", "AATT"), 160)
    add("terms_k14b1", blk.encode(), lens, 14, 1, **terms_want(14, 1))

    # k_seq_ctx: 64 segments per wave, 2048-byte windows
    for nr in (64, 65, 128, 129):
        k, b = kb()
        add(f"onebase_{nr}_k{k}b{b}", _rand(100 + nr, nr), [1] * nr, k, b, hz={("len", 1): nr})
    s = _rand(7, 20) + _rand(8, 5000) + _rand(9, 60)
    add("long_beside_ones_k10b1", s, [1] * 20 + [5000] + [1] * 60, 10, 1, hz={"pieces": 81, ("len", 1): 80})
    add("long_beside_ones_k3b0", s, [1] * 20 + [5000] + [1] * 60, 3, 0, hz={"pieces": 81, ("len", 1): 80})
    add("zero_then_long_k11b1", _rand(10, 5200), [0, 5000, 200], 11, 1, hz={"steps": 5200})
    add("zero_then_long_k2b0", _rand(10, 5200), [0, 5000, 200], 2, 0, hz={"steps": 5200})
    s = _rand(11, 2040) + b"N" * 20 + _rand(12, 2030) + b"RYN" * 5 + _rand(13, 100)
    add("lit_window_k12b1", s, [len(s)], 12, 1, invalid=70)
    add("lit_window_k6b0", s, [3000, len(s) - 3000], 6, 0, invalid=35)

    # exact per-context run lengths at k = 1, 2 (4 and 16 contexts): one
    # symbol only (counts saturate and halve every step) and mixed symbols
    for c in RUN_LENGTHS:
        # poly-A, k = 1, one strand: context A codes all but the first base
        add(f"run1_{c}_k1b0", b"A" * (c + 1), [c + 1], 1, 0, runs=[c])
        # both strands, k = 2: the reverse context TT counts every base
        # but the first (whose reverse context still holds a seed base)
        add(f"run1_{c}_k2b1", b"A" * (c + 1), [c + 1], 2, 1, runs=[c])
        s = _exact(_rand(200 + c, 40 * c + 64), 2, 0, c)
        add(f"runx_{c}_k2b0", s, [len(s)], 2, 0, runs=[c])
        s = _exact(_rand(300 + c, 8 * c + 64), 1, 1, c)
        add(f"runx_{c}_k1b1", s, [len(s)], 1, 1, runs=[c])

    # the tile width: 4096 with tiles inside one run, 256 at k = 10; tiles of
    # invalid keys only
    add("span4096_k1b0", _rand(20, 20000), [20000], 1, 0, span=4096, tiles_inside_run=1, runs_crossing=3)
    add("span4096_k1b1", _rand(21, 10000), [100] * 100, 1, 1, span=4096, tiles_inside_run=1, runs_crossing=3)
    # (k = 10: 600 records of 10 bases give the seed context a run of 600,
    # which holds a whole tile of 256, and its successors 150 each)
    s = _rand(22, 6000) + b"N" * 700 + _rand(23, 300)
    for b in (0, 1):
        add(f"span256_k10b{b}", s, [10] * 600 + [1000], 10, b, span=256, tiles_invalid_only=2,
            tiles_inside_run=1, runs_crossing=2)
    add("span_mid_k4b0", _rand(24, 1500) + b"N" * 3000, [4500], 4, 0, span=4096, tiles_invalid_only=1)
    add("span_mid_k5b1", _rand(25, 3000), [3000], 5, 1, span=1536)

    # very low entropy: the tightest case of the encoder's size bounds
    for name, m in (("polyA", "A"), ("polyAT", "AT")):
        for k, b in ((10, 0), (12, 1)):
            s = _rep(m, 100_000)
            add(f"{name}_100k_k{k}b{b}", s.encode(), [100_000], k, b, nkeys=100_000 * (1 + b))
            add(f"{name}_100k_recs_k{k}b{b}", s.encode(), [250] * 400, k, b, nkeys=100_000 * (1 + b))

    # (the compressed lengths of these cover every residue mod 16 as they
    # are, test_compressed_lengths_cover_every_residue: no fillers)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)
