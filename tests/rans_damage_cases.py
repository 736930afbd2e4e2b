"""Damaged rANS 4x16 container streams (test_rans_damage_cases.py,
test_rans_damaged_gpu.py, golden/make_golden_rans_damaged.py): base streams of
every transform coded by the oracle, a tolerant walker over their header
fields, and structured damage of each field.  Seeded and deterministic; no GPU
code is imported.

Bounded by construction: the rANS chains of the order-1 compressed table (u)
and of the RLE meta-data (um / 2) take their step count from the stream alone,
so no case carries a u or um / 2 over LIMIT, no size or ulen over CAP_MAX, and
no decode capacity over CAP_MAX: no chain of the corpus exceeds 2^18 symbols.
corpus() asserts that by walking every damaged header; nothing is dropped."""
import functools
import hashlib

import numpy as np

import host_rans_cases as hc

LIMIT = 1 << 17
CAP_MAX = 150_001
RLE_CHUNK = 65536

F_STRIPE, F_NOSZ, F_CAT, F_RLE, F_PACK, F_X32 = 8, 0x10, 0x20, 0x40, 0x80, 4

varint = hc._varint


def vget(b, p, end):
    """var_get_u32: (value, bytes used); at most 6 bytes, none past `end`."""
    v = n = 0
    while p + n < end:
        c = b[p + n]
        n += 1
        v = ((v << 7) | (c & 0x7f)) & 0xffffffff
        if not (c & 0x80) or n == 6:
            break
    return v, n


# ---- the header walker ------------------------------------------------------

class _Stop(Exception):
    pass


def _alphabet(b, p, end):
    """The run-length coded symbol list of a frequency table: (symbols, next)."""
    if p >= end:
        raise _Stop
    have = [False] * 256
    s, run = b[p], 0
    p += 1
    while True:
        have[s] = True
        if run:
            run -= 1
            s += 1
            if s > 255:
                raise _Stop
        elif p < end and b[p] == s + 1:
            if p + 1 >= end:
                raise _Stop
            s, run = b[p], b[p + 1]
            p += 2
        else:
            if p >= end:
                raise _Stop
            s = b[p]
            p += 1
        if not s:
            break
    return [i for i in range(256) if have[i]], p


def _table_o0(b, p, end):
    syms, p = _alphabet(b, p, end)
    for _ in syms:
        if p >= end:
            raise _Stop
        p += vget(b, p, end)[1]
    return p


def _table_o1(b, p, end):
    syms, p = _alphabet(b, p, end)
    if p >= end:
        raise _Stop
    for _ in syms:
        zrun = 0
        for _ in syms:
            if zrun:
                zrun -= 1
                continue
            if p >= end:
                raise _Stop
            f, k = vget(b, p, end)
            p += k
            if not f:
                if p >= end:
                    raise _Stop
                zrun = b[p]
                p += 1
    return p


class Walk:
    """fields: [(name, start, end)] in stream order, tiling the stream;
    vals: name -> the value read for every length field."""

    def __init__(self, b, cap=None):
        self.b, self.fields, self.vals = bytes(b), [], {}
        self.p = 0
        try:
            if self.b:
                self._stream(len(self.b), cap, "", True)
        except _Stop:
            pass
        if self.p < len(self.b):
            self.fields.append(("rest", self.p, len(self.b)))

    def span(self, name):
        for f in self.fields:
            if f[0] == name:
                return f[1], f[2]
        return None

    def _add(self, name, n, end):
        n = min(n, end - self.p)
        if n > 0:
            self.fields.append((name, self.p, self.p + n))
            self.p += n

    def _var(self, name, end):
        v, k = vget(self.b, self.p, end)
        self.vals[name] = v
        self._add(name, k, end)
        return v

    def _byte(self, name, end):
        if self.p >= end:
            raise _Stop
        v = self.b[self.p]
        self.vals[name] = v
        self._add(name, 1, end)
        return v

    def _entropy(self, end, o1, nx, pre):
        b = self.b
        if self.p >= end:
            return
        if o1:
            h = self._byte(pre + "o1hdr", end)
            if h & 1:
                self._var(pre + "u", end)
                c = self._var(pre + "c", end)
                self._entropy(min(end, self.p + c), False, 4, pre + "tab.")
            else:
                try:
                    q = _table_o1(b, self.p, end)
                except _Stop:
                    q = end
                self._add(pre + "table", q - self.p, end)
        else:
            try:
                q = _table_o0(b, self.p, end)
            except _Stop:
                q = end
            self._add(pre + "table", q - self.p, end)
        self._add(pre + "states", 4 * nx, end)
        self._add(pre + "payload", end - self.p, end)

    def _stream(self, end, cap, pre, top):
        b = self.b
        order = self._byte(pre + "order", end)
        if order & F_STRIPE:
            if not top:
                raise _Stop
            ulen = self._var("ulen", end)
            n = self._byte("N", end)
            clen = [self._var(f"clen{i}", end) for i in range(n)]
            for i in range(n):
                if not clen[i] or self.p >= end:
                    raise _Stop
                sub = ulen // n + (ulen % n > i)
                self._stream(min(end, self.p + clen[i]), sub, f"s{i}.", False)
            return
        osz = cap if order & F_NOSZ else self._var(pre + "size", end)
        nx = 32 if order & F_X32 else 4
        if order & F_PACK:
            ns = self._byte(pre + "nsym", end) or 256
            if ns <= 16:
                self._add(pre + "map", ns, end)
            self._var(pre + "plen", end)
        if order & F_RLE:
            um = self._var(pre + "um", end)
            self._var(pre + "rl", end)
            if um & 1:
                mend = min(end, self.p + um // 2)
                if self.p < mend:
                    ns = self._byte(pre + "rle_nsyms", mend) or 256
                    self._add(pre + "rle_syms", ns, mend)
                    self._add(pre + "rle_runs", mend - self.p, mend)
            else:
                cm = self._var(pre + "cm", end)
                self._entropy(min(end, self.p + cm), False, nx, pre + "meta.")
        if self.p >= end:
            return
        if order & F_CAT:
            self._add(pre + "payload", end - self.p, end)
        else:
            self._entropy(end, order & 1, nx, pre)


# ---- base streams -----------------------------------------------------------

def _skew(n, k, seed, base=33, power=2):
    r = np.random.default_rng(seed)
    p = np.arange(k, 0, -1, dtype=float) ** power
    d = r.choice(k, n, p=p / p.sum())
    d[:min(k, n)] = np.arange(min(k, n))                 # every symbol is there
    return (d * 3 + base).astype(np.uint8).tobytes()


def _runs_raw(n, seed):
    """Mostly single bytes of 20 symbols and a few long runs of one more: so
    little RLE meta-data that the encoder stores it raw.  Ends in a run."""
    r = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n - 160:
        out += bytes((r.integers(0, 20, int(r.integers(60, 120))) * 2 + 40).astype(np.uint8))
        out += bytes([7]) * int(r.integers(90, 140))
    out += bytes([9]) + bytes([7]) * (n - len(out) - 1)
    return bytes(out)


def _runs_short(n, seed):
    """Runs of mean length 2.25 over 6 symbols, every symbol an RLE symbol:
    more than RLE_CHUNK literals and run bytes at n = 149 990."""
    r = np.random.default_rng(seed)
    m = n
    ln = r.choice([1, 2, 3, 4], m, p=[.25, .4, .2, .15])
    step = r.integers(1, 6, m)
    sym = (np.cumsum(step) % 6 + 60).astype(np.uint8)      # never the previous symbol
    return np.repeat(sym, ln)[:n].tobytes()


def _plain_body(ora, data, order):
    """The oracle's plain stream of `data` without order byte and size."""
    c = ora.rans_compress(data, order)
    assert c[0] == order, (c[0], order)
    return c[1 + vget(c, 1, len(c))[1]:]


def rle_parts(data):
    """(literals, RLE symbols, run lengths) of `data` as the encoder cuts it
    (rle.c:48-137): the symbols that repeat more often than not."""
    d = np.frombuffer(data, np.uint8)
    score = np.zeros(256, np.int64)
    rep = np.concatenate([[False], d[1:] == d[:-1]])
    np.add.at(score, d, np.where(rep, 1, -1))
    syms = [s for s in range(256) if score[s] > 0]
    is_rle = np.zeros(256, bool)
    is_rle[syms] = True
    lit = ~(rep & is_rle[d])
    pos = np.flatnonzero(lit)
    lits = d[pos]
    nxt = np.concatenate([pos[1:], [len(d)]])
    runs = [int(nxt[k] - pos[k] - 1) for k in np.flatnonzero(is_rle[lits])]
    return lits.tobytes(), syms, runs


def craft_rle(ora, lits, syms, runs, osz):
    """An RLE stream (order 0x40) with raw meta-data, from the format: `runs`
    holds a run length or the bytes of its varint per RLE-symbol literal."""
    meta = bytes([len(syms) & 0xff]) + bytes(syms)
    meta += b"".join(r if isinstance(r, bytes) else varint(r) for r in runs)
    return (bytes([F_RLE]) + varint(osz) + varint(2 * len(meta) + 1) + varint(len(lits))
            + meta + _plain_body(ora, lits, 0))


@functools.lru_cache(maxsize=None)
def bases():
    """[(name, class, stream, data)] — the undamaged streams."""
    from oracle import binding
    ora = binding.oracle()
    out = []

    def add(name, cls, data, order, want=None, mask=0xff):
        c = ora.rans_compress(data, order)
        if want is not None:
            assert c[0] & mask == want, (name, hex(c[0]), hex(want))
        out.append((name, cls, c, data))
        return c

    for k in (1, 2, 4, 16):
        d = _skew(4099, k, 10 + k, power=4)
        for o in (0x80, 0x81):
            c = add(f"pack{k}/o{o:x}", "pack", d, o, F_PACK, F_PACK)
            assert Walk(c).vals["nsym"] == k, (k, c[:8])
    d = _skew(4099, 17, 27)
    for o in (0, 1):
        # more than 16 symbols: the encoder drops PACK; the decoder's raw
        # "pack" of such a stream is [nsym > 16][packed length = size]
        c = ora.rans_compress(d, o)
        assert c[0] == o
        k = vget(c, 1, len(c))[1]
        out.append((f"pack17/o{0x80 | o:x}", "pack",
                    bytes([0x80 | o]) + c[1:1 + k] + bytes([17]) + varint(len(d)) + c[1 + k:], d))
    for o in (0x40, 0x41):
        c = add(f"rle_raw/o{o:x}", "rle", _runs_raw(5003, 31), o, F_RLE, F_RLE | F_PACK)
        assert Walk(c).vals["um"] & 1
        c = add(f"rle_coded/o{o:x}", "rle", hc._runs(70001, 12, 0.9, 32).tobytes(), o,
                F_RLE, F_RLE | F_PACK)
        assert not Walk(c).vals["um"] & 1
        d = _runs_short(149_990, 33)
        c = add(f"rle_big/o{o:x}", "rle", d, o, F_RLE, F_RLE | F_PACK)
        w = Walk(c)
        assert w.vals["rl"] > RLE_CHUNK and w.vals["um"] // 2 - 7 > RLE_CHUNK
    for o in (0xC0, 0xC1):
        add(f"packrle/o{o:x}", "packrle", hc._runs(70001, 4, 0.9, 34).tobytes(), o,
            F_RLE | F_PACK, F_RLE | F_PACK)
    for N, n in ((4, 21), (4, 1027), (4, 40001), (3, 40001), (150, 40001)):
        d = _skew(n, 24, 40 + N + n % 7)
        for o in (8, 9):
            c = add(f"stripe{N}/{n}/o{o:x}", "stripe", d, (N << 8) | o, F_STRIPE, F_STRIPE)
            assert Walk(c).vals["N"] == N
    add("cat/300", "cat", _skew(300, 30, 50), F_CAT, F_CAT)
    for n in (1027, 70001):
        for o in (4, 5, 0x84):
            add(f"x32/{n}/o{o:x}", "x32", _skew(n, 8, 60 + o), o, o)
    for o in (0x10, 0x11):
        add(f"nosz/o{o:x}", "nosz", _skew(1027, 12, 70), o, o)
    c = add("o1comp/70001", "o1comp", hc.alphabets(70001)["o1_comp_table"].tobytes(), 1, 1)
    assert Walk(c).vals["o1hdr"] & 1                        # the compressed-table bit
    return out


# ---- damage -----------------------------------------------------------------


def _splice(b, a, e, new):
    return b[:a] + new + b[e:]


def _len_values(true, over, top):
    vals = [0, 1, true - 1, true + 1, 2 * true, over]
    out = []
    for v in vals:
        v = min(max(v, 0), top)
        if v != true and v not in out:
            out.append(v)
    return out


def _field_cases(name, b, n):
    """Structured damage of one base: [(case, mutation class, stream)]."""
    w = Walk(b, n)
    V = w.vals
    out = []
    is_stripe = b[0] & F_STRIPE
    ent_n = V.get("plen", V.get("size", n))
    for f, a, e in w.fields:
        true = V.get(f)
        # the first value over the bound each length is checked against: the
        # capacity, the stage's size, or the bytes the stream has left
        if f in ("size", "ulen"):
            vals = _len_values(true, n + 1, CAP_MAX)
        elif f == "plen":
            vals = _len_values(true, V.get("size", n) + 1, CAP_MAX)
        elif f == "rl":
            vals = _len_values(true, ent_n + 1, CAP_MAX)
        elif f == "um":            # the meta-data size, its raw / coded bit kept
            vals = [2 * v + (true & 1) for v in _len_values(true // 2, len(b) - e + 1, LIMIT)]
        elif f == "u":
            vals = _len_values(true, LIMIT, LIMIT)
        elif f in ("cm", "c") or (f.startswith("clen") and
                                  int(f[4:]) in (0, V["N"] // 2, V["N"] - 1)):
            vals = _len_values(true, len(b) - e + 1, CAP_MAX)
        else:
            continue
        for v in vals:
            out.append((f"{name}:{f}={v}", "len", _splice(b, a, e, varint(v))))
    if is_stripe:
        a, e = w.span("N")
        N = V["N"]
        for v in (0, 1, N - 1, N + 1, 255):
            if v != N:
                out.append((f"{name}:N={v}", "stripeN", _splice(b, a, e, bytes([v]))))
    if w.span("nsym"):
        a, e = w.span("nsym")
        for v in (0, 1, 2, 3, 16, 17):
            if v != V["nsym"]:
                out.append((f"{name}:nsym={v}", "nsym", _splice(b, a, e, bytes([v]))))
    if w.span("rle_nsyms"):
        a, e = w.span("rle_nsyms")
        t = V["rle_nsyms"]
        for v in sorted({0, t - 1, t + 1} - {t}):
            out.append((f"{name}:rle_nsyms={v}", "rlesyms", _splice(b, a, e, bytes([v & 0xff]))))
    for bit in (1, F_X32, F_STRIPE, F_NOSZ, F_CAT, F_RLE, F_PACK):
        out.append((f"{name}:order^{bit:#x}", "order", bytes([b[0] ^ bit]) + b[1:]))
    return out


# the chains whose state words are set below 2^15: plain order-0 and order-1,
# 32 states, a stripe's first sub-stream (words of the next one follow it),
# the RLE meta-data's chain and the compressed order-1 table's
STATE_FIELDS = {"nosz/o10": "states", "nosz/o11": "states", "x32/1027/o4": "states",
                "x32/1027/o5": "states", "stripe4/1027/o8": "s0.states",
                "stripe4/40001/o9": "s0.states", "rle_coded/o40": "meta.states",
                "rle_big/o41": "meta.states", "o1comp/70001": "tab.states",
                "packrle/oc1": "tab.states"}


def _state_cases(name, b, n):
    """The first and the last state word set to 0 and to 2^15 - 1: the
    reference refuses a state below 2^15 before it decodes a symbol."""
    f = STATE_FIELDS.get(name)
    if f is None:
        return []
    a, e = Walk(b, n).span(f)
    assert (e - a) in (16, 128), (name, e - a)
    out = []
    for z, at in (("first", a), ("last", e - 4)):
        for v in (0, 0x7fff):
            out.append((f"{name}:{f}.{z}={v:#x}", "state",
                        _splice(b, at, at + 4, v.to_bytes(4, "little"))))
    return out


def _cut_cases(name, b, seed, count):
    if len(b) < 400:
        return [(f"{name}:prefix{k}", "prefix", b[:k]) for k in range(len(b))]
    r = np.random.default_rng(seed)
    cuts = sorted(set(int(x) for x in r.integers(1, len(b), count)))
    return [(f"{name}:cut{k}", "cut", b[:k]) for k in cuts]


def _flip_cases(name, b, n, seed, count):
    """Single-byte flips confined to table bytes, state words and payload."""
    w = Walk(b, n)
    pos = [p for f, a, e in w.fields
           if f.split(".")[-1] in ("table", "states", "payload") for p in range(a, e)]
    r = np.random.default_rng(seed)
    out = []
    for p in sorted(set(int(x) for x in r.choice(pos, min(count, len(pos)), replace=False))):
        m = bytearray(b)
        m[p] ^= int(r.integers(1, 256))
        out.append((f"{name}:flip{p}", "flip", bytes(m)))
    return out


RUN_R = (("exact", None), ("past", None), ("r7fffffff", 0x7fffffff), ("rffffffff", 0xffffffff),
         ("six", b"\x8f\xff\xff\xff\xff\x7f"))


@functools.lru_cache(maxsize=None)
def run_cases():
    """The crafted run-varint cases [(case, "runs", stream, capacity)]: an RLE
    stream with raw meta-data whose last literal is an RLE symbol, its run
    ending exactly at the stored size, one byte past it, and of 2^31 - 1,
    2^32 - 1 and a 6-byte varint; on the small raw base and with that literal
    in the second RLE_CHUNK of literals."""
    from oracle import binding
    ora = binding.oracle()
    out = []
    for tag, data in (("small", _runs_raw(5003, 31)), ("chunk2", _runs_short(149_990, 33))):
        lits, syms, runs = rle_parts(data)
        if tag == "chunk2":                       # cut after a literal of the second chunk
            keep = RLE_CHUNK + 400
            while lits[keep - 1] not in syms:
                keep += 1
            nr = sum(1 for x in lits[:keep] if x in set(syms))
            lits, runs = lits[:keep], runs[:nr]
        assert lits[-1] in syms
        before = len(lits) - 1 + sum(runs[:-1])   # bytes the earlier literals expand to
        osz = before + runs[-1] + 1 + 50
        sound = craft_rle(ora, lits, syms, runs, before + runs[-1] + 1)
        out.append((f"runs/{tag}:sound", "base", sound, before + runs[-1] + 1))
        for name, r in RUN_R:
            if name == "exact":
                r = osz - before - 1
            elif name == "past":
                r = osz - before
            out.append((f"runs/{tag}:{name}", "runs",
                        craft_rle(ora, lits, syms, runs[:-1] + [r], osz), osz))
        # the same runs on the first RLE-symbol literal, with literals after it
        for name, r in RUN_R[2:]:
            out.append((f"runs/{tag}:first_{name}", "runs",
                        craft_rle(ora, lits, syms, [r] + runs[1:], osz), osz))
    return out


def _over(stream, cap):
    """The length fields of a stream over the module's bound: [(name, top)]."""
    out = []
    for k, v in Walk(stream, cap).vals.items():
        f = k.split(".")[-1]
        if f == "u" and v > LIMIT:
            out.append((k, LIMIT))
        elif f == "um" and v // 2 > LIMIT:
            out.append((k, 2 * LIMIT + (v & 1)))
        elif f in ("size", "ulen") and v > CAP_MAX:
            out.append((k, CAP_MAX))
    return out


def bounded(stream, cap):
    """`stream` with every length field over the bound rewritten to the bound
    (damage moves the fields behind it, and a field read from the moved bytes
    can hold anything): how the corpus is bounded by construction."""
    for _ in range(16):
        over = _over(stream, cap)
        if not over:
            break
        a, e = Walk(stream, cap).span(over[0][0])
        stream = _splice(stream, a, e, varint(over[0][1]))
    return stream


def check_bound(stream, cap):
    """The condition every case meets (module docstring)."""
    assert cap <= CAP_MAX, cap
    assert not _over(stream, cap), _over(stream, cap)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(case, mutation class, stream, capacity)], the undamaged bases (class
    "base") first in each group.  Sized for GPU tests of a few seconds, about
    3 000 pairs: every prefix of a stream under 400 bytes, 32 seeded cuts of a
    longer RLE or stripe stream and 12 of another, 64 seeded flips per class
    of base spread over its streams, crafted state words (STATE_FIELDS),
    the three capacities for the undamaged streams, and of a stripe's
    sub-stream lengths the first, the middle and the last."""
    out = []
    flips = {}
    for i, (name, cls, b, data) in enumerate(bases()):
        n = len(data)
        out.append((f"{name}:base", "base", b, n))
        for cap in (n - 1, n + 7) if not b[0] & F_NOSZ else (n - 1, n + 1):
            out.append((f"{name}:cap{cap}", "cap", b, cap))
        ncut = 32 if cls in ("rle", "packrle", "stripe") else 12
        for case, mc, s in (_field_cases(name, b, n) + _state_cases(name, b, n)
                            + _cut_cases(name, b, 500 + i, ncut)):
            out.append((case, mc, bounded(s, n), n))
        flips.setdefault(cls, []).append((name, b, n, 700 + i))
    for cls, group in flips.items():             # 64 flips per class of base
        per = -(-64 // len(group))
        for name, b, n, seed in group:
            for case, mc, s in _flip_cases(name, b, n, seed, per):
                out.append((case, mc, s, n))
    out += run_cases()
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    for case, mc, s, cap in out:
        check_bound(s, cap)
    return out


def base_of(case):
    return case.split(":")[0]


def md5(b):
    return hashlib.md5(b).hexdigest()
