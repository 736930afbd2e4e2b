"""Streams for the host rANS 4x16 decoder tests (test_host_rans.py,
test_host_rans_gpu.py): the oracle's streams of seeded data, hand-coded tiny
entropy streams (the encoder stores inputs that small uncoded), and damaged
copies.  Computed once per process."""
import functools

import numpy as np

SIZES = (0, 1, 3, 4, 5, 7, 1023, 1027, 70001)
PLAIN = 0x11                     # order bits of a plain entropy stream: order-1, NOSZ


def _runs(n, k, stay, seed, base=40):
    r = np.random.default_rng(seed)
    if not n:
        return np.zeros(0, np.uint8)
    sw = r.random(n) > stay
    sym = r.integers(0, k, n)
    idx = np.maximum.accumulate(np.where(sw, np.arange(n), 0))
    return (sym[idx] + base).astype(np.uint8)


def _markov(n, k, seed, conc):
    r = np.random.default_rng(seed)
    cs = r.dirichlet(np.full(k, conc), k).cumsum(1)
    u = r.random(n)
    out = np.zeros(n, np.uint8)
    s = 0
    for i in range(n):
        s = min(int(np.searchsorted(cs[s], u[i])), k - 1)
        out[i] = s
    return out


def alphabets(n):
    """name -> n seeded bytes: one symbol, two, skewed ACGTN, all 256 symbols,
    order-1 data for TF_SHIFT 10 (an 8-state chain), for 12 (long runs of 16
    symbols) and for a compressed table (a 40-state chain)."""
    rng = np.random.default_rng(1000 + n)
    return {
        "one": np.full(n, 65, np.uint8),
        "two": rng.choice(np.array([3, 200], np.uint8), n, p=[.9, .1]),
        "acgtn": np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, n, p=[.4, .3, .15, .1, .05])],
        "all256": np.concatenate([np.arange(256, dtype=np.uint8),
                                  np.minimum(rng.geometric(0.03, n) - 1, 255).astype(np.uint8)])[:n]
        if n else np.zeros(0, np.uint8),
        "o1_shift10": _markov(n, 8, 1, 0.3),
        "o1_shift12": _runs(n, 16, 0.999, 5),
        "o1_comp_table": _markov(n, 40, 2, 0.1),
    }


def o1_header(comp):
    """(shift, compressed table) of an order-1 stream with a size."""
    p = 1
    while comp[p] & 0x80:
        p += 1
    return comp[p + 1] >> 4, comp[p + 1] & 1


# ---- a tiny encoder of plain 4x16 streams, from the format alone ------------

def _varint(v):
    out = [v & 0x7f]
    v >>= 7
    while v:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    return bytes(reversed(out))


def _alphabet(present):
    out, s = bytearray(), 0
    while s < 256:
        if present[s]:
            out.append(s)
            if s and present[s - 1]:
                e = s + 1
                while e < 256 and present[e]:
                    e += 1
                out.append(e - s - 1)
                s = e - 1
        s += 1
    out.append(0)
    return bytes(out)


def _normalise(cnt, total):
    """Counts to frequencies of sum `total`, every present symbol >= 1."""
    cnt = [int(c) for c in cnt]
    n = sum(cnt)
    f = [max(1, c * total // n) if c else 0 for c in cnt]
    top = max(range(256), key=lambda s: f[s])
    f[top] += total - sum(f)
    assert f[top] > 0
    return f


def craft(data: bytes, order: int, bits: int = 12) -> bytes:
    """A plain order-0 (bits 12) or order-1 (bits 10 or 12) stream of `data`."""
    n = len(data)
    assert n > 0
    isz = n // 4
    if order == 0:
        rows = {0: _normalise(np.bincount(np.frombuffer(data, np.uint8), minlength=256), 4096)}
        events = [(i % 4, 0, data[i]) for i in range(n)]
        present = [x > 0 for x in rows[0]]
        table = _alphabet(present) + b"".join(_varint(rows[0][s]) for s in range(256) if present[s])
        bits = 12
    else:
        lane = [(z * isz, (z + 1) * isz if z < 3 else n) for z in range(4)]
        cnt = {}
        ctx_of = {}
        for z, (a, b) in enumerate(lane):
            c = 0
            for i in range(a, b):
                cnt.setdefault(c, [0] * 256)[data[i]] += 1
                ctx_of[i] = c
                c = data[i]
        present = [False] * 256
        present[0] = True
        for b in data:
            present[b] = True
        rows = {c: _normalise(v, 1 << bits) for c, v in cnt.items()}
        table = bytearray([bits << 4]) + _alphabet(present)
        for c in range(256):
            if not present[c]:
                continue
            row, zrun = rows.get(c, [0] * 256), 0
            for s in range(256):
                if not present[s]:
                    continue
                if not row[s]:
                    zrun += 1
                    continue
                if zrun:
                    table += bytes([0, zrun - 1])
                    zrun = 0
                table += _varint(row[s])
            if zrun:
                table += bytes([0, zrun - 1])
        table = bytes(table)
        events = []
        for t in range(n - 3 * isz):
            for z in range(4):
                i = lane[z][0] + t
                if i < lane[z][1]:
                    events.append((z, ctx_of[i], data[i]))
    x = [1 << 15] * 4
    words = []
    for z, c, s in reversed(events):
        f = rows[c][s]
        start = sum(rows[c][:s])
        if x[z] >= ((1 << 15 >> bits) << 16) * f:
            words.append(x[z] & 0xffff)
            x[z] >>= 16
        x[z] = ((x[z] // f) << bits) + x[z] % f + start
    body = b"".join(v.to_bytes(4, "little") for v in x)
    body += b"".join(w.to_bytes(2, "little") for w in reversed(words))
    return bytes([order]) + _varint(n) + table + body


@functools.lru_cache(maxsize=None)
def streams():
    """[(name, stream, data or None)]: None where the decoder must refuse the
    stream (the encoder stored it uncoded: an order byte beyond order-1 and
    NOSZ).  The oracle's streams of every alphabet at every size, orders 0 and
    1, then hand-coded entropy streams of the small sizes."""
    from oracle import binding
    ora = binding.oracle()
    out = []
    for n in SIZES:
        for name, d in alphabets(n).items():
            d = d.tobytes()
            for o in (0, 1):
                c = ora.rans_compress(d, o)
                out.append((f"{name}/{n}/o{o}", c, d if not (c[0] & ~PLAIN) else None))
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 4, 5, 6, 7, 9, 30):
        for name, d in (("one", bytes([65]) * n), ("two", bytes(rng.choice([3, 200], n))),
                        ("acgtn", bytes(rng.choice(list(b"ACGTN"), n))),
                        ("zero", bytes(rng.choice([0, 1, 2], n)))):
            out.append((f"craft/{name}/{n}/o0", craft(d, 0), d))
            out.append((f"craft/{name}/{n}/o1s10", craft(d, 1, 10), d))
            out.append((f"craft/{name}/{n}/o1s12", craft(d, 1, 12), d))
    return out


@functools.lru_cache(maxsize=None)
def small_pair():
    """One small order-0 and one small order-1 stream (the oracle's, skewed
    ACGTN, 1027 bytes) for the damage tests."""
    from oracle import binding
    d = alphabets(1027)["acgtn"].tobytes()
    ora = binding.oracle()
    return [(ora.rans_compress(d, o), d) for o in (0, 1)]


def damaged(comp: bytes, order: int):
    """Every prefix of the stream, then a byte flipped at 64 seeded positions."""
    out = [comp[:k] for k in range(len(comp))]
    rng = np.random.default_rng(900 + order)
    for pos in rng.integers(0, len(comp), 64):
        b = bytearray(comp)
        b[int(pos)] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out
