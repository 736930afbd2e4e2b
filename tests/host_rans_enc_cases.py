"""Inputs and a model for the tests of the encoder's bare rANS 4x16 chains on
host cores (test_host_rans_enc.py, test_host_rans_enc_gpu.py): seeded data of
every size and alphabet, frequency tables from the format alone, a parser of
the tables in the reference's streams, and a pure-Python model of the chain
(the textbook rANS step, no reciprocals) that gives the checkpoints the
kernels leave in EncJob::ck.  Computed once per process."""
import functools

import numpy as np

from host_rans_cases import _normalise

# every n % 4, one step either side of a 256-step chunk boundary (order-0: 1024
# symbols a chunk; order-1: 256 a quarter), a final chunk holding one step, an
# order-1 tail that lives only in state 3
SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 2, 70001)
LOW = 1 << 15
CHUNK = 256
PLAIN = 0x11                     # order bits of a plain entropy stream: order-1, NOSZ


def alphabets(n):
    """name -> n seeded bytes: one symbol (f = 4096), two, skewed ACGTN, all 256
    symbols, and one symbol with a single other byte (frequency 1 from 4097
    bytes on)."""
    rng = np.random.default_rng(2000 + n)
    rare = np.full(n, 65, np.uint8)
    rare[n // 2] = 66
    return {
        "one": np.full(n, 65, np.uint8),
        "two": rng.choice(np.array([3, 200], np.uint8), n, p=[.9, .1]),
        "acgtn": np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, n, p=[.4, .3, .15, .1, .05])],
        "all256": np.concatenate([np.arange(256, dtype=np.uint8),
                                  np.minimum(rng.geometric(0.03, n) - 1, 255).astype(np.uint8)])[:n],
        "rare": rare,
    }


# ---- the events of a chain: (step, state, context, symbol) ------------------

def steps_of(n, order):
    return n - 3 * (n // 4) if order else (n + 3) // 4


def events(data, order):
    """Per step k (ascending) the (state, context, symbol) it codes."""
    n = len(data)
    T = steps_of(n, order)
    out = [[] for _ in range(T)]
    if order == 0:
        for i in range(n):
            out[i // 4].append((i % 4, 0, data[i]))
    else:
        isz = n // 4
        for z in range(4):
            a = z * isz
            b = a + isz if z < 3 else n
            for i in range(a, b):
                out[i - a].append((z, data[i - 1] if i > a else 0, data[i]))
    return out


# ---- tables -----------------------------------------------------------------

def table_of(data, order, bits):
    """The frequencies of `data` normalised from the format alone (not the
    reference's normaliser): order 0 -> [256]; order 1 -> [256 * 256], row =
    context byte."""
    if order == 0:
        return _normalise(np.bincount(np.frombuffer(bytes(data), np.uint8), minlength=256), 1 << bits)
    cnt = {}
    for ev in events(data, 1):
        for z, c, s in ev:
            cnt.setdefault(c, [0] * 256)[s] += 1
    flat = [0] * 65536
    for c, row in cnt.items():
        flat[c * 256:(c + 1) * 256] = _normalise(row, 1 << bits)
    return flat


def _varint(b, p):
    v = 0
    while True:
        c = b[p]
        p += 1
        v = (v << 7) | (c & 0x7f)
        if not c & 0x80:
            return v, p


def _alphabet(b, p):
    present = [False] * 256
    s, run = b[p], 0
    p += 1
    while True:
        present[s] = True
        if run:
            run -= 1
            s += 1
        elif b[p] == s + 1:
            s, run = b[p], b[p + 1]
            p += 2
        else:
            s = b[p]
            p += 1
        if not s:
            return present, p


def _shift_to(row, total):
    t = sum(row)
    while t and t < total:
        row = [2 * f for f in row]
        t *= 2
    return row


def _freq0(b, p):
    present, p = _alphabet(b, p)
    row = [0] * 256
    for s in range(256):
        if present[s]:
            row[s], p = _varint(b, p)
    return _shift_to(row, 4096), p


def parse_plain(comp, order, o0_decode=None):
    """(bits, table as table_of gives it, the payload) of a reference stream
    that is a plain order-`order` entropy stream, else None (stored uncoded, or
    coded at another order).  o0_decode(stream, size) decodes the order-0
    stream of a compressed order-1 table."""
    if comp[0] & ~PLAIN or (comp[0] & 1) != order:
        return None
    p = 1
    if not comp[0] & 0x10:
        _, p = _varint(comp, p)
    if order == 0:
        row, p = _freq0(comp, p)
        return 12, row, comp[p:]
    bits = comp[p] >> 4
    if comp[p] & 1:
        u, q = _varint(comp, p + 1)
        c, q = _varint(comp, q)
        tab = o0_decode(bytes([0x10]) + comp[q:q + c], u)
        end = q + c
    else:
        tab, end = comp[p + 1:], None
    present, q = _alphabet(tab, 0)
    flat = [0] * 65536
    for ctx in range(256):
        if not present[ctx]:
            continue
        row, zrun = [0] * 256, 0
        for s in range(256):
            if not present[s]:
                continue
            if zrun:
                zrun -= 1
                continue
            row[s], q = _varint(tab, q)
            if not row[s]:
                zrun = tab[q]
                q += 1
        flat[ctx * 256:(ctx + 1) * 256] = _shift_to(row, 1 << bits)
    if end is None:
        end = p + 1 + q
    return bits, flat, comp[end:]


# ---- the model --------------------------------------------------------------

def model(data, order, bits, table):
    """The checkpoints of the bare chain: four states before every chunk of
    256 steps from the top step down, the first RANS_LOW, the last the final
    states.  The step is the format's: a state at or above ((L >> bits) << 16)
    * f drops its low word, then x = (x // f << bits) + x % f + start."""
    ev = events(data, order)
    starts = {}
    x = [LOW] * 4
    ck = list(x)
    for k in range(len(ev) - 1, -1, -1):
        for z, c, s in ev[k]:
            row = table[c * 256:(c + 1) * 256] if order else table
            f = row[s]
            if (c, s) not in starts:
                starts[c, s] = sum(row[:s])
            if x[z] >= ((LOW >> bits) << 16) * f:
                x[z] >>= 16
            x[z] = ((x[z] // f) << bits) + x[z] % f + starts[c, s]
        if k % CHUNK == 0:
            ck += x
    return ck


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data, order, bits, table, checkpoints of the model)] over every
    size and alphabet: order 0, and order 1 with 10 and 12 bits."""
    out = []
    for n in SIZES:
        for name, d in alphabets(n).items():
            d = d.tobytes()
            for order, bits in ((0, 12), (1, 10), (1, 12)):
                t = table_of(d, order, bits)
                out.append((f"{name}/{n}/o{order}b{bits}", d, order, bits, t, model(d, order, bits, t)))
    return out
