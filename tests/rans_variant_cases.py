"""Inputs that select every body of the rANS chain kernels
(test_rans_variant_cases.py, test_rans_variants_gpu.py).

k_rans_dec picks its body from (order, NX, table rows, table shift, symbol
count) and the encoder its chain kernel from (order, NX, alphabet size); the
lengths below sit on the bodies' group, chunk and ring constants, not on any
workload's sizes.  Nothing is generated at import: data(case) and
stream(case) compute on first use and keep the result for the process.

Kinds of data over an alphabet of A distinct byte values (byte 0 among them,
as the order-1 table always has a row for it, so rows == A once n >= A):
  flat   independent, uniform
  skew   independent, Dirichlet(0.4) probabilities
  walk   the alphabet index moves on by a uniform step of 0..3: four equally
         likely successors per context, so an order-1 table of any A rows
         pays, and the reference's cost estimate keeps 10-bit frequencies
  runs   long runs (a switch every ~1000 bytes): successors rarer than
         1/1024, for which the estimate picks 12-bit frequencies
Every kind starts with a permutation of the alphabet so that all A symbols
occur."""
import functools
from collections import Counter, namedtuple

import numpy as np

ALPHABETS = (*range(1, 13), 16, 17, *range(32, 39), *range(63, 67), *range(95, 99),
             128, 200, 256)
LENGTHS = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65,          # tails and tiny
           1023, 1024, 1025, 1027,                         # dec4_body G = 256 x 4, X32 G = 32 x 32
           2047, 2048, 2049, 2051,                         # lean decoder G = 512 x 4
           4097, 40003, 70001)                             # the 4096-word ring once and twice
ALPHABET_LENGTHS = (1025, 4097, 40003)
ORDERS = (0, 1, 4, 5)                # bit 0: order-1, bit 2: 32 states (X32)
KINDS = ("flat", "skew", "walk", "runs")

Case = namedtuple("Case", "A kind n order")

# One input per decoder body and per encoder chain (A, kind, order), run at
# every length of LENGTHS; the body named is the one its n = 40003 stream
# selects (asserted from the oracle's stream in test_rans_variant_cases.py).
# Lengths up to 1000 lose X32 in the reference, and short ones change the
# table's rows or are stored uncoded: dec_jobs() says what each one selects.
DEC_CLASS_INPUT = {
    **{f"O0_REG{k}": (k, "skew", 0) for k in range(1, 9)},
    "O0_LEAN": (9, "skew", 0),
    "O1_LEAN": (4, "skew", 1),
    "O1_LDS": (16, "walk", 1),
    "O1_SPLIT": (64, "walk", 1),
    "O1_GLOBAL": (128, "walk", 1),
    "X32_O0": (9, "skew", 4),
    "X32_O1_LDS": (16, "walk", 5),
    "X32_O1_SPLIT": (64, "walk", 5),
    "X32_O1_GLOBAL": (128, "walk", 5),
}
ENC_CLASS_INPUT = {
    "E2W_O0": (9, "skew", 0),
    "E2W_O1": (64, "walk", 1),
    "E1W_O1_COMPACT": (65, "walk", 1),
    "E32_O0": (9, "skew", 4),
    "E32_O1": (64, "walk", 5),
    "E32_O1_COMPACT": (65, "walk", 5),
}
CLASS_N = 40003                      # the length of a class's own case

# The order-1 decoder's table placement by (rows, shift), kernels.h:129-153
# (DEC_TAB_LDS_MAX, dec_tab_words, DEC_LEAN_ENTRIES, dec_lean, dec_table_mode):
# the last row count of the lean body (NX = 4 only), of the LDS table and of
# the SPLIT table.
O1_LAST_ROWS = {12: (2, 9, 33), 10: (8, 36, 96)}
# (rows, shift) on both sides of every change of the order-1 decoder's body
# or table placement, kernels.h:129-153 (DEC_TAB_LDS_MAX = 147456 bytes,
# DEC_LEAN_ENTRIES = 8192, dec_tab_words, dec_lean, dec_table_mode), and the
# body each side runs with 4 states.  With 32 states there is no lean body:
# X32_O1_LDS on both sides of the first threshold of a shift (x32_name).
THRESHOLDS = [
    ((2, 12), "O1_LEAN"), ((3, 12), "O1_LDS"),        # 2 << 12 = 8192 entries | 3 << 12
    ((9, 12), "O1_LDS"), ((10, 12), "O1_SPLIT"),      # 9 * 16384 = 147456 bytes | 163840
    ((33, 12), "O1_SPLIT"), ((34, 12), "O1_GLOBAL"),  # 135168 + 33 * 256 = 143616 | 147968
    ((8, 10), "O1_LEAN"), ((9, 10), "O1_LDS"),        # 8 << 10 = 8192 entries | 9 << 10
    ((36, 10), "O1_LDS"), ((37, 10), "O1_SPLIT"),     # 36 * 4096 = 147456 bytes | 151552
    ((96, 10), "O1_SPLIT"), ((97, 10), "O1_GLOBAL"),  # 98304 + 96 * 512 = 147456 | 148992
]


def x32_name(name: str) -> str:
    return "X32_" + ("O1_LDS" if name == "O1_LEAN" else name)


# the encoder's order-1 table: 16-byte entries in LDS up to A = 64, compact beyond
ENC_LDS_LAST_A = 64


def symbols(A: int) -> np.ndarray:
    """A distinct byte values, byte 0 first."""
    rng = np.random.default_rng(5000 + A)
    return np.concatenate([[0], rng.choice(np.arange(1, 256), A - 1, replace=False)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def data(A: int, kind: str, n: int, seed: int = 0) -> bytes:
    """The case table's inputs have seed 0; other seeds give further inputs
    of the same kind (the hedged batches)."""
    rng = np.random.default_rng([A, KINDS.index(kind), n] + ([seed] if seed else []))
    if kind == "flat":
        idx = rng.integers(0, A, n)
    elif kind == "skew":
        idx = rng.choice(A, n, p=rng.dirichlet(np.full(A, 0.4)))
    elif kind == "walk":
        idx = np.cumsum(rng.integers(0, 4, n)) % A
    else:
        switch = rng.random(n) > (0.999 if A > 5 else 0.995)
        pick = rng.integers(0, A, n)
        idx = pick[np.maximum.accumulate(np.where(switch, np.arange(n), 0))] if n else pick
    head = rng.permutation(A)[:n]
    idx[:len(head)] = head
    return symbols(A)[idx].tobytes()


def class_cases():
    """Every decoder and encoder class's input at every length."""
    seen, out = set(), []
    for A, kind, order in (*DEC_CLASS_INPUT.values(), *ENC_CLASS_INPUT.values()):
        for n in LENGTHS:
            c = Case(A, kind, n, order)
            if c not in seen:
                seen.add(c)
                out.append(c)
    return out


def alphabet_cases():
    """Every alphabet at three lengths, flat and skewed, and for the order-1
    table's shift a long walk and a long run input, at every order."""
    out = []
    for A in ALPHABETS:
        for order in ORDERS:
            for kind in ("flat", "skew"):
                out += [Case(A, kind, n, order) for n in ALPHABET_LENGTHS]
            if order & 1:
                out += [Case(A, "walk", CLASS_N, order), Case(A, "runs", CLASS_N, order)]
    return out


def transform_cases():
    """RLE (64), PACK (128) and both in front of order-1: a small subset (the
    transforms have their own tests)."""
    return [Case(A, kind, n, order) for order in (65, 129, 193)
            for A, kind in ((4, "runs"), (16, "skew")) for n in (1025, 40003)]


def ring_cases():
    """Payloads that pass the decoders' 4096-word ring twice and more: 70001
    flat bytes of 4 symbols (2 bits each, 8750 words) and of 200."""
    return [Case(A, "flat", 70001, order) for A in (4, 200) for order in ORDERS]


def all_cases():
    seen, out = set(), []
    for c in (*class_cases(), *alphabet_cases(), *ring_cases()):
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def stream(c: Case) -> bytes:
    """The oracle's stream of a case."""
    from oracle import binding
    return binding.oracle().rans_compress(data(c.A, c.kind, c.n), c.order)


# ---- reading a bare stream's header (the layout rans_format.hpp parses) -----

def _varint(b, p):
    v = 0
    while True:
        c = b[p]
        p += 1
        v = v << 7 | (c & 0x7f)
        if not c & 0x80:
            return v, p


def _alphabet(b, p):
    """The symbols of a run-length coded alphabet and the position after it."""
    syms, rle = [], 0
    j = b[p]
    p += 1
    while True:
        syms.append(j)
        if not rle and j + 1 == b[p]:
            j, rle = b[p], b[p + 1]
            p += 2
        elif rle:
            rle -= 1
            j += 1
        else:
            j = b[p]
            p += 1
        if not j:
            return syms, p


def _bare(s):
    """(order byte, uncompressed size, position of the frequency table) of a
    stream with a size and none of the transforms; None if it is stored."""
    assert not s[0] & (0x08 | 0x10 | 0x40 | 0x80), hex(s[0])
    n, p = _varint(s, 1)
    return None if s[0] & 0x20 else (s[0], n, p)


def o1_rows_bits(s: bytes):
    """(rows, shift, table compressed) of an order-1 / order-5 stream: the
    context rows of its frequency table and the shift nibble of its header
    byte shift << 4 | compressed."""
    order, _, p = _bare(s)
    assert order & 1
    bits, comp = s[p] >> 4, s[p] & 1
    if not comp:
        return len(_alphabet(s, p + 1)[0]), bits, False
    return len(_alphabet(_o1_table(s, p)[0], 0)[0]), bits, True


def _o1_table(s, p):
    """A compressed order-1 table, uncompressed by the oracle: it is a bare
    order-0 payload of `u` bytes in `c`."""
    from oracle import binding
    u, q = _varint(s, p + 1)
    c, q = _varint(s, q)
    size = bytearray()
    v = u
    while True:
        size.insert(0, (v & 0x7f) | (0x80 if size else 0))
        v >>= 7
        if not v:
            break
    inner = bytes([0]) + bytes(size) + s[q:q + c]
    tab = binding.oracle().rans_uncompress(inner)
    assert len(tab) == u
    return tab, inner


def _o0_class(s, p):
    k = len(_alphabet(s, p)[0])
    return f"O0_REG{k}" if k <= 8 else "O0_LEAN"


def dec_jobs(s: bytes) -> list:
    """The decoder bodies a bare stream runs, by name: its own, and for an
    order-1 stream with a compressed table the order-0 NX = 4 chain that
    uncompresses the table.  [] for an empty or stored stream."""
    hdr = _bare(s)
    if hdr is None or not hdr[1]:
        return []
    order, _, p = hdr
    x32 = bool(order & 4)
    if not order & 1:
        return ["X32_O0" if x32 else _o0_class(s, p)]
    bits, comp = s[p] >> 4, s[p] & 1
    out = []
    if comp:
        tab, inner = _o1_table(s, p)
        rows = len(_alphabet(tab, 0)[0])
        out = dec_jobs(inner)
    else:
        rows = len(_alphabet(s, p + 1)[0])
    lean, lds, split = O1_LAST_ROWS[bits]
    if rows <= lean and not x32:
        name = "O1_LEAN"
    else:
        name = "O1_LDS" if rows <= lds else "O1_SPLIT" if rows <= split else "O1_GLOBAL"
        if x32:
            name = "X32_" + name
    return [name] + out


def enc_job(c: Case):
    """The encoder chain a bare case runs, by name (None: no chain).  The
    reference codes inputs of up to 1000 bytes with 4 states, order-1 inputs
    of under 8 bytes as order-0, and the order-1 alphabet has byte 0."""
    d = data(c.A, c.kind, c.n)
    if not d:
        return None
    x32 = bool(c.order & 4) and len(d) > 1000
    if not c.order & 1 or len(d) < 8:
        return "E32_O0" if x32 else "E2W_O0"
    A = len(set(d) | {0})
    if A <= ENC_LDS_LAST_A:
        return "E32_O1" if x32 else "E2W_O1"
    return "E32_O1_COMPACT" if x32 else "E1W_O1_COMPACT"


@functools.lru_cache(maxsize=None)
def o1_pairs() -> dict:
    """(states, rows, shift) -> the cases of all_cases() whose order-1
    stream has them."""
    out = {}
    for c in all_cases():
        s = stream(c)
        if c.order & 1 and c.n and s[0] & 1 and not s[0] & 0x20:
            rows, bits, _ = o1_rows_bits(s)
            out.setdefault((32 if s[0] & 4 else 4, rows, bits), []).append(c)
    return out


def dec_count(cases) -> Counter:
    out = Counter()
    for c in cases:
        out.update(dec_jobs(stream(c)))
    return out
