"""Seeded fqzcomp_qual blocks coded with caller-supplied parameters, with
reversal (vers 3) and with empty records: the paths of the codec that
fqz_pick_parameters never takes (it always makes one parameter block).

Inputs are regenerated, not stored.  Parameter sets are written by hand and
fill every field compress_block_fqz2f / fqz_store_parameters read
(htscodecs/fqzcomp_qual.c:707-769, :1008-1247): the caller's tables are the
unshifted ones fqz_pick_parameters would build (:950-975); a call shifts
them in place, so every call gets a fresh block from Case.gp().

Per case: `var` names the general decoder's variant of launch_group
(4 * two model registers + 2 * sequence context + 1 * one shared qtab),
`small` the small decoder's variant where the stream is eligible for it
(8, or 9 with delta terms), `fix` the fix-up kernels its decode runs and
`enc` the encoder that takes it.
"""
from __future__ import annotations

import hashlib

import numpy as np

from fqz_cases import ILLUMINA8, NOVA4
from fqzcomp5_amd.lib import fqz_gparams, fqz_gparams_state

GF_MULTI, GF_STAB, GF_REV, GF_SEQ = 1, 2, 4, 8
PF_DEDUP, PF_LEN, PF_SEL, PF_QMAP, PF_PTAB, PF_DTAB, PF_QTAB = 2, 4, 8, 16, 32, 64, 128
F_REVERSE = 16
INT_MAX = 2**31 - 1
DSQR = ([0] + [1] * 3 + [2] * 5 + [3] * 7 + [4] * 9 + [5] * 11 + [6] * 13 + [7] * 15)


def block(qbits=0, qshift=0, qloc=0, pbits=0, pshift=0, ploc=0, dbits=0, dshift=0, dloc=0,
          sloc=0, bbits=0, bloc=0, boff=0, sel=0, dedup=0, fixed=0, qtab=None, alphabet=None,
          max_sym=0, max_sel=0, context=0):
    """One fqz_param as a dict of its fields.  alphabet: store a qmap of these
    values (max_sym = nsym = their count); qtab: a custom table."""
    b = dict(context=context, do_sel=sel, do_dedup=dedup, fixed_len=fixed,
             qbits=qbits, qshift=qshift, qloc=qloc, pbits=pbits, pshift=pshift, ploc=ploc,
             dbits=dbits, dshift=dshift, dloc=dloc, sloc=sloc, bbits=bbits, bloc=bloc, boff=boff,
             qmask=(1 << qbits) - 1, max_sel=max_sel,
             use_qtab=int(qtab is not None), use_ptab=int(pbits > 0), use_dtab=int(dbits > 0),
             store_qmap=int(alphabet is not None))
    if alphabet is not None:
        qmap = [INT_MAX] * 256
        for j, s in enumerate(sorted(int(x) for x in alphabet)):
            qmap[s] = j
        b.update(qmap=qmap, max_sym=len(alphabet), nsym=len(alphabet))
    else:
        b.update(qmap=list(range(256)), max_sym=max_sym, nsym=255)
    b["qtab"] = list(qtab) if qtab is not None else list(range(256))
    cap = (1 << pbits) - 1
    b["ptab"] = [min(k >> pshift, cap) for k in range(1024)] if pbits else [0] * 1024
    dcap = (1 << dbits) - 1
    b["dtab"] = ([min(DSQR[min(k >> dshift, 63)], dcap) for k in range(256)] if dbits
                 else [0] * 256)
    b["pflags"] = ((PF_QTAB if qtab is not None else 0) | (PF_DTAB if dbits else 0) |
                   (PF_PTAB if pbits else 0) | (PF_SEL if sel else 0) | (PF_LEN if fixed else 0) |
                   (PF_DEDUP if dedup else 0) | (PF_QMAP if alphabet is not None else 0))
    return b


class Case:
    def __init__(self, name, q, lens, flags, seq=None, gflags=0, blocks=None, max_sel=0,
                 stab=None, vers=4, strats=(0,), var=None, small=None, fix=(), enc="serial",
                 decodes=True, gpu=True):
        self.name, self.q, self.seq = name, q, seq
        self.lens = np.asarray(lens, np.uint32)
        self.flags = np.asarray(flags, np.uint32)
        self.gflags, self.blocks, self.max_sel, self.stab = gflags, blocks, max_sel, stab
        self.vers, self.strats = vers, strats
        self.var, self.small, self.fix, self.enc = var, small, tuple(fix), enc
        # decodes: the reference reads its own stream; gpu: the GPU codec
        # takes these parameters (the host decoder takes every stream)
        self.decodes, self.gpu = decodes, gpu

    def gp(self):
        """A fresh caller block (None: the codec picks its parameters)."""
        if self.blocks is None:
            return None
        stab = None
        if self.stab is not None:
            stab = list(self.stab) + [self.stab[-1]] * (256 - len(self.stab))
        return fqz_gparams(self.gflags, self.blocks, self.max_sel, stab)


def gp_digest(gp):
    """md5 of what a call left in the caller's block: gflags, each block's
    bbits / bloc and its shifted position and delta tables (None: no block)."""
    if gp is None:
        return None
    st = fqz_gparams_state(gp)
    words = [st["gflags"]]
    for b in st["blocks"]:
        words += [b["bbits"], b["bloc"]] + b["ptab"] + b["dtab"]
    return hashlib.md5(np.asarray(words, np.uint32).tobytes()).hexdigest()


def _walk(rng, n, lo, hi):
    return (np.cumsum(rng.integers(-3, 4, n)) % (hi - lo + 1) + lo).astype(np.uint8)


def _hifi(rng, n):
    return np.where(rng.random(n) < 0.6, 93, rng.integers(0, 93, n)).astype(np.uint8)


def _seq(rng, n):
    return np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, int(n))].tobytes()


def _cat(recs):
    return np.concatenate(recs).tobytes() if recs else b""


COARSE = [s // 4 for s in range(256)]
HIFI_TAB = []
_v = 0
for _s in range(256):
    if _s in (93, 94) or _s % 16 == 0:
        _v += 1
    HIFI_TAB.append(_v)


def two_qtab(rng, nrec, rlen, wide=False, seq=False, name=None, alphabets=None):
    """GF_MULTI | GF_STAB, two blocks whose qtabs differ; selectors 0 and 2
    alternate and sit in the context at sloc.  (The table is 0,0,1,1,...: a
    run of exactly 255 equal entries at its end, as in 0,1,1,..., is stored
    with a byte that read_array never takes, fqzcomp_qual.c:111-199, so the
    reference cannot read its own stream.)"""
    if alphabets:
        recs = [rng.choice(alphabets[r & 1], rlen).astype(np.uint8) for r in range(nrec)]
    elif wide:
        recs = [_hifi(rng, rlen) for _ in range(nrec)]
    else:
        recs = [_walk(rng, rlen, 2, 41) for _ in range(nrec)]
    top = 93 if wide else 41
    a0, a1 = alphabets if alphabets else (None, None)
    if seq:
        b0 = block(qbits=8, qshift=4, pbits=4, pshift=3, ploc=8, dbits=2, dshift=1, dloc=12,
                   sloc=14, sel=1, max_sym=top, max_sel=2, alphabet=a0)
        b1 = block(qbits=9, qshift=3, bbits=6, bloc=9, boff=2, sloc=14, sel=1, max_sym=top,
                   max_sel=2, qtab=HIFI_TAB if wide else COARSE, alphabet=a1)
    else:
        b0 = block(qbits=8, qshift=4, pbits=4, pshift=3, ploc=8, dbits=2, dshift=1, dloc=12,
                   sloc=14, sel=1, max_sym=top, max_sel=2, alphabet=a0)
        b1 = block(qbits=9, qshift=3, pbits=3, pshift=4, ploc=9, dbits=2, dshift=2, dloc=12,
                   sloc=14, sel=1, max_sym=top, max_sel=2, qtab=HIFI_TAB if wide else COARSE,
                   alphabet=a1)
    lens = [rlen] * nrec
    return Case(name or ("wide_" if wide else "") + "two_qtab" + ("_seq" if seq else ""),
                _cat(recs), lens, [(r & 1) << 17 for r in range(nrec)],
                _seq(rng, sum(lens)) if seq else None, GF_MULTI | GF_STAB, [b0, b1], 2, [0, 0, 1],
                var=(4 if wide else 0) + (2 if seq else 0), fix=("map_recs",) if alphabets else ())


def two_qmap(rng, nrec=500, rlen=100):
    """Two blocks with different stored qmaps, qtab the identity: at most 9
    live symbols, so the small decoder takes it (no delta terms: variant 8)."""
    recs = [rng.choice(ILLUMINA8 if r % 3 == 1 else NOVA4, rlen).astype(np.uint8)
            for r in range(nrec)]
    kw = dict(qbits=9, qshift=3, pbits=4, pshift=3, ploc=9, sloc=13, sel=1, max_sel=2)
    return Case("two_qmap", _cat(recs), [rlen] * nrec,
                [(2 if r % 3 == 1 else 0) << 16 for r in range(nrec)], None,
                GF_MULTI | GF_STAB, [block(alphabet=NOVA4, **kw), block(alphabet=ILLUMINA8, **kw)],
                2, [0, 0, 1], var=1, small=8, fix=("map_recs",))


def one_block(rng):
    """One caller-supplied block without GF_MULTI: the parallel encoder with
    caller parameters, a stored qmap over the whole block, duplicates."""
    recs = [rng.choice(NOVA4, 75, p=[.01, .04, .10, .85]).astype(np.uint8) for _ in range(600)]
    for r in range(1, 600, 4):
        recs[r] = recs[r - 1].copy()
    b = block(qbits=8, qshift=2, pbits=5, pshift=2, ploc=8, dbits=2, dshift=1, dloc=13,
              dedup=1, fixed=1, alphabet=NOVA4)
    return Case("one_block", _cat(recs), [75] * 600, [0] * 600, None, 0, [b], 0, None,
                var=1, small=9, fix=("map_all", "dups"), enc="parallel")


def multi_nostab(rng):
    """GF_MULTI without a selector table (block = selector).  Block 1 codes
    no lengths (fixed_len): each of its records takes the length last coded,
    which belongs to a record of another block and changes along the
    stream."""
    out, sels, coded = [], [], 0
    for r in range(900):
        sel = 0 if r == 0 else int(rng.integers(0, 3))
        if sel != 1:
            coded = int(rng.integers(40, 200))
        q = _walk(rng, coded, 2, 41)
        out.append(ILLUMINA8[np.searchsorted(ILLUMINA8, q, side="right") - 1])
        sels.append(sel)
    kw = dict(qbits=6, qshift=3, pbits=5, pshift=3, ploc=6, dbits=2, dshift=1, dloc=11, sloc=13,
              alphabet=ILLUMINA8, max_sel=3)
    blocks = [block(**kw), block(fixed=1, **kw), block(**dict(kw, pshift=2))]
    return Case("multi_nostab", _cat(out), [len(r) for r in out], [s << 16 for s in sels], None,
                GF_MULTI, blocks, 3, None, var=1, small=9, fix=("map_recs",))


def stab_fold(rng):
    """Four blocks behind six selectors (stab 0,1,1,2,2,3: the folding of the
    reference's manual-parameters comment); duplicates are looked for in
    blocks 1 and 3 only; block 3 has sequence bases in its context."""
    nrec, rlen = 900, 80
    recs = [_walk(rng, rlen, 2, 41) for _ in range(nrec)]
    sels = [int(x) for x in rng.integers(0, 6, nrec)]
    for r in range(1, nrec, 3):
        recs[r] = recs[r - 1].copy()          # a duplicate, coded as one in blocks 1 and 3
    kw = dict(qbits=6, qshift=3, pbits=3, pshift=4, ploc=6, dbits=2, dshift=1, dloc=9, sloc=13,
              sel=1, max_sym=41, max_sel=5)
    blocks = [block(**kw), block(dedup=1, **kw), block(**dict(kw, qshift=2)),
              block(dedup=1, bbits=2, bloc=11, boff=1, **kw)]
    return Case("stab_fold", _cat(recs), [rlen] * nrec, [s << 16 for s in sels],
                _seq(rng, nrec * rlen), GF_MULTI | GF_STAB, blocks, 5, [0, 1, 1, 2, 2, 3],
                var=3, fix=("dups",))


def _rev_records(rng, lens, gen):
    """Records and FQZ_FREVERSE flags: a seeded half is flagged; every fifth
    record is its predecessor reversed and every seventh its predecessor as
    it is, so whether it is a duplicate depends on the two flags."""
    recs, flags = [], []
    for r, L in enumerate(lens):
        q = gen(L)
        if r and L == len(recs[-1]):
            if r % 5 == 0:
                q = recs[-1][::-1].copy()
            elif r % 7 == 0:
                q = recs[-1].copy()
        recs.append(q)
        flags.append(F_REVERSE if rng.random() < 0.5 else 0)
    return recs, flags


def rev_auto(rng, nrec=900, rlen=None, all_rev=False, name="rev_auto"):
    """vers 3 with picked parameters: GFLAG_DO_REV.  The lengths leave a tail
    that the last record takes (fqzcomp_qual.c:835-837, :1091)."""
    if rlen is None:
        lens = [int(x) for x in rng.choice([1, 2, 3, 50, 50, 50, 51, 51, 64, 100], nrec)]
    else:
        lens = [rlen] * nrec
    recs, flags = _rev_records(rng, lens, lambda L: _hifi(rng, L))
    if all_rev:
        flags = [F_REVERSE] * nrec
    tail = [] if rlen else [_hifi(rng, 37)]
    return Case(name, _cat(recs + tail), lens, flags, None, vers=3, strats=(0, 1, 2), var=5,
                fix=("dups", "revs"), enc="parallel")


def rev_multi(rng, nrec=600, rlen=120):
    """GF_REV | GF_MULTI | GF_STAB with caller parameters: two blocks with
    their own stored qmaps of more than 62 values, duplicates, reversal and
    sequence context in block 1."""
    vals = rng.permutation(94)
    a0, a1 = np.sort(vals[:66]), np.sort(vals[20:84])
    lens = [rlen] * nrec
    sels = [int(x) for x in rng.integers(0, 2, nrec)]
    recs, flags = [], []
    for r in range(nrec):
        q = rng.choice(a1 if sels[r] else a0, rlen).astype(np.uint8)
        if r and r % 5 == 0:
            q, sels[r] = recs[-1][::-1].copy(), sels[r - 1]
        elif r and r % 7 == 0:
            q, sels[r] = recs[-1].copy(), sels[r - 1]
        recs.append(q)
        flags.append(F_REVERSE if rng.random() < 0.5 else 0)
    kw = dict(qbits=7, qshift=7, pbits=3, pshift=4, ploc=7, sloc=14, sel=1, dedup=1, max_sel=2)
    blocks = [block(alphabet=a0, **kw), block(alphabet=a1, bbits=4, bloc=10, boff=1, **kw)]
    return Case("rev_multi", _cat(recs), lens, [f | (s << 17) for f, s in zip(flags, sels)],
                _seq(rng, sum(lens)), GF_REV | GF_MULTI | GF_STAB, blocks, 2, [0, 0, 1],
                vers=3, var=7, fix=("map_recs", "dups", "revs"))


def empty_records(rng):
    """Picked parameters and records of length 0, in the middle and at the
    end: the reference's loop codes the next record's first byte inside an
    empty record, which only the serial encoder reproduces.  Its decoder
    refuses a zero length."""
    lens = [int(x) for x in rng.choice([0, 30, 30, 75, 100], 700)]
    lens[0], lens[-1] = 60, 0
    recs = [rng.choice(NOVA4, L, p=[.01, .04, .10, .85]).astype(np.uint8) for L in lens]
    return Case("empty_records", _cat(recs), lens, [0] * len(lens), None, strats=(0, 1),
                decodes=False)


def no_records(rng):
    return Case("no_records", _walk(rng, 40000, 2, 41).tobytes(), [], [], None, strats=(1,),
                decodes=False)


def five_blocks(rng):
    """More parameter blocks than the GPU codec holds (FQZ_MAX_PARAMS = 4)."""
    nrec, rlen = 400, 90
    recs = [_walk(rng, rlen, 2, 41) for _ in range(nrec)]
    kw = dict(qbits=7, qshift=4, pbits=4, pshift=3, ploc=7, dbits=2, dshift=1, dloc=11, sloc=13,
              sel=1, max_sym=41, max_sel=4)
    blocks = [block(**dict(kw, qshift=2 + k)) for k in range(5)]
    return Case("five_blocks", _cat(recs), [rlen] * nrec, [(r % 5) << 16 for r in range(nrec)],
                None, GF_MULTI | GF_STAB, blocks, 4, [0, 1, 2, 3, 4], gpu=False)


def cases():
    rng = np.random.default_rng(20250317)
    return [two_qtab(rng, 500, 100), two_qtab(rng, 500, 100, seq=True),
            two_qtab(rng, 60, 900, wide=True), two_qtab(rng, 60, 900, wide=True, seq=True),
            two_qmap(rng), one_block(rng), multi_nostab(rng), stab_fold(rng), rev_auto(rng), rev_multi(rng),
            empty_records(rng), no_records(rng), five_blocks(rng)]


def regrowth_cases():
    """More than 1024 listed records, so a decode that is told no lengths
    outgrows its record lists and is launched again (see dec_lists)."""
    rng = np.random.default_rng(20250318)
    rev = rev_auto(rng, 2400, 20, all_rev=True, name="regrow_rev")
    rev.strats = (1,)
    recs = [_walk(rng, 40, 2, 41) for _ in range(2400)]
    for r in range(1, 2400, 2):
        recs[r] = recs[r - 1].copy()
    dups = Case("regrow_dups", _cat(recs), [40] * 2400, [0] * 2400, None, strats=(1,), var=1,
                fix=("dups",), enc="parallel")
    vals = rng.permutation(94)
    wide = two_qtab(rng, 2400, 24, wide=True, name="regrow_wide",
                    alphabets=(np.sort(vals[:70]), np.sort(vals[24:])))
    small = two_qmap(rng, 2400, 24)
    small.name = "regrow_small"
    return [rev, dups, wide, small]


def hedge_case():
    """rev_multi at about 1.1 M symbols in few long records: a block long
    enough for hedged copies, each with lists of its own."""
    rng = np.random.default_rng(20250319)
    c = rev_multi(rng, 44, 25000)
    c.name = "hedge_rev_multi"
    return c


def bad_selector(stream: bytes) -> bytes:
    """A two_qtab stream whose selector table sends selector 2 to block 2 of
    2: the stored table 0,0,1,... (run lengths 2, 254) becomes 0,0,2,...
    (run lengths 2, 0, 254)."""
    k = 1
    while stream[k - 1] & 0x80:
        k += 1
    assert stream[k:k + 4] == bytes([5, GF_MULTI | GF_STAB, 2, 2]) and \
        stream[k + 4:k + 6] == bytes([2, 254])
    return stream[:k + 4] + bytes([2, 0, 254]) + stream[k + 6:]
