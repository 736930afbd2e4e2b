"""fqz_compress with caller-supplied parameters, reversal and empty records
on the CPU: the restatement (oracle/fqz_oracle.c) against golden vectors from
the compiled reference (tests/golden/fqz_params.json), what a call leaves in
the caller's parameter block, twelve random parameter sets against the
reference itself where it is built, and the library's host decoder
(fqz5_fqz_decompress_host, no GPU) on every stream."""
import hashlib
import json
import os

import numpy as np
import pytest

from fqz_param_cases import (COARSE, F_REVERSE, GF_MULTI, GF_REV, GF_STAB, Case, bad_selector,
                             block, cases, gp_digest)
from fqzcomp5_amd import lib
from oracle import binding

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    vec = json.load(open(os.path.join(HERE, "golden", "fqz_params.json")))
    blob = open(os.path.join(HERE, "golden", "fqz_params.bin"), "rb").read()
    return {c.name: c for c in cases()}, vec, blob


@pytest.fixture(scope="module")
def streams(golden):
    """Every vector's stream (the stored bytes, or the oracle's where only
    the md5 is stored) and the record lengths its encode left behind."""
    cs, vec, blob = golden
    ora = binding.oracle()
    res = []
    for v in vec:
        c = cs[v["case"]]
        comp = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), v["strat"], c.seq, c.vers,
                                c.gp())
        lens = np.asarray(ora.last_lens, np.uint32)
        if v["off"] is not None:
            comp = blob[v["off"]:v["off"] + v["len"]]
        else:
            assert hashlib.md5(comp).hexdigest() == v["md5"], v["case"]
        res.append((v, c, comp, lens))
    return res


def test_golden_file_sizes():
    small = os.path.getsize(os.path.join(HERE, "golden", "fqz_small.bin"))
    assert os.path.getsize(os.path.join(HERE, "golden", "fqz_params.bin")) <= small


def test_oracle_encodes_golden(golden):
    cs, vec, _ = golden
    ora = binding.oracle()
    assert {v["case"] for v in vec} == set(cs)
    for v in vec:
        c = cs[v["case"]]
        gp = c.gp()
        out = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), v["strat"], c.seq, c.vers, gp)
        assert (len(out), hashlib.md5(out).hexdigest()) == (v["len"], v["md5"]), v["case"]
        # the caller's block as the reference leaves it
        assert gp_digest(gp) == v["gp_md5"], v["case"]
        assert all(f < 65536 for f in ora.last_flags), v["case"]      # selector bits cleared
        assert (ora.last_lens[-1] if ora.last_lens else None) == v["last_len"], v["case"]


def test_oracle_decodes_golden(streams):
    ora = binding.oracle()
    n = 0
    for v, c, comp, lens in streams:
        try:
            got = ora.fqz_decompress(comp, lens, c.flags & 0xffff, c.seq)
        except RuntimeError:
            got = None
        assert got == (c.q if v["decodes"] else None), (v["case"], v["strat"])
        n += v["off"] is not None
    assert n >= 8


def test_host_decodes_golden(streams):
    """fqz5_fqz_decompress_host on every stream: the input and the record
    lengths, or a failure where the reference fails (a zero length)."""
    for v, c, comp, lens in streams:
        try:
            got, got_lens = lib.fqz_decompress(comp, lens.copy(), c.flags & 0xffff, c.seq, host=True)
        except lib.NativeError:
            got, got_lens = None, None
        assert got == (c.q if v["decodes"] else None), (v["case"], v["strat"])
        if got is not None:
            assert got_lens == [int(x) for x in lens], v["case"]


def test_bad_selector_host_and_oracle(streams):
    """A selector whose table entry is past the parameter blocks: the decoders
    refuse the stream (fqzcomp_qual.c:1494-1496)."""
    v, c, comp, lens = next(s for s in streams if s[0]["case"] == "two_qtab")
    bad = bad_selector(comp)
    with pytest.raises(RuntimeError):
        binding.oracle().fqz_decompress(bad, lens, c.flags & 0xffff, None)
    with pytest.raises(lib.NativeError):
        lib.fqz_decompress(bad, lens.copy(), c.flags & 0xffff, None, host=True)


def random_case(seed: int) -> Case:
    """A seeded random parameter set: 1..4 blocks, random context layout
    (bits, shifts, locations; the context is a masked sum, so any layout is
    legal), selector tables, dedup, fixed lengths, stored qmaps, custom
    qtabs, sequence context and reversal."""
    rng = np.random.default_rng(seed)
    nparam = int(rng.integers(1, 5))
    stab_on = nparam == 1 or rng.random() < 0.6
    gflags = (GF_MULTI if nparam > 1 or rng.random() < 0.3 else 0) | (GF_STAB if stab_on else 0)
    if rng.random() < 0.5:
        gflags |= GF_REV
    fixed_any = rng.random() < 0.4
    if stab_on:
        # selectors 0..nsel-1 onto the blocks, onto and in order; the first
        # two share block 0 (see two_qtab on tables that end in a run of 255)
        nsel = int(rng.integers(nparam + 1, nparam + 4))
        cut = np.sort(rng.choice(np.arange(2, nsel), nparam - 1, replace=False)) if nparam > 1 else []
        stab = [int(np.searchsorted(cut, s, side="right")) for s in range(nsel)]
        max_sel = nsel - 1
    else:
        nsel, stab, max_sel = nparam, None, nparam
    coded_sel = bool(gflags & GF_MULTI) or rng.random() < 0.7
    blocks, alphas = [], []
    for k in range(nparam):
        alpha = np.sort(rng.choice(np.arange(0, 61), int(rng.integers(3, 41)), replace=False))
        stored = rng.random() < 0.5
        qbits = int(rng.integers(0, 11))
        bbits = int(rng.integers(0, 7)) if rng.random() < 0.4 else 0
        # (dbits 1 with dshift 0 is the table 0,1,1,...: a final run of 255
        # entries, which the reference stores in a form it cannot read)
        dbits = int(rng.integers(0, 4))
        blocks.append(block(
            qbits=qbits, qshift=int(rng.integers(0, 8)), qloc=int(rng.integers(0, 8)),
            pbits=int(rng.integers(0, 7)), pshift=int(rng.integers(0, 6)), ploc=int(rng.integers(0, 13)),
            dbits=dbits, dshift=int(rng.integers(dbits == 1, 4)), dloc=int(rng.integers(0, 15)),
            sloc=int(rng.integers(0, 16)), bbits=bbits, bloc=int(rng.integers(0, 12)),
            boff=int(rng.integers(0, 4)), sel=int(coded_sel and stab_on), dedup=int(rng.random() < 0.5),
            fixed=int(fixed_any and rng.random() < 0.6),
            qtab=COARSE if qbits and rng.random() < 0.4 else None,
            alphabet=alpha if stored else None, max_sym=int(alpha[-1]), max_sel=max_sel,
            context=int(rng.integers(0, 65536))))
        alphas.append(alpha)
    nrec = 300
    lens = [60] * nrec if fixed_any else [int(x) for x in rng.integers(1, 121, nrec)]
    recs, flags = [], []
    for r in range(nrec):
        sel = int(rng.integers(0, nsel)) if coded_sel else 0
        x = stab[sel] if stab_on else sel
        q = rng.choice(alphas[x], lens[r]).astype(np.uint8)
        if r and lens[r] == lens[r - 1] and rng.random() < 0.2 and \
                set(recs[-1].tolist()) <= set(alphas[x].tolist()):
            q = recs[-1][::-1].copy() if rng.random() < 0.5 else recs[-1].copy()
        recs.append(q)
        flags.append((sel << 16) | (F_REVERSE if rng.random() < 0.5 else 0))
    seq = None
    if rng.random() < 0.6:
        seq = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, sum(lens) + 4)].tobytes()
    return Case("random%d" % seed, np.concatenate(recs).tobytes(), lens, flags, seq, gflags, blocks,
                max_sel, stab, vers=3 + seed % 2)


@pytest.mark.skipif(not binding.have_ref(), reason="reference not built")
@pytest.mark.parametrize("seed", range(12))
def test_random_params_vs_reference(seed):
    c = random_case(seed)
    ora, ref = binding.oracle(), binding.ref()
    g1, g2 = c.gp(), c.gp()
    a = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), 0, c.seq, c.vers, g1)
    b = ref.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), 0, c.seq, c.vers, g2)
    assert a == b
    assert gp_digest(g1) == gp_digest(g2)
    assert ora.last_flags == ref.last_flags and all(f < 65536 for f in ora.last_flags)
    assert ref.fqz_decompress(a, c.lens, c.flags & 0xffff, c.seq) == c.q
    assert ora.fqz_decompress(a, c.lens, c.flags & 0xffff, c.seq) == c.q
    got, got_lens = lib.fqz_decompress(a, c.lens.copy(), c.flags & 0xffff, c.seq, host=True)
    assert got == c.q and got_lens == [int(x) for x in c.lens]
