"""GPU parity of fqz_compress / fqz_decompress on the paths the picked
parameters never reach: caller-supplied parameter blocks (several blocks,
selector tables, per-block qtabs and qmaps), reversal (vers 3), empty
records, and record lists that outgrow their first size.

Every comparison is exact bytes: encodes against the reference's golden
vectors (tests/golden/fqz_params.json), decodes against the input, damaged
streams against the oracle's answer.  fqz5_fqz_path_counts says which decoder
variant, fix-up kernels and encoder took each block; the last test fails if
any of them never ran."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

from fqz_param_cases import bad_selector, cases, gp_digest, hedge_case, regrowth_cases
from fqzcomp5_amd import lib
from oracle import binding

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
VEC = json.load(open(os.path.join(HERE, "golden", "fqz_params.json")))
IDS = ["%s-%d" % (v["case"], v["strat"]) for v in VEC]
DEC_KEYS = lib.FQZ_PATH_NAMES[:10]
FIX_KEYS = ["map_all", "map_recs", "dups", "revs"]
MODES = ["general", "small", "small_sets1", "host"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def start_counts():
    return lib.fqz_path_counts()


@pytest.fixture(scope="module")
def streams(start_counts):
    """Per golden vector: (vector, case, the oracle's stream, pinned to the
    golden md5, and the record lengths its encode left)."""
    cs = {c.name: c for c in cases()}
    ora = binding.oracle()
    res = {}
    for v, vid in zip(VEC, IDS):
        c = cs[v["case"]]
        comp = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), v["strat"], c.seq, c.vers,
                                c.gp())
        assert (len(comp), hashlib.md5(comp).hexdigest()) == (v["len"], v["md5"]), vid
        res[vid] = (v, c, comp, np.asarray(ora.last_lens, np.uint32))
    return res


@pytest.fixture(params=MODES)
def mode(request):
    so = lib.load()
    prev = so.fqz5_set_dec_small(0 if request.param == "general" else 1)
    old = os.environ.pop("FQZ5_DEC_SETS", None)
    if request.param == "small_sets1":
        os.environ["FQZ5_DEC_SETS"] = "1"
    try:
        yield request.param
    finally:
        so.fqz5_set_dec_small(prev)
        os.environ.pop("FQZ5_DEC_SETS", None)
        if old is not None:
            os.environ["FQZ5_DEC_SETS"] = old


def _delta(a, b):
    return {k: b[k] - a[k] for k in b if b[k] != a[k]}


def _decode(comp, lens, flags, seq, host=False):
    """(bytes, lengths, counter delta); (None, None, delta) where it fails."""
    c0 = lib.fqz_path_counts()
    try:
        out, got = lib.fqz_decompress(comp, None if lens is None else lens.copy(),
                                      None if lens is None else (flags & 0xffff), seq, host=host)
    except lib.NativeError:
        out, got = None, None
    return out, got, _delta(c0, lib.fqz_path_counts())


@pytest.mark.parametrize("vid", IDS)
def test_encode_golden(streams, vid):
    v, c, _, lens_after = streams[vid]
    gp, lens, flags = c.gp(), c.lens.copy(), c.flags.copy()
    c0 = lib.fqz_path_counts()
    if not c.gpu:
        with pytest.raises(lib.NativeError):
            lib.fqz_compress(c.q, lens, flags, v["strat"], c.seq, c.vers, gp)
        return
    out = lib.fqz_compress(c.q, lens, flags, v["strat"], c.seq, c.vers, gp)
    d = _delta(c0, lib.fqz_path_counts())
    assert (len(out), hashlib.md5(out).hexdigest()) == (v["len"], v["md5"])
    assert gp_digest(gp) == v["gp_md5"]                  # the caller's block, as the oracle's
    assert (flags == (c.flags & 0xffff)).all()           # selector bits cleared again
    assert [int(x) for x in lens] == [int(x) for x in lens_after]
    assert d == {"enc_" + c.enc: 1}


@pytest.mark.parametrize("vid", IDS)
def test_decode(streams, mode, vid):
    v, c, comp, lens = streams[vid]
    host = mode == "host"
    out, got_lens, d = _decode(comp, lens, c.flags, c.seq, host)
    ok = v["decodes"] and (host or c.gpu)
    assert out == (c.q if ok else None)
    if host:
        assert d == {}
    if not ok:
        return
    assert got_lens == [int(x) for x in lens]
    if host:
        return
    var = c.small if (mode != "general" and c.small is not None) else c.var
    want = {DEC_KEYS[var]: 1}
    want.update({k: 1 for k in c.fix})
    assert d == want


def test_five_blocks_leaves_process_usable(streams):
    """More blocks than FQZ_MAX_PARAMS: encode and decode fail cleanly (the
    host decoder reads the stream, test_decode[host]) and the next call
    works."""
    v, c, comp, lens = streams["five_blocks-0"]
    with pytest.raises(lib.NativeError):
        lib.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), 0, c.seq, c.vers, c.gp())
    with pytest.raises(lib.NativeError):
        lib.fqz_decompress(comp, lens.copy(), c.flags & 0xffff, c.seq)
    v, c, comp, lens = streams["two_qtab-0"]
    out, got_lens, _ = _decode(comp, lens, c.flags, c.seq)
    assert out == c.q and got_lens == [int(x) for x in lens]


def test_bad_selector(streams, mode):
    """A selector table entry past the parameter blocks: the oracle refuses
    the stream, and so must every decoder."""
    v, c, comp, lens = streams["two_qtab-0"]
    bad = bad_selector(comp)
    try:
        exp = binding.oracle().fqz_decompress(bad, lens, c.flags & 0xffff, c.seq)
    except RuntimeError:
        exp = None
    out, _, _ = _decode(bad, lens, c.flags, c.seq, mode == "host")
    assert out == exp


@pytest.mark.parametrize("name", ["regrow_rev", "regrow_dups", "regrow_wide", "regrow_small"])
def test_list_regrowth(name):
    """More than 1024 listed records.  Told no lengths, the decode outgrows
    its lists (1025 entries) and the block is launched a second time, once;
    told the lengths, it is not.  regrow_wide is a relaunched block with two
    model registers, whose first launch has written models to back_hi."""
    c = next(x for x in regrowth_cases() if x.name == name)
    ora = binding.oracle()
    comp = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), c.strats[0], c.seq, c.vers, c.gp())
    lens = np.asarray(ora.last_lens, np.uint32)
    out, _, d = _decode(comp, None, None, None)
    var = DEC_KEYS[c.small if c.small is not None else c.var]
    assert out == c.q
    assert d.get("relaunched") == 1 and d.get(var) == 2, d
    out, got_lens, d = _decode(comp, lens, c.flags, None)
    assert out == c.q and got_lens == [int(x) for x in lens]
    assert "relaunched" not in d and d.get(var) == 1, d


@pytest.mark.parametrize("name", ["two_qtab", "rev_multi", "stab_fold"])
def test_damaged_vs_oracle(streams, name):
    """Cut and flipped streams: the general decoder, the small decoder's
    setting and the host decoder give the oracle's bytes or its failure."""
    v, c, comp, lens = streams[name + "-0"]
    ora = binding.oracle()
    rng = np.random.default_rng(9)
    bads = [comp[:-cut] for cut in (1, 3, 9, 40)]
    for _ in range(3):
        b = bytearray(comp)
        b[int(rng.integers(len(b) // 2, len(b)))] ^= 0x5A
        bads.append(bytes(b))
    so = lib.load()
    for bad in bads:
        try:
            exp = ora.fqz_decompress(bad, lens, c.flags & 0xffff, c.seq)
        except RuntimeError:
            exp = None
        for m in ("general", "small", "host"):
            prev = so.fqz5_set_dec_small(0 if m == "general" else 1)
            try:
                out, _, _ = _decode(bad, lens, c.flags, c.seq, m == "host")
            finally:
                so.fqz5_set_dec_small(prev)
            assert out == exp, (m, len(bad))


def test_hedged_copies_with_lists():
    """A block long enough for hedged copies (2^20 symbols), with all three
    record lists."""
    c = hedge_case()
    ora = binding.oracle()
    comp = ora.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), 0, c.seq, c.vers, c.gp())
    t0 = time.perf_counter()
    out, got_lens, d = _decode(comp, c.lens, c.flags, c.seq)
    print("hedged decode of %d symbols: %.2f s" % (len(c.q), time.perf_counter() - t0))
    assert out == c.q and got_lens == [int(x) for x in c.lens]
    assert d == {DEC_KEYS[c.var]: 1, "map_recs": 1, "dups": 1, "revs": 1}


def test_every_path_ran(start_counts):
    """Over this module every decoder variant, every fix-up kernel, the
    relaunch and both encoders took at least one block.  (It looks back
    over the tests above, so it fails when selected on its own: a body
    that no test reached is a failure, not a skip.)"""
    d = _delta(start_counts, lib.fqz_path_counts())
    print("fqz path counts over the module:", json.dumps(d))
    missing = [k for k in DEC_KEYS + FIX_KEYS + ["relaunched", "enc_serial", "enc_parallel"]
               if not d.get(k)]
    assert not missing, missing
