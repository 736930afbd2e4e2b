"""Where the decoder runs its plain rANS 4x16 chains (fqz5_set_host_decode):
all on the GPU (0), every 4-state chain on host cores (1), by cost among the
chains of 2^20 symbols and more (2, the default), every other one (3).  Every
placement returns the same bytes and the same verdict on a damaged stream."""
import numpy as np
import pytest

import host_rans_cases as hc
from fqzcomp5_amd import fqz5file, lib, synth

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2, 3)
ORDERS = (0, 1, 4, 128, 129, 193, (4 << 8) | 8)       # 4: X32, the last: STRIPE of 4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(params=MODES)
def mode(request):
    so = lib.load()
    prev = so.fqz5_set_host_decode(request.param)
    yield request.param
    so.fqz5_set_host_decode(prev)


def _quality(n, seed):
    rng = np.random.default_rng(seed)
    lv = np.array([2, 12, 18, 23, 27, 32, 36, 40], np.uint8) + 33
    return lv[rng.choice(8, n, p=[.02, .03, .05, .08, .12, .2, .2, .3])].tobytes()


@pytest.fixture(scope="module")
def coded():
    """(data, stream) per order and size, coded once on the GPU."""
    out = []
    for n in (70001, 5):
        d = _quality(n, 11 + n)
        for o in ORDERS:
            out.append((o, d, lib.rans_compress(d, o)))
    return out


def test_stream_round_trips(mode, coded):
    for o, d, c in coded:
        assert lib.rans_uncompress(c) == d, (mode, hex(o), len(d))


def test_crafted_tiny_streams(mode):
    for name, c, d in hc.streams():
        if name.startswith("craft/"):
            assert lib.rans_uncompress_to(c, len(d)) == d, (mode, name)


@pytest.fixture(scope="module")
def long_chain():
    rng = np.random.default_rng(21)
    d = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, 1_500_000, p=[.3, .25, .25, .19, .01])].tobytes()
    c = lib.rans_compress(d, 0)
    assert c[0] == 0                                   # one plain order-0 chain
    return d, c


def test_one_long_chain(mode, long_chain):
    d, c = long_chain
    h0, g0 = lib.rans_chain_counts()
    assert lib.rans_uncompress(c) == d
    h1, g1 = lib.rans_chain_counts()
    if mode == 0:
        assert h1 == h0 and g1 == g0 + 1
    if mode == 1:
        assert g1 == g0 and h1 == h0 + 1
    if mode == 2:
        assert (h1 - h0) + (g1 - g0) == 1
    if mode == 3:                                      # the one eligible chain is position 0
        assert h1 == h0 + 1 and g1 == g0


@pytest.fixture(scope="module")
def blocks():
    r = synth.illumina(6000, seed=8, with_names=True)
    text = synth.fastq_chunk(r, 0, r.num_records).tobytes()
    return text, {lv: fqz5file.compress_bytes(text, lv, blk_size=300_000) for lv in (1, 3)}


@pytest.mark.parametrize("level", [1, 3])
def test_block_round_trips(mode, blocks, level):
    text, z = blocks
    assert fqz5file.decompress_bytes(z[level]) == text, (mode, level)


def _outcome(comp, cap):
    try:
        return lib.rans_uncompress_to(comp, cap)
    except lib.NativeError:
        return None


def test_damaged_streams_same_outcome():
    from oracle import binding
    ora = binding.oracle()
    so = lib.load()
    prev = so.fqz5_set_host_decode(2)
    try:
        for order, (comp, data) in enumerate(hc.small_pair()):
            bad = hc.damaged(comp, order)
            res = {}
            for m in (0, 1):
                so.fqz5_set_host_decode(m)
                assert _outcome(comp, len(data)) == data
                res[m] = [_outcome(b, len(data)) for b in bad]
            diff = [k for k in range(len(bad)) if res[0][k] != res[1][k]]
            assert not diff, (order, diff[:10])
            # and it is the reference's outcome (the oracle's): a stream cut in
            # its table or states is refused, one cut in its words decodes on
            # with the states it has (test_rans_damaged_gpu.py)
            want = [ora.rans_uncompress_to(b, len(data)) for b in bad]
            diff = [k for k in range(len(bad)) if res[0][k] != want[k]]
            assert not diff, (order, diff[:10])
            # the damage is real: cut tables fail, cut words and flips decode to other bytes
            assert sum(r is None for r in res[0]) > 16
            assert sum(r is not None and r != data for r in res[0]) > 64
    finally:
        so.fqz5_set_host_decode(prev)
