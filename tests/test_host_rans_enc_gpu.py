"""Where the compressor runs its bare rANS 4x16 chains (fqz5_set_host_encode):
all on the GPU (0), every NX = 4 chain on host cores (1), by cost among the
chains of 2^20 symbols and more (2, the default), every other one (3).  Every
placement gives the reference's bytes: a host-placed chain leaves the
checkpoints k_enc_chain2w would have left, and the replay kernels emit the
stream from them."""
import numpy as np
import pytest

import host_rans_enc_cases as ec
from fqzcomp5_amd import fqz5file, lib, synth
from oracle import binding

pytestmark = pytest.mark.gpu

ORDERS = (0, 1)
PACKED = (129, 193)              # PACK, RLE + PACK: their packed streams are NX = 4 chains too
PACKED_SIZES = (1025, 3 * 1024 + 2, 70001)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def inputs():
    """[(name, data, order, the reference's stream)] over every size and
    alphabet at orders 0 and 1, a few at 129 and 193."""
    ora = binding.oracle()
    out = []
    for n in ec.SIZES:
        for name, d in ec.alphabets(n).items():
            d = d.tobytes()
            for o in ORDERS + (PACKED if n in PACKED_SIZES and name in ("two", "acgtn") else ()):
                out.append((f"{name}/{n}/{o}", d, o, ora.rans_compress(d, o)))
    return out


def _compress(d, o):
    # (the caller-buffer entry point: one batch per call, nothing coded ahead)
    return lib.rans_compress_to(d, o, lib.compress_bound(len(d), o))


@pytest.mark.parametrize("mode", [0, 1, 3])
def test_same_bytes_as_the_reference(mode, inputs):
    prev = lib.set_host_encode(mode)
    try:
        h0, g0 = lib.rans_enc_chain_counts()
        for name, d, o, want in inputs:
            assert _compress(d, o) == want, (mode, name)
        h1, g1 = lib.rans_enc_chain_counts()
    finally:
        lib.set_host_encode(prev)
    if mode == 0:
        assert h1 == h0 and g1 > g0
    if mode == 1:                                # every chain here has four states
        assert h1 > h0 and g1 == g0
    if mode == 3:
        assert h1 > h0


def test_default_mode_leaves_short_chains_on_the_gpu(inputs):
    prev = lib.set_host_encode(2)
    try:
        h0, g0 = lib.rans_enc_chain_counts()
        for name, d, o, want in inputs:          # all under 2^20 symbols
            if len(d) == 70001:
                assert _compress(d, o) == want, name
        h1, g1 = lib.rans_enc_chain_counts()
    finally:
        lib.set_host_encode(prev)
    assert h1 == h0 and g1 > g0


def test_host_and_gpu_chain_share_one_input():
    """One batch with the order-0 and the order-1 stream of the same device
    input, every other chain on a host core: the host chain's pinned copy and
    the GPU chain read the same bytes."""
    import torch
    ora = binding.oracle()
    d = ec.alphabets(70001)["acgtn"].tobytes()
    src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    outs = [torch.zeros(lib.compress_bound(len(d), o), dtype=torch.uint8, device="cuda") for o in ORDERS]
    lib.after_torch()
    prev = lib.set_host_encode(3)
    try:
        h0, g0 = lib.rans_enc_chain_counts()
        jobs = [lib.RansJob(src.data_ptr(), b.data_ptr(), src.numel(), b.numel(), o, 0, 0, 0)
                for o, b in zip(ORDERS, outs)]
        lib.compress_batch_dev(jobs)
        h1, g1 = lib.rans_enc_chain_counts()
    finally:
        lib.set_host_encode(prev)
    assert all(j.status == 0 for j in jobs)
    assert h1 - h0 == 1 and g1 - g0 == 1
    for o, j, b in zip(ORDERS, jobs, outs):
        assert bytes(b[:j.out_size].cpu().numpy()) == ora.rans_compress(d, o), o


def test_block_encoder_same_blocks():
    """A two-block run through the block encoder (fqz5_sections_try and
    commit; under 2 MB a section), every chain on host cores against none."""
    r = synth.illumina(6000, seed=8, with_names=True)
    text = synth.fastq_chunk(r, 0, r.num_records).tobytes()
    blk = len(text) // 2 + 1000
    z = {}
    prev = lib.set_host_encode(0)
    try:
        for mode in (0, 1):
            lib.set_host_encode(mode)
            h0, _ = lib.rans_enc_chain_counts()
            z[mode] = fqz5file.compress_bytes(text, 3, blk_size=blk)
            h1, _ = lib.rans_enc_chain_counts()
            assert (h1 > h0) == (mode == 1)
    finally:
        lib.set_host_encode(prev)
    assert z[0] == z[1]
    assert fqz5file.decompress_bytes(z[1]) == text
