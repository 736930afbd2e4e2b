"""The host unlzp against the kernel, and the name sections' decode with and
without it (fqz5_set_host_decode: 0 runs k_lzp_dec for the names' lzp streams
and fetches the blocks one after another; any other mode expands them on host
cores, one host task per block, each block uploaded as it completes).

Streams: the valid and damaged streams of host_lzp_cases through fqz5_unlzp
(the kernel) and fqz5_unlzp_host: bytes, length and verdict must be equal.

Name sections of all three strategies (TLZP3, TOK3_3, TOK3_3_LZP) decode to
the names they were coded from, with the same statuses and sizes, in every
mode.  (The READ2 flags decode_names derives are not part of
fqz5_decode_sections' results: the /1 and /2 suffixes they come from are
checked as part of the names.)"""
import struct

import numpy as np
import pytest
import torch

import host_lzp_cases as lc
from fqzcomp5_amd import lib, sections as S
from oracle import binding

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)
STRATS = {0: S.TLZP3, 1: S.TOK3_3, 2: S.TOK3_3_LZP}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


# ---- streams ---------------------------------------------------------------

def test_valid_streams_kernel_and_host():
    ora = binding.oracle()
    n = 0
    for name, z, data in lc.hand_built() + lc.oracle_streams(ora):
        for cap in (len(data), len(data) + 7):
            k, h = lib.unlzp(z, cap), lib.unlzp_host(z, cap)
            assert k == data and h == data, (name, cap, k is None, h is None)
        n += 1
    assert n >= 19 + 17


def test_damaged_streams_kernel_and_host():
    for name, z, cap in lc.damaged():
        assert lib.unlzp(z, cap) is None, name
        assert lib.unlzp_host(z, cap) is None, name
    # every prefix of the small valid streams: the same verdict and bytes
    for name, z, data in lc.hand_built():
        if len(z) > 16:
            continue
        for cut in range(len(z)):
            assert lib.unlzp(z[:cut], len(data)) == lib.unlzp_host(z[:cut], len(data)), (name, cut)


# ---- name sections ----------------------------------------------------------

def _names(n, seed, comment=True, suffix=True, same_comment=False, tabs=True):
    rng = np.random.default_rng(seed)
    out = []
    x = 1000
    for i in range(n):
        x += int(rng.integers(1, 40))
        nm = f"A00217:{seed}:HFX5:{1 + i * 4 // max(n, 1)}:{1101 + i * 8 // max(n, 1)}:{x}:{int(rng.integers(1000, 30000))}"
        if suffix:
            nm += "/1" if i % 2 == 0 else "/2"
        if comment:
            idx = "ATCACG" if same_comment else ("ATCACG", "CGATGT", "TTAGGC")[int(rng.integers(0, 3))]
            sep = "\t" if (tabs and not same_comment and i % 11 == 0) else " "
            nm += f"{sep}{1 + i % 2}:N:0:{idx}"
        out.append(nm.encode() + b"\0")
    return b"".join(out)


def _blocks():
    """name -> the block's names ('\\0' after each)"""
    some_empty = bytearray()
    for i, nm in enumerate(_names(700, 5).split(b"\0")[:-1]):
        some_empty += (b"" if i % 9 == 0 else nm) + b"\0"
    return {
        "mixed_300": _names(300, 1),
        "mixed_3000": _names(3000, 2),
        "spaces_1200": _names(1200, 6, tabs=False),                # (tok3 takes these whole, strat 1)
        "no_comments": _names(900, 3, comment=False),              # strat 2: clen2 == 0
        "some_empty_names": bytes(some_empty),
        # 6000 identical comments of 13 bytes: 78 000 bytes of one period, so
        # matches of the 65 535 cap and the ones that follow them
        "same_comment_6000": _names(6000, 4, suffix=False, same_comment=True),
    }


def _sections(bufs, out, caps):
    """One name section per device buffer, its output at the next cap bytes of out."""
    secs, oo = [], 0
    for b, cap in zip(bufs, caps):
        secs.append(S.Section(b.data_ptr(), out.data_ptr() + oo, b.numel(), cap, 0, S.SEC_NAME,
                              None, None, 0, None))
        oo += cap
    return secs


def _dev(b):
    return torch.from_numpy(np.frombuffer(b or b"\0", np.uint8).copy()).to("cuda:0")


def _encode(blocks, method):
    """The blocks as name sections of `method` (None where the coder refuses)."""
    src = [_dev(b)[:len(b)] for b in blocks]
    caps = [2 * len(b) + 1000 + 65536 for b in blocks]
    enc = torch.zeros(sum(caps), dtype=torch.uint8, device="cuda:0")
    secs = _sections(src, enc, caps)
    S.sections_try(secs, np.full(len(secs), 1 << method, np.uint32))
    res = S.sections_commit(secs, np.full(len(secs), method, np.int32))
    torch.cuda.synchronize()
    out, eo = [], 0
    for r, cap in zip(res, caps):
        out.append(enc[eo:eo + r.clen].cpu().numpy().tobytes() if r.status == 0 else None)
        eo += cap
    return out


def _decode(streams, ulens):
    """fqz5_decode_sections over name sections: [(status, usize, bytes)]"""
    comp = [_dev(s)[:len(s)] for s in streams]
    out = torch.full((sum(ulens) + 1,), 0xA5, dtype=torch.uint8, device="cuda:0")
    res = S.decode(_sections(comp, out, ulens))
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    got, oo = [], 0
    for r, n in zip(res, ulens):
        got.append((r.status, r.usize if r.status == 0 else 0,
                    host[oo:oo + n] if r.status == 0 else None))
        oo += n
    return got


@pytest.fixture(scope="module")
def coded():
    """(block name, strat) -> (section bytes, names), coded once"""
    blocks = _blocks()
    out = {}
    for strat, method in STRATS.items():
        secs = _encode(list(blocks.values()), method)
        for (name, data), sec in zip(blocks.items(), secs):
            if sec is not None:
                assert sec[4] == strat, (name, strat)
                out[(name, strat)] = (sec, data)
    # every block codes under every strategy, but where a comment follows a
    # tab and tok3 gets the whole names (strat 1): its tokenise loop refuses a
    # byte below ' ' (tok3_encode_names returns NULL)
    missing = {k for k in ((n, s) for n in blocks for s in STRATS) if k not in out}
    assert missing == {(n, 1) for n, data in blocks.items() if b"\t" in data}, missing
    assert {n for n, _ in missing} == {"mixed_300", "mixed_3000", "some_empty_names"}
    return out


@pytest.fixture(params=MODES)
def mode(request):
    so = lib.load()
    prev = so.fqz5_set_host_decode(request.param)
    yield request.param
    so.fqz5_set_host_decode(prev)


# decode_names' stitch takes a comment for every record once the section has
# any, and stops at a record that adds no byte: a block with empty names does
# not come back as it went in under strat 2, in the reference as here.  What
# it decodes to is still the same in every mode.
NOT_ROUND_TRIP = {("some_empty_names", 2)}


def _set_mode(m):
    return lib.load().fqz5_set_host_decode(m)


@pytest.fixture(scope="module")
def on_gpu(coded):
    """Every section decoded as one batch with the names' lzp on the GPU (mode 0)."""
    keys = sorted(coded)
    prev = _set_mode(0)
    try:
        got = _decode([coded[k][0] for k in keys], [len(coded[k][1]) for k in keys])
    finally:
        _set_mode(prev)
    return dict(zip(keys, got))


def test_sections_round_trip_on_gpu(coded, on_gpu):
    for k, (st, usize, data) in on_gpu.items():
        assert (st, usize) == (0, len(coded[k][1])), k
        if k not in NOT_ROUND_TRIP:
            assert data == coded[k][1], k
    assert on_gpu[("some_empty_names", 0)][2] == coded[("some_empty_names", 0)][1]
    # the cases the blocks are there for
    sec, data = coded[("no_comments", 2)]
    clen1, clenf = struct.unpack("<II", sec[9:17])
    assert len(sec) - 9 - 8 - clen1 - clenf == 0                    # clen2 == 0
    sec, data = coded[("same_comment_6000", 2)]
    assert sum(len(nm.split(b" ", 1)[1]) + 1 for nm in data.split(b"\0")[:-1]) > 65535


def test_sections_decode_the_same_in_every_mode(mode, coded, on_gpu):
    keys = sorted(coded)
    got = _decode([coded[k][0] for k in keys], [len(coded[k][1]) for k in keys])
    for k, g in zip(keys, got):
        assert g == on_gpu[k], (mode, k)


def test_one_block_at_a_time_equals_the_batch(mode, coded):
    keys = [k for k in sorted(coded) if k[0] in ("mixed_300", "same_comment_6000", "no_comments")]
    batch = _decode([coded[k][0] for k in keys], [len(coded[k][1]) for k in keys])
    for k, b in zip(keys, batch):
        assert _decode([coded[k][0]], [len(coded[k][1])]) == [b], (mode, k)


def _damage_comments(sec):
    """A strat-2 section whose comments' lzp stream ends on a predicted marker
    (its rANS stage is sound): decode_names fails in unlzp."""
    ora = binding.oracle()
    u_len, strat, c_len = struct.unpack("<IBI", sec[:9])
    assert strat == 2 and len(sec) == 9 + c_len
    clen1, clenf = struct.unpack("<II", sec[9:17])
    head = sec[9:17 + clen1 + clenf]
    lz = ora.rans_uncompress(sec[17 + clen1 + clenf:])
    bad = lz + bytes([233])
    with pytest.raises(RuntimeError):
        ora.unlzp(bad, u_len)
    tail = ora.rans_compress(bad, 5)
    return struct.pack("<IBI", u_len, 2, len(head) + len(tail)) + head + tail


def test_damaged_middle_block(mode, coded):
    a, da = coded[("mixed_300", 2)]
    b, db = coded[("same_comment_6000", 2)]
    c, dc = coded[("mixed_3000", 2)]
    got = _decode([a, _damage_comments(b), c], [len(da), len(db), len(dc)])
    assert got[0] == (0, len(da), da), mode
    assert got[1][0] != 0, mode
    assert got[2] == (0, len(dc), dc), mode
    # and sound again in the same place
    assert _decode([a, b, c], [len(da), len(db), len(dc)])[1] == (0, len(db), db), mode
