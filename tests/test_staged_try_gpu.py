"""The staged try (fqz5_sections_try_staged): outside the trial windows a
sequence or quality section codes the trial's pick only, predicted from the
window's rANS sizes.  Methods, framing and bytes equal the unstaged try's in
every case; only what was coded, and when, differs (fqz5_staged_counts)."""
import ctypes as C

import numpy as np
import pytest
import torch

from fqzcomp5_amd import lib, sections as S, synth

pytestmark = pytest.mark.gpu
GEN = {"illumina": synth.illumina, "novaseq": synth.novaseq}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _dev():
    return torch.device("cuda", 0)


def _encode(reads, blocks, av, staged, state=None, names=True):
    """encode_run with staged tries on or off: (run, results, methods, the
    counters' and the decisions' increase)."""
    run = S.Run(reads, blocks, _dev(), names=names)
    prev = S.set_staged_try(staged)
    c0, d0 = S.staged_counts(), S.staged_decisions()
    try:
        res, meth, *_ = S.encode_run(run.enc_secs(), av, state if state is not None else S.new_state())
    finally:
        S.set_staged_try(prev)
    cnt = tuple(b - a for a, b in zip(c0, S.staged_counts()))
    dec = [b - a for a, b in zip(d0, S.staged_decisions())]
    assert all(r.status == 0 for r in res)
    return run, res, [int(m) for m in meth], cnt, dec


def _same(run_a, res_a, meth_a, run_b, res_b, meth_b):
    assert meth_a == meth_b
    assert [(r.method, r.strat, r.clen, r.usize) for r in res_a] == \
        [(r.method, r.strat, r.clen, r.usize) for r in res_b]
    for i in range(len(res_a)):
        assert run_a.chosen(res_a, i) == run_b.chosen(res_b, i), i


def _roundtrip(run, res):
    dres = S.decode(run.dec_secs(res))
    assert all(r.status == 0 for r in dres)
    torch.cuda.synchronize()
    assert run.roundtrip_ok()


CASES = [(3, "illumina", 52000, 2_700_000),     # sections just over 2^20 B: host chains
         (5, "illumina", 52000, 2_700_000),
         (5, "novaseq", 52000, 2_700_000),
         (3, "illumina", 3600, 200_000),        # small blocks: every chain on the GPU
         (5, "novaseq", 3600, 200_000)]
_plain = {}


def _case(level, kind, nreads, blk):
    """The unstaged run of a case, computed once."""
    key = (level, kind, nreads, blk)
    if key not in _plain:
        reads = GEN[kind](nreads, seed=21)
        blocks = synth.split_blocks(reads, blk)[:6]
        assert len(blocks) == 6
        av = S.masks(level, True)
        _plain[key] = (reads, blocks, av) + _encode(reads, blocks, av, False)
    return _plain[key]


@pytest.mark.parametrize("level,kind,nreads,blk", CASES)
def test_staged_equals_unstaged(level, kind, nreads, blk):
    reads, blocks, av, run_a, res_a, meth_a, cnt_a, dec_a = _case(level, kind, nreads, blk)
    if blk > 1_000_000:
        assert all(e - s > 1 << 20 for sec, s, e, fl, k in run_a.spans if sec in (S.SEC_SEQ, S.SEC_QUAL))
    assert cnt_a == (0, 0, 0, 0) and dec_a == [0, 0, 0, 0]
    run_b, res_b, meth_b, cnt, dec = _encode(reads, blocks, av, True)
    print(f"-{level} {kind} {blk}: first-stage candidates {cnt[0]}, follow sections coded {cnt[1]}, "
          f"overturned {cnt[2]}, skipped {cnt[3]}; methods {sorted(set(meth_b))}")
    _same(run_a, res_a, meth_a, run_b, res_b, meth_b)
    assert cnt[1] > 0 and cnt[3] > 0
    assert cnt[1] <= 2 * 3                       # at most the three follow blocks' two sections
    assert dec[S.SEC_SEQ] == 1 and dec[S.SEC_QUAL] == 1
    _roundtrip(run_b, res_b)


def test_overturned_prediction():
    """Amplicon sequences (3 distinct reads): LZP3 wins the sequence trial,
    but its helper ends after the rANS batches, so the follow sections were
    coded with the best rANS method; the commit codes LZP3 late."""
    rng = np.random.default_rng(3)
    reads = synth.illumina(30000, seed=3)
    pool = reads.seq[:150 * 3].reshape(3, 150).copy()
    reads.seq[:] = pool[rng.integers(0, 3, reads.num_records)].reshape(-1)
    blocks = synth.split_blocks(reads, 2_000_000)[:5]
    assert len(blocks) == 5
    av = S.masks(3)
    run_a, res_a, meth_a, _, _ = _encode(reads, blocks, av, False, names=False)
    run_b, res_b, meth_b, cnt, _ = _encode(reads, blocks, av, True, names=False)
    seq = [i for i, sp in enumerate(run_b.spans) if sp[0] == S.SEC_SEQ]
    assert [meth_b[i] for i in seq] == [S.LZP3] * 5
    _same(run_a, res_a, meth_a, run_b, res_b, meth_b)
    assert cnt[2] >= 2 and cnt[1] >= cnt[2]      # the two follow sequence sections at least
    _roundtrip(run_b, res_b)


def test_retrial_inside_the_call():
    """110 blocks of a few KB at -3: the re-trial window (blocks 104-106) and
    the blocks after it give a second decision per kind."""
    reads = synth.illumina(1400, seed=23)
    blocks = synth.split_blocks(reads, 3000)[:110]
    assert len(blocks) == 110
    av = S.masks(3)
    run_a, res_a, meth_a, _, _ = _encode(reads, blocks, av, False)
    run_b, res_b, meth_b, cnt, dec = _encode(reads, blocks, av, True)
    _same(run_a, res_a, meth_a, run_b, res_b, meth_b)
    assert dec[S.SEC_SEQ] == 2 and dec[S.SEC_QUAL] == 2
    assert cnt[1] > 0 and cnt[3] > 0
    _roundtrip(run_b, res_b)


def test_carried_state():
    """Blocks 0-4 in one call, 5-9 in a second with the returned state: the
    second call's sections are settled, one candidate each and no second
    stage; the bytes are the one-call run's."""
    reads = synth.illumina(18000, seed=25)
    blocks = synth.split_blocks(reads, 600_000)[:10]
    assert len(blocks) == 10
    av = S.masks(3)
    run_a, res_a, meth_a, _, _ = _encode(reads, blocks, av, True)
    st = S.new_state()
    run_1, res_1, meth_1, _, _ = _encode(reads, blocks[:5], av, True, state=st)
    assert st.sec[S.SEC_SEQ].trial < -1000 and st.sec[S.SEC_QUAL].trial < -1000   # decided
    run_2, res_2, meth_2, cnt, dec = _encode(reads, blocks[5:], av, True, state=st)
    nsq = sum(1 for sp in run_2.spans if sp[0] in (S.SEC_SEQ, S.SEC_QUAL))
    assert nsq == 10
    assert cnt[0] == nsq and cnt[1] == 0 and cnt[2] == 0 and cnt[3] > 0
    assert dec == [0, 0, 0, 0]
    n1 = len(res_1)
    assert meth_1 + meth_2 == meth_a
    for i in range(len(res_a)):
        got = run_1.chosen(res_1, i) if i < n1 else run_2.chosen(res_2, i - n1)
        assert got == run_a.chosen(res_a, i), i
    _roundtrip(run_2, res_2)


@pytest.mark.parametrize("level", [3, 5])
def test_c_api(level):
    """fqz5_encode_sections (try, replay and commit in one C call) uses the
    staged entry: its bytes are encode_run's."""
    reads, blocks, av, run_a, res_a, meth_a, _, _ = _case(level, "illumina", 52000, 2_700_000)
    run = S.Run(reads, blocks, _dev())
    secs = run.enc_secs()
    so = S._load()
    so.fqz5_encode_sections.restype = C.c_int
    so.fqz5_encode_sections.argtypes = [C.POINTER(S.Section), C.c_int, C.POINTER(C.c_uint32),
                                        C.POINTER(S.TrialState), C.POINTER(S.SectionResult)]
    res = (S.SectionResult * len(secs))()
    st = S.new_state()
    avl = np.ascontiguousarray(av, np.uint32)
    c0 = S.staged_counts()
    lib.after_torch()
    rc = so.fqz5_encode_sections(S._arr(S.Section, secs), len(secs),
                                 avl.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st), res)
    assert rc == 0, lib.last_error()
    cnt = tuple(b - a for a, b in zip(c0, S.staged_counts()))
    res = list(res)
    assert all(r.status == 0 for r in res)
    _same(run_a, res_a, meth_a, run, res, [r.method for r in res])
    assert cnt[1] > 0 and cnt[3] > 0
    _roundtrip(run, res)
