"""rans_uncompress_to_4x16 on the GPU over the damaged-stream corpus
(rans_damage_cases.py): NULL exactly where the compiled reference returned
NULL, else its bytes (golden/rans_damaged.json); in a batch a damaged job
leaves every byte outside its own capacity alone.  A "stale" case (the
reference decodes it from tables an earlier call left behind,
make_golden_rans_damaged.py) is held to the oracle's outcome instead: its
tables start zeroed, and it refuses an order-1 table without a row for
context 0, in which every state starts."""
import json
import os
import time

import numpy as np
import pytest

import rans_damage_cases as rd
from fqzcomp5_amd import lib
from oracle import binding

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 0xA5
EDGE = 64                            # guard bytes before the first and after the last job


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def expected():
    """case name -> None or [length, md5]: the reference's outcome, the
    oracle's for a stale case."""
    with open(os.path.join(HERE, "golden", "rans_damaged.json")) as f:
        fx = json.load(f)
    corpus = rd.corpus()
    assert [c[:3] for c in fx["cases"]] == [[n, rd.md5(s), cap] for n, _, s, cap in corpus]
    ora = binding.oracle()
    out = {}
    for (name, _, stream, cap), rec in zip(corpus, fx["cases"]):
        out[name] = _sig(ora.rans_uncompress_to(stream, cap)) if rec[3] == "stale" else rec[3]
    return out


def _sig(r):
    return None if r is None else [len(r), rd.md5(r)]


def _differs(got, want, cap):
    return got != want


def _report(bad):
    assert not bad, (len(bad), bad[:20])


@pytest.mark.parametrize("mode", [0, 1])
def test_outcomes_equal_reference(mode, expected):
    so = lib.load()
    prev = so.fqz5_set_host_decode(mode)
    try:
        t0 = time.perf_counter()
        for name, _, stream, data in rd.bases():
            assert lib.rans_uncompress_to(stream, len(data)) == data, (mode, name)
        bad = []
        for name, _, stream, cap in rd.corpus():
            got = _sig(lib.rans_uncompress_to(stream, cap))
            if _differs(got, expected[name], cap):
                bad.append((name, got, expected[name]))
        print(f"mode {mode}: {len(rd.corpus())} cases in {time.perf_counter() - t0:.2f} s")
        _report(bad)
    finally:
        so.fqz5_set_host_decode(prev)


def _run_batch(jobs_in):
    """jobs_in: [(name, stream, capacity)].  The outputs lie back to back in
    one buffer filled with GUARD, job i in exactly its capacity:
    [(status, out_size, the bytes of its capacity)], and the guard's verdict."""
    import torch
    caps = [c for _, _, c in jobs_in]
    ooff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64) + EDGE
    ioff = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in jobs_in])]).astype(np.int64)
    blob = bytearray(b"".join(s for _, s, _ in jobs_in)) or bytearray(1)
    src = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    dst = torch.full((int(ooff[-1]) + EDGE,), GUARD, dtype=torch.uint8, device="cuda")
    lib.after_torch()
    jobs = [lib.RansJob(src.data_ptr() + int(i), dst.data_ptr() + int(o), len(s), c, 0, 0, 0, 0)
            for i, o, (_, s, c) in zip(ioff, ooff, jobs_in)]
    lib.uncompress_batch_dev(jobs)
    host = dst.cpu().numpy()
    edges_ok = not np.any(host[:EDGE] != GUARD) and not np.any(host[int(ooff[-1]):] != GUARD)
    return [(j.status, j.out_size, host[int(o):int(o) + c]) for j, o, c in zip(jobs, ooff, caps)], edges_ok


def _check_batch(jobs_in, expected, sound):
    """sound: name -> data of the undamaged jobs of the batch."""
    res, edges_ok = _run_batch(jobs_in)
    bad = []
    if not edges_ok:
        bad.append(("a byte outside every job's capacity was written", jobs_in[0][0], None))
    for (name, _, cap), (status, n, region) in zip(jobs_in, res):
        want = expected[name]
        if want is None:
            # refused: whatever it wrote lies inside `region`; the neighbours'
            # checks and the edges show a write outside it
            if status == 0:
                bad.append((name, [n], None))
            continue
        got = None if status != 0 else [int(n), rd.md5(region[:n].tobytes())]
        if got != want:
            bad.append((name, got, want))
        elif name in sound and region[:n].tobytes() != sound[name]:
            bad.append((name, "sound neighbour damaged", want))
        elif np.any(region[n:] != GUARD):
            # a decoded job's bytes end at its size: the rest of its capacity
            # belongs to it, but nothing of the stream goes there
            bad.append((name, "wrote past its size", want))
    return bad


def test_batch_isolation(expected):
    corpus = rd.corpus()
    data = {name + ":base": d for name, _, _, d in rd.bases()}
    by_base = {}
    for name, mc, stream, cap in corpus:
        by_base.setdefault(rd.base_of(name), []).append((name, stream, cap))
    t0 = time.perf_counter()
    bad, nb = [], 0
    for base, cases in by_base.items():
        sound_case = cases[0]                     # the group's undamaged stream
        assert expected[sound_case[0]] is not None
        for k in range(0, len(cases), 32):
            batch = []
            for c in cases[k:k + 32]:
                batch.append(sound_case)          # a sound stream before every damaged one:
                batch.append(c)                   # an overrun of any job lands in a checked one
            assert len(batch) <= 64
            bad += _check_batch(batch, expected, data)
            nb += 1
    print(f"{len(corpus)} cases in {nb} batches, {time.perf_counter() - t0:.2f} s")
    _report(bad)


def test_rle_run_bounds(expected):
    """Run lengths of 2^31 - 1, 2^32 - 1, a 6-byte varint and runs that end at
    and one byte past the stored size, at the last literal and at the first,
    in the first and the second chunk of literals: refused or decoded as the
    reference does, one call each and all in one batch."""
    cases = rd.run_cases()
    t0 = time.perf_counter()
    bad = []
    for name, _, stream, cap in cases:
        got = _sig(lib.rans_uncompress_to(stream, cap))
        if _differs(got, expected[name], cap):
            bad.append((name, got, expected[name]))
    bad += _check_batch([(n, s, c) for n, _, s, c in cases], expected, {})
    print(f"{len(cases)} run cases in {time.perf_counter() - t0:.2f} s")
    assert sum(expected[n] is None for n, _, _, _ in cases) >= 10
    _report(bad)
