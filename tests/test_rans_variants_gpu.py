"""Every body of the rANS chain kernels against the oracle, bit-exact, with the
proof that it ran: the inputs of rans_variant_cases.py select each body of
k_rans_dec (plain and hedged) and each encoder chain by table size, shift,
symbol count and state count, and fqz5_rans_variant_counts says which body a
job was launched with.  All chains run on the GPU here (no host placement)."""
import json
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import rans_variant_cases as V
from fqzcomp5_amd import lib
from host_rans_cases import craft
from oracle import binding

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NBATCH = 6                           # mixed decode / encode batches
ALIGN = 16
GUARD = 0xA5                         # fill of the output buffer between the jobs' bytes
DEC_CLASSES = tuple(V.DEC_CLASS_INPUT)
HEDGE_SEEDS = (0, 1, 2)              # jobs of one hedged batch: equal n, so all get copies


@pytest.fixture(scope="module", autouse=True)
def _all_chains_on_the_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())
    so = lib.load()
    prev_dec = so.fqz5_set_host_decode(0)
    prev_enc = lib.set_host_encode(0)
    prev_hedge = so.fqz5_set_hedge(0)
    yield
    so.fqz5_set_hedge(prev_hedge)
    lib.set_host_encode(prev_enc)
    so.fqz5_set_host_decode(prev_dec)


def _delta(before, after):
    return Counter({k: after[k] - before[k] for k in after if after[k] != before[k]})


def _layout(sizes):
    offs, p = [], 0
    for n in sizes:
        offs.append(p)
        p += (n + ALIGN) // ALIGN * ALIGN            # at least one guard byte behind each
    return offs, p


def _device_batch(ins, caps):
    """The inputs in one device buffer and one guarded output buffer:
    (input offsets, output offsets, tensors)."""
    import torch
    ioff, itot = _layout([len(b) for b in ins])
    ooff, otot = _layout(caps)
    blob = bytearray(itot)
    for o, b in zip(ioff, ins):
        blob[o:o + len(b)] = b
    src = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    dst = torch.full((otot,), GUARD, dtype=torch.uint8, device="cuda")
    lib.after_torch()
    return ioff, ooff, src, dst


def _check_guards(host, ooff, sizes, total):
    for k, (o, n) in enumerate(zip(ooff, sizes)):
        end = ooff[k + 1] if k + 1 < len(ooff) else total
        assert not np.any(host[o + n:end] != GUARD), f"job {k} wrote past its {n} bytes"


def _decode(streams, sizes):
    """fqz5_rans_uncompress_batch of device streams: the outputs."""
    ioff, ooff, src, dst = _device_batch(streams, sizes)
    jobs = [lib.RansJob(src.data_ptr() + i, dst.data_ptr() + o, len(s), n, 0, 0, 0, 0)
            for i, o, s, n in zip(ioff, ooff, streams, sizes)]
    lib.uncompress_batch_dev(jobs)
    host = dst.cpu().numpy()
    bad = [(k, j.status, j.out_size) for k, (j, n) in enumerate(zip(jobs, sizes))
           if j.status != 0 or j.out_size != n]
    assert not bad, bad[:10]
    _check_guards(host, ooff, sizes, len(host))
    return [host[o:o + n].tobytes() for o, n in zip(ooff, sizes)]


def _decode_cases(cases):
    outs = _decode([V.stream(c) for c in cases], [c.n for c in cases])
    bad = [c for c, got in zip(cases, outs) if got != V.data(c.A, c.kind, c.n)]
    assert not bad, bad[:10]


# ---- decode, one copy per job ------------------------------------------------

def test_mixed_batches_decode_and_every_body_runs():
    """Every case, in batches that each carry all kinds of job (a launch has
    lean, LDS, SPLIT, GLOBAL and X32 jobs under its largest LDS size): the
    inputs come back, and each batch launches exactly the bodies dec_jobs
    reads off its streams; over all batches every body but O1REG* ran."""
    cases = V.all_cases()
    total = Counter()
    for k in range(NBATCH):
        batch = cases[k::NBATCH]
        want = V.dec_count(batch)
        assert {"O0_LEAN", "O1_LEAN", "O1_SPLIT", "O1_GLOBAL", "X32_O1_LDS"} <= set(want)
        d0, h0, _ = lib.rans_variant_counts()
        _decode_cases(batch)
        d1, h1, _ = lib.rans_variant_counts()
        print(f"batch {k}: {dict(_delta(d0, d1))}")
        assert _delta(d0, d1) == want, k
        assert not _delta(h0, h1), k
        total += _delta(d0, d1)
    missing = [c for c in DEC_CLASSES if total[c] <= 0]
    assert not missing, missing
    assert not [c for c in total if c.startswith("O1REG")]


@pytest.mark.parametrize("name", DEC_CLASSES)
def test_a_class_input_runs_its_body(name):
    """One job, one launch: the counter that moves is the class's (and, for a
    compressed order-1 table, the order-0 chain of the table before it)."""
    A, kind, order = V.DEC_CLASS_INPUT[name]
    c = V.Case(A, kind, V.CLASS_N, order)
    want = V.dec_jobs(V.stream(c))
    assert want[0] == name and all(w.startswith("O0_") for w in want[1:])
    d0, _, _ = lib.rans_variant_counts()
    _decode_cases([c])
    d1, _, _ = lib.rans_variant_counts()
    assert _delta(d0, d1) == Counter(want)


@pytest.mark.parametrize("states", [4, 32])
@pytest.mark.parametrize("rows,bits,name", [(r, b, nm) for (r, b), nm in V.THRESHOLDS])
def test_a_stream_at_a_threshold_runs_the_body_of_its_side(rows, bits, name, states):
    """One job, one launch, for a stream on each side of every threshold of
    the order-1 table placement: the body listed in THRESHOLDS runs it."""
    c = V.o1_pairs()[(states, rows, bits)][0]
    name = name if states == 4 else V.x32_name(name)
    want = V.dec_jobs(V.stream(c))
    assert want[0] == name
    d0, _, _ = lib.rans_variant_counts()
    _decode_cases([c])
    d1, _, _ = lib.rans_variant_counts()
    assert _delta(d0, d1) == Counter(want), c


def test_transforms_in_front_decode():
    _decode_cases(V.transform_cases())


# ---- decode, hedged ----------------------------------------------------------

@pytest.mark.parametrize("n", [V.CLASS_N, 777, 1024, 2048])
def test_hedged_copies_give_the_same_bytes(n):
    """Per class a launch of three equal-length jobs, fewer than CUs, so every
    job runs in several copies that race group by group (hedge_claim /
    hedge_first / hedge_lost): the bytes of the single-copy run, and each job
    counted as hedged under the body its stream selects.  40003 bytes are
    many groups of every body, 777 less than one (and, under 1000 bytes, four
    states), 1024 and 2048 end on a group's edge."""
    ora = binding.oracle()
    so = lib.load()
    total = Counter()
    batches = [(name, A, kind, order, None) for name, (A, kind, order) in V.DEC_CLASS_INPUT.items()]
    if n == 777:
        # The reference stores 777 bytes over 64 or 128 symbols uncoded, and
        # codes short inputs with 10-bit frequencies: no stream of its own
        # runs the SPLIT or GLOBAL body for less than a group.  Streams coded
        # from the format with 12-bit frequencies do (host_rans_cases.craft):
        # 16 rows are a SPLIT table, 64 a GLOBAL one.
        batches += [("O1_SPLIT", 16, "walk", 1, 12), ("O1_GLOBAL", 64, "walk", 1, 12)]
    for name, A, kind, order, craft_bits in batches:
        datas = [V.data(A, kind, n, seed) for seed in HEDGE_SEEDS]
        if craft_bits:
            streams = [craft(d, order, craft_bits) for d in datas]
            assert all(V.dec_jobs(s) == [name] for s in streams)
            assert all(ora.rans_uncompress(s) == d for s, d in zip(streams, datas))
        else:
            streams = [ora.rans_compress(d, order) for d in datas]
        want = Counter()
        for s in streams:
            want.update(V.dec_jobs(s))
        plain = _decode(streams, [n] * len(streams))
        assert plain == datas, name
        so.fqz5_set_hedge(1)
        try:
            d0, h0, _ = lib.rans_variant_counts()
            hedged = _decode(streams, [n] * len(streams))
            d1, h1, _ = lib.rans_variant_counts()
        finally:
            so.fqz5_set_hedge(0)
        assert hedged == plain, name
        print(f"{name} n={n}: hedged {dict(_delta(h0, h1))}")
        assert _delta(d0, d1) == want, name
        assert _delta(h0, h1) == want, name
        total += _delta(h0, h1)
    if n == V.CLASS_N:
        missing = [c for c in DEC_CLASSES if total[c] <= 0]
        assert not missing, missing


# ---- encode -------------------------------------------------------------------

@pytest.mark.parametrize("order", V.ORDERS + (65, 129, 193))
def test_encoder_makes_the_oracle_stream(order):
    cases = [c for c in V.all_cases() + V.transform_cases() if c.order == order]
    bad = [c for c in cases if lib.rans_compress(V.data(c.A, c.kind, c.n), c.order) != V.stream(c)]
    assert not bad, bad[:10]


def _encode(cases):
    """fqz5_rans_compress_batch of device inputs: the streams."""
    datas = [V.data(c.A, c.kind, c.n) for c in cases]
    caps = [lib.compress_bound(c.n, c.order) for c in cases]
    ioff, ooff, src, dst = _device_batch(datas, caps)
    jobs = [lib.RansJob(src.data_ptr() + i, dst.data_ptr() + o, len(d), cap, c.order, 0, 0, 0)
            for i, o, d, cap, c in zip(ioff, ooff, datas, caps, cases)]
    lib.compress_batch_dev(jobs)
    host = dst.cpu().numpy()
    assert all(j.status == 0 for j in jobs)
    _check_guards(host, ooff, [j.out_size for j in jobs], len(host))
    return [host[o:o + j.out_size].tobytes() for o, j in zip(ooff, jobs)]


def test_mixed_batches_encode_and_every_chain_runs():
    """The batch form, every batch with all six kinds of chain: the oracle's
    streams, and each chain kernel variant launched as often as enc_job says
    (E2W_O0 more often: an order-1 table of over 1000 bytes is itself coded
    by an order-0 chain)."""
    cases = V.all_cases()
    total = Counter()
    for k in range(NBATCH):
        batch = cases[k::NBATCH]
        want = Counter(V.enc_job(c) for c in batch)
        del want[None]
        assert set(want) == set(V.ENC_CLASS_INPUT)
        _, _, e0 = lib.rans_variant_counts()
        outs = _encode(batch)
        _, _, e1 = lib.rans_variant_counts()
        bad = [c for c, got in zip(batch, outs) if got != V.stream(c)]
        assert not bad, bad[:10]
        got = _delta(e0, e1)
        print(f"batch {k}: {dict(got)}")
        tables = got["E2W_O0"] - want["E2W_O0"]
        assert 0 <= tables <= sum(1 for c in batch if c.order & 1), k
        assert {c: v for c, v in got.items() if c != "E2W_O0"} == \
               {c: v for c, v in want.items() if c != "E2W_O0"}, k
        total += got
    assert all(total[c] > 0 for c in V.ENC_CLASS_INPUT), total


@pytest.mark.parametrize("name", tuple(V.ENC_CLASS_INPUT))
def test_a_class_input_runs_its_encoder_chain(name):
    A, kind, order = V.ENC_CLASS_INPUT[name]
    c = V.Case(A, kind, V.CLASS_N, order)
    d = V.data(A, kind, c.n)
    _, _, e0 = lib.rans_variant_counts()
    got = lib.rans_compress_to(d, order, lib.compress_bound(len(d), order))
    _, _, e1 = lib.rans_variant_counts()
    assert got == V.stream(c)
    delta = _delta(e0, e1)
    table = delta - Counter({name: 1})           # the order-0 chain of a big order-1 table
    assert delta[name] >= 1 and table in (Counter(), Counter({"E2W_O0": 1})), delta


# ---- the opt-in order-1 register decoder --------------------------------------

def test_o1_register_decoder_in_a_child_process():
    """dec4_o1reg_body<1..4> runs only in a process started with
    $FQZ5_O1REG=1 (rans_decompress.cpp o1reg_decoder): o1reg_child.py decodes
    the order-1 cases of up to 16 symbols there, plain and hedged."""
    env = dict(os.environ, FQZ5_O1REG="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "o1reg_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["cases"] > 0 and rep["bad"] == [], rep["bad"][:10]
    for k in ("O1REG1", "O1REG2", "O1REG3", "O1REG4"):
        assert rep["dec"][k] > 0 and rep["hedged"][k] > 0, (k, rep)
