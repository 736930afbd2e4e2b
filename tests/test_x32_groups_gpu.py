"""The lane-group form of the 32-state rANS encoder chain (k_enc_chain_x32g:
eight one-wave workgroups of four states per job) against the oracle and
against the one-wave chain, bit-exact, with the proof of which body ran
(fqz5_rans_variant_counts).  The threshold is forced to 0 so that the small
inputs of x32_groups_cases.py run as groups; all chains run on the GPU."""
import hashlib
import json
import os
import subprocess
import sys
from collections import Counter

import pytest

import rans_variant_cases as V
import x32_groups_cases as X
from fqzcomp5_amd import lib
from oracle import binding

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_MIN = 1 << 20
SPLIT_MIN = 32 * 256                 # mixed batch: m >= 256 grouped, m < 256 one wave


@pytest.fixture(scope="module", autouse=True)
def _grouped_and_on_the_gpu():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())
    prev_enc = lib.set_host_encode(0)
    prev_min = lib.set_x32_group_min(0)
    assert prev_min == DEFAULT_MIN
    yield
    lib.set_x32_group_min(prev_min)
    lib.set_host_encode(prev_enc)


@pytest.fixture(scope="module")
def ungrouped():
    """Every case's stream from a process started with $FQZ5_X32_GROUPS=0
    (the threshold at 0 there too), by md5, and that process's counters."""
    env = dict(os.environ, FQZ5_X32_GROUPS="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "x32_groups_cases.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert not [k for k, v in rep["enc"].items() if k.startswith("E32G") and v], rep["enc"]
    assert rep["enc"]["E32_O0"] > 0 and rep["enc"]["E32_O1"] > 0 and rep["enc"]["E32_O1_COMPACT"] > 0
    return rep["md5"]


def _delta(before, after):
    return Counter({k: after[k] - before[k] for k in after if after[k] != before[k]})


def _oracle(c):
    return binding.oracle().rans_compress(V.data(c.A, c.kind, c.n), c.order)


@pytest.mark.parametrize("order", [4, 5])
def test_grouped_streams_are_the_oracles_and_the_one_wave_chains(order, ungrouped):
    batch = X.cases(order)
    want = Counter(X.grouped_name(c) for c in batch)
    assert None not in want and len(want) == (2 if order & 1 else 1)
    _, _, e0 = lib.rans_variant_counts()
    outs = X.encode(batch)
    _, _, e1 = lib.rans_variant_counts()
    bad = [c for c, got in zip(batch, outs) if got != _oracle(c)]
    assert not bad, bad[:10]
    bad = [c for c, got in zip(batch, outs)
           if hashlib.md5(got).hexdigest() != ungrouped["%d %s %d %d" % c]]
    assert not bad, bad[:10]
    got = _delta(e0, e1)
    print(dict(got))
    # (an order-1 table of over 1000 bytes is itself coded by an order-0 NX = 4 chain)
    assert 0 <= got.pop("E2W_O0", 0) <= len(batch)
    assert got == want


def _mixed_batch():
    x32 = [c for order in (4, 5) for c in X.cases(order)]
    nx4 = [V.Case(c.A, c.kind, c.n, c.order & 1) for c in x32[::3]]
    return x32 + nx4


def _mixed_want(batch, group_min):
    want = Counter()
    for c in batch:
        g = X.grouped_name(c)
        want[g if g and c.n >= group_min else V.enc_job(c)] += 1
    return want


def _run_mixed(group_min):
    batch = _mixed_batch()
    prev = lib.set_x32_group_min(group_min)
    try:
        _, _, e0 = lib.rans_variant_counts()
        outs = X.encode(batch)
        _, _, e1 = lib.rans_variant_counts()
    finally:
        lib.set_x32_group_min(prev)
    bad = [c for c, got in zip(batch, outs) if got != _oracle(c)]
    assert not bad, bad[:10]
    got, want = _delta(e0, e1), _mixed_want(batch, group_min)
    print(dict(got))
    tables = got["E2W_O0"] - want["E2W_O0"]
    assert 0 <= tables <= sum(1 for c in batch if c.order & 1)
    assert {k: v for k, v in got.items() if k != "E2W_O0"} == \
           {k: v for k, v in want.items() if k != "E2W_O0"}
    return want


def test_a_mixed_batch_runs_grouped_one_wave_and_two_wave_jobs():
    """One launch sequence with lane groups (n >= 8192), one-wave 32-state
    chains (shorter), two-wave and compact NX = 4 chains: every stream is the
    oracle's and every body ran as often as the cases say."""
    want = _run_mixed(SPLIT_MIN)
    assert {"E32G_O0", "E32G_O1", "E32G_O1_COMPACT", "E32_O0", "E32_O1", "E32_O1_COMPACT",
            "E2W_O0", "E2W_O1", "E1W_O1_COMPACT"} <= set(want)


def test_the_default_threshold_keeps_small_jobs_on_the_old_bodies():
    want = _run_mixed(DEFAULT_MIN)
    assert not [k for k in want if k.startswith("E32G")]


def test_a_long_stream_is_grouped_by_default(ungrouped):
    c = V.Case(*X.LZP3, X.BIG_N, 5)
    prev = lib.set_x32_group_min(DEFAULT_MIN)
    try:
        _, _, e0 = lib.rans_variant_counts()
        got = X.encode([c])[0]
        _, _, e1 = lib.rans_variant_counts()
    finally:
        lib.set_x32_group_min(prev)
    assert _delta(e0, e1) == Counter({"E32G_O1": 1})
    assert hashlib.md5(got).hexdigest() == ungrouped["big"]
