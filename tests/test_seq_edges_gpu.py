"""The sequence context model's kernels on the GPU at their edges: the case
table of seq_edge_cases.py (every context size of 1..14, both decoders'
forwarding terms, the model pass's lane / wave split and tiles, k_seq_ctx's
windows and segment groups) against the reference's golden vectors
(tests/golden/make_golden_seq_edges.py), fqz5_seq_path_counts for the path
each call took, and fqz5_seq_decode_many for batches, misaligned input and
per-stream statuses."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seq_edge_cases as E
from fqzcomp5_amd import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = E.cases()
GROUPS = ("rep_", "cut_", "terms_", ("onebase_", "long_", "zero_", "lit_"), "run1_", "runx_", "span", "poly")
IDS = [g if isinstance(g, str) else g[0] + "etc" for g in GROUPS]
assert all(sum(c.name.startswith(g) for g in GROUPS) == 1 for c in CASES)


@pytest.fixture(scope="module")
def gold():
    g = json.load(open(os.path.join(HERE, "golden", "seq_edges.json")))
    blob = open(os.path.join(HERE, "golden", "seq_edges.bin"), "rb").read()
    recs = {r["case"]: r for r in g}
    streams = {n: blob[r["off"]:r["off"] + r["len"]] for n, r in recs.items() if r["off"] is not None}
    return recs, streams


def delta(before):
    after = lib.seq_path_counts()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def dec_path(k):
    return "dec_one_step" if k <= 2 else "dec_lookahead"


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_encode_golden(group, gold):
    """Every case gives the reference's bytes (length and md5), through one
    k_seq_model_runs launch of the tile width the census predicts.  The poly
    group is the tightest input of the encoder's size bounds (a size outside
    [lb, ub] raises)."""
    recs, _ = gold
    for c in (c for c in CASES if c.name.startswith(group)):
        before = lib.seq_path_counts()
        z = lib.seq_encode(c.seq, c.lens, c.both, c.k)
        span = E.model_span(len(c.seq) * (1 + c.both), c.k)
        assert delta(before) == {"model_span_%d" % span: 1}, c.name
        assert (len(z), hashlib.md5(z).hexdigest()) == (recs[c.name]["len"], recs[c.name]["md5"]), c.name


@pytest.mark.parametrize("group", GROUPS, ids=IDS)
def test_decode_golden(group, gold):
    """Every kept reference stream gives back the input: k = 1, 2 by
    k_seq_dec, k = 3..14 by k_seq_dec_la, one job each."""
    _, streams = gold
    n = 0
    for c in (c for c in CASES if c.name.startswith(group)):
        before = lib.seq_path_counts()
        out = lib.seq_decode(streams[c.name], c.lens, c.both, c.k, len(c.seq))
        assert delta(before) == {dec_path(c.k): 1}, c.name
        assert out == c.seq, c.name
        n += 1
    assert n


def test_every_stream_is_kept(gold):
    recs, streams = gold
    assert set(streams) == {c.name for c in CASES}
    assert {recs[c.name]["len"] % 16 for c in CASES} == set(range(16))
    assert {(c.k, c.both) for c in CASES} >= {(k, b) for k in range(1, 14) for b in (0, 1)} | {(14, 1)}


def _eight(gold):
    """Eight streams of k = 1, 2, 3, 10, 13 and both strand modes whose
    starts, packed back to back, all differ mod 16"""
    recs, streams = gold
    pool = [c for c in CASES if 64 <= recs[c.name]["len"] <= 3000 and len(c.seq) >= 300]
    picked, off, used = [], 0, {0}
    for i, k in enumerate((1, 13, 2, 3, 10, 1, 3, 2)):
        for c in pool:
            nxt = (off + recs[c.name]["len"]) % 16
            if c.k == k and c.both == (i & 1) and c not in picked and (i == 7 or nxt not in used):
                picked.append(c)
                off += recs[c.name]["len"]
                used.add(nxt)
                break
    assert len(picked) == 8 and len(used) == 8, [c.name for c in picked]
    assert {c.k for c in picked} == {1, 2, 3, 10, 13} and {c.both for c in picked} == {0, 1}
    return picked, [(streams[c.name], c.lens, c.both, c.k, len(c.seq)) for c in picked]


@pytest.mark.parametrize("in_offset", (0, 1, 7, 15))
def test_decode_many(in_offset, gold):
    picked, jobs = _eight(gold)
    before = lib.seq_path_counts()
    got = lib.seq_decode_many(jobs, in_offset)
    assert delta(before) == {"dec_lookahead": sum(c.k >= 3 for c in picked),
                             "dec_one_step": sum(c.k <= 2 for c in picked)}
    for c, (st, out) in zip(picked, got):
        assert st == 0 and out == c.seq, (c.name, st)


@pytest.mark.parametrize("victim", (2, 3))          # a one-step job, a look-ahead job
def test_decode_many_one_damaged(victim, gold):
    picked, jobs = _eight(gold)
    assert dec_path(picked[victim].k) == ("dec_one_step", "dec_lookahead")[victim - 2]
    z = jobs[victim][0]
    jobs[victim] = (z[:len(z) // 2],) + jobs[victim][1:]
    got = lib.seq_decode_many(jobs, 7)
    for i, (c, (st, out)) in enumerate(zip(picked, got)):
        if i == victim:
            assert st == -1, c.name
        else:
            assert st == 0 and out == c.seq, (c.name, st)


def test_decode_many_refuses_per_stream(gold):
    # a context size out of range and records that run out: that stream's
    # status alone
    picked, jobs = _eight(gold)
    jobs[1] = jobs[1][:3] + (15,) + jobs[1][4:]
    jobs[4] = (jobs[4][0], [10, 10], *jobs[4][2:])
    got = lib.seq_decode_many(jobs, 3)
    for i, (c, (st, out)) in enumerate(zip(picked, got)):
        if i in (1, 4):
            assert st == -1, c.name
        else:
            assert st == 0 and out == c.seq, (c.name, st)
    assert lib.seq_decode_many([], 0) == []
    with pytest.raises(lib.NativeError):
        lib.seq_decode_many(jobs, 16)


def test_per_event_model_pass_in_a_child_process(gold):
    """$FQZ5_SEQ_MODEL_EVENTS is read once per process: seq_model_child.py
    encodes the run-length and tile cases there through k_seq_model."""
    env = dict(os.environ, FQZ5_SEQ_MODEL_EVENTS="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "seq_model_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(rep)
    assert rep["cases"] > 60 and rep["bad"] == [], rep["bad"][:10]
    assert {k: v for k, v in rep["counts"].items() if v} == {"model_events": rep["cases"]}


@pytest.mark.parametrize("group", ("rep_", "terms_k"))
def test_damaged_streams(group, gold):
    """Cut and byte-flipped streams of the repeat and small-k cases: each call
    raises NativeError or returns out_size bytes (test_seq_host_damaged's
    contract), and a valid decode straight after is exact."""
    _, streams = gold
    rng = np.random.default_rng(31)
    for c in (c for c in CASES if c.name.startswith(group) and (group == "rep_" or c.k <= 5)):
        z = streams[c.name]
        bad = [z[:7], z[:len(z) // 2]]
        for _ in range(3):
            b = bytearray(z)
            for j in rng.integers(4, len(z), 2):
                b[int(j)] ^= int(rng.integers(1, 256))
            bad.append(bytes(b))
        for s in bad:
            try:
                assert len(lib.seq_decode(s, c.lens, c.both, c.k, len(c.seq))) == len(c.seq)
            except lib.NativeError:
                pass
        assert lib.seq_decode(z, c.lens, c.both, c.k, len(c.seq)) == c.seq, c.name


def test_context_size_bounds():
    c = E.by_name("terms_k2b1")
    for k in (0, 15):
        with pytest.raises(lib.NativeError):
            lib.seq_encode(c.seq, c.lens, c.both, k)
        for host in (False, True):
            for n in (len(c.seq), 0):       # (0: no stream is damaged, the bound refuses)
                with pytest.raises(lib.NativeError):
                    lib.seq_decode(b"\x00" * 64, c.lens, c.both, k, n, host=host)
