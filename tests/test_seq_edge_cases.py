"""The sequence model's edge-case table (seq_edge_cases.py) on the CPU: the
census proves what each input reaches (conditions on the inputs alone), the
oracle round-trips every case and agrees with the golden vectors of the
reference (tests/golden/make_golden_seq_edges.py), and the host decoder
(fqz5_seq_decode_host) returns every input."""
import functools
import hashlib
import json
import os

import pytest

import seq_edge_cases as E
from fqzcomp5_amd import lib
from oracle import binding

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = E.cases()
IDS = [c.name for c in CASES]


def golden():
    g = json.load(open(os.path.join(GOLD, "seq_edges.json")))
    return {r["case"]: r for r in g}, open(os.path.join(GOLD, "seq_edges.bin"), "rb").read()


@functools.lru_cache(maxsize=None)
def hz(name):
    c = E.by_name(name)
    return E.hazards(c.seq, c.lens, c.k, c.both)


@functools.lru_cache(maxsize=None)
def mr(name):
    c = E.by_name(name)
    return E.model_runs(c.seq, c.lens, c.k, c.both)


@functools.lru_cache(maxsize=None)
def oracle_stream(name):
    c = E.by_name(name)
    return binding.seq_oracle().encode(c.seq, c.lens, c.both, c.k)


def test_declared_minima():
    for c in CASES:
        for key, want in c.want.items():
            if key == "hz":
                h = hz(c.name)
                for t, least in want.items():
                    assert h[t] >= least, (c.name, t, h[t])
            elif key == "runs":
                assert all(r in mr(c.name)["runs"] for r in want), (c.name, want)
            elif key == "span":
                assert mr(c.name)["span"] == want, (c.name, mr(c.name)["span"])
            else:
                assert mr(c.name)[key] >= want, (c.name, key, mr(c.name)[key])
    assert all(c.want for c in CASES)


def _brute(k, term):
    """record_reaching's answer by trying every record of up to k + 1 bases"""
    mask, top = (1 << (2 * k)) - 1, 2 * k - 2

    def rec(fw, rv, depth):
        for b in range(4):
            fn, rn = ((fw << 2) + b) & mask, (rv >> 2) + ((3 - b) << top)
            if (fn == rn if term == "fn_rn" else rn == fw) or (depth < k and rec(fn, rn, depth + 1)):
                return True
        return False
    return rec(*E.seeds(k), 0)


def test_forwarding_terms_reached():
    """Each of the seven forwarding terms at least 50 times in one case at an
    odd look-ahead k, at an even one and at k = 3, and k_seq_dec's own three at
    k = 1 or 2 — but for fn == rn at odd k and rn == fw at even k, which no
    input reaches at any k (record_reaching; every record of up to k + 1 bases
    tried for k <= 6)."""
    for k in range(1, 15):
        for term in ("fn_rn", "rn_fw"):
            can = E.record_reaching(k, term) is not None
            assert can == ((term == "fn_rn") == (k % 2 == 0)), (k, term)
            if k <= 6:
                assert _brute(k, term) == can, (k, term)
    both = [c for c in CASES if c.both and len(c.seq) <= 20000]
    classes = {"odd": [c for c in both if c.k >= 3 and c.k % 2], "even": [c for c in both if c.k >= 4 and not c.k % 2],
               "k3": [c for c in both if c.k == 3], "one_step": [c for c in both if c.k <= 2]}
    for cls, cs in classes.items():
        for t in E.ONE_STEP_TERMS if cls == "one_step" else E.TERMS:
            if (t, cls) in (("fn_rn", "odd"), ("fn_rn", "k3"), ("rn_fw", "even")):
                assert all(hz(c.name)[t] == 0 for c in cs), (t, cls)
                continue
            assert max(hz(c.name)[t] for c in cs) >= 50, (t, cls)
    # and one strand, where only fw's own stores are forwarded
    one = [c for c in CASES if not c.both and len(c.seq) <= 20000]
    for lo, hi in ((1, 2), (3, 3), (4, 13)):
        for t in ("fn_fw", "fn_hf"):
            assert max(hz(c.name)[t] for c in one if lo <= c.k <= hi) >= 50, (t, lo)
    # every distance and both histories of the look-ahead ring
    for t in ("fn_hf1", "fn_hf2", "fn_hr1", "fn_hr2", "rn_hf1", "rn_hf2", "rn_hr1", "rn_hr2"):
        assert max(hz(c.name)[t] for c in classes["odd"] + classes["even"]) >= 50, t
    # pieces of 1..4 bases and ending at every ring position, at k >= 3
    for key in [("len", L) for L in (1, 2, 3, 4)] + [("ring", r) for r in (0, 1, 2)]:
        assert sum(hz(c.name)[key] for c in both if c.k >= 3) >= 50, key


def test_table_covers():
    kb = {(c.k, c.both) for c in CASES}
    assert kb >= {(k, b) for k in range(1, 14) for b in (0, 1)}
    assert [(c.k, c.both) for c in CASES if c.k > 13] == [(14, 1)]
    # every listed run length, from one symbol and from mixed ones, with one
    # strand and with both
    for tag in ("run1", "runx"):
        for b in (0, 1):
            got = set()
            for c in CASES:
                if c.name.startswith(tag) and c.both == b:
                    got |= set(mr(c.name)["runs"])
            assert got >= set(E.RUN_LENGTHS), (tag, b)
    spans = {mr(c.name)["span"] for c in CASES if len(c.seq)}
    assert {256, 4096} <= spans and len(spans) > 4
    # k_seq_ctx: a record longer than a window, a literal run across a
    # window's end, 64 / 65 / 128 / 129 segments, a long record in a group of
    # 64 segments with one-base records, a zero-length record before a long one
    nseg = {len(E.segments(c.lens, len(c.seq))) - 1 for c in CASES}
    assert {64, 65, 128, 129} <= nseg
    c = E.by_name("long_beside_ones_k10b1")
    seg = E.segments(c.lens, len(c.seq))
    assert seg[21] - seg[20] == 5000 and len(seg) - 1 > 64 and seg[63] - seg[62] == 1
    c = E.by_name("zero_then_long_k11b1")
    assert E.segments(c.lens, len(c.seq)) == [0, len(c.seq)] and len(c.seq) > 2 * E.SEQ_CTX_W
    c = E.by_name("lit_window_k12b1")
    assert c.seq[E.SEQ_CTX_W - 3:E.SEQ_CTX_W + 3] == b"N" * 6


def test_compressed_lengths_cover_every_residue():
    gold, _ = golden()
    assert {gold[c.name]["len"] % 16 for c in CASES} == set(range(16))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_round_trip_and_golden(case):
    gold, blob = golden()
    z = oracle_stream(case.name)
    assert binding.seq_oracle().decode(z, case.lens, case.both, case.k, len(case.seq)) == case.seq
    r = gold[case.name]
    assert (r["k"], r["both"], r["n"]) == (case.k, case.both, len(case.seq))
    assert (len(z), hashlib.md5(z).hexdigest()) == (r["len"], r["md5"])
    if r["off"] is not None:
        assert blob[r["off"]:r["off"] + r["len"]] == z


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_decoder(case):
    z = oracle_stream(case.name)
    assert lib.seq_decode(z, case.lens, case.both, case.k, len(case.seq), host=True) == case.seq


@pytest.mark.skipif(not binding.have_seq_ref(), reason="oracle/_ref not built")
def test_reference_gives_the_oracles_bytes():
    ref = binding.seq_ref()
    for c in CASES:
        assert ref.encode(c.seq, c.lens, c.both, c.k) == oracle_stream(c.name), c.name


def test_host_decoder_context_size_bounds():
    # as the GPU entries: 1..14.  (With nothing to decode no stream is
    # damaged: the refusal is the bound's.)
    c = E.by_name("terms_k2b1")
    z = oracle_stream(c.name)
    for k in (0, 15, 16, -1):
        for n in (len(c.seq), 0):
            with pytest.raises(lib.NativeError):
                lib.seq_decode(z, c.lens, c.both, k, n, host=True)
    assert lib.seq_decode(z, c.lens, c.both, 14, 0, host=True) == b""
