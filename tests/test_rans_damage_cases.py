"""The damaged rANS 4x16 corpus (rans_damage_cases.py) against its fixture
(golden/rans_damaged.json, the compiled reference's outcomes): the corpus is
what the fixture recorded, its header walker tiles every base stream, its
chain-length bound holds, the oracle (and the reference, where built here)
gives the recorded outcome on every case, and the RLE expansion's run
arithmetic ends and refuses runs past the output."""
import json
import os

import pytest

import rans_damage_cases as rd
from fqzcomp5_amd import lib
from oracle import binding

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "rans_damaged.json")) as f:
        return json.load(f)


def test_corpus_is_the_fixtures(fixture):
    corpus = rd.corpus()
    assert fixture["excluded"] == 0
    assert len(corpus) == fixture["count"] == len(fixture["cases"])
    got = [[name, rd.md5(s), cap] for name, _, s, cap in corpus]
    assert got == [c[:3] for c in fixture["cases"]]
    # the damage is real: every class has a refused case, some case decodes to other bytes
    for mc, c in fixture["classes"].items():
        assert c["cases"] == sum(1 for x in corpus if x[1] == mc)
        assert mc == "base" or c["null"] > 0, mc
    assert sum(c["other"] for c in fixture["classes"].values()) > 0
    assert sum(c["stale"] for c in fixture["classes"].values()) <= 3


def test_walker_tiles_every_base():
    for name, _, stream, data in rd.bases():
        w = rd.Walk(stream, len(data))
        p = 0
        for f, a, e in w.fields:
            assert a == p and e > a and f != "rest", (name, f, a, e)
            p = e
        assert p == len(stream), name


def test_bases_reach_each_boundary():
    by = {name: (stream, data) for name, _, stream, data in rd.bases()}
    v = rd.Walk(by["rle_raw/o40"][0]).vals
    assert v["um"] & 1
    for o in ("o40", "o41"):
        v = rd.Walk(by[f"rle_big/{o}"][0]).vals
        assert v["rl"] > rd.RLE_CHUNK and not v["um"] & 1
    assert rd.Walk(by["o1comp/70001"][0]).vals["o1hdr"] & 1
    assert sorted({len(d) for n, (s, d) in by.items() if n.startswith("stripe4/")}) == [21, 1027, 40001]
    assert by["pack17/o80"][0][3] == 17


def test_chain_lengths_are_bounded():
    for name, _, stream, cap in rd.corpus():
        rd.check_bound(stream, cap)
        v = rd.Walk(stream, cap).vals
        for k, x in v.items():
            f = k.split(".")[-1]
            if f == "u" or f == "um":
                assert x >> (f == "um") <= 1 << 17, (name, k, x)
        assert cap <= 150_001, name


def _compare(codec, fixture):
    """"stale" cases (make_golden_rans_damaged.py: the reference decodes them
    from tables an earlier call left behind) have no recorded outcome: the
    oracle gives the same one twice, and test_rans_damaged_gpu.py holds the
    GPU to it."""
    bad = []
    for (name, _, stream, cap), rec in zip(rd.corpus(), fixture["cases"]):
        r = codec.rans_uncompress_to(stream, cap)
        got = None if r is None else [len(r), rd.md5(r)]
        want = rec[3]
        if want == "stale":
            if codec is not binding.oracle():
                continue
            r = codec.rans_uncompress_to(stream, cap)
            want = None if r is None else [len(r), rd.md5(r)]
        if got != want:
            bad.append((name, got, want))
    assert not bad, (len(bad), bad[:20])


def test_oracle_gives_the_recorded_outcomes(fixture):
    _compare(binding.oracle(), fixture)


@pytest.mark.skipif(not binding.have_ref(), reason="the reference is not built here")
def test_reference_still_gives_the_recorded_outcomes(fixture):
    _compare(binding.ref(), fixture)


def test_bases_decode_to_their_data(fixture):
    rec = {c[0]: c for c in fixture["cases"]}
    for name, _, stream, data in rd.bases():
        assert rec[name + ":base"][3] == [len(data), rd.md5(data)], name


# ---- the run arithmetic of the RLE expansion (kernels.h unrle_*) -------------

NOUT = 1000


@pytest.mark.parametrize("runs, fits", [
    (rd.varint(NOUT - 1), True),                 # the run ends exactly at nout
    (rd.varint(NOUT), False),                    # one past
    (rd.varint(0x7fffffff), False),
    (rd.varint(0xffffffff), False),
    (b"\x8f\xff\xff\xff\xff\x7f", False),        # a 6-byte varint
])
def test_unrle_run_saturates(runs, fits):
    end, trips, longest = lib.unrle_selftest(runs, 1, NOUT, 0)
    assert trips <= NOUT and longest <= NOUT     # the write loop ends inside the output
    assert (end <= NOUT) == fits
    assert end == (NOUT if fits else NOUT + 1)


@pytest.mark.parametrize("nout", [1000, 65535, 65536, 150_001, (1 << 32) - 2])
def test_unrle_sizes_never_wrap(nout):
    # 70 000 literals of run 2^32 - 1 (each adds 0 in 32-bit arithmetic), and
    # of a run that fits once: per-literal sizes of nout + 1 summed over more
    # than 65 536 literals stay at nout + 1
    for r in (0xffffffff, 0x7fffffff, nout - 1, nout):
        end, trips, longest = lib.unrle_selftest(rd.varint(r) * 70_000, 70_000, nout, 0)
        assert end == nout + 1 and trips <= nout and longest <= nout, (r, end, trips)
    # from an offset past the output nothing is written
    end, trips, _ = lib.unrle_selftest(rd.varint(5) * 10, 10, nout, nout)
    assert end == nout + 1 and trips == 0
    # sound runs add up exactly
    end, trips, _ = lib.unrle_selftest(rd.varint(3) * 100, 100, nout, 7)
    assert end == 407 and trips == 400
