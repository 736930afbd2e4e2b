"""The plain rANS 4x16 decoders on a host core (host_rans.cpp behind
fqz5_rans_dec_host) and the placement plan with pre-loaded cores.  CPU tests:
the library's own C++ decoder against the reference's golden vectors, the
oracle's streams of seeded data (sizes 0..70 001; one symbol, two, ACGTN, all
256; order-1 with TF_SHIFT 10, 12 and a compressed table), hand-coded tiny
entropy streams (every n % 4 tail, the order-1 quarter split), damaged streams,
and the same under AddressSanitizer / UBSan in a stand-alone program."""
import os
import shutil
import struct
import subprocess

import host_rans_cases as hc
from fqzcomp5_amd import lib
from oracle import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden_plain(golden_rans):
    inputs, cases = golden_rans
    return [(f"{name}/{order}", exp, inputs[name]) for name, order, ln, md5, exp in cases
            if exp is not None and order in (0, 1)]


def test_golden(golden_rans):
    n = 0
    for name, comp, data in _golden_plain(golden_rans):
        got = lib.rans_dec_host(comp, len(data))
        if comp[0] & ~hc.PLAIN:
            assert got is None, name            # stored uncoded: not this decoder's
            continue
        assert got == data, name
        n += 1
    assert n > 10


def test_oracle_streams_and_crafted():
    coded = {}
    for name, comp, data in hc.streams():
        got = lib.rans_dec_host(comp, len(data) if data is not None else 70001)
        assert got == data, name
        if data is not None:
            coded[name] = comp
    # the cases the sizes and alphabets are there for
    for n in (1023, 1027, 70001):
        for a in ("one", "two", "acgtn", "o1_shift10"):
            assert f"{a}/{n}/o0" in coded and f"{a}/{n}/o1" in coded, (a, n)
    assert "all256/70001/o0" in coded and "all256/70001/o1" in coded
    assert hc.o1_header(coded["o1_shift10/70001/o1"]) == (10, 0)
    assert hc.o1_header(coded["o1_shift12/70001/o1"]) == (12, 0)
    assert hc.o1_header(coded["o1_comp_table/70001/o1"])[1] == 1
    assert sum(k.startswith("craft/") for k in coded) == 9 * 4 * 3


def test_crafted_streams_are_the_format():
    """The hand-coded streams decode with the reference's decoder too."""
    ora = binding.oracle()
    for name, comp, data in hc.streams():
        if name.startswith("craft/"):
            assert ora.rans_uncompress(comp) == data, name


def test_other_orders_refused():
    d = hc.alphabets(1027)["acgtn"].tobytes()
    ora = binding.oracle()
    refused = 0
    for order in (4, 5, 64, 65, 128, 129, 193, (4 << 8) | 8):
        comp = ora.rans_compress(d, order)
        if comp[0] & ~hc.PLAIN:
            assert lib.rans_dec_host(comp, len(d)) is None, order
            refused += 1
        else:                                   # (the encoder dropped a transform that did not pay)
            assert lib.rans_dec_host(comp, len(d)) == d, order
    assert refused >= 5
    assert lib.rans_dec_host(b"", 10) is None
    # the size is the capacity: a stream that claims more is refused
    comp = ora.rans_compress(d, 0)
    assert lib.rans_dec_host(comp, len(d) - 1) is None


def test_damaged_streams_fail_or_decode():
    for order, (comp, data) in enumerate(hc.small_pair()):
        assert lib.rans_dec_host(comp, len(data)) == data
        for bad in hc.damaged(comp, order):
            got = lib.rans_dec_host(bad, len(data))
            assert got is None or len(got) <= len(data)


def test_sanitized_program(tmp_path, golden_rans):
    """host_rans.cpp alone (no HIP, no Python) under ASan + UBSan: the goldens,
    every stream above, and the small streams cut at every prefix and with 64
    flipped bytes; any report aborts the program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_rans_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "host_rans_check.cpp"),
                    os.path.join(ROOT, "fqzcomp5_amd", "csrc", "host_rans.cpp"), "-o", exe],
                   check=True)
    cases = str(tmp_path / "cases.bin")
    with open(cases, "wb") as f:
        def put(comp, cap, data, damage=0):
            f.write(struct.pack("<4I", len(comp), cap, 0xffffffff if data is None else len(data),
                                damage))
            f.write(comp)
            f.write(data or b"")
        for name, comp, data in _golden_plain(golden_rans):
            put(comp, len(data), None if comp[0] & ~hc.PLAIN else data)
        for name, comp, data in hc.streams():
            put(comp, len(data) if data is not None else 70001, data)
        for comp, data in hc.small_pair():
            put(comp, len(data), data, damage=64)
    r = subprocess.run([exe, cases], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert " 0 bad" in r.stdout


# ---- the placement plan (host_sched.cpp plan) -------------------------------

CK_RANS_O0, CK_RANS_O1 = 3, 4


def test_plan_long_chains_take_idle_cores():
    n = [44_000_000] * 10
    assert lib.host_plan(n, [CK_RANS_O0] * 10, 16) == [1] * 10
    assert lib.host_plan(n, [CK_RANS_O0] * 10, 16, [0.0] * 16) == [1] * 10


def test_plan_busy_cores_leave_chains_on_gpu():
    # the GPU takes 44 M x 13.6 ns = 0.6 s for such a chain: cores busy for
    # longer than that cannot finish one sooner
    n = [44_000_000] * 10
    assert lib.host_plan(n, [CK_RANS_O0] * 10, 16, [2e9] * 16) == [0] * 10


def test_plan_without_load_is_the_old_plan():
    import numpy as np
    rng = np.random.default_rng(3)
    for it in range(20):
        cnt = int(rng.integers(1, 40))
        n = [int(x) for x in rng.integers(1, 60_000_000, cnt)]
        kind = [int(x) for x in rng.integers(0, 5, cnt)]
        th = int(rng.integers(1, 17))
        assert lib.host_plan(n, kind, th) == lib.host_plan(n, kind, th, [0.0] * th), it
    # the adaptive kinds alone keep their placements: 16 fqz chains on 16
    # cores all go to the host (16 x faster there), 400 of them do not all fit
    assert lib.host_plan([30_000_000] * 16, [1] * 16, 16) == [1] * 16
    many = lib.host_plan([30_000_000] * 400, [1] * 400, 16)
    assert 0 < sum(many) < 400
