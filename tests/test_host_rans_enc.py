"""The encoder's bare rANS 4x16 chains on a host core (host_rans.cpp
rans_enc_chain_o0 / _o1 behind fqz5_rans_enc_chain_host) and the placement plan
with the encoder's chain kinds.  CPU tests: every checkpoint against a
pure-Python model of the chain (sizes 1..70 001 around the 256-step chunk
boundaries; one symbol, two, ACGTN, all 256, a symbol of frequency 1; order 0,
order 1 with 10 and 12 bits), the final states against the four states at the
head of the reference's payload (its own table, parsed from its stream), and
the same cases under AddressSanitizer / UBSan in a stand-alone program."""
import os
import shutil
import struct
import subprocess

import host_rans_cases as hc
import host_rans_enc_cases as ec
from fqzcomp5_amd import lib
from oracle import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checkpoints_are_the_models():
    seen = set()
    for name, d, order, bits, table, want in ec.cases():
        got = lib.rans_enc_chain_host(d, order, bits, table)
        assert got is not None, name
        steps = ec.steps_of(len(d), order)
        assert len(got) == ((steps + 255) // 256 + 1) * 4, name
        assert got[:4] == [ec.LOW] * 4, name
        assert got == want, name
        seen.add((name.split("/")[0], len(d), order, bits))
    assert len(seen) == len(ec.SIZES) * 5 * 3
    # what the sizes and alphabets are there for
    t = ec.table_of(ec.alphabets(70001)["rare"].tobytes(), 0, 12)
    assert sorted(f for f in t if f) == [1, 4095]
    assert max(ec.table_of(ec.alphabets(2049)["one"].tobytes(), 0, 12)) == 4096
    assert sum(1 for f in ec.table_of(ec.alphabets(70001)["all256"].tobytes(), 0, 12) if f) == 256
    assert ec.steps_of(1025, 0) == 257 and ec.steps_of(1025, 1) == 257    # a final chunk of one step
    assert ec.steps_of(3 * 1024 + 2, 1) == 768 + 2                       # a tail in state 3 alone


def test_final_states_are_the_references():
    ora = binding.oracle()

    def o0_decode(stream, size):
        return ora.rans_uncompress(bytes([0]) + hc._varint(size) + stream[1:])

    checked = {0: 0, 10: 0, 12: 0}
    for n in ec.SIZES:
        inputs = dict(ec.alphabets(n))
        if n == 70001:      # data the reference codes with 12 bits, and with a compressed table
            inputs["o1_shift12"] = hc.alphabets(n)["o1_shift12"]
            inputs["o1_comp_table"] = hc.alphabets(n)["o1_comp_table"]
        for name, d in inputs.items():
            d = d.tobytes()
            for order in (0, 1):
                comp = ora.rans_compress(d, order)
                parsed = ec.parse_plain(comp, order, o0_decode)
                if parsed is None:               # stored uncoded, or coded at order 0 instead
                    continue
                bits, table, payload = parsed
                ck = lib.rans_enc_chain_host(d, order, bits, table)
                assert ck is not None, (name, n, order)
                assert ck[-4:] == list(struct.unpack("<4I", payload[:16])), (name, n, order)
                # and the model agrees with the reference on its own table
                assert ck == ec.model(d, order, bits, table), (name, n, order)
                checked[bits if order else 0] += 1
    # (the reference stores the smallest inputs uncoded: the sizes from 1023 on
    # are coded, 8 sizes x 5 alphabets less the few it codes another way)
    assert checked[0] >= 30 and checked[10] >= 30 and checked[12] >= 1, checked


def test_refusals():
    d = ec.alphabets(1025)["acgtn"].tobytes()
    t0 = ec.table_of(d, 0, 12)
    assert lib.rans_enc_chain_host(d, 0, 10, t0) is None            # order 0 has 12 bits
    assert lib.rans_enc_chain_host(d + b"\x07", 0, 12, t0) is None  # a byte without a frequency
    bad = list(t0)
    bad[65] += 1
    assert lib.rans_enc_chain_host(d, 0, 12, bad) is None           # does not sum to 4096
    t1 = ec.table_of(d, 1, 12)
    assert lib.rans_enc_chain_host(d, 1, 11, t1) is None
    assert lib.rans_enc_chain_host(d + b"\x07", 1, 12, t1) is None  # a pair without a frequency
    assert lib.rans_enc_chain_host(b"", 0, 12, t0) is None


def test_sanitized_program(tmp_path):
    """host_rans.cpp alone (no HIP, no Python) under ASan + UBSan: every case
    above from exact-size heap buffers; any report aborts the program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_rans_enc_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "host_rans_enc_check.cpp"),
                    os.path.join(ROOT, "fqzcomp5_amd", "csrc", "host_rans.cpp"), "-o", exe],
                   check=True)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for name, d, order, bits, table, want in ec.cases():
            nz = [(i, v) for i, v in enumerate(table) if v]
            f.write(struct.pack("<5I", len(d), order, bits, len(nz), len(want)))
            f.write(d)
            f.write(struct.pack(f"<{2 * len(nz)}I", *[x for p in nz for x in p]))
            f.write(struct.pack(f"<{len(want)}I", *want))
    r = subprocess.run([exe, path, "--time"], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert f"{len(ec.cases())} cases, 0 bad" in r.stdout
    assert "ns per symbol" in r.stdout


# ---- the placement plan with the encoder's kinds (host_sched.cpp plan) -------

CK_RANS_ENC_O0, CK_RANS_ENC_O1 = 5, 6


def test_plan_places_the_bench_chains_on_idle_cores():
    # the -3 step's plain batch: 20 order-0 and 20 order-1 chains of 44.5 M
    # symbols.  The GPU takes 44.5 M x 4.6 ns = 205 ms for any of them; 16
    # cores finish three rounds of chains that cost a few ns per symbol sooner
    n = [44_500_000] * 40
    kind = [CK_RANS_ENC_O0, CK_RANS_ENC_O1] * 20
    assert lib.host_plan(n, kind, 16) == [1] * 40
    assert lib.host_plan(n, kind, 16, [0.0] * 16) == [1] * 40


def test_plan_preloaded_cores_leave_chains_on_gpu():
    # cores committed for longer than the GPU needs cannot finish one sooner
    n = [44_500_000] * 8
    for kind in (CK_RANS_ENC_O0, CK_RANS_ENC_O1):
        assert lib.host_plan(n, [kind] * 8, 16, [1e9] * 16) == [0] * 8
    # four idle cores among busy ones take what they finish within the GPU's
    # 205 ms; the call's finish time is the busy cores' either way, so ties go
    # to the host until a core would pass the GPU's time
    cores = [1e9] * 12 + [0.0] * 4
    on = lib.host_plan(n, [CK_RANS_ENC_O0] * 8, 16, cores)
    assert sum(on) >= 4


def test_plan_one_core_shares_with_the_gpu():
    # one core against the GPU: it takes chains while its finish time stays
    # under the GPU's launch (all chains there run side by side)
    on = lib.host_plan([44_500_000] * 40, [CK_RANS_ENC_O1] * 40, 1)
    assert 0 < sum(on) < 40
