"""unlzp on a host core (host_lzp.cpp behind fqz5_unlzp_host).  CPU tests:
valid streams against the oracle's unlzp (every case of lzp_cases, the LZP
goldens, hand-built streams for each token kind), damaged streams against the
stated verdict (a failure, and nothing written past the capacity:
lib.unlzp_host checks a guard behind the buffer), and the same under
AddressSanitizer / UBSan in a stand-alone program."""
import json
import os
import shutil
import struct
import subprocess

import host_lzp_cases as lc
from fqzcomp5_amd import lib
from oracle import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def test_hand_built_streams():
    ora = binding.oracle()
    for name, z, data in lc.hand_built():
        assert ora.unlzp(z, len(data)) == data, name          # the stream is the format
        assert lib.unlzp_host(z, len(data)) == data, name     # output exactly equal to cap
        assert lib.unlzp_host(z, len(data) + 100) == data, name
    names = [n for n, _, _ in lc.hand_built()]
    assert len(set(names)) == len(names) >= 19


def test_lzp_cases_vs_oracle():
    ora = binding.oracle()
    for name, z, data in lc.oracle_streams(ora):
        exp = ora.unlzp(z, len(data))
        assert exp == data, name
        assert lib.unlzp_host(z, len(data)) == exp, name


def test_goldens():
    """The committed LZP3 streams (made by the reference): their rANS stage
    decoded by the oracle, the lzp stream by the host unlzp."""
    ora = binding.oracle()
    gold = json.load(open(os.path.join(HERE, "golden", "lzp.json")))
    small = open(os.path.join(HERE, "golden", "lzp_small.bin"), "rb").read()
    data = dict(lc.cases())
    n = 0
    for g in gold:
        if g["off"] is None:
            continue
        z = ora.rans_uncompress(small[g["off"]:g["off"] + g["lzp3_len"]])
        assert len(z) == g["lzp_len"], g["case"]
        want = data[g["case"]]
        assert ora.unlzp(z, len(want)) == want, g["case"]
        assert lib.unlzp_host(z, len(want)) == want, g["case"]
        n += 1
    assert n >= 5


def test_damaged_streams_fail_within_cap():
    for name, z, cap in lc.damaged():
        assert lib.unlzp_host(z, cap) is None, name
    # every valid stream fails one byte short of its size, and cut after any
    # marker token's first byte where that byte has a prediction
    for name, z, data in lc.hand_built():
        if data:
            assert lib.unlzp_host(z, len(data) - 1) is None, name
        for cut in range(len(z)):
            got = lib.unlzp_host(z[:cut], len(data))
            assert got is None or data.startswith(got), (name, cut)


def test_sanitized_program(tmp_path):
    """host_lzp.cpp alone (no HIP, no Python) under ASan + UBSan: every valid
    stream above, the damaged ones, and the small streams cut at every prefix,
    decoded into every smaller capacity and with changed bytes; any report
    aborts the program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_lzp_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "host_lzp_check.cpp"),
                    os.path.join(ROOT, "fqzcomp5_amd", "csrc", "host_lzp.cpp"), "-o", exe],
                   check=True)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        def put(z, cap, data, damage=0):
            f.write(struct.pack("<4I", len(z), cap, 0xffffffff if data is None else len(data),
                                damage))
            f.write(z)
            f.write(data or b"")
        for name, z, data in lc.hand_built():
            put(z, len(data), data, damage=0 if len(data) > 1000 else 64)
        for name, z, data in lc.oracle_streams(binding.oracle()):
            put(z, len(data), data, damage=64 if len(z) < 64 else 0)
        for name, z, cap in lc.damaged():
            put(z, cap, None)
    r = subprocess.run([exe, path], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert " 0 bad" in r.stdout
