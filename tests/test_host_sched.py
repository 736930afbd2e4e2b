"""The host scheduling module (host_sched.cpp: the mode switch place(), the
cost model's measured(), the worker loop behind parallel_for and Jobs) in a
stand-alone program (tools/host_sched_check.cpp: no HIP, no Python), built
once under AddressSanitizer + UBSan and once under ThreadSanitizer.  CPU
test: any failed check or sanitizer report is a non-zero exit or a line on
stderr."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [
    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    ["-fsanitize=thread"],
], ids=["asan_ubsan", "tsan"])
def test_sanitized_program(tmp_path, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_sched_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread"] + flags +
                   [os.path.join(ROOT, "tools", "host_sched_check.cpp"),
                    os.path.join(ROOT, "fqzcomp5_amd", "csrc", "host_sched.cpp"), "-o", exe],
                   check=True)
    # four host threads whatever the machine has, so that the pools are pools
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, FQZ5_HOST_THREADS="4", ASAN_OPTIONS="detect_leaks=0",
                                UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "host_sched_check: ok (4 host threads)" in r.stdout
