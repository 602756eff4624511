"""CPU tier: the owner types of csrc/mem.hpp (DevBuf, Owned) in a stand-alone program under the host sanitizers.

tests/mem_owner_main.cpp defines the two raw functions over malloc / free with its own counters and a switch that makes the n-th
allocation fail; it is built with the host compiler and -fsanitize=address,undefined and run as a process of its own (no HIP, no
Python inside it).  The checks are in the program: empty owners, balance, moves, allocate-once, grow, count 0, failure, a struct
of owners cleaned up by its destructor or by move-assigning an empty one, counters at 0 at exit."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "mem_owner_main.cpp")


def _compilers():
    found = [c for c in (shutil.which("g++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)]
    return found


@pytest.mark.parametrize("compiler", _compilers() or [None], ids=lambda c: os.path.basename(c) if c else "none")
def test_owners_under_host_sanitizers(compiler, tmp_path):
    assert compiler, "no host C++ compiler found (g++ or /opt/rocm/llvm/bin/clang++)"
    exe = str(tmp_path / "mem_owner")
    # the sanitizer runtimes are linked statically: a shared AddressSanitizer runtime refuses to start unless it comes first in the
    # process's library list, a statically linked one has no such condition
    static = ["-static-libsan"] if "clang" in os.path.basename(compiler) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all"] + static + ["-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = dict(ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")      # all the program needs
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mem owners: ok" in run.stdout
