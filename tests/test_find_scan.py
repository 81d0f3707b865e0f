"""The arithmetic of FIND's column scan on the CPU: tests/cpp/find_scan_test.cpp is compiled against
nebula_amd/csrc/find_scan.h with the host compiler (its own main, no HIP, no GPU) and checks, against
scalar restatements: the sign-extended element of a lane's words at every stored width, the lane's
pass mask for every compare op with constants at each width's minimum and maximum and just outside
them, all 256 pass and presence patterns, the in-lane ranks, the tail-tile bounds for columns of 0,
1, 7, 8, 9, 2047, 2048 and 2049 entries, and the row search over row_ptr arrays with leading, trailing
and interior runs of empty rows."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "find_scan_test.cpp"
INC = ROOT / "nebula_amd" / "csrc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("find_scan") / "find_scan_test"
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{INC}", str(SRC), "-o", str(exe)]
    # a stand-alone host program: AddressSanitizer + UBSan where the toolchain ships their runtimes
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    mode = "address+undefined sanitizers"
    if san.returncode != 0:
        mode = "plain (the sanitized build failed: " + (san.stderr.strip().splitlines() or ["?"])[-1][:200] + ")"
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    return exe, mode


def test_find_scan_arithmetic(program):
    exe, mode = program
    print(f"find_scan_test build: {mode}")  # which build ran (shown with -s / -rP and on failure)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"[{mode}] " + r.stdout + r.stderr
    assert "find_scan ok" in r.stdout, mode
