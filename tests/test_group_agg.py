"""The arithmetic of GROUP BY's aggregates on the CPU: tests/cpp/group_agg_test.cpp is compiled against
nebula_amd/csrc/group_agg.h with the host compiler (its own main, no HIP, no GPU) and checks the
MIN / MAX key round trip at the int64 extremes, both zeros, both infinities, NaN payloads and
denormals, the operators' identities, the wrapped integer sum at INT64_MAX + 1, the AVG divisions,
and the fixed segment tree on lengths on both sides of every class boundary against a scalar
restatement of the same tree."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "group_agg_test.cpp"
INC = ROOT / "nebula_amd" / "csrc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("group_agg") / "group_agg_test"
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


def test_group_agg_arithmetic(program):
    exe, mode = program
    print(f"group_agg_test build: {mode}")  # which build ran (shown with -s / -rP and on failure)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"[{mode}] " + r.stdout + r.stderr
    assert "group_agg ok" in r.stdout, mode
