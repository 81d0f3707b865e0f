"""The packed-predicate arithmetic on the CPU: tests/cpp/qpred_test.cpp is compiled against
nebula_amd/csrc/qpred.h with the host compiler (its own main, no HIP, no GPU) and checks, over
bucket bits 3..8, gidx bits 1..28, column minima and ranges from one value to the whole int64 range
(q_range wrapping to 0), every compare op and constants on every edge: q_bucket against the bucket
edges make_qargs_core computes, q_test against the exact compare, that only the bucket holding the
constant is undecided, fin_args' word ranges against q_test (the pad word included), and k_bu_fin's
CLS-1 sign tests against the generic range tests wherever fin_cls1_ok allows them."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "qpred_test.cpp"
INC = ROOT / "nebula_amd" / "csrc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("qpred") / "qpred_test"
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


def test_packed_predicate_arithmetic(program):
    exe, mode = program
    print(f"qpred_test build: {mode}")  # which build ran (shown with -s / -rP and on failure)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"[{mode}] " + r.stdout + r.stderr
    assert "qpred ok" in r.stdout, mode
