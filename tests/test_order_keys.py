"""The ORDER BY key encoding on the CPU: tests/cpp/order_keys_test.cpp is compiled against
nebula_amd/csrc/order_keys.h with the host compiler (its own main, no HIP, no GPU) and checks
a < b <=> key(a) < key(b) and a == b <=> key(a) == key(b) for ints, doubles (+-0.0, denormals,
+-inf, NaN payloads), bools and strings (chunk + length key sequences against std::string::compare),
each under ASC and DESC."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "cpp" / "order_keys_test.cpp"
INC = ROOT / "nebula_amd" / "csrc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("order_keys") / "order_keys_test"
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", f"-I{INC}", str(SRC), "-o", str(exe)]
    # a stand-alone host program: AddressSanitizer + UBSan where the toolchain ships their runtimes
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    return exe


def test_key_order_matches_value_order(program):
    r = subprocess.run([str(program)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "order_keys ok" in r.stdout
