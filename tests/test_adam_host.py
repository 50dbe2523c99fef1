"""The Adam solver's host-side sampling under sanitizers: tests/host/adam_shuffle_harness.cpp, a stand-alone program
with its own main over sampler.cpp's epoch shuffle and rank split, is compiled with g++ under AddressSanitizer +
UndefinedBehaviorSanitizer and run as a process of its own. No GPU, and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_adam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "host", "adam_shuffle_harness.cpp"),
       os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc", "sampler.cpp")]
INC = os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adam_host") / "adam_shuffle_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + INC, *SRC, "-o", out], check=True, capture_output=True, text=True)
    return out


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)


def test_shuffle_and_rank_split_under_asan_ubsan(exe):
    r = run(exe)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "adam shuffle harness ok" in r.stdout


@pytest.mark.parametrize("N,seed", [(37, 123), (257, 7)])
def test_harness_orders_match_numpy_restatement(exe, N, seed):
    """The same C++ function the library exports, here without the library: its orders are the numpy restatement's."""
    r = run(exe, N, seed, 3)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [list(map(int, ln.split()[1:])) for ln in r.stdout.splitlines() if ln.startswith("order")]
    assert np.array_equal(np.asarray(rows, np.int32), ref_adam.epoch_orders_ref(N, seed, 3))
