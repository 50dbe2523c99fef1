"""The tridiagonal eigensolver under sanitizers: tests/host/tridiag_harness.cpp, a stand-alone program with its own main
over csrc/tridiag.cpp, is compiled with g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a process
of its own. No GPU, and nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "host", "tridiag_harness.cpp"),
       os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc", "tridiag.cpp")]
INC = os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lanczos_host") / "tridiag_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + INC, *SRC, "-o", out], check=True, capture_output=True, text=True)
    return out


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)


def test_tridiag_self_checks_under_asan_ubsan(exe):
    r = run(exe)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "tridiag harness ok" in r.stdout


@pytest.mark.parametrize("m,seed", [(1, 3), (5, 11), (64, 7)])
def test_harness_eigenvalues_match_numpy(exe, m, seed):
    """The same C++ function the library exports, here without the library, against numpy.linalg.eigh."""
    r = run(exe, m, seed)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = {ln.split()[0]: np.array(ln.split()[1:], np.float64) for ln in r.stdout.splitlines() if ln.strip()}
    a, b = rows["alpha"], rows["beta"]
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    ev, S = np.linalg.eigh(T)
    tol = 16 * m * 2.0 ** -52 * np.linalg.norm(T, 2)
    assert np.abs(rows["theta"] - ev).max() <= tol
    assert np.abs(rows["weight"] - S[0] ** 2).max() <= 1e-10  # eigenvectors: 2^-52 over the smallest gap
    assert abs(rows["weight"].sum() - 1.0) <= 1e-13
