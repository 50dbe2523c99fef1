"""The C++ drop-in header on a CPU: tests/host/dropin_harness.cpp drives every class of
include/lbfgs_amd/hip_backend.hpp against tests/host/fake_lbf_abi.cpp, a host-only implementation of the lbf_*
functions the header calls that records every argument. The harness checks each field of each parameter struct
the header fills (Unified{LBFGS,SLBFGS,GD,SGD,HF,OWLQN}_HIP, HipLBFGS, HipHF, HipOWLQN), the launcher's call
order (l2, re-draw, solve, scan), the host scan of evaluate() against long double, the metrics rescaling, the
recorder, the history CSV, HostMatrix, DeviceBuffer and MNISTLoader (over the engine's own csrc/idx.cpp).
That program links without the entry points fake_lbf_abi.cpp leaves out (the link proof of DESIGN.md §17).
tests/host/dropin_harness_v2.cpp does the same for the classes that call them (HipNetwork::gradSq,
HipHFPreconditioned, HipAdam, UnifiedHFPreconditioned_HIP, UnifiedAdam_HIP), linked with fake_lbf_abi_v2.cpp as well.

Built with g++ twice, plain and under AddressSanitizer + UndefinedBehaviorSanitizer, and run as a process of
its own (the pattern of test_host_sanitizers.py). No GPU, nothing loaded into Python.
"""
import os
import shutil
import signal
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
SRC = [os.path.join(HOST, "dropin_harness.cpp"), os.path.join(HOST, "fake_lbf_abi.cpp"),
       os.path.join(ROOT, "lbfgs-ffnn_amd", "csrc", "idx.cpp")]
# idx.cpp includes the library's internal.hpp, which names HIP types: their declarations are enough for g++
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

FLAGS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


SRC_V2 = [os.path.join(HOST, "dropin_harness_v2.cpp"), os.path.join(HOST, "fake_lbf_abi_v2.cpp"), *SRC[1:]]


def build(tmp_path_factory, flavour, name, src):
    exe = str(tmp_path_factory.mktemp(name + "_" + flavour) / name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", *FLAGS[flavour], *INC, *src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "warning" not in r.stderr, r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module", params=list(FLAGS))
def harness(request, tmp_path_factory):
    return build(tmp_path_factory, request.param, "dropin_harness", SRC)


@pytest.fixture(scope="module", params=list(FLAGS))
def harness_v2(request, tmp_path_factory):
    return build(tmp_path_factory, request.param, "dropin_harness_v2", SRC_V2)


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)


def test_header_against_recording_abi(harness, tmp_path):
    r = run(harness, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "dropin harness ok" in r.stdout
    # the history files land in the working directory, named after the config
    assert (tmp_path / "cfgname_history.csv").exists() and (tmp_path / "run_history.csv").exists()
    assert not (tmp_path / "silent_history.csv").exists()


def test_negative_l2_before_bind_aborts(harness, tmp_path):
    """hip_check's abort, in a child that is expected to die: host code, no GPU."""
    r = run(harness, tmp_path, "abort_l2")
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert "HIP engine error: lbf_mlp_set_l2" in r.stderr
    assert "setL2(-1) returned" not in r.stdout


def test_later_classes_against_both_recording_abis(harness_v2, tmp_path):
    r = run(harness_v2, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "dropin harness v2 ok" in r.stdout
    assert (tmp_path / "v2name_history.csv").exists()
