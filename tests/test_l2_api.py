"""CPU checks of the weight-decay setting's public surface (no GPU): the library exports lbf_mlp_set_l2 /
lbf_mlp_get_l2 with the declared signatures at ABI 3, the Python layers have the fields and setters and reject a
bad value before touching the device, and the C++ header compiles standalone with setL2 calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

TU = r"""
#include "lbfgs_amd/hip_backend.hpp"

int main() {
  UnifiedLauncher<HipBackend> launcher;
  launcher.addLayer<784, 128, hip_mlp::ReLU>();
  launcher.addLayer<128, 10, hip_mlp::Linear>();
  launcher.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  launcher.setL2(1e-3);
  launcher.buildNetwork();
  UnifiedConfig cfg;
  cfg.l2 = 5e-4;
  hip_mlp::HipNetwork &net = launcher.getWrapper().getInternal();
  net.setL2(cfg.l2);
  UnifiedLBFGS_HIP lbfgs;
  launcher.train(lbfgs, cfg);  // applies cfg.l2 (instantiation only: nothing runs here)
  return net.l2() == 5e-4 ? 0 : 1;
}
"""


def test_cpp_set_l2_compiles_standalone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{INCLUDE}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_l2_functions(pkg):
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lbf_\w+)", out))
    assert {"lbf_mlp_set_l2", "lbf_mlp_get_l2"} <= exported
    hdr = open(os.path.join(INCLUDE, "lbfgs_amd.h")).read()
    assert re.search(r"\bint\s+lbf_mlp_set_l2\s*\(\s*lbf_mlp\s*\*\s*net\s*,\s*double\s+l2\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+lbf_mlp_get_l2\s*\(\s*const\s+lbf_mlp\s*\*\s*net\s*,\s*double\s*\*\s*l2\s*\)\s*;", hdr)
    assert re.search(r"#define\s+LBF_ABI_VERSION\s+3\b", hdr)
    assert L.lbf_abi_version() == 3
    assert L.lbf_mlp_set_l2.restype is C.c_int and L.lbf_mlp_get_l2.restype is C.c_int
    assert L.lbf_mlp_set_l2.argtypes == [C.c_void_p, C.c_double]
    assert L.lbf_mlp_get_l2.argtypes == [C.c_void_p, C.POINTER(C.c_double)]
    assert {"lbf_mlp_set_l2", "lbf_mlp_get_l2"} <= set(pkg._lib.EXPORTS)
    # null handles are reported, not dereferenced
    assert L.lbf_mlp_set_l2(None, 0.1) == 1
    assert L.lbf_mlp_get_l2(None, None) == 1


@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), -float("inf"), "x", None])
def test_bad_l2_is_rejected_before_the_device(pkg, bad):
    # ctx = None: a constructor that went on to the device would fail on it with another error
    with pytest.raises(pkg.LbfError, match="l2 must be"):
        pkg.Mlp(None, [784, 128, 10], ["relu", "linear"], l2=bad)
    from lbfgs_ffnn_amd import unified
    w = unified._DeviceNet(None)
    with pytest.raises(pkg.LbfError, match="l2 must be"):
        w.setL2(bad)
    assert w.l2 == 0.0


def test_python_fields_and_setters_exist(pkg):
    from lbfgs_ffnn_amd import unified
    assert pkg.UnifiedConfig().l2 == 0.0
    assert pkg.UnifiedConfig(l2=1e-3).l2 == 1e-3
    assert callable(pkg.UnifiedLauncher.setL2)
    assert isinstance(pkg.Mlp.l2, property) and pkg.Mlp.l2.fset is not None
    w = unified._DeviceNet(None)
    w.setL2(2e-3)  # before buildNetwork(): kept for the network that bindParams() creates
    assert w.l2 == 2e-3
