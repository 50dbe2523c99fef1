"""CPU checks of the loss selection's public surface (no GPU): the C++ header's setLoss compiles in standalone
mode, the library exports lbf_mlp_set_loss / lbf_mlp_get_loss with the documented codes, and the Python layers
reject an unknown loss name before touching the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

TU = r"""
#include "lbfgs_amd/hip_backend.hpp"

static_assert(int(hip_mlp::Loss::MeanSquaredError) == LBF_LOSS_MSE, "loss codes");
static_assert(int(hip_mlp::Loss::SoftmaxCrossEntropy) == LBF_LOSS_SOFTMAX_XENT, "loss codes");

int main() {
  UnifiedLauncher<HipBackend> launcher;
  launcher.addLayer<784, 128, hip_mlp::ReLU>();
  launcher.addLayer<128, 10, hip_mlp::Linear>();
  launcher.setLoss(hip_mlp::Loss::SoftmaxCrossEntropy);
  launcher.buildNetwork();
  hip_mlp::HipNetwork &net = launcher.getWrapper().getInternal();
  net.setLoss(hip_mlp::Loss::MeanSquaredError);
  return net.loss() == hip_mlp::Loss::MeanSquaredError ? 0 : 1;
}
"""


def test_cpp_set_loss_compiles_standalone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{INCLUDE}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_loss_functions(pkg):
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lbf_\w+)", out))
    assert {"lbf_mlp_set_loss", "lbf_mlp_get_loss"} <= exported
    assert hasattr(L, "lbf_mlp_set_loss") and hasattr(L, "lbf_mlp_get_loss")
    hdr = open(os.path.join(INCLUDE, "lbfgs_amd.h")).read()
    assert re.search(r"#define\s+LBF_LOSS_MSE\s+0\b", hdr) and re.search(r"#define\s+LBF_LOSS_SOFTMAX_XENT\s+1\b", hdr)
    assert re.search(r"#define\s+LBF_ABI_VERSION\s+3\b", hdr)
    assert pkg._lib.LOSSES == {"mse": 0, "softmax_xent": 1}
    # null handles are reported, not dereferenced
    assert L.lbf_mlp_set_loss(None, 1) == 1
    assert L.lbf_mlp_get_loss(None, None) == 1


def test_unknown_loss_name_is_rejected_before_the_device(pkg):
    # ctx = None: a constructor that went on to the device would fail on it with another error
    with pytest.raises(pkg.LbfError, match="unknown loss"):
        pkg.Mlp(None, [784, 128, 10], ["relu", "linear"], loss="hinge")
    assert pkg.UnifiedConfig().loss == "mse"
    assert callable(pkg.lbfgs_solve_fn) and callable(pkg.UnifiedLauncher.setLoss)
