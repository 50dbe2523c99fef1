"""The interface of the leaky-ReLU, ELU and softplus activations, checked without a GPU: the ids of the
C header against the Python table, the shared initialisation gain, the error for an unknown name, the C++ tags, and
the torch reference's forms and through-y identities (ref_acts.py) against autograd in fp64.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ref_acts
import ref_mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["linear", "tanh", "relu", "sigmoid", "leaky_relu", "elu", "softplus"]


def test_header_ids_equal_python_table(pkg):
    text = open(os.path.join(ROOT, "include", "lbfgs_amd.h")).read()
    header = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+LBF_ACT_(\w+)\s+(\d+)", text)}
    from lbfgs_ffnn_amd import _lib
    assert header == _lib.ACTS
    assert sorted(header) == sorted(NAMES)
    assert sorted(header.values()) == list(range(7))
    assert (header["leaky_relu"], header["elu"], header["softplus"]) == (4, 5, 6)


@pytest.mark.parametrize("mode", ["cpu", "cuda"])
def test_rectifiers_share_relu_start_point(pkg, mode):
    """Swapping ReLU for one of its stand-ins keeps the seed's start point bit for bit (the same sqrt(2) gain and
    the same draws); tanh has gain 1 and differs."""
    dims = [20, 16, 3]
    relu = pkg.init_params_host(dims, ["relu", "linear"], 123, mode)
    for a in ref_acts.NEW_ACTS:
        got = pkg.init_params_host(dims, [a, "linear"], 123, mode)
        assert got.tobytes() == relu.tobytes(), a
    assert pkg.init_params_host(dims, ["tanh", "linear"], 123, mode).tobytes() != relu.tobytes()


def test_unknown_name_raises_lbf_error(pkg):
    with pytest.raises(pkg.LbfError, match="known: .*softplus"):
        pkg.init_params_host([4, 3], ["gelu"], 123, "cpu")
    from lbfgs_ffnn_amd import _lib
    with pytest.raises(pkg.LbfError, match="gelu"):
        _lib.act_ids(["relu", "gelu"])
    assert _lib.act_ids(["elu", 6, "linear"]) == [5, 6, 0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
def test_activation_tags_compile(tmp_path):
    """A translation unit over the drop-in header that names the three tags and builds a network from them."""
    src = tmp_path / "act_tags_tu.cpp"
    src.write_text('#include "lbfgs_amd/hip_backend.hpp"\n'
                   "static_assert(hip_mlp::LeakyReLU::id == LBF_ACT_LEAKY_RELU && LBF_ACT_LEAKY_RELU == 4, \"\");\n"
                   "static_assert(hip_mlp::ELU::id == LBF_ACT_ELU && LBF_ACT_ELU == 5, \"\");\n"
                   "static_assert(hip_mlp::Softplus::id == LBF_ACT_SOFTPLUS && LBF_ACT_SOFTPLUS == 6, \"\");\n"
                   "static_assert(hip_mlp::ActivationId<hip_mlp::ELU>::value == 5, \"\");\n"
                   "void drive() { UnifiedLauncher<HipBackend> l; l.addLayer<8, 6, hip_mlp::ELU>();\n"
                   "  l.addLayer<6, 5, hip_mlp::Softplus>(); l.addLayer<5, 4, hip_mlp::LeakyReLU>();\n"
                   "  l.addLayer<4, 2, hip_mlp::Linear>(); l.buildNetwork(); }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{os.path.join(ROOT, 'include')}",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


GRID = np.concatenate([np.linspace(-30.0, 30.0, 2401), [-1e-3, 1e-3, -1e-8, 1e-8, 0.0]])


@pytest.mark.parametrize("name", ref_acts.NEW_ACTS)
def test_reference_forms_and_identities_fp64(name):
    """On x in [-30, 30] (both ends and 0 on the grid): the reference's act equals the textbook formula, and act'
    and act'' taken through y = act(x) equal autograd's. The bound is absolute, 4 ulp of 1.0 in fp64 (8.9e-16): y
    carries a rounding error of up to one ulp of its own size (at most 2^-53 below |y| = 1, where ELU's y + 1
    turns it into an absolute error of the derivative), and the identities add a few operations on values <= 1."""
    tol = 4 * 2.0 ** -52
    x = torch.tensor(GRID, dtype=torch.float64, requires_grad=True)
    y = ref_mlp.ACTS[name](x)
    (d1,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    d2 = torch.autograd.grad(d1.sum(), x)[0] if d1.requires_grad else torch.zeros_like(x)
    yn, xn = y.detach().numpy(), GRID
    book = {"leaky_relu": np.where(xn > 0, xn, 0.01 * xn), "elu": np.where(xn > 0, xn, np.expm1(np.minimum(xn, 0))),
            "softplus": np.maximum(xn, 0) + np.log1p(np.exp(-np.abs(xn)))}[name]
    assert np.all(np.abs(yn - book) <= tol * np.maximum(1.0, np.abs(book)))
    assert np.all(np.diff(yn[:2401]) > 0)  # strictly increasing on the grid: y determines x
    e1 = np.abs(ref_acts.dact_y(name, yn) - d1.detach().numpy()).max()
    e2 = np.abs(ref_acts.d2act_y(name, yn) - d2.numpy()).max()
    print(f"{name}: act' through y {e1:.2e}, act'' through y {e2:.2e}")
    assert e1 <= tol and e2 <= tol
    assert np.array_equal(ref_acts.act(name, GRID), yn)
