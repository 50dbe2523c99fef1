"""The Gauss-Newton product's interface without a GPU: the built library exports lbf_mlp_gnvp, the binding
carries its signature, the header defines the LBF_HVP_* modes without an ABI bump, and slbfgs_params accepts the
mode by name."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")


def defines():
    with open(HEADER) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(LBF_\w+)\s+(\d+)\s*$", f.read(), re.M)}


def test_library_exports_gnvp(pkg):
    L = pkg.lib()
    f = L.lbf_mlp_gnvp
    assert f.restype is C.c_int
    assert f.argtypes == L.lbf_mlp_hvp.argtypes and len(f.argtypes) == 10
    assert "lbf_mlp_gnvp" in pkg._lib.EXPORTS


def test_header_modes_and_abi_version():
    d = defines()
    assert (d["LBF_HVP_FD"], d["LBF_HVP_EXACT"], d["LBF_HVP_GAUSS_NEWTON"]) == (0, 1, 2)
    assert d["LBF_ABI_VERSION"] == 3
    with open(HEADER) as f:
        assert re.search(r"\bint lbf_mlp_gnvp\(lbf_mlp \*net,", f.read())


def test_null_arguments_are_invalid(pkg):
    """lbf_mlp_hvp's argument checks: a null handle is LBF_ERR_INVALID before anything touches a device."""
    assert pkg.lib().lbf_mlp_gnvp(None, None, None, None, None, None, 0, 1.0, 0.0, None) != 0


def test_slbfgs_params_accepts_mode_names(pkg):
    assert pkg.engine.slbfgs_params(hvp_exact="gauss_newton").hvp_exact == 2
    assert pkg.engine.slbfgs_params(hvp_exact="exact").hvp_exact == 1
    assert pkg.engine.slbfgs_params(hvp_exact="fd").hvp_exact == 0
    assert pkg.engine.slbfgs_params().hvp_exact == 0
    for k in (0, 1, 2):
        assert pkg.engine.slbfgs_params(hvp_exact=k).hvp_exact == k
    with pytest.raises(pkg.LbfError):
        pkg.engine.slbfgs_params(hvp_exact="newton")
    assert pkg.UnifiedConfig().curvature == "fd"
