"""The preconditioned Hessian-free interface without a GPU: the built library exports
lbf_mlp_grad_sq, lbf_mlp_gn_pcg, lbf_hf_precond_default and lbf_hf_solve_pc, the header declares them without an ABI
bump, lbf_hf_precond has the header's layout and the documented defaults, null handles are LBF_ERR_INVALID, the Python
layers reject an unknown preconditioner before anything touches a device, and the new C++ drop-in classes compile."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")
BACKEND = os.path.join(ROOT, "include", "lbfgs_amd", "hip_backend.hpp")
CTYPES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}
NEW = ("lbf_mlp_grad_sq", "lbf_mlp_gn_pcg", "lbf_hf_precond_default", "lbf_hf_solve_pc")


def header():
    with open(HEADER) as f:
        return f.read()


def struct_fields(name):
    """[(field, ctype)] of `typedef struct name { ... } name;` in the header (comments stripped)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        t = re.match(r"(long long|int|double)\s+(.*)", decl)
        assert t, decl
        for nm in t.group(2).split(","):
            out.append((nm.strip(), CTYPES[t.group(1)]))
    return out


def test_library_exports_and_header_declares(pkg):
    L = pkg.lib()
    h = header()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in pkg._lib.EXPORTS
        assert re.search(r"\b%s\(" % name, h), name
    # lbf_mlp_gn_pcg is lbf_mlp_gn_cg with d_minv after d_b
    cg, pcg = L.lbf_mlp_gn_cg.argtypes, L.lbf_mlp_gn_pcg.argtypes
    assert L.lbf_mlp_gn_pcg.restype is C.c_int and len(pcg) == len(cg) + 1 == 12
    assert list(pcg[:3]) + list(pcg[4:]) == list(cg)
    # lbf_hf_solve_pc is lbf_hf_solve with the lbf_hf_precond pointer after the parameters
    hf, hpc = L.lbf_hf_solve.argtypes, L.lbf_hf_solve_pc.argtypes
    assert list(hpc[:2]) + list(hpc[3:]) == list(hf) and hpc[2] == C.POINTER(pkg._lib.HfPrecond)
    assert L.lbf_mlp_grad_sq.restype is C.c_int and len(L.lbf_mlp_grad_sq.argtypes) == 8
    assert re.search(r"^#define\s+LBF_PRECOND_NONE\s+0\s*$", h, re.M)
    assert re.search(r"^#define\s+LBF_PRECOND_GRAD_SQ\s+1\s*$", h, re.M)
    assert pkg._lib.PRECONDS == {"none": 0, "grad_sq": 1}


def test_abi_version_unchanged(pkg):
    assert re.search(r"^#define\s+LBF_ABI_VERSION\s+3\s*$", header(), re.M)
    assert pkg.lib().lbf_abi_version() == 3 and pkg._lib.ABI_VERSION == 3


def test_precond_struct_layout_and_defaults(pkg):
    want = struct_fields("lbf_hf_precond")
    S = pkg._lib.HfPrecond
    assert [(n, t) for n, t in S._fields_] == want == [("mode", C.c_int), ("exponent", C.c_double),
                                                       ("refresh", C.c_int)]
    assert C.sizeof(S) == 24  # int, pad, double, int, pad
    p = S(7, 7.0, 7)
    pkg.lib().lbf_hf_precond_default(C.byref(p))
    assert (p.mode, p.exponent, p.refresh) == (0, 0.75, 1)
    pkg.lib().lbf_hf_precond_default(None)  # tolerated, like the other *_default_params
    q = pkg.engine.hf_precond("grad_sq", 0.5, 3)
    assert (q.mode, q.exponent, q.refresh) == (1, 0.5, 3)
    u = pkg.UnifiedConfig()
    assert (u.precond, u.precond_exponent) == ("none", 0.75)
    # the pinned structs are what they were
    assert C.sizeof(pkg._lib.HfParams) == 144 and C.sizeof(pkg._lib.CgParams) == 32 and C.sizeof(pkg._lib.CgInfo) == 48


def test_null_handles_are_invalid(pkg):
    L = pkg.lib()
    c = pkg._lib.CgParams()
    L.lbf_cg_default_params(C.byref(c))
    ci = pkg._lib.CgInfo()
    assert L.lbf_mlp_grad_sq(None, None, None, None, None, 0, 1.0, None) == 1
    assert L.lbf_mlp_gn_pcg(None, None, None, None, None, None, None, 0, 1.0, C.byref(c), None, C.byref(ci)) == 1
    p = pkg.engine.hf_params()
    pc = pkg._lib.HfPrecond()
    L.lbf_hf_precond_default(C.byref(pc))
    assert L.lbf_hf_solve_pc(None, C.byref(p), C.byref(pc), None, None, None, 0, 1, None, None) == 1
    assert L.lbf_hf_solve_pc(None, C.byref(p), None, None, None, None, 0, 1, None, None) == 1


def test_unknown_preconditioner_is_rejected_before_the_device(pkg):
    # net = None / ctx = None: a call that went on to the device would fail on it with another error
    with pytest.raises(pkg.LbfError, match="unknown preconditioner"):
        pkg.engine.hf_solve(None, None, None, None, precond="bogus")
    with pytest.raises(pkg.LbfError, match="precond_exponent"):
        pkg.engine.hf_solve(None, None, None, None, precond="grad_sq", precond_exponent=1.5)
    with pytest.raises(pkg.LbfError, match="precond_refresh"):
        pkg.engine.hf_solve(None, None, None, None, precond="grad_sq", precond_refresh=0)
    from lbfgs_ffnn_amd import unified
    with pytest.raises(pkg.LbfError, match="unknown preconditioner"):
        pkg.UnifiedHF().optimize(unified._DeviceNet(None), None, pkg.UnifiedConfig(precond="bogus"))


def test_new_symbols_stay_out_of_the_existing_classes():
    """The header names the new entry points only inside HipNetwork::gradSq and the two new classes, so a program that
    uses the classes that existed before still links against a library without them."""
    with open(BACKEND) as f:
        src = re.sub(r"///.*", "", f.read())
    # the header cut at every class definition: [(class name, text up to the next class)]
    parts = re.split(r"\nclass (\w+)", src)
    bodies = dict(zip(parts[1::2], parts[2::2]))
    allowed = {"HipNetwork", "HipHFPreconditioned", "UnifiedHFPreconditioned_HIP"}
    assert allowed <= set(bodies) and {"HipHF", "UnifiedHF_HIP"} <= set(bodies)
    new = re.compile(r"lbf_mlp_grad_sq|lbf_mlp_gn_pcg|lbf_hf_solve_pc|lbf_hf_precond|LBF_PRECOND_")
    assert not new.search(parts[0])
    for name, body in bodies.items():
        if name not in allowed:
            assert not new.search(body), name
    assert new.findall(bodies["HipNetwork"]) == ["lbf_mlp_grad_sq", "lbf_mlp_grad_sq"]  # the call and its message
    assert "lbf_hf_solve_pc(" in bodies["HipHFPreconditioned"] and "lbf_hf_solve_pc(" in bodies["UnifiedHFPreconditioned_HIP"]


TU = r"""
#include <lbfgs_amd/hip_backend.hpp>
int main() {
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  net.addLayer(4, 3, LBF_ACT_TANH);
  net.addLayer(3, 2, LBF_ACT_LINEAR);
  net.bindParams();
  hip_mlp::DeviceBuffer<hip_mlp::HipScalar> x(h), y(h), d(h);
  net.gradSq(x.data(), y.data(), 0, 1.0, d.data());
  hip_mlp::HipHFPreconditioned hf(h, net);
  hf.setCG(20, 0.1);
  hf.setDamping(1.0);
  hf.setCurvatureRows(0);
  hf.setPreconditioner(0.75, 2);
  hf.setMaxIterations(3);
  hf.solve(int(net.params_size()), net.params_data(), x.data(), y.data(), 0, {});
  UnifiedHFPreconditioned_HIP u;
  u.setPreconditioner(0.5);
  return hf.iterations();
}
"""


def test_new_cxx_classes_compile(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the drop-in header's syntax check"
    src = tmp_path / "pcg_tu.cpp"
    src.write_text(TU)
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
