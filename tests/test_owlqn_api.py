"""The OWL-QN interface without a GPU: the built library exports lbf_owlqn_default_params, lbf_owlqn_solve,
lbf_mlp_l1_pseudo_grad and lbf_mlp_l1_trial, the header declares them (and the two structs) without an ABI bump, the
ctypes structs have the header's field lists, the defaults are the documented ones, null handles and invalid
parameters are LBF_ERR_INVALID, and owlqn_params rejects unknown names."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")
CTYPES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}
SYMBOLS = ("lbf_owlqn_default_params", "lbf_owlqn_solve", "lbf_mlp_l1_pseudo_grad", "lbf_mlp_l1_trial")


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
            nm = nm.strip()
            if nm.startswith("*"):
                out.append((nm[1:].strip(), C.POINTER(CTYPES[t.group(1)])))
            else:
                out.append((nm, CTYPES[t.group(1)]))
    return out


def c_layout(fields):
    """sizeof of a C struct with these fields under the natural-alignment rules the compiler applies."""
    class S(C.Structure):
        _fields_ = fields
    return C.sizeof(S)


def test_library_exports_and_header_declares(pkg):
    L = pkg.lib()
    h = header()
    for name in SYMBOLS:
        assert getattr(L, name) is not None
        assert name in pkg._lib.EXPORTS
        assert re.search(r"\b%s\(" % name, h), name
    for name in ("lbf_owlqn_params", "lbf_owlqn_stats"):
        assert re.search(r"typedef struct %s \{" % name, h), name
    assert L.lbf_owlqn_solve.restype is C.c_int
    assert L.lbf_owlqn_solve.argtypes[2:9] == L.lbf_gd_solve.argtypes[2:] and len(L.lbf_owlqn_solve.argtypes) == 10
    assert len(L.lbf_mlp_l1_pseudo_grad.argtypes) == 7 and len(L.lbf_mlp_l1_trial.argtypes) == 12
    assert L.lbf_mlp_l1_trial.argtypes[6] is C.c_float


def test_abi_version_unchanged(pkg):
    assert re.search(r"^#define\s+LBF_ABI_VERSION\s+3\s*$", header(), re.M)
    assert pkg.lib().lbf_abi_version() == 3 and pkg._lib.ABI_VERSION == 3


@pytest.mark.parametrize("cname,pyname", [("lbf_owlqn_params", "OwlqnParams"), ("lbf_owlqn_stats", "OwlqnStats")])
def test_struct_layouts_match_header(pkg, cname, pyname):
    want = struct_fields(cname)
    S = getattr(pkg._lib, pyname)
    assert [(n, t) for n, t in S._fields_] == want
    assert C.sizeof(S) == c_layout(want)


def test_struct_sizes(pkg):
    # int, int, double | double, int, pad | double, double | int, pad, pointer | int, pad
    assert C.sizeof(pkg._lib.OwlqnParams) == 72
    assert C.sizeof(pkg._lib.OwlqnStats) == 32


def test_defaults(pkg):
    p = pkg.engine.owlqn_params()
    assert (p.m, p.max_iters, p.tol) == (10, 100, 1e-6)
    assert (p.l1, p.l1_bias) == (0.0, 0)
    assert (p.c1, p.rho, p.max_line_iters) == (1e-4, 0.5, 20)
    assert not p.zeros_trace and p.trace_cap == 0
    pkg.lib().lbf_owlqn_default_params(None)  # tolerated, like the other *_default_params
    assert pkg.UnifiedConfig().l1 == 0.0
    assert issubclass(pkg.UnifiedOWLQN, pkg.unified.UnifiedOptimizer)


def test_null_handles_are_invalid(pkg):
    L = pkg.lib()
    p = pkg.engine.owlqn_params()
    info, st = pkg._lib.SolveInfo(), pkg._lib.OwlqnStats()
    assert L.lbf_owlqn_solve(None, C.byref(p), None, None, None, 0, 1, None, C.byref(info), C.byref(st)) == 1
    assert "invalid argument" in L.lbf_last_error().decode()
    assert L.lbf_owlqn_solve(None, None, None, None, None, 0, 1, None, None, None) == 1
    assert L.lbf_mlp_l1_pseudo_grad(None, None, None, 0.1, 0, None, C.byref(st)) == 1
    z = C.c_longlong(0)
    assert L.lbf_mlp_l1_trial(None, None, None, None, 0.1, 0, 1.0, None, None, None, None, C.byref(z)) == 1


def test_owlqn_params_keywords(pkg):
    p = pkg.engine.owlqn_params(m=5, max_iters=7, l1=0.25, l1_bias=True, rho=0.25)
    assert (p.m, p.max_iters, p.l1, p.l1_bias, p.rho) == (5, 7, 0.25, 1, 0.25)
    with pytest.raises(pkg.LbfError):
        pkg.engine.owlqn_params(bogus=1)
    with pytest.raises(pkg.LbfError):
        pkg.engine.owlqn_params(trace_cap=4)  # the trace is owlqn_solve's


def test_cpp_wrappers_compile_with_plain_gxx(tmp_path):
    """HipOWLQN and UnifiedOWLQN_HIP need nothing but C++17 and the C ABI, like the rest of hip_backend.hpp."""
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "lbfgs_amd/hip_backend.hpp"\n'
                   "int main(){ UnifiedConfig c; c.l1 = 1e-3; UnifiedOWLQN_HIP o; (void)o;\n"
                   "  static_assert(sizeof(lbf_owlqn_params) == 72 && sizeof(lbf_owlqn_stats) == 32, \"layout\");\n"
                   "  return sizeof(hip_mlp::HipOWLQN) > 0 ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
