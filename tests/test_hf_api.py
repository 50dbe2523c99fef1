"""The Hessian-free interface without a GPU: the built library exports lbf_mlp_gn_cg, lbf_hf_default_params and
lbf_hf_solve, the header declares them without an ABI bump, the ctypes structs have the header's field lists, the
defaults are the documented ones, null handles are LBF_ERR_INVALID and hf_params rejects unknown names."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")
CTYPES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}


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
    for name in ("lbf_mlp_gn_cg", "lbf_hf_default_params", "lbf_hf_solve"):
        assert getattr(L, name) is not None
        assert name in pkg._lib.EXPORTS
        assert re.search(r"\b%s\(" % name, h), name
    assert L.lbf_mlp_gn_cg.restype is C.c_int and len(L.lbf_mlp_gn_cg.argtypes) == 11
    assert L.lbf_hf_solve.restype is C.c_int and L.lbf_hf_solve.argtypes[2:] == L.lbf_gd_solve.argtypes[2:]


def test_abi_version_unchanged(pkg):
    assert re.search(r"^#define\s+LBF_ABI_VERSION\s+3\s*$", header(), re.M)
    assert pkg.lib().lbf_abi_version() == 3 and pkg._lib.ABI_VERSION == 3


@pytest.mark.parametrize("cname,pyname", [("lbf_cg_params", "CgParams"), ("lbf_cg_info", "CgInfo"),
                                          ("lbf_hf_params", "HfParams")])
def test_struct_layouts_match_header(pkg, cname, pyname):
    want = struct_fields(cname)
    S = getattr(pkg._lib, pyname)
    assert [(n, t) for n, t in S._fields_] == want
    assert C.sizeof(S) == c_layout(want)


def test_struct_sizes(pkg):
    assert C.sizeof(pkg._lib.CgParams) == 32   # int, pad, double, double, int, pad
    assert C.sizeof(pkg._lib.CgInfo) == 48     # 2 int, 5 double
    assert C.sizeof(pkg._lib.HfParams) == 144


def test_defaults(pkg):
    L = pkg.lib()
    c = pkg._lib.CgParams()
    L.lbf_cg_default_params(C.byref(c))
    assert (c.max_iters, c.rtol, c.damping, c.check) == (50, 0.1, 0.0, 10)
    p = pkg.engine.hf_params()
    assert (p.damping0, p.damp_up, p.damp_down, p.ratio_lo, p.ratio_hi) == (1.0, 1.5, 2.0 / 3.0, 0.25, 0.75)
    assert (p.c1, p.rho, p.max_line_iters, p.curv_rows) == (1e-4, 0.5, 20, 0)
    assert (p.cg_iters, p.cg_rtol, p.cg_check) == (50, 0.1, 10)
    assert not p.damping_trace and not p.ratio_trace and not p.cg_trace and p.trace_cap == 0
    L.lbf_hf_default_params(None)  # tolerated, like the other *_default_params
    u = pkg.UnifiedConfig()
    assert (u.cg_iters, u.cg_rtol, u.damping) == (50, 0.1, 1.0)
    assert issubclass(pkg.UnifiedHF, pkg.unified.UnifiedOptimizer)


def test_null_handles_are_invalid(pkg):
    L = pkg.lib()
    c = pkg._lib.CgParams()
    L.lbf_cg_default_params(C.byref(c))
    ci = pkg._lib.CgInfo()
    assert L.lbf_mlp_gn_cg(None, None, None, None, None, None, 0, 1.0, C.byref(c), None, C.byref(ci)) == 1
    p = pkg.engine.hf_params()
    assert L.lbf_hf_solve(None, C.byref(p), None, None, None, 0, 1, None, None) == 1
    assert L.lbf_mlp_gn_cg_residual(None, None) == 1


def test_hf_params_keywords(pkg):
    p = pkg.engine.hf_params(max_iters=7, cg_iters=3, damping0=0.5, curv_rows=64)
    assert (p.max_iters, p.cg_iters, p.damping0, p.curv_rows) == (7, 3, 0.5, 64)
    with pytest.raises(pkg.LbfError):
        pkg.engine.hf_params(bogus=1)
    with pytest.raises(pkg.LbfError):
        pkg.engine.hf_params(trace_cap=4)  # the traces are hf_solve's
