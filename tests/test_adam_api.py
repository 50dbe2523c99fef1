"""The Adam interface without a GPU: the built library exports the lbf_adam_* functions, the header declares them (and
the two structs) without an ABI bump, the ctypes structs have the header's field lists, the defaults are the documented
ones, null handles and every invalid parameter of the documented list are LBF_ERR_INVALID, lbf_adam_coefs and
lbf_adam_epoch_orders are bit for bit their Python restatements, and adam_params rejects unknown names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_adam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")
CTYPES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong, "unsigned": C.c_uint, "float": C.c_float}
SYMBOLS = ("lbf_adam_default_params", "lbf_adam_coefs", "lbf_adam_epoch_orders", "lbf_adam_step", "lbf_adam_solve",
           "lbf_adam_begin", "lbf_adam_iterate", "lbf_adam_end")


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
        t = re.match(r"(long long|int|double|unsigned|float)\s+(.*)", decl)
        assert t, decl
        for nm in t.group(2).split(","):
            nm = nm.strip()
            if nm.startswith("*"):
                out.append((nm[1:].strip(), C.POINTER(CTYPES[t.group(1)])))
            else:
                out.append((nm, CTYPES[t.group(1)]))
    return out


def c_layout(fields):
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
    for name in ("lbf_adam_params", "lbf_adam_coef"):
        assert re.search(r"typedef struct %s \{" % name, h), name
    assert L.lbf_adam_solve.restype is C.c_int
    assert L.lbf_adam_solve.argtypes[2:] == L.lbf_sgd_solve.argtypes[2:]   # the same call shape as SGD
    assert len(L.lbf_adam_begin.argtypes) == 7 and len(L.lbf_adam_iterate.argtypes) == 5
    assert len(L.lbf_adam_step.argtypes) == 8 and L.lbf_adam_coefs.argtypes[1] is C.c_double


def test_abi_version_unchanged(pkg):
    assert re.search(r"^#define\s+LBF_ABI_VERSION\s+3\s*$", header(), re.M)
    assert pkg.lib().lbf_abi_version() == 3 and pkg._lib.ABI_VERSION == 3


@pytest.mark.parametrize("cname,pyname", [("lbf_adam_params", "AdamParams"), ("lbf_adam_coef", "AdamCoef")])
def test_struct_layouts_match_header(pkg, cname, pyname):
    want = struct_fields(cname)
    S = getattr(pkg._lib, pyname)
    assert [(n, t) for n, t in S._fields_] == want
    assert C.sizeof(S) == c_layout(want)


def test_struct_sizes(pkg):
    # 6 doubles | int, int, unsigned, pad | double | int, int | double | pointer | int, pad
    assert C.sizeof(pkg._lib.AdamParams) == 104
    assert C.sizeof(pkg._lib.AdamCoef) == 36


def test_defaults(pkg):
    p = pkg.adam_params()
    assert (p.lr, p.beta1, p.beta2, p.eps) == (1e-3, 0.9, 0.999, 1e-8)
    assert (p.weight_decay, p.clip_norm) == (0.0, 0.0)
    assert (p.batch, p.shuffle, p.seed) == (128, 1, 123)
    s = pkg._lib.SgdParams()
    pkg.lib().lbf_sgd_default_params(C.byref(s))
    assert (p.decay_rate, p.decay_step) == (s.decay_rate, s.decay_step) == (1.0, 0)
    assert (p.max_epochs, p.tol) == (200, s.tol)
    assert not p.loss_trace and p.trace_cap == 0
    pkg.lib().lbf_adam_default_params(None)  # tolerated, like the other *_default_params
    cfg = pkg.UnifiedConfig()
    assert (cfg.beta1, cfg.beta2, cfg.adam_eps, cfg.weight_decay, cfg.clip_norm, cfg.shuffle) == \
        (0.9, 0.999, 1e-8, 0.0, 0.0, True)
    assert issubclass(pkg.UnifiedAdam, pkg.unified.UnifiedOptimizer)


def test_null_handles_are_invalid(pkg):
    L = pkg.lib()
    p, info, k, h = pkg.adam_params(), pkg._lib.SolveInfo(), pkg._lib.AdamCoef(), C.c_void_p()
    assert L.lbf_adam_solve(None, C.byref(p), None, None, None, 10, None, C.byref(info)) == 1
    assert "invalid argument: null" in L.lbf_last_error().decode()
    assert L.lbf_adam_solve(None, None, None, None, None, 10, None, None) == 1
    assert L.lbf_adam_begin(None, C.byref(p), None, None, None, 10, C.byref(h)) == 1 and not h.value
    assert L.lbf_adam_begin(None, C.byref(p), None, None, None, 10, None) == 1
    assert L.lbf_adam_iterate(None, 1, None, C.byref(info), None) == 1
    assert L.lbf_adam_step(None, 4, C.byref(k), None, None, None, None, None) == 1
    assert L.lbf_adam_coefs(None, 1e-3, 1, C.byref(k)) == 1 and L.lbf_adam_coefs(C.byref(p), 1e-3, 1, None) == 1
    assert L.lbf_adam_epoch_orders(5, 1, 1, None) == 1
    assert L.lbf_adam_end(None) == 0   # like free(NULL), as the other *_end


INVALID = [("batch", 0, "batch"), ("batch", -3, "batch"), ("lr", 0.0, "lr"), ("lr", -1e-3, "lr"),
           ("eps", 0.0, "eps"), ("eps", -1e-8, "eps"), ("beta1", 1.0, "beta1"), ("beta1", -0.1, "beta1"),
           ("beta2", 1.0, "beta2"), ("beta2", -0.1, "beta2"), ("beta2", float("nan"), "beta2"),
           ("weight_decay", -1e-2, "weight_decay"), ("weight_decay", float("inf"), "weight_decay"),
           ("weight_decay", float("nan"), "weight_decay"), ("clip_norm", -1.0, "clip_norm"),
           ("clip_norm", float("inf"), "clip_norm"), ("clip_norm", float("nan"), "clip_norm")]


@pytest.mark.parametrize("field,value,word", INVALID)
def test_invalid_parameters(pkg, field, value, word):
    """The parameters are checked before the handles, so the message names the field even without a network; the
    solver and the host-side coefficient function apply the same check."""
    L = pkg.lib()
    p, h, k = pkg.adam_params(**{field: value}), C.c_void_p(), pkg._lib.AdamCoef()
    assert L.lbf_adam_begin(None, C.byref(p), None, None, None, 10, C.byref(h)) == 1
    assert word in L.lbf_last_error().decode() and "null" not in L.lbf_last_error().decode()
    assert L.lbf_adam_solve(None, C.byref(p), None, None, None, 10, None, None) == 1
    assert word in L.lbf_last_error().decode()
    assert L.lbf_adam_coefs(C.byref(p), 1e-3, 1, C.byref(k)) == 1
    assert word in L.lbf_last_error().decode()


@pytest.mark.parametrize("N", [2 ** 31, 2 ** 31 + 5, 0, -1])
def test_row_count_out_of_range(pkg, N):
    L = pkg.lib()
    p, h = pkg.adam_params(), C.c_void_p()
    assert L.lbf_adam_begin(None, C.byref(p), None, None, None, N, C.byref(h)) == 1
    assert "2^31" in L.lbf_last_error().decode()
    assert L.lbf_adam_epoch_orders(N, 1, 0, (C.c_int * 1)()) == 1
    # the largest legal count passes this check and fails on the handles instead
    assert L.lbf_adam_begin(None, C.byref(p), None, None, None, 2 ** 31 - 1, C.byref(h)) == 1
    assert "null" in L.lbf_last_error().decode()


def f32(x):
    return np.float32(x)


@pytest.mark.parametrize("kw", [{}, dict(beta1=0.8, beta2=0.99, eps=1e-7, weight_decay=1e-2, clip_norm=0.5),
                                dict(beta1=0.0, beta2=0.0)])
@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_coefs_match_python_restatement(pkg, t, kw):
    lr_now = 1e-3 * 0.7   # a decayed rate
    k = pkg.adam_coefs(pkg.adam_params(**kw), lr_now, t)
    want = ref_adam.coefs_ref(t, lr_now, **kw)   # fp64 expressions; rounded once to float here
    for name, _ in pkg._lib.AdamCoef._fields_:
        got = f32(getattr(k, name))
        assert got.view(np.uint32) == f32(want[name]).view(np.uint32), (name, got, want[name])
    L = pkg.lib()
    p, out = pkg.adam_params(**kw), pkg._lib.AdamCoef()
    assert L.lbf_adam_coefs(C.byref(p), lr_now, 0, C.byref(out)) == 1      # steps count from 1
    assert L.lbf_adam_coefs(C.byref(p), 0.0, 1, C.byref(out)) == 1


@pytest.mark.parametrize("N", [1, 2, 37, 257])
def test_epoch_orders_match_numpy_restatement(pkg, N):
    got = pkg.adam_epoch_orders(N, 123, 3)
    assert got.dtype == np.int32 and got.shape == (3, N)
    assert np.array_equal(got, ref_adam.epoch_orders_ref(N, 123, 3))
    for row in got:
        assert np.array_equal(np.sort(row), np.arange(N))   # a permutation
    # epochs continue one stream: fewer epochs are a prefix, and another seed another order
    assert np.array_equal(pkg.adam_epoch_orders(N, 123, 2), got[:2])
    if N >= 37:
        assert not np.array_equal(got[0], got[1])
        assert not np.array_equal(pkg.adam_epoch_orders(N, 124, 1)[0], got[0])


def test_adam_params_keywords(pkg):
    p = pkg.adam_params(lr=2e-3, beta1=0.5, weight_decay=0.1, clip_norm=1.5, batch=7, shuffle=False, seed=9,
                        decay_rate=0.5, decay_step=2, max_epochs=4, tol=0.0)
    assert (p.lr, p.beta1, p.weight_decay, p.clip_norm, p.batch, p.shuffle, p.seed) == (2e-3, 0.5, 0.1, 1.5, 7, 0, 9)
    assert (p.decay_rate, p.decay_step, p.max_epochs, p.tol) == (0.5, 2, 4, 0.0)
    with pytest.raises(pkg.LbfError):
        pkg.adam_params(bogus=1)
    with pytest.raises(pkg.LbfError):
        pkg.adam_params(trace_cap=4)  # the trace is adam_solve's


def test_cpp_wrappers_compile_with_plain_gxx(tmp_path):
    """HipAdam and UnifiedAdam_HIP need nothing but C++17 and the C ABI, like the rest of hip_backend.hpp."""
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "lbfgs_amd/hip_backend.hpp"\n'
                   "int main(){ UnifiedConfig c; c.weight_decay = 1e-2; c.clip_norm = 1.0; c.shuffle = false;\n"
                   "  UnifiedAdam_HIP o; (void)o;\n"
                   "  static_assert(sizeof(lbf_adam_params) == 104 && sizeof(lbf_adam_coef) == 36, \"layout\");\n"
                   "  return sizeof(hip_mlp::HipAdam) > 0 ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
