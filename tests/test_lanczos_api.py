"""The Lanczos interface without a GPU: the built library exports lbf_mlp_lanczos,
lbf_lanczos_default_params and lbf_tridiag_eig, the header declares them without an ABI bump, the structs have the
header's layout and the documented defaults, every invalid argument is LBF_ERR_INVALID, lbf_tridiag_eig agrees with
numpy.linalg.eigh, slq_density integrates to 1, and the C++ class compiles and keeps the new names to itself."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lbfgs_amd.h")
BACKEND = os.path.join(ROOT, "include", "lbfgs_amd", "hip_backend.hpp")
CTYPES = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}
NEW = ("lbf_lanczos_default_params", "lbf_mlp_lanczos", "lbf_tridiag_eig")
# lbf_tridiag_eig's eigenvalues agree with numpy's within QL_MULTIPLE * m * 2^-52 * |T|_2, the backward-error scale of
# a QL sweep; the worst ratio to m * 2^-52 * |T|_2 measured over the cases below is 0.6
QL_MULTIPLE = 16


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
    assert L.lbf_mlp_lanczos.restype is C.c_int and len(L.lbf_mlp_lanczos.argtypes) == 14
    assert L.lbf_tridiag_eig.restype is C.c_int and len(L.lbf_tridiag_eig.argtypes) == 6
    assert re.search(r"^#define\s+LBF_ABI_VERSION\s+3\s*$", h, re.M)
    assert L.lbf_abi_version() == 3 and pkg._lib.ABI_VERSION == 3
    assert pkg._lib.LANCZOS_MATRICES == {"hessian": 1, "gauss_newton": 2}
    for name in ("LanczosResult", "slq_density", "spectral_density", "tridiag_eig"):
        assert hasattr(pkg, name), name
    assert hasattr(pkg.Mlp, "lanczos") and hasattr(pkg.UnifiedLauncher, "spectrum")


def test_struct_layouts_and_defaults(pkg):
    P, I = pkg._lib.LanczosParams, pkg._lib.LanczosInfo
    assert list(P._fields_) == struct_fields("lbf_lanczos_params") == [
        ("steps", C.c_int), ("matrix", C.c_int), ("reorth", C.c_int), ("check", C.c_int), ("l2", C.c_double),
        ("breakdown_rtol", C.c_double)]
    assert list(I._fields_) == struct_fields("lbf_lanczos_info") == [
        ("steps", C.c_int), ("status", C.c_int), ("v0_norm", C.c_double)]
    assert C.sizeof(P) == 32 and C.sizeof(I) == 16
    p = P(7, 7, 7, 7, 7.0, 7.0)
    pkg.lib().lbf_lanczos_default_params(C.byref(p))
    assert (p.steps, p.matrix, p.reorth, p.check, p.l2) == (32, 2, 1, 8, 0.0)
    assert 0.0 < p.breakdown_rtol < 1.0
    m = re.search(r"double breakdown_rtol; /\* ([0-9.e+-]+):", header())
    assert m and float(m.group(1)) == p.breakdown_rtol  # the header states the default the library sets
    pkg.lib().lbf_lanczos_default_params(None)  # tolerated, like the other *_default_params
    # the pinned structs are what they were
    assert C.sizeof(pkg._lib.CgParams) == 32 and C.sizeof(pkg._lib.CgInfo) == 48 and C.sizeof(pkg._lib.HfParams) == 144


def lanczos_rc(pkg, net=None, ptrs=None, ld=0, basis=None, **fields):
    """lbf_mlp_lanczos with the default parameters changed by `fields`; every device pointer is the (never
    dereferenced) address of a host buffer unless net is None, when the call has to stop at the first check."""
    L = pkg.lib()
    p = pkg._lib.LanczosParams()
    L.lbf_lanczos_default_params(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    a, b = (C.c_double * 128)(), (C.c_double * 128)()
    info = pkg._lib.LanczosInfo()
    return L.lbf_mlp_lanczos(net, ptrs, ptrs, ptrs, ptrs, None, 0, 1.0, C.byref(p), a, b, basis, ld, C.byref(info))


def test_null_handles_are_invalid(pkg):
    L = pkg.lib()
    assert lanczos_rc(pkg) == 1
    assert "invalid argument: null handle" in L.lbf_last_error().decode()
    a = (C.c_double * 4)()
    info = pkg._lib.LanczosInfo()
    assert L.lbf_mlp_lanczos(None, None, None, None, None, None, 0, 1.0, None, a, a, None, 0, C.byref(info)) == 1
    assert "null parameters" in L.lbf_last_error().decode()
    # the parameters are checked in front of the handles, so each message names its own field without a device
    for bad in (dict(steps=0), dict(steps=129), dict(steps=-1), dict(matrix=0), dict(matrix=3), dict(matrix=-1),
                dict(reorth=2), dict(reorth=-1), dict(check=0), dict(l2=-1.0), dict(l2=float("nan")),
                dict(l2=float("inf")), dict(breakdown_rtol=-1e-3), dict(breakdown_rtol=float("nan")),
                dict(breakdown_rtol=float("inf"))):
        assert lanczos_rc(pkg, **bad) == 1, bad
        (field,) = bad
        assert f"invalid argument: {field} must be" in L.lbf_last_error().decode(), bad


def test_unknown_matrix_is_rejected_before_the_device(pkg):
    with pytest.raises(pkg.LbfError, match="unknown matrix"):
        pkg.Mlp.lanczos(None, None, None, None, matrix="fd")
    with pytest.raises(pkg.LbfError, match="ritz_vectors needs"):
        pkg.LanczosResult(alpha=np.ones(2), beta=np.zeros(2), steps=2, status=0, v0_norm=1.0).ritz_vectors()


# ---------------------------------------------------------------- lbf_tridiag_eig
def tridiag_cases():
    rng = np.random.default_rng(23)
    out = {}
    for m in (1, 2, 3, 32, 128):
        out[f"random{m}"] = (rng.standard_normal(m), rng.standard_normal(max(m - 1, 0)))
    a, b = rng.standard_normal(32), rng.standard_normal(31)
    b[[0, 10, 30]] = 0.0
    out["zero_beta"] = (a, b)
    out["repeated"] = (np.full(16, 2.0), np.zeros(15))                       # one eigenvalue, sixteen times
    out["repeated_blocks"] = (np.tile([1.0, 3.0], 8), np.tile([0.5, 0.0], 8)[:15])  # eight equal 2 x 2 blocks
    out["graded"] = (10.0 ** (8.0 - np.arange(24)), 0.1 * 10.0 ** (7.0 - np.arange(23)))
    out["lanczos_like"] = (np.linspace(3.0, 0.1, 128), np.geomspace(1.0, 1e-9, 127))
    return out


@pytest.mark.parametrize("name", list(tridiag_cases()))
def test_tridiag_eig_matches_numpy(pkg, name):
    a, b = tridiag_cases()[name]
    m = a.size
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    ev, S = np.linalg.eigh(T)
    theta, w, V = pkg.tridiag_eig(a, b, vectors=True)
    unit = m * 2.0 ** -52 * np.linalg.norm(T, 2)
    ratio = np.abs(theta - ev).max() / unit
    res = np.abs(T @ V - V * theta[None, :]).max() / unit
    print(f"tridiag {name}: m {m}, |theta - numpy| / (m 2^-52 |T|) = {ratio:.2f}, residual ratio {res:.2f}")
    assert np.all(np.diff(theta) >= 0.0)
    assert ratio <= QL_MULTIPLE and res <= QL_MULTIPLE
    assert np.abs(V.T @ V - np.eye(m)).max() <= QL_MULTIPLE * m * 2.0 ** -52
    assert abs(w.sum() - 1.0) <= 1e-13 and np.all(w >= 0.0)
    assert np.abs(w - V[0] ** 2).max() <= 1e-15
    theta2, w2 = pkg.tridiag_eig(a, b)
    assert np.array_equal(theta, theta2) and np.abs(w - w2).max() <= 1e-13
    if name.startswith("random"):  # simple eigenvalues: the weights are numpy's
        assert np.abs(w - S[0] ** 2).max() <= 1e-10


def test_tridiag_eig_arguments(pkg):
    L = pkg.lib()
    a, out = (C.c_double * 3)(1.0, 2.0, 3.0), (C.c_double * 3)()
    assert L.lbf_tridiag_eig(0, a, a, out, None, None) == 1
    assert L.lbf_tridiag_eig(3, None, a, out, None, None) == 1
    assert L.lbf_tridiag_eig(3, a, None, out, None, None) == 1
    assert L.lbf_tridiag_eig(3, a, a, None, None, None) == 1
    assert L.lbf_tridiag_eig(1, a, None, out, None, None) == 0 and out[0] == 1.0
    bad = (C.c_double * 3)(1.0, float("nan"), 3.0)
    assert L.lbf_tridiag_eig(3, bad, a, out, None, None) == 1
    with pytest.raises(pkg.LbfError, match="off-diagonal"):
        pkg.tridiag_eig(np.ones(4), np.ones(2))


# ---------------------------------------------------------------- stochastic Lanczos quadrature
def test_slq_density_integrates_to_one(pkg):
    rng = np.random.default_rng(5)
    ritz = [np.sort(rng.uniform(-1.0, 4.0, 12)) for _ in range(3)]
    weights = [w / w.sum() for w in (rng.uniform(0.1, 1.0, 12) for _ in range(3))]
    grid = np.linspace(-3.0, 6.0, 4001)
    d = pkg.slq_density(ritz, weights, grid, 0.05)
    assert d.shape == grid.shape and np.all(d >= 0.0)
    integral = lambda f: float(((f[1:] + f[:-1]) * 0.5 * np.diff(grid)).sum())  # noqa: E731
    assert abs(integral(d) - 1.0) <= 1e-9
    mean = integral(d * grid)
    assert abs(mean - np.mean([(t * w).sum() for t, w in zip(ritz, weights)])) <= 1e-9
    one = pkg.slq_density([[1.0]], [[1.0]], np.array([1.0, 1.2]), 0.2)  # a single Gaussian at its mean and one sigma
    peak = 1.0 / (0.2 * np.sqrt(2.0 * np.pi))
    assert np.allclose(one, [peak, peak * np.exp(-0.5)], rtol=1e-14)
    with pytest.raises(pkg.LbfError):
        pkg.slq_density([], [], grid, 0.1)
    with pytest.raises(pkg.LbfError):
        pkg.slq_density(ritz, weights, grid, 0.0)


# ---------------------------------------------------------------- the C++ class
def test_new_symbols_stay_inside_hip_spectrum():
    """The header names the new entry points only inside HipSpectrum, so a program that uses the classes that existed
    before still links against a library without them (tests/host/fake_lbf_abi*.cpp have none of them)."""
    with open(BACKEND) as f:
        src = re.sub(r"///.*", "", f.read())
    parts = re.split(r"\nclass (\w+)", src)
    bodies = dict(zip(parts[1::2], parts[2::2]))
    assert "HipSpectrum" in bodies and {"HipNetwork", "HipHF", "HipAdam"} <= set(bodies)
    new = re.compile(r"lbf_mlp_lanczos|lbf_tridiag_eig|lbf_lanczos_")
    assert not new.search(parts[0])
    for name, body in bodies.items():
        if name != "HipSpectrum":
            assert not new.search(body), name
    assert "lbf_mlp_lanczos(" in bodies["HipSpectrum"] and "lbf_tridiag_eig(" in bodies["HipSpectrum"]
    for fake in ("fake_lbf_abi.cpp", "fake_lbf_abi_v2.cpp"):
        with open(os.path.join(ROOT, "tests", "host", fake)) as f:
            assert not new.search(f.read()), fake


TU = r"""
#include <lbfgs_amd/hip_backend.hpp>
int main() {
  hip_mlp::HipHandle h;
  hip_mlp::HipNetwork net(h);
  net.addLayer(4, 3, LBF_ACT_TANH);
  net.addLayer(3, 2, LBF_ACT_LINEAR);
  net.bindParams();
  hip_mlp::DeviceBuffer<hip_mlp::HipScalar> x(h), y(h), v(h), q(h);
  hip_mlp::HipSpectrum sp(h, net);
  sp.setSteps(8);
  sp.setMatrix(LBF_HVP_EXACT);
  sp.setReorthogonalize(false);
  sp.setL2(1e-3);
  sp.setCheck(4);
  sp.setBreakdownTolerance(1e-3);
  int status = sp.lanczos(v.data(), x.data(), y.data(), 0, q.data(), 32);
  std::vector<double> w;
  std::vector<double> theta = sp.ritz(&w);
  return status + sp.steps() + sp.status() + int(theta.size() + sp.alpha().size() + sp.beta().size());
}
"""


def test_hip_spectrum_compiles(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the drop-in header's syntax check"
    src = tmp_path / "lanczos_tu.cpp"
    src.write_text(TU)
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
