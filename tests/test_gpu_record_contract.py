"""The lbf_record / lbf_solve_info contract every solver driver keeps (include/lbfgs_amd.h), driven through the C
entry points with the package's ctypes Record on a 12-16-4 tanh/linear network, N = 96, fp32.

For L-BFGS (Wolfe, Armijo), S-LBFGS, GD, SGD, HF and OWL-QN:
  * a record of capacity 3 under a longer solve holds exactly the first three rows of the same solve with room
    for all of them (every column but time_ms bitwise), reports size 3, leaves the four entries past the
    capacity of every array untouched, and the solve's lbf_solve_info does not depend on the capacity;
  * NULL columns are skipped: with only `loss` given, that column and size are those of the full record.
For L-BFGS through begin / iterate / end, iterate(2) twice on one record appends: the four rows are bitwise
those of one iterate(4).
The solves are deterministic (fixed seeds, bitwise-reproducible kernels), so every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS, ACTS, N = [12, 16, 4], ["tanh", "linear"], 96
ITERS, LONG_CAP, PAD = 8, 16, 4
SOLVERS = ["wolfe", "armijo", "slbfgs", "gd", "sgd", "hf", "owlqn"]
COLS = ("loss", "grad_norm", "time_ms", "alpha", "ls_trials", "accepted")
INT_COLS = ("ls_trials", "accepted")
SENT_D, SENT_I = -12345.5, -4242
INFO_FIELDS = ("iterations", "n_evals", "final_loss", "final_grad_norm", "n_rows", "n_loss_only", "n_grad_after_loss")


class Rec:
    """A Record over sentinel-filled arrays of cap + PAD entries; columns not in `cols` are NULL."""

    def __init__(self, pkg, cap, cols=COLS):
        self.cap, self.cols, self.a = cap, cols, {}
        ptrs = []
        for c in COLS:
            if c not in cols:
                ptrs.append(None)
            elif c in INT_COLS:
                self.a[c] = np.full(cap + PAD, SENT_I, np.int32)
                ptrs.append(self.a[c].ctypes.data_as(C.POINTER(C.c_int)))
            else:
                self.a[c] = np.full(cap + PAD, SENT_D, np.float64)
                ptrs.append(self.a[c].ctypes.data_as(C.POINTER(C.c_double)))
        self.rec = pkg._lib.Record(*ptrs, cap, 0)

    @property
    def size(self):
        return int(self.rec.size)

    def guards_untouched(self):
        return all((a[self.cap:] == (SENT_I if c in INT_COLS else SENT_D)).all() and
                   (a[self.size:self.cap] == (SENT_I if c in INT_COLS else SENT_D)).all()
                   for c, a in self.a.items())

    def rows(self, c, n):
        return self.a[c][:n].tobytes()


@pytest.fixture(scope="module")
def prob(pkg, ctx):
    rng = np.random.default_rng(20)
    X = torch.from_numpy(rng.standard_normal((N, DIMS[0])).astype(np.float32)).cuda()
    Y = torch.from_numpy(rng.standard_normal((N, DIMS[-1])).astype(np.float32)).cuda()
    P0 = torch.from_numpy(pkg.init_params_host(DIMS, ACTS, 123, "cpu")).cuda()
    return dict(net=pkg.Mlp(ctx, DIMS, ACTS), X=X, Y=Y, P0=P0, long={})  # one network: its counters keep running


def info_tuple(info):
    return tuple(getattr(info, f) for f in INFO_FIELDS)


def solve(pkg, prob, name, rec, iters=ITERS):
    """One solve of `name` from the start point into rec; returns lbf_solve_info as a tuple."""
    L, E, lib_ = pkg.lib(), pkg.engine, pkg._lib
    net, X, Y, P = prob["net"], prob["X"], prob["Y"], prob["P0"].clone()
    h, p, x, y, r, info = net.h, lib_.ptr(P), lib_.ptr(X), lib_.ptr(Y), C.byref(rec.rec), lib_.SolveInfo()
    if name in ("wolfe", "armijo"):
        prm = E.lbfgs_params(name, m=4, max_iters=iters, tol=0.0)
        rc = L.lbf_lbfgs_solve(h, C.byref(prm), p, x, y, N, N, r, C.byref(info))
    elif name == "slbfgs":
        prm = E.slbfgs_params(max_epochs=iters, tol=0.0, M=4, L=2, b=16, b_H=16, step=0.01, lam=1e-4, seed=7)
        rc = L.lbf_slbfgs_solve(h, C.byref(prm), p, x, y, N, r, C.byref(info))
    elif name == "gd":
        prm = lib_.GdParams()
        L.lbf_gd_default_params(C.byref(prm))
        prm.lr, prm.max_iters, prm.tol = 0.05, iters, 0.0
        rc = L.lbf_gd_solve(h, C.byref(prm), p, x, y, N, N, r, C.byref(info))
    elif name == "sgd":
        prm = lib_.SgdParams()
        L.lbf_sgd_default_params(C.byref(prm))
        prm.lr, prm.batch, prm.max_epochs, prm.tol = 0.02, 32, iters, 0.0
        rc = L.lbf_sgd_solve(h, C.byref(prm), p, x, y, N, r, C.byref(info))
    elif name == "hf":
        prm = E.hf_params(max_iters=iters, tol=0.0, cg_iters=10)
        rc = L.lbf_hf_solve(h, C.byref(prm), p, x, y, N, N, r, C.byref(info))
    else:
        prm = E.owlqn_params(m=4, max_iters=iters, tol=0.0, l1=1e-3)
        rc = L.lbf_owlqn_solve(h, C.byref(prm), p, x, y, N, N, r, C.byref(info), None)
    lib_.check(rc, name)
    return info_tuple(info)


def long_run(pkg, prob, name):
    """The solve with room for every row, computed once per solver and left unchanged."""
    if name not in prob["long"]:
        rec = Rec(pkg, LONG_CAP)
        prob["long"][name] = (rec, solve(pkg, prob, name, rec))
    return prob["long"][name]


@pytest.mark.parametrize("name", SOLVERS)
def test_capacity_three(pkg, prob, name):
    full, info_full = long_run(pkg, prob, name)
    assert 6 <= full.size <= LONG_CAP and full.guards_untouched()
    t = full.a["time_ms"][:full.size]
    assert (t >= 0.0).all() and (np.diff(t) >= 0.0).all()
    if name == "sgd":  # the record of the start point (sgd.cuh:93-98)
        assert t[0] == 0.0
    short = Rec(pkg, 3)
    info_short = solve(pkg, prob, name, short)
    assert short.size == 3
    for c in COLS:
        if c != "time_ms":
            assert short.rows(c, 3) == full.rows(c, 3), c
    assert (short.a["time_ms"][:3] >= 0.0).all()
    assert short.guards_untouched()
    assert info_short == info_full


@pytest.mark.parametrize("name", SOLVERS)
def test_only_loss_column(pkg, prob, name):
    full, info_full = long_run(pkg, prob, name)
    only = Rec(pkg, LONG_CAP, cols=("loss",))
    info = solve(pkg, prob, name, only)
    assert only.size == full.size
    assert only.rows("loss", only.size) == full.rows("loss", full.size)
    assert only.guards_untouched()
    assert info == info_full


@pytest.mark.parametrize("name", ["wolfe", "armijo"])
def test_iterate_appends(pkg, prob, name):
    L, E, lib_ = pkg.lib(), pkg.engine, pkg._lib
    out = []
    for calls in ((4,), (2, 2)):
        P, rec, info, h = prob["P0"].clone(), Rec(pkg, LONG_CAP), lib_.SolveInfo(), C.c_void_p()
        prm = E.lbfgs_params(name, m=4, max_iters=1 << 30, tol=0.0)
        lib_.check(L.lbf_lbfgs_begin(prob["net"].h, C.byref(prm), lib_.ptr(P), lib_.ptr(prob["X"]), lib_.ptr(prob["Y"]),
                                     N, N, C.byref(h)), "lbf_lbfgs_begin")
        try:
            for k in calls:
                lib_.check(L.lbf_lbfgs_iterate(h, k, C.byref(rec.rec), C.byref(info)), "lbf_lbfgs_iterate")
        finally:
            L.lbf_lbfgs_end(h)
        assert rec.size == 4 and rec.guards_untouched()
        out.append(([rec.rows(c, 4) for c in COLS if c != "time_ms"], info_tuple(info), P.cpu().numpy().tobytes()))
    assert out[0] == out[1]
