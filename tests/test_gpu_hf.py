"""Hessian-free optimisation: the device-side Gauss-Newton conjugate gradients (Mlp.gn_cg /
lbf_mlp_gn_cg, lbfgs-ffnn_amd/csrc/cg.hip) and the solver built on them (engine.hf_solve / lbf_hf_solve).

The reference is torch fp64 on the CPU (ref_mlp.py): the Gauss-Newton product (jvp of the network output, the
loss's Hessian in closed form, vjp back), textbook CG from x = 0 on it, and the outer iteration of lbfgs_amd.h
(Armijo backtracking from alpha = 1, Levenberg-Marquardt damping from the first trial's reduction ratio). The
same code run in fp32 on the CPU gives the error an fp32 implementation is allowed.

Bounds. Few-step CG iterates: max(1e-4, 3 x the CPU fp32 restatement's error), the project's gradient rule.
Converged CG and the least-squares known answer: 1e-4 (condition numbers <= 25, the fp32 restatement is below
4e-7). Trajectories: equal decisions, damping to 1e-12, loss and parameters to 1e-3 (the project's trajectory
bound); the reference's reduction ratios are first shown to stay 5e-3 away from both thresholds, so an fp32
evaluation cannot flip a damping decision.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev, gpu_args, make_net, run_ranks, solver_inputs
from ref_mlp import NETS, SMALL, XENT, gn_matrix, gn_ref, hf_ref, host_args, make_case, nparams, pcg_ref, rel

pytestmark = pytest.mark.gpu


def case(pkg, name, loss=None, seed=0):
    """`wide` regresses on synth_mnist's one-hot labels here."""
    return make_case(pkg, NETS, name, loss, seed, keep_labels=True)


def run_cg(pkg, ctx, c, net=None, **kw):
    net = net or make_net(pkg, ctx, c)
    P, b, X, Y, idx = gpu_args(c)
    return net.gn_cg(P, b, X, Y, idx=idx, **kw)


# ---------------------------------------------------------------- CG against fp64
@pytest.mark.parametrize("damping", [0.1, 0.01])
@pytest.mark.parametrize("name", list(NETS))
def test_cg_five_steps_match_fp64(ctx, pkg, name, damping):
    c = case(pkg, name)
    ref = {}
    for dt in (torch.float64, torch.float32):
        P, b, X, Y = host_args(c, dt)
        A = lambda v: gn_ref(c["dims"], c["acts"], c["loss"], P, v, X, Y, 1.0 / X.shape[0], damping)  # noqa: E731
        ref[dt] = pcg_ref(A, b, None, 5, 0.0)[0]
    own = rel(ref[torch.float32], ref[torch.float64])
    x, info = run_cg(pkg, ctx, c, damping=damping, max_iters=5, rtol=0.0)
    err = rel(x, ref[torch.float64])
    print(f"cg k=5 {name} damping={damping}: rel {err:.2e}, cpu fp32 {own:.2e}")
    assert info["iterations"] == 5 and info["status"] == 1
    assert err <= max(1e-4, 3 * own)


@pytest.mark.parametrize("name", SMALL)
def test_cg_converged_matches_dense_solve(ctx, pkg, name):
    c = case(pkg, name)
    P, b, X, Y = host_args(c, torch.float64)
    G = gn_matrix(c["dims"], c["acts"], c["loss"], P, X, Y, 1.0 / X.shape[0]).numpy()
    A = G + 0.1 * np.eye(G.shape[0])
    want = np.linalg.solve(A, b.numpy())
    x, info = run_cg(pkg, ctx, c, damping=0.1, max_iters=40, rtol=0.0)
    err = rel(x, want)
    print(f"cg converged {name}: rel {err:.2e}, cond {np.linalg.cond(A):.1f}, iterations {info['iterations']}")
    assert err <= 1e-4


def test_cg_least_squares_known_answer(ctx, pkg):
    """One linear layer with the squared error: G is the exact Hessian, so P + x with G x = -g is the minimiser."""
    dims, acts, N = [40, 8], ["linear"], 257
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 40)).astype(np.float32)
    Y = rng.standard_normal((N, 8)).astype(np.float32)
    P = rng.standard_normal(nparams(dims)).astype(np.float32)
    net = pkg.Mlp(ctx, dims, acts)
    Pd, Xd, Yd = dev(P), dev(X), dev(Y)
    _, g = net.loss_grad(Pd, Xd, Yd)
    x, info = net.gn_cg(Pd, -g, Xd, Yd, damping=0.0, max_iters=30, rtol=0.0)
    A1 = np.hstack([X.astype(np.float64), np.ones((N, 1))])
    W = np.linalg.lstsq(A1, Y.astype(np.float64), rcond=None)[0]  # [41, 8]: weights then the bias row
    want = np.concatenate([W[:40].ravel(), W[40]])
    err = rel(Pd + x, want)
    print(f"least squares: rel {err:.2e}, iterations {info['iterations']}")
    assert err <= 1e-4


# ---------------------------------------------------------------- stopping and freezing
@pytest.mark.parametrize("name", list(NETS))
def test_cg_stops_at_rtol_and_freezes(ctx, pkg, name):
    c = case(pkg, name)
    net = make_net(pkg, ctx, c)
    P, b, X, Y, idx = gpu_args(c)
    x, info = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=50, rtol=0.1, check=50, residual=True)
    assert info["status"] == 0 and 0 < info["iterations"] < 50
    Ax = net.gnvp(P, x, X, Y, idx=idx, l2=0.1)
    true = float((b.double() - Ax.double()).norm() / b.double().norm())
    rnorm = float(info["r"].double().norm())
    print(f"stop {name}: {info['iterations']} iterations, true residual {true:.3e}, sqrt(rr) {info['rr'] ** 0.5:.6e}")
    assert true <= 0.1 + 1e-4
    assert abs(info["rr"] ** 0.5 - rnorm) <= 1e-6 * rnorm
    assert info["rr"] <= 0.01 * info["rr0"]
    # the iterations enqueued past the stopping one change nothing
    x1, i1 = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=50, rtol=0.1, check=1, residual=True)
    x7, i7 = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=info["iterations"], rtol=0.0, check=7,
                       residual=True)
    assert torch.equal(x, x1) and torch.equal(x, x7)
    assert torch.equal(info["r"], i1["r"]) and torch.equal(info["r"], i7["r"])
    for k in ("iterations", "rr", "rr0", "xb", "xr", "xx"):
        assert info[k] == i1[k] == i7[k], k
    assert (i1["status"], i7["status"]) == (0, 1)
    # run to run
    x2, i2 = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=50, rtol=0.1, check=50)
    assert torch.equal(x, x2) and i2["rr"] == info["rr"]


@pytest.mark.parametrize("name", ["n387", "mnist"])
def test_cg_zero_rhs_and_indefinite(ctx, pkg, name):
    c = case(pkg, name)
    net = make_net(pkg, ctx, c)
    P, b, X, Y, idx = gpu_args(c)
    x, info = net.gn_cg(P, torch.zeros_like(b), X, Y, idx=idx, damping=0.1, out=torch.full_like(b, 7.0))
    assert info["iterations"] == 0 and info["status"] == 0 and info["rr0"] == 0.0
    assert torch.equal(x, torch.zeros_like(x))
    # G's largest eigenvalue is <= 2.6 on these nets: G - 10 I is negative definite, p.Ap < 0 at once
    x, info = net.gn_cg(P, b, X, Y, idx=idx, damping=-10.0, max_iters=20, check=20)
    assert info["status"] == 2 and info["iterations"] == 0
    assert bool(torch.isfinite(x).all()) and torch.equal(x, torch.zeros_like(x))
    # and the network still works
    x, info = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1)
    assert info["status"] == 0


# ---------------------------------------------------------------- workspace and pointers
@pytest.mark.parametrize("name", ["n387", "mnist", "wide"])
def test_cg_after_other_evaluations_is_bitwise(ctx, pkg, name):
    c = case(pkg, name)
    P, b, X, Y, idx = gpu_args(c)
    fresh, _ = make_net(pkg, ctx, c).gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=8, rtol=0.0)
    net = make_net(pkg, ctx, c)
    net.loss_grad(P, X, Y)  # the fused forward on all rows: another batch size, another workspace state
    x1, _ = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=8, rtol=0.0)
    net.evaluate(P, X, Y)
    x2, _ = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=8, rtol=0.0)
    net.hvp(P, b, X, Y, idx=idx)
    x3, _ = net.gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=8, rtol=0.0)
    assert torch.equal(fresh, x1) and torch.equal(fresh, x2) and torch.equal(fresh, x3)


@pytest.mark.parametrize("name", ["n387", "xent10", "wide"])
def test_cg_unaligned_pointers(ctx, pkg, name):
    c = case(pkg, name)
    P, b, X, Y, idx = gpu_args(c)
    n = P.numel()
    want, wi = make_net(pkg, ctx, c).gn_cg(P, b, X, Y, idx=idx, damping=0.1, max_iters=6, rtol=0.0)
    bufs = [torch.full((n + 8,), 1234.5, device="cuda") for _ in range(3)]
    Pu, bu, xu = (t[1:n + 1] for t in bufs)
    assert Pu.data_ptr() % 16 == 4
    Pu.copy_(P)
    bu.copy_(b)
    keep = [t.clone() for t in bufs[:2]]
    x, info = make_net(pkg, ctx, c).gn_cg(Pu, bu, X, Y, idx=idx, damping=0.1, max_iters=6, rtol=0.0, out=xu)
    assert x.data_ptr() == xu.data_ptr()
    err = rel(x, want)
    print(f"unaligned {name}: rel {err:.2e}")
    assert err <= 1e-6
    assert torch.equal(bufs[0], keep[0]) and torch.equal(bufs[1], keep[1])
    assert bool((bufs[2][:1] == 1234.5).all()) and bool((bufs[2][n + 1:] == 1234.5).all())


@pytest.mark.parametrize("name", list(NETS))
def test_cg_first_iteration_is_the_gauss_newton_product(ctx, pkg, name):
    """max_iters = 1: x = alpha b with alpha = b.b / b.Ab, A b from Mlp.gnvp (its own forward pass)."""
    c = case(pkg, name)
    net = make_net(pkg, ctx, c)
    P, b, X, Y, idx = gpu_args(c)
    x, info = net.gn_cg(P, b, X, Y, idx=idx, damping=0.05, max_iters=1, rtol=0.0)
    Ab = net.gnvp(P, b, X, Y, idx=idx, l2=0.05).double()
    bd = b.double()
    alpha = float(bd @ bd) / float(bd @ Ab)
    assert abs(info["rr0"] - float(bd @ bd)) <= 1e-12 * info["rr0"]
    assert abs(info["xb"] / info["rr0"] - alpha) <= 1e-6 * alpha
    assert rel(x, alpha * bd) <= 1e-6
    rr = float((bd - alpha * Ab).norm() ** 2)
    assert abs(info["rr"] - rr) <= 1e-5 * rr


# ---------------------------------------------------------------- the solver
TRAJ = [(n, l, l2) for n in SMALL for l in ("mse", XENT) for l2 in (0.0, 1e-3)]
TRAJ_SEED = 2  # every reduction ratio of the fp64 reference >= 8e-3 from 0.25 and 0.75 on all twelve cases


@pytest.mark.parametrize("name,loss,l2", TRAJ, ids=[f"{n}-{l}-{l2}" for n, l, l2 in TRAJ])
def test_hf_trajectory_matches_fp64(ctx, pkg, name, loss, l2):
    c = case(pkg, name, loss, TRAJ_SEED)
    ref = hf_ref(c, torch.float64, l2, 8)
    margin = min(min(abs(r - 0.25), abs(r - 0.75)) for r in ref["ratio"])
    assert margin >= 5e-3, ref["ratio"]
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=8, tol=0.0, damping0=1.0, cg_iters=10, cg_rtol=0.1)
    dl = float(np.abs(hist["loss"] - np.array(ref["loss"])).max())
    dp = rel(P, ref["P"])
    print(f"hf {name} {loss} l2={l2}: loss dev {dl:.2e}, params rel {dp:.2e}, ratio margin {margin:.3f}, "
          f"cg {list(tr['cg'])}, trials {list(hist['ls_trials'])}")
    assert info.iterations == 8
    assert list(tr["cg"]) == ref["cg"]
    assert list(hist["ls_trials"]) == ref["trials"] and list(hist["accepted"]) == ref["accepted"]
    np.testing.assert_allclose(tr["damping"], ref["damping"], rtol=1e-12, atol=0)
    assert dl <= 1e-3
    assert dp <= 1e-3


@pytest.mark.parametrize("name", SMALL)
def test_hf_backtracking(ctx, pkg, name):
    """A nearly undamped step overshoots: the line search has to cut it."""
    c = case(pkg, name)
    l2 = 1e-3
    kw = dict(damping0=1e-4, cg_iters=30, cg_rtol=1e-3)
    ref = hf_ref(c, torch.float64, l2, 1, **kw)
    assert 2 <= ref["trials"][0] <= 3, ref["trials"]
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    P0 = P.clone()
    hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=1, tol=0.0, **kw)
    print(f"backtracking {name}: trials {hist['ls_trials'][0]}, alpha {hist['alpha'][0]}, ratio {tr['ratio'][0]:.3f}")
    assert hist["ls_trials"][0] == ref["trials"][0] and hist["alpha"][0] == ref["alpha"][0]
    assert hist["accepted"][0] == 1
    assert tr["damping"][0] == 1e-4 * 1.5  # damping0 * damp_up, the product the solver forms
    # Armijo at the accepted point, recomputed: f = data loss + 0.5 l2 |w|^2, g.p from the step itself
    f0, g = net.loss_grad(P0, X, Y, l2=l2)
    step = (P - P0).double()
    f1 = net.loss(P, X, Y) + 0.5 * l2 * float(P.double() @ P.double())
    assert f1 <= f0 + 1e-4 * float(g.double() @ step) + 1e-7 * abs(f0)


def test_hf_properties(ctx, pkg):
    c = case(pkg, "mnist")
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    P0 = P.clone()
    hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=15, tol=0.0)
    assert info.iterations == 15 and len(hist["loss"]) == 15
    assert np.all(np.diff(hist["loss"]) <= 0.0), hist["loss"]
    assert info.final_loss <= hist["loss"][-1]
    assert info.n_evals == 16 and info.n_loss_only == int(hist["ls_trials"].sum())
    assert info.n_rows == 16 * X.shape[0]
    _, ginfo = pkg.gd_solve(net, P0, X, Y, max_iters=int(info.n_evals) - 1, tol=0.0)
    assert ginfo.n_evals == info.n_evals
    print(f"hf loss {info.final_loss:.5f} against gd {ginfo.final_loss:.5f} at {info.n_evals} gradient evaluations")
    assert info.final_loss < ginfo.final_loss


def test_hf_curv_rows(ctx, pkg):
    c = case(pkg, "xent10")
    N = len(c["X"])
    runs = []
    for cr in (0, N):
        P, X, Y = solver_inputs(c)
        hist, info, tr = pkg.hf_solve(make_net(pkg, ctx, c), P, X, Y, max_iters=4, tol=0.0, curv_rows=cr)
        runs.append((P, hist["loss"], tr["damping"]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    # a window of N / 4 rows: the first step is gn_cg on rows [0, N / 4) with inv_scale 4 / N
    w = N // 4
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    P0 = P.clone()
    hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=1, tol=0.0, curv_rows=w, cg_iters=10, cg_rtol=0.1)
    _, g = net.loss_grad(P0, X, Y)
    step, ci = net.gn_cg(P0, -g, X[:w].contiguous(), Y[:w].contiguous(), damping=1.0, max_iters=10, rtol=0.1)
    assert tr["cg"][0] == ci["iterations"] and hist["accepted"][0] == 1
    alpha = float(hist["alpha"][0])  # a power of two: alpha * step is exact, so the sum rounds once either way
    assert torch.equal(P, P0 + alpha * step)


def test_hf_curv_rows_needs_a_single_rank(pkg):
    c = case(pkg, "n387")
    cx = pkg.Context(0, use_torch_stream=False)
    pkg.Context.comm_init_local([cx])
    net = make_net(pkg, cx, c)
    P, X, Y = solver_inputs(c)
    with pytest.raises(pkg.LbfError, match="status 1"):
        pkg.hf_solve(net, P, X, Y, max_iters=1, curv_rows=8)
    hist, info, _ = pkg.hf_solve(net, P, X, Y, max_iters=2, tol=0.0)  # all rows: fine on a communicator
    assert info.iterations == 2


# ---------------------------------------------------------------- two ranks
@pytest.mark.parametrize("split", [100, 0], ids=["unequal", "empty-shard"])
def test_world2_cg(ctx, pkg, split):
    """Shards [0, split) and [split, N): both ranks bitwise equal, the single rank's answer, and an early stop
    whose frozen iterations still all-reduce."""
    c = case(pkg, "xent10")
    N = len(c["X"])
    P, b, X, Y, _ = gpu_args(c)
    one, oi = make_net(pkg, ctx, c).gn_cg(P, b, X, Y, damping=0.1, max_iters=50, rtol=0.1, check=1)
    bounds = [(0, split), (split, N)]

    def body(r, cx):
        lo, hi = bounds[r]
        net = make_net(pkg, cx, c)
        Xr, Yr = X[lo:hi].contiguous(), Y[lo:hi].contiguous()
        res = []
        for check in (50, 1):
            x, info = net.gn_cg(P.clone(), b.clone(), Xr, Yr, inv_scale=1.0 / N, damping=0.1, max_iters=50,
                                rtol=0.1, check=check)
            res.append((x, info))
        return res

    out = run_ranks(pkg, 2, body)
    for r in range(2):
        (xa, ia), (xb, ib) = out[r]
        assert torch.equal(xa, xb) and ia == ib  # check = 50 against check = 1
        assert bool(torch.isfinite(xa).all())
        assert torch.equal(xa, out[0][0][0]) and ia == out[0][0][1]  # against rank 0
    assert out[0][0][1]["iterations"] == oi["iterations"] < 50
    err = rel(out[0][0][0], one)
    print(f"world 2 cg (split {split}): against one rank rel {err:.2e}")
    assert err <= 1e-5


def test_world2_hf(ctx, pkg):
    c = case(pkg, "xent10")
    N = len(c["X"])
    P, X, Y = solver_inputs(c)
    h1, i1, t1 = pkg.hf_solve(make_net(pkg, ctx, c, l2=1e-3), P, X, Y, max_iters=5, tol=0.0, cg_iters=10)
    bounds = [(0, 100), (100, N)]

    def body(r, cx):
        lo, hi = bounds[r]
        Pr = dev(c["P"])
        h, i, t = pkg.hf_solve(make_net(pkg, cx, c, l2=1e-3), Pr, X[lo:hi].contiguous(), Y[lo:hi].contiguous(),
                               n_global=N, max_iters=5, tol=0.0, cg_iters=10)
        return Pr, h, t

    out = run_ranks(pkg, 2, body)
    assert torch.equal(out[0][0], out[1][0])
    for k in ("loss", "ls_trials", "accepted", "alpha"):
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    assert np.array_equal(out[0][2]["damping"], out[1][2]["damping"])
    dl = float(np.abs(out[0][1]["loss"] - h1["loss"]).max())
    print(f"world 2 hf: loss against one rank {dl:.2e}")
    assert dl <= 1e-5
    assert np.array_equal(out[0][1]["ls_trials"], h1["ls_trials"]) and np.array_equal(out[0][2]["cg"], t1["cg"])
    assert np.array_equal(out[0][2]["damping"], t1["damping"])


# ---------------------------------------------------------------- unified layer
def test_unified_hf(pkg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    c = case(pkg, "xent10")
    data = pkg.UnifiedDataset(train_x=c["X"], train_y=c["Y"], test_x=c["X"][:32], test_y=c["Y"][:32])
    cfg = pkg.UnifiedConfig(name="hf_test", max_iters=4, tolerance=0.0, cg_iters=10, cg_rtol=0.1, damping=1.0,
                            loss=XENT)
    launcher = pkg.UnifiedLauncher()
    for i in range(len(c["acts"])):
        launcher.addLayer(c["dims"][i], c["dims"][i + 1], c["acts"][i])
    launcher.buildNetwork()
    launcher.setData(data)
    opt = pkg.UnifiedHF()
    launcher.train(opt, cfg)
    assert opt.info.iterations == 4 and len(opt.traces["cg"]) == 4
    assert np.all(np.diff(opt.history["loss"]) <= 0.0)
    csvs = list(tmp_path.rglob("*.csv"))
    assert csvs and any("hf_test" in p.name for p in csvs)
    # a curvature window has no shard split: rejected under a communicator, even a one-rank one
    pkg.Context.comm_init_local([launcher.ctx])
    cfg.curv_rows = 64
    with pytest.raises(pkg.LbfError, match="status 1"):
        launcher.train(pkg.UnifiedHF(), cfg)
