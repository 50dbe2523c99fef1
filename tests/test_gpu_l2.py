"""L2 weight decay of the full-batch solvers (lbf_mlp_set_l2): lbfgs_solve / LbfgsRun, gd_solve and sgd_solve
minimise and report

    data loss + 0.5 * l2 * ||w||^2,        gradient: data gradient + l2 * w,

against torch fp64 autograd of that objective (ref_mlp.objective). Both losses, three nets:
  [784,32,10] relu/linear, N = 256      the fused-head route
  [37,50,3] tanh/linear, N = 100        the generic route; n = 2053 parameters: every w.w partial kernel has a
                                        ragged last block (2053 is no multiple of 64 or 256)
  [20,16,16,4] tanh/tanh/linear, N = 63 three layers
l2 is chosen per case so that at the start point the penalty equals RATIO x the data term (asserted to lie in
[0.1, 10]): a dropped penalty cannot hide inside a tolerance. Bounds are the project's own: loss 1e-5 and
gradient 1e-4 (test_cfg2_loss_grad_full_size), trajectories 1e-3 (test_lbfgs_matches_callback_objective), data
parallel 1e-5 / 1e-4 (test_ranks_cfg2_full_size_trajectory), GD / SGD 1e-3 (test_gpu_gd.py). Every test prints
what it measured.

The w.w of a trial point is one block of fp64 partials written by the kernel that wrote the point and summed in one
order by every consumer, so a loss-only trial, the early Armijo test and the full evaluation of a
point add the same penalty bits: the bitwise tests below (speculation depths, early exit on / off, chunked runs,
repeated runs) are the check of that.
"""
import numpy as np
import pytest
import torch

import ref_mlp
from gpu_helpers import dev, host, run_ranks, shard
from ref_mlp import MSE, XENT, rel

pytestmark = pytest.mark.gpu

NETS = {
    "mnist32": ([784, 32, 10], ["relu", "linear"], 256),
    "tanh50": ([37, 50, 3], ["tanh", "linear"], 100),
    "deep3": ([20, 16, 16, 4], ["tanh", "tanh", "linear"], 63),
}
RATIO = 1.0  # penalty / data term at the start point


def data_of(pkg, case):
    dims, acts, N = NETS[case]
    if case == "mnist32":
        return pkg.synth_mnist(N)
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    return X, ref_mlp.one_hot(rng, N, dims[-1])


def objective(dims, acts, Xh, Yh, lam, loss):
    return ref_mlp.objective(dims, acts, loss, torch.from_numpy(Xh).double(), torch.from_numpy(Yh).double(),
                             1.0 / len(Xh), lam)


def value_grad(f, P):
    p = P.detach().double().cpu().requires_grad_(True)
    l = f(p)
    (g,) = torch.autograd.grad(l, p)
    return float(l.detach()), g


def pick_l2(dims, acts, P, Xh, Yh, loss, ratio=RATIO):
    """l2 with penalty = ratio x data term at P (three significant digits), and the asserted ratio."""
    data = float(objective(dims, acts, Xh, Yh, 0.0, loss)(P.double().cpu()))
    pen1 = 0.5 * float((P.double() ** 2).sum())
    lam = float(f"{ratio * data / pen1:.3g}")
    got = lam * pen1 / data
    assert 0.1 <= got <= 10.0, (lam, got)
    return lam


def setup(ctx, pkg, case, loss, init="cpu", seed=123, ratio=RATIO):
    dims, acts, _ = NETS[case]
    Xh, Yh = data_of(pkg, case)
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(seed, init)
    lam = pick_l2(dims, acts, P, Xh, Yh, loss, ratio)
    return dims, acts, Xh, Yh, net, P, lam


# ---------------------------------------------------------------------------------------------------------------
# 1. the reported objective and gradient norm are those of the returned point
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 5])
@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
@pytest.mark.parametrize("loss", [XENT, MSE])
@pytest.mark.parametrize("case", sorted(NETS))
def test_objective_at_returned_point(ctx, pkg, case, loss, line_search, iters):
    dims, acts, Xh, Yh, net, P0, lam = setup(ctx, pkg, case, loss)
    X, Y = dev(Xh), dev(Yh)
    net.l2 = lam
    P = P0.clone()
    _, info = pkg.lbfgs_solve(net, P, X, Y, line_search=line_search, m=5, max_iters=iters, tol=0.0)
    f_ref, g_ref = value_grad(objective(dims, acts, Xh, Yh, lam, loss), P)
    gn_ref = float(g_ref.norm())
    dl, dg = abs(info.final_loss - f_ref) / abs(f_ref), abs(info.final_grad_norm - gn_ref) / gn_ref
    print(f"l2 {case} {loss} {line_search} it={iters} l2={lam:g}: loss rel {dl:.2e}, |g| rel {dg:.2e}")
    assert dl <= 1e-5
    assert dg <= 1e-4
    net.l2 = 0.0
    Q = P0.clone()
    pkg.lbfgs_solve(net, Q, X, Y, line_search=line_search, m=5, max_iters=iters, tol=0.0)
    assert not torch.equal(P, Q)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_objective_at_returned_point_wide_partial_blocks(ctx, pkg, line_search):
    """n = 2,108,426 > 2^21 parameters: the w.w partials cover 512 elements each (ww_block_elems) and come from a
    launch of their own behind the streaming combine / axpy_to, on the unfused route; the same check as above."""
    dims, acts, N = [2048, 1024, 10], ["relu", "linear"], 64
    rng = np.random.default_rng(3)
    Xh = rng.standard_normal((N, dims[0])).astype(np.float32)
    Yh = np.zeros((N, dims[-1]), np.float32)
    Yh[np.arange(N), rng.integers(0, dims[-1], N)] = 1.0
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    assert net.nparams > 1 << 21
    P = net.init_params(123, "cpu")
    lam = pick_l2(dims, acts, P, Xh, Yh, XENT)
    net.l2 = lam
    hist, info = pkg.lbfgs_solve(net, P, dev(Xh), dev(Yh), line_search=line_search, m=5, max_iters=5, tol=0.0)
    f_ref, g_ref = value_grad(objective(dims, acts, Xh, Yh, lam, XENT), P)
    gn_ref = float(g_ref.norm())
    dl, dg = abs(info.final_loss - f_ref) / abs(f_ref), abs(info.final_grad_norm - gn_ref) / gn_ref
    print(f"l2 wide {line_search} l2={lam:g}: loss rel {dl:.2e}, |g| rel {dg:.2e}, trials {hist['ls_trials']}, "
          f"n_loss_only {info.n_loss_only}")
    assert dl <= 1e-5
    assert dg <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# 2. trajectory against the callback solver on the torch fp64 regularised objective
# ---------------------------------------------------------------------------------------------------------------
def callback_of(f):
    def fn(p, g):
        l, gr = value_grad(f, p)
        g.copy_(gr.float())
        return l
    return fn


def check_trajectory(ctx, pkg, case, loss, line_search, m, iters):
    dims, acts, Xh, Yh, net, P, lam = setup(ctx, pkg, case, loss)
    net.l2 = lam
    Pf = P.clone()
    hist, _ = pkg.lbfgs_solve(net, P, dev(Xh), dev(Yh), line_search=line_search, m=m, max_iters=iters, tol=0.0)
    fn = callback_of(objective(dims, acts, Xh, Yh, lam, loss))
    ref, _ = pkg.lbfgs_solve_fn(ctx, Pf, fn, line_search=line_search, m=m, max_iters=iters, tol=0.0)
    assert len(hist["loss"]) == len(ref["loss"]) == iters
    r = np.abs(hist["loss"] - ref["loss"]) / np.abs(ref["loss"])
    print(f"l2 lbfgs {case} {loss} {line_search} m={m} l2={lam:g}: loss rel max {r.max():.2e}; "
          f"trials {hist['ls_trials']} / {ref['ls_trials']}")
    assert r.max() <= 1e-3, r
    assert np.all(np.diff(hist["loss"]) <= 0)
    assert np.array_equal(hist["ls_trials"], ref["ls_trials"])


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
@pytest.mark.parametrize("loss", [XENT, MSE])
@pytest.mark.parametrize("case", sorted(NETS))
def test_lbfgs_matches_callback_objective(ctx, pkg, case, loss, line_search):
    check_trajectory(ctx, pkg, case, loss, line_search, m=5, iters=10)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_unfused_gram_route_matches_callback_objective(ctx, pkg, line_search):
    """m = 40 > TAIL_MAXM: the unfused Gram route, whose trial points come from the streaming combine and get
    their w.w partials from a launch of their own."""
    check_trajectory(ctx, pkg, "mnist32", XENT, line_search, m=40, iters=15)


# ---------------------------------------------------------------------------------------------------------------
# 3. / 4. bitwise invariants with l2 > 0 on [784,32,10], N = 256, 40 iterations
# ---------------------------------------------------------------------------------------------------------------
SPEC_SEED = 7
SPEC_RATIO = 0.2


def spec_run(pkg, ctx, monkeypatch, depth, line_search, iters=40, chunks=1, fused=True, m=5):
    monkeypatch.setenv("LBF_SPEC_DEPTH", str(depth))
    monkeypatch.setenv("LBF_FUSED_TAIL", "1" if fused else "0")
    dims, acts, Xh, Yh, net, P, lam = setup(ctx, pkg, "mnist32", XENT, "cuda" if line_search == "armijo" else "cpu",
                                            SPEC_SEED, SPEC_RATIO)
    net.l2 = lam
    run = pkg.LbfgsRun(net, P, dev(Xh), dev(Yh), line_search=line_search, m=m, max_iters=iters, tol=0.0)
    for _ in range(chunks):
        run.iterate(iters // chunks)
    info = run.info
    h = run.hist.as_dict()
    run.close()
    return h, (info.iterations, info.n_evals, info.final_loss, info.final_grad_norm, info.n_loss_only), host(P)


def same(h, ref, keys=("loss", "grad_norm", "alpha", "ls_trials", "accepted")):
    return all(np.array_equal(h[k], ref[k]) for k in keys)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_speculative_line_search_is_exact(ctx, pkg, monkeypatch, line_search):
    """Depth 0 (host loop: every later trial a loss-only evaluation, then the gradient of the same point) against
    the unfused speculative route, bitwise. This is also the check that a loss-only trial's loss equals the fused
    evaluation's: every recorded loss of a host-finished iteration (ls_trials > 1) is equal between the routes."""
    ref, ref_info, ref_P = spec_run(pkg, ctx, monkeypatch, 0, line_search)
    assert np.any(ref["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    for depth in (1, 3, 8):
        h, info, P = spec_run(pkg, ctx, monkeypatch, depth, line_search, fused=False)
        assert same(h, ref), depth
        assert info == ref_info, (depth, info, ref_info)
        assert np.array_equal(P, ref_P)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_fused_tail_matches_host_loop(ctx, pkg, monkeypatch, line_search):
    ref, ref_info, ref_P = spec_run(pkg, ctx, monkeypatch, 0, line_search)
    assert np.any(ref["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    base, base_info, base_P = spec_run(pkg, ctx, monkeypatch, 1, line_search)
    for depth, chunks in [(3, 1), (8, 1), (3, 5)]:
        h, info, P = spec_run(pkg, ctx, monkeypatch, depth, line_search, chunks=chunks)
        assert same(h, base), (depth, chunks)
        assert info == base_info and np.array_equal(P, base_P)
    assert np.array_equal(base["ls_trials"], ref["ls_trials"])
    assert np.array_equal(base["accepted"], ref["accepted"])
    r = np.abs(base["loss"] - ref["loss"]) / np.abs(ref["loss"])
    print(f"l2 fused tail {line_search}: loss rel max {r.max():.2e}, n_loss_only {base_info[4]}")
    assert r.max() <= 1e-9, r


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_early_exit_is_exact(ctx, pkg, monkeypatch, line_search):
    """The first backward launch's Armijo test with the penalty from the trial point's w.w partials against
    LBF_NO_EARLY=1: the same records and parameters, bit for bit, and rejected first trials that ran their
    forward only."""
    runs = {}
    for off in (True, False):
        if off:
            monkeypatch.setenv("LBF_NO_EARLY", "1")
        else:
            monkeypatch.delenv("LBF_NO_EARLY", raising=False)
        runs[off] = spec_run(pkg, ctx, monkeypatch, 3, line_search)
    (h0, i0, p0), (h1, i1, p1) = runs[True], runs[False]
    print(f"l2 early {line_search}: n_evals {i0[1]} -> {i1[1]}, n_loss_only {i0[4]} -> {i1[4]}")
    assert np.any(h0["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    assert same(h1, h0) and np.array_equal(p0, p1)
    assert i1[4] > 0  # n_loss_only: at least one first trial rejected early
    assert i0[1] - i1[1] == i1[4] - i0[4] >= 0


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_two_runs_are_bitwise_equal(ctx, pkg, monkeypatch, line_search):
    """Determinism of the partials: no atomics, a fixed order, a count that depends on n only."""
    a = spec_run(pkg, ctx, monkeypatch, 3, line_search)
    b = spec_run(pkg, ctx, monkeypatch, 3, line_search)
    assert same(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------
# 5. data parallel: the penalty once, after the all-reduce
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_two_ranks_trajectory(ctx, pkg, line_search):
    dims, acts, N, world = [784, 64, 10], ["relu", "linear"], 2049, 2
    Xh, Yh = pkg.synth_mnist(N)
    net1 = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P0 = net1.init_params(7, "cpu")
    lam = pick_l2(dims, acts, P0, Xh, Yh, XENT)
    net1.l2 = lam
    P1 = P0.clone()
    h1, _ = pkg.lbfgs_solve(net1, P1, dev(Xh), dev(Yh), line_search=line_search, m=10, max_iters=10, tol=0.0)
    shards = [shard(N, world, r) for r in range(world)]
    Xs = [dev(Xh[lo:hi]) for lo, hi in shards]
    Ys = [dev(Yh[lo:hi]) for lo, hi in shards]

    def body(r, c):
        net = pkg.Mlp(c, dims, acts, loss=XENT, l2=lam)
        P = P0.clone()
        h, _ = pkg.lbfgs_solve(net, P, Xs[r], Ys[r], n_global=N, line_search=line_search, m=10, max_iters=10, tol=0.0)
        return h, P

    res = run_ranks(pkg, world, body)
    for h, P in res[1:]:
        assert same(h, res[0][0]) and torch.equal(P, res[0][1])
    h = res[0][0]
    dl = np.max(np.abs(h["loss"] - h1["loss"]) / np.abs(h1["loss"]))
    dp = rel(host(res[0][1]), host(P1))
    print(f"l2 2 ranks {line_search} l2={lam:g}: loss rel {dl:.2e}, params rel {dp:.2e}, trials {h['ls_trials']}")
    assert np.array_equal(h["ls_trials"], h1["ls_trials"]), (h["ls_trials"], h1["ls_trials"])
    assert np.array_equal(h["accepted"], h1["accepted"])
    assert dl <= 1e-5
    assert dp <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# 6. GD and SGD: a torch fp64 restatement of the two update rules (gd.cuh:38-106, sgd.cuh:50-153)
# ---------------------------------------------------------------------------------------------------------------
def torch_gd(f, P0, lr, momentum, iters):
    x, v, losses = P0.double().cpu().clone(), torch.zeros(P0.numel(), dtype=torch.float64), []
    _, g = value_grad(f, x)
    for _ in range(iters):
        if momentum > 0:
            v = momentum * v - lr * g
            x = x + v
        else:
            x = x - lr * g
        l, g = value_grad(f, x)
        losses.append(l)
    return x.numpy(), np.array(losses)


def torch_sgd(make_f, N, P0, lr, momentum, batch, epochs):
    """make_f(lo, hi): the objective over rows [lo, hi) with its own 1 / rows scale. Records the full objective at
    the start point and after every epoch."""
    x, v = P0.double().cpu().clone(), torch.zeros(P0.numel(), dtype=torch.float64)
    full = make_f(0, N)
    losses = [value_grad(full, x)[0]]
    for _ in range(epochs):
        for lo in range(0, N, batch):
            _, g = value_grad(make_f(lo, min(N, lo + batch)), x)
            if momentum > 0:
                v = momentum * v - lr * g
                x = x + v
            else:
                x = x - lr * g
        losses.append(value_grad(full, x)[0])
    return x.numpy(), np.array(losses)


@pytest.mark.parametrize("loss", [XENT, MSE])
def test_gd_and_sgd(ctx, pkg, loss):
    """The restatement is first checked against the engine at l2 = 0 (the route the oracle tests cover), then the
    engine against it with l2 > 0: 20 GD iterations; 3 SGD epochs of batch 32 on N = 100 (ragged last batch)."""
    dims, acts, Xh, Yh, net, P0, lam = setup(ctx, pkg, "tanh50", loss, "cuda")
    N = len(Xh)
    X, Y = dev(Xh), dev(Yh)
    Xt, Yt = torch.from_numpy(Xh).double(), torch.from_numpy(Yh).double()
    for l2 in (0.0, lam):
        net.l2 = l2
        P = P0.clone()
        hist, info = pkg.gd_solve(net, P, X, Y, lr=0.1, momentum=0.9, max_iters=20, tol=0.0)
        Pr, ref = torch_gd(objective(dims, acts, Xh, Yh, l2, loss), P0, 0.1, 0.9, 20)
        r, dp = np.abs(hist["loss"] - ref) / np.abs(ref), rel(host(P), Pr)
        print(f"l2 gd {loss} l2={l2:g}: loss rel max {r.max():.2e}, params rel {dp:.2e}")
        assert len(hist["loss"]) == 20 and r.max() <= 1e-3 and dp <= 1e-3
        f_end = value_grad(objective(dims, acts, Xh, Yh, l2, loss), P)
        assert abs(info.final_loss - f_end[0]) <= 1e-5 * abs(f_end[0])
        assert abs(info.final_grad_norm - float(f_end[1].norm())) <= 1e-4 * float(f_end[1].norm())

        def make_f(lo, hi, l2=l2):
            return ref_mlp.objective(dims, acts, loss, Xt[lo:hi], Yt[lo:hi], 1.0 / (hi - lo), l2)

        P = P0.clone()
        hist, _ = pkg.sgd_solve(net, P, X, Y, batch=32, lr=0.05, momentum=0.9, max_epochs=3, tol=0.0)
        Pr, ref = torch_sgd(make_f, N, P0, 0.05, 0.9, 32, 3)
        r, dp = np.abs(hist["loss"] - ref) / np.abs(ref), rel(host(P), Pr)
        print(f"l2 sgd {loss} l2={l2:g}: loss rel max {r.max():.2e}, params rel {dp:.2e}")
        assert len(hist["loss"]) == 4 and r.max() <= 1e-3 and dp <= 1e-3


# ---------------------------------------------------------------------------------------------------------------
# 7. errors and defaults
# ---------------------------------------------------------------------------------------------------------------
def test_errors_and_round_trip(ctx, pkg):
    L = pkg.lib()
    net = pkg.Mlp(ctx, [20, 8, 4], ["tanh", "linear"])
    assert net.l2 == 0.0
    for bad in (-1e-3, float("nan"), float("inf")):
        assert L.lbf_mlp_set_l2(net.h, bad) == 1  # LBF_ERR_INVALID
        assert "invalid argument" in L.lbf_last_error().decode()
        with pytest.raises(pkg.LbfError):
            net.l2 = bad
        with pytest.raises(pkg.LbfError):
            pkg.Mlp(ctx, [20, 8, 4], ["tanh", "linear"], l2=bad)
    assert net.l2 == 0.0
    net.l2 = 0.125
    assert net.l2 == 0.125
    assert pkg.Mlp(ctx, [20, 8, 4], ["tanh", "linear"], l2=3e-4).l2 == 3e-4


def test_explicit_zero_is_the_default(ctx, pkg):
    """l2 = 0 set explicitly: records and parameters bitwise those of a net that never called the setter."""
    dims, acts, Xh, Yh, _, P0, _ = setup(ctx, pkg, "mnist32", XENT)
    X, Y = dev(Xh), dev(Yh)
    keys = ("loss", "grad_norm", "alpha", "ls_trials", "accepted")
    solves = [lambda n, p: pkg.lbfgs_solve(n, p, X, Y, line_search="wolfe", m=5, max_iters=15, tol=0.0),
              lambda n, p: pkg.lbfgs_solve(n, p, X, Y, line_search="armijo", m=5, max_iters=15, tol=0.0),
              lambda n, p: pkg.gd_solve(n, p, X, Y, lr=0.1, momentum=0.9, max_iters=5, tol=0.0),
              lambda n, p: pkg.sgd_solve(n, p, X, Y, batch=64, lr=0.05, momentum=0.9, max_epochs=2, tol=0.0)]
    for solve in solves:
        out = []
        for explicit in (False, True):
            net = pkg.Mlp(ctx, dims, acts, loss=XENT)
            if explicit:
                net.l2 = 0.0
            P = P0.clone()
            h, _ = solve(net, P)
            out.append((h, P))
        assert same(out[0][0], out[1][0], keys) and torch.equal(out[0][1], out[1][1])


def test_slbfgs_ignores_net_l2(ctx, pkg):
    dims, acts = [784, 16, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(512)
    X, Y = dev(Xh), dev(Yh)
    kw = dict(M=5, L=4, b=32, b_H=16, step=0.02, tol=0.0, lam=1e-4, max_epochs=2)
    out = []
    for l2 in (0.0, 0.05):
        net = pkg.Mlp(ctx, dims, acts, loss=XENT, l2=l2)
        P = net.init_params(123, "cpu")
        h, _ = pkg.slbfgs_solve(net, P, X, Y, **kw)
        out.append((h["loss"], P))
    assert np.array_equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
