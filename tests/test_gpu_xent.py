"""Softmax cross-entropy loss (lbf_mlp_set_loss, LBF_LOSS_SOFTMAX_XENT) on every output-layer route, against
torch fp64 autograd on the CPU (the oracle has the squared error only):

    loss = inv_scale * sum_b sum_o y_bo (lse_b - z_bo) + 0.5 * l2 * ||w||^2,   lse = logsumexp of the logits z.

Bounds (the project's own): loss relative 1e-5 and gradient ||dg|| / ||g|| <= max(1e-4, 3 x the same torch
computation in fp32 against fp64) (test_gpu_parity.py); exact HVP 1e-4 (test_gpu_hvp.py); FD-HVP 2e-2 (fp32
differencing); 10-iteration L-BFGS trajectory loss relative 1e-3. Every test prints the deviation it measured.

Routes (Mlp::forward_phase; confirmed from a kernel trace of these shapes on 256 CUs):
  EPI_HEAD   last hidden width <= 128, unsplit forward GEMM: the head in that GEMM's epilogue
  head       last hidden width 129..256 (or a split forward at a batch the row head does not take): head_kernel
  rowhead    Out <= 16, H <= 256 and the last hidden forward split-K (small batches on a wide input layer)
  generic    Out > 16, H > 256 or a single layer: loss_xent on the stored logits
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev, host, run_ranks, shard
from ref_mlp import XENT, hess_ref, loss_grad, objective, one_hot, rel

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4
HVP_RTOL = 1e-4


def targets(rng, N, Out, soft):
    if soft:  # rows of rng.random, normalised
        Y = rng.random((N, Out))
        return (Y / Y.sum(1, keepdims=True)).astype(np.float32)
    return one_hot(rng, N, Out)


def check_loss_grad(ctx, pkg, dims, acts, X, Y, rows=None, l2=0.0, P=None, tag=""):
    """loss_grad of the cross-entropy net on rows `rows` of X / Y against torch fp64; returns the net and P."""
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    if P is None:
        P = net.init_params(123, "cpu")
    idx = None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda()
    sel = np.arange(X.shape[0]) if rows is None else rows
    B = len(sel)
    loss, g = net.loss_grad(P, dev(X), dev(Y), idx=idx, l2=l2)
    Ph = P.cpu().numpy()
    l_ref, g_ref = loss_grad(dims, acts, XENT, Ph, X[sel], Y[sel], 1.0 / B, l2)
    _, g32 = loss_grad(dims, acts, XENT, Ph, X[sel], Y[sel], 1.0 / B, l2, torch.float32)
    dl, dg, d32 = abs(loss - l_ref) / abs(l_ref), rel(host(g), g_ref), rel(g32, g_ref)
    print(f"xent {tag} {dims} B={B}: loss rel {dl:.2e}, grad rel {dg:.2e} (torch fp32: {d32:.2e})")
    assert np.isfinite(loss) and bool(torch.isfinite(g).all())
    assert dl <= LOSS_RTOL
    assert dg <= max(GRAD_RTOL, 3.0 * d32)
    return net, P


def problem(dims, N, soft, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    Y = targets(rng, N, dims[-1], soft)
    rows = np.sort(rng.permutation(N)[:max(1, N - N // 3)]) if soft else None  # soft: gathered rows, l2 = 1e-4
    return X, Y, rows, (1e-4 if soft else 0.0)


MODES = [False, True]
MODE_IDS = ["onehot", "soft_l2_gather"]

# EPI_HEAD (the 129-130-65-10 net: its 65-wide last hidden layer)
EPI_NETS = [([784, 128, 10], ["relu", "linear"]), ([784, 128, 64, 10], ["relu", "relu", "linear"]),
            ([37, 50, 3], ["tanh", "linear"]), ([129, 130, 65, 10], ["relu", "tanh", "linear"])]


@pytest.mark.parametrize("soft", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dims,acts", EPI_NETS)
@pytest.mark.parametrize("N", [1, 31, 257, 1000])
def test_loss_grad_epi_head(ctx, pkg, dims, acts, N, soft):
    X, Y, rows, l2 = problem(dims, N, soft, seed=N)
    check_loss_grad(ctx, pkg, dims, acts, X, Y, rows, l2, tag="epi_head")


# standalone head_kernel: H = 132 / 256 staged through registers, 255 on the scalar path; 48-255-16: all 16
# output lanes live
@pytest.mark.parametrize("soft", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("H,Out,N", [(H, 10, N) for H in (132, 255, 256) for N in (1, 63, 256)] + [(255, 16, 63)] +
                         [(256, 10, 4200)])  # more than 64 tiles: one workgroup per tile, no split of H
def test_loss_grad_standalone_head(ctx, pkg, H, Out, N, soft):
    dims, acts = [48, H, Out], ["relu", "linear"]
    X, Y, rows, l2 = problem(dims, N, soft, seed=H + N)
    check_loss_grad(ctx, pkg, dims, acts, X, Y, rows, l2, tag="head")


# generic route (loss_xent): Out > 16, H > 256, a single layer; 32-40-130: Out beyond two wavefronts
GEN_NETS = [([784, 300, 20], ["relu", "linear"]), ([16, 300, 4], ["tanh", "linear"]), ([50, 7], ["linear"]),
            ([32, 40, 130], ["tanh", "linear"])]


@pytest.mark.parametrize("soft", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("dims,acts", GEN_NETS)
@pytest.mark.parametrize("N", [1, 31, 257])
def test_loss_grad_generic(ctx, pkg, dims, acts, N, soft):
    X, Y, rows, l2 = problem(dims, N, soft, seed=N + 5)
    check_loss_grad(ctx, pkg, dims, acts, X, Y, rows, l2, tag="generic")


def test_loss_grad_rowhead(ctx, pkg):
    """The S-LBFGS minibatch shape: 245 gathered rows of 1000 on 784-512-256-10, whose last hidden forward is
    split-K, so the row head finishes it (rowhead_kernel)."""
    dims, acts = [784, 512, 256, 10], ["tanh", "tanh", "linear"]
    rng = np.random.default_rng(11)
    X = rng.standard_normal((1000, 784)).astype(np.float32)
    Y = targets(rng, 1000, 10, False)
    rows = rng.permutation(1000)[:245]
    check_loss_grad(ctx, pkg, dims, acts, X, Y, rows, 1e-4, tag="rowhead")


@pytest.mark.parametrize("N", [8192, 8200, 60000])
def test_loss_grad_gemm_tiles(ctx, pkg, N):
    """The 32-, 64- and 128-row forward tiles with the fused head (Mlp::plan: 32 x 128 at 8192 rows, 64 x 128 at
    8200, 128 x 128 at 60000 on 256 CUs)."""
    dims, acts = [784, 128, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(N, 784, 10, 7)
    check_loss_grad(ctx, pkg, dims, acts, Xh, Yh, tag="tile")


def test_saturated_logits(ctx, pkg):
    """Output weights x 1e3: logits in the hundreds; the loss and gradient stay finite and within the bounds."""
    dims, acts = [784, 128, 10], ["relu", "linear"]
    X, Y, _, _ = problem(dims, 257, False, seed=3)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    off = (784 + 1) * 128
    P[off:off + 128 * 10] *= 1e3
    z = net.forward(P, dev(X))
    assert float(z.abs().max()) > 100.0
    check_loss_grad(ctx, pkg, dims, acts, X, Y, P=P, tag="saturated")


@pytest.mark.parametrize("dims,acts", [EPI_NETS[0], ([48, 255, 10], ["relu", "linear"]), GEN_NETS[0]])
@pytest.mark.parametrize("N", [257, 20000])
def test_loss_only_bitwise_and_deterministic(ctx, pkg, dims, acts, N):
    X, Y, _, _ = problem(dims, N, False, seed=7)
    Xd, Yd = dev(X), dev(Y)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    lf = net.loss(P, Xd, Yd)
    l1, g1 = net.loss_grad(P, Xd, Yd)
    l2, g2 = net.loss_grad(P, Xd, Yd)
    assert lf == l1 == l2 and torch.equal(g1, g2)


HVP_NETS = [([20, 16, 3], ["tanh", "linear"]), ([30, 24, 12, 4], ["sigmoid", "relu", "linear"]),
            ([784, 128, 10], ["relu", "linear"]), ([4, 6, 12], ["tanh", "linear"]), ([784, 300, 20], ["relu", "linear"])]


@pytest.mark.parametrize("dims,acts", HVP_NETS)
@pytest.mark.parametrize("lam,gather", [(0.0, False), (1e-4, True)])
def test_hvp_matches_torch_fp64(ctx, pkg, dims, acts, lam, gather):
    rng = np.random.default_rng(len(dims) * 7 + dims[0])
    N = 37
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    # one-hot rows, or (gathered case) unnormalised non-negative rows: Ysum differs from row to row
    Y = rng.random((N, dims[-1])).astype(np.float32) if gather else targets(rng, N, dims[-1], False)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    v = torch.from_numpy(rng.standard_normal(net.nparams).astype(np.float32)).cuda()
    idx, rows = None, np.arange(N)
    if gather:
        rows = rng.permutation(N)[:23]
        idx = torch.from_numpy(rows.astype(np.int32)).cuda()
    B = len(rows)
    hv = net.hvp(P, v, dev(X), dev(Y), idx=idx, inv_scale=1.0 / B, l2=lam)
    ref = hess_ref(dims, acts, XENT, P.double().cpu(), v.double().cpu(), torch.from_numpy(X[rows]).double(),
                   torch.from_numpy(Y[rows]).double(), 1.0 / B, lam)
    err = float((hv.double().cpu() - ref).norm() / ref.norm())
    print(f"xent hvp {dims} lam={lam} gather={gather}: rel {err:.2e}")
    assert err <= HVP_RTOL


def test_hvp_linear_in_v_and_symmetric(ctx, pkg):
    dims, acts = [784, 128, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(4096)
    X, Y = dev(Xh), dev(Yh)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn(net.nparams, device="cuda", generator=g)
    w = torch.randn(net.nparams, device="cuda", generator=g)
    Hu = net.hvp(P, u, X, Y).double()
    Hw = net.hvp(P, w, X, Y).double()
    Hc = net.hvp(P, 2.0 * u - 0.5 * w, X, Y).double()
    lin = float((Hc - (2.0 * Hu - 0.5 * Hw)).norm() / Hc.norm())
    a, b = float(w.double() @ Hu), float(u.double() @ Hw)
    print(f"xent hvp linearity {lin:.2e}, symmetry {abs(a - b) / max(abs(a), abs(b)):.2e}")
    assert lin <= 1e-5
    assert abs(a - b) <= 1e-4 * max(abs(a), abs(b))


def test_fd_hvp_matches_torch_central_difference(ctx, pkg):
    """lbf_mlp_fd_hvp on a tanh net (no kinks) against the fp64 central difference at the same eps."""
    dims, acts = [20, 16, 3], ["tanh", "linear"]
    rng = np.random.default_rng(9)
    N, eps = 37, 1e-3
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    Y = targets(rng, N, dims[-1], True)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    v = torch.from_numpy(rng.standard_normal(net.nparams).astype(np.float32)).cuda()
    y_fd = host(net.fd_hvp(P, v, dev(X), dev(Y), inv_scale=1.0 / N, l2=1e-4, eps=eps))
    Ph, vh = host(P), host(v)
    _, gp = loss_grad(dims, acts, XENT, Ph + eps * vh, X, Y, 1.0 / N, 1e-4)
    _, gm = loss_grad(dims, acts, XENT, Ph - eps * vh, X, Y, 1.0 / N, 1e-4)
    err = rel(y_fd, (gp - gm) / (2 * eps))
    print(f"xent fd-hvp: rel {err:.2e}")
    assert err <= 2e-2


LBFGS_CASES = {"mnist32": ([784, 32, 10], ["relu", "linear"], 256), "tanh50": ([37, 50, 3], ["tanh", "linear"], 100)}


@pytest.mark.parametrize("case", sorted(LBFGS_CASES))
@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_lbfgs_matches_callback_objective(ctx, pkg, case, line_search):
    """The fused L-BFGS with the new loss against the engine's L-BFGS on a callback that evaluates the torch fp64
    cross-entropy on the CPU (lbf_lbfgs_solve_fn: the same, already verified solver on an objective that does not
    run the new kernels)."""
    dims, acts, N = LBFGS_CASES[case]
    if case == "mnist32":
        Xh, Yh = pkg.synth_mnist(N)
    else:
        Xh, Yh, _, _ = problem(dims, N, False, seed=1)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    Pf = P.clone()
    hist, _ = pkg.lbfgs_solve(net, P, dev(Xh), dev(Yh), line_search=line_search, m=5, max_iters=10, tol=0.0)
    f = objective(dims, acts, XENT, torch.from_numpy(Xh).double(), torch.from_numpy(Yh).double(), 1.0 / N, 0.0)

    def fn(p, g):
        p64 = p.double().cpu().requires_grad_(True)
        l = f(p64)
        (gr,) = torch.autograd.grad(l, p64)
        g.copy_(gr.float())
        return float(l.detach())

    ref, _ = pkg.lbfgs_solve_fn(ctx, Pf, fn, line_search=line_search, m=5, max_iters=10, tol=0.0)
    assert len(hist["loss"]) == len(ref["loss"]) == 10
    r = np.abs(hist["loss"] - ref["loss"]) / np.abs(ref["loss"])
    print(f"xent lbfgs {case} {line_search}: loss rel max {r.max():.2e}; trials {hist['ls_trials']} / {ref['ls_trials']}")
    assert r.max() <= 1e-3, r
    assert np.all(np.diff(hist["loss"]) <= 0)


SPEC_SEED = 7


def _spec_run(pkg, ctx, monkeypatch, depth, line_search, iters, chunks=1, fused=True, m=5):
    monkeypatch.setenv("LBF_SPEC_DEPTH", str(depth))
    monkeypatch.setenv("LBF_FUSED_TAIL", "1" if fused else "0")
    dims, acts = [784, 32, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(256)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(SPEC_SEED, "cuda" if line_search == "armijo" else "cpu")
    run = pkg.LbfgsRun(net, P, dev(Xh), dev(Yh), line_search=line_search, m=m, max_iters=iters, tol=0.0)
    for c in range(chunks):
        run.iterate(iters // chunks)
    info = run.info
    h = run.hist.as_dict()
    run.close()
    return h, (info.iterations, info.n_evals, info.final_loss, info.final_grad_norm, info.n_loss_only), host(P)


def _same(h, ref, keys=("loss", "grad_norm", "alpha", "ls_trials", "accepted")):
    return all(np.array_equal(h[k], ref[k]) for k in keys)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_speculative_line_search_is_exact(ctx, pkg, monkeypatch, line_search):
    ref, ref_info, ref_P = _spec_run(pkg, ctx, monkeypatch, 0, line_search, 40)
    assert np.any(ref["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    for depth in (1, 3, 8):
        h, info, P = _spec_run(pkg, ctx, monkeypatch, depth, line_search, 40, fused=False)
        assert _same(h, ref), depth
        assert info == ref_info, (depth, info, ref_info)
        assert np.array_equal(P, ref_P)


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_fused_tail_matches_host_loop(ctx, pkg, monkeypatch, line_search):
    # 40 iterations: this problem's Wolfe run rejects no first trial in its first 30
    ref, ref_info, ref_P = _spec_run(pkg, ctx, monkeypatch, 0, line_search, 40)
    assert np.any(ref["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    base, base_info, base_P = _spec_run(pkg, ctx, monkeypatch, 1, line_search, 40)
    for depth, chunks in [(3, 1), (8, 1), (3, 5)]:
        h, info, P = _spec_run(pkg, ctx, monkeypatch, depth, line_search, 40, chunks)
        assert _same(h, base), (depth, chunks)
        assert info == base_info and np.array_equal(P, base_P)
    assert np.array_equal(base["ls_trials"], ref["ls_trials"])
    assert np.array_equal(base["accepted"], ref["accepted"])
    assert base_info[0] == ref_info[0] and base_info[1] + base_info[4] == ref_info[1] + ref_info[4]
    r = np.abs(base["loss"] - ref["loss"]) / np.abs(ref["loss"])
    print(f"xent fused tail {line_search}: loss rel max {r.max():.2e}")
    assert r.max() <= 1e-9, r


def test_armijo_early_exit_is_exact(ctx, pkg, monkeypatch):
    """The first backward launch's Armijo test on the forward's loss partials (EarlyLs) against LBF_NO_EARLY=1:
    the same records and parameters, bit for bit, and rejected first trials that ran their forward only."""
    runs = {}
    for off in (True, False):
        if off:
            monkeypatch.setenv("LBF_NO_EARLY", "1")
        else:
            monkeypatch.delenv("LBF_NO_EARLY", raising=False)
        runs[off] = _spec_run(pkg, ctx, monkeypatch, 3, "armijo", 40)
    (h0, i0, p0), (h1, i1, p1) = runs[True], runs[False]
    assert np.any(h0["ls_trials"][1:] > 1), "problem must exercise rejected first trials"
    assert _same(h1, h0) and np.array_equal(p0, p1)
    assert i1[4] > 0  # n_loss_only
    assert i0[1] - i1[1] == i1[4] - i0[4] >= 0


def test_shard_sum_equals_full_batch(ctx, pkg):
    dims, acts = [784, 128, 10], ["relu", "linear"]
    N = 4096
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = dev(Xh), dev(Yh)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    lf, gf = net.loss_grad(P, X, Y)
    gs = torch.zeros_like(gf, dtype=torch.float64)
    ls = 0.0
    for r in range(8):
        lo, hi = N * r // 8, N * (r + 1) // 8
        l, g = net.loss_grad(P, X[lo:hi].contiguous(), Y[lo:hi].contiguous(), inv_scale=1.0 / N)
        gs += g.double()
        ls += l
    print(f"xent shards: loss rel {abs(ls - lf) / abs(lf):.2e}, grad rel {rel(gs.cpu().numpy(), host(gf)):.2e}")
    assert abs(ls - lf) <= 1e-6 * abs(lf)
    assert rel(gs.cpu().numpy(), host(gf)) <= 1e-5


def test_two_ranks_loss_grad_equals_single(ctx, pkg):
    dims, acts, N, world = [784, 128, 10], ["relu", "linear"], 4096, 2
    Xh, Yh = pkg.synth_mnist(N)
    net1 = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net1.init_params(123, "cpu")
    l1, g1 = net1.loss_grad(P, dev(Xh), dev(Yh), inv_scale=1.0 / N)
    shards = [shard(N, world, r) for r in range(world)]
    Xs = [dev(Xh[lo:hi]) for lo, hi in shards]
    Ys = [dev(Yh[lo:hi]) for lo, hi in shards]

    def body(r, c):
        net = pkg.Mlp(c, dims, acts, loss=XENT)
        return net.loss_grad(P, Xs[r], Ys[r], inv_scale=1.0 / N)

    res = run_ranks(pkg, world, body)
    for lr, gr in res:
        assert lr == res[0][0] and torch.equal(gr, res[0][1])  # replicated, bitwise
    print(f"xent 2 ranks: loss rel {abs(res[0][0] - l1) / abs(l1):.2e}, grad rel {rel(host(res[0][1]), host(g1)):.2e}")
    assert abs(res[0][0] - l1) <= 1e-6 * abs(l1)
    assert rel(host(res[0][1]), host(g1)) <= 1e-5


def test_batch_grads_match_per_minibatch_loss_grad(ctx, pkg):
    """lbf_mlp_batch_grads (S-LBFGS's anchor gradients; the generic output route on every net) against one
    loss_grad per minibatch: the same sums in another order, so fp32 rounding apart."""
    dims, acts = [784, 64, 10], ["relu", "linear"]
    nmb, cnt = 4, 64
    Xh, Yh = pkg.synth_mnist(nmb * cnt)
    X, Y = dev(Xh), dev(Yh)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    G = net.batch_grads(P, X, Y, nmb, l2=1e-4)
    worst = 0.0
    for t in range(nmb):
        _, g = net.loss_grad(P, X[t * cnt:(t + 1) * cnt].contiguous(), Y[t * cnt:(t + 1) * cnt].contiguous(), l2=1e-4)
        ref = host(g)
        worst = max(worst, np.abs(host(G[t]) - ref).max() / np.abs(ref).max())
    print(f"xent batch_grads vs loss_grad: max |diff| / max |g| {worst:.2e}")
    assert worst <= 1e-5  # test_gpu_dp.py::test_batch_grads_equal_per_minibatch_loss_grad's bound


def _objective_at(dims, acts, P, Xh, Yh, lam, loss):
    """The torch fp64 objective at P, without and with the 0.5 lam ||w||^2 term."""
    X, Y = torch.from_numpy(Xh).double(), torch.from_numpy(Yh).double()
    p = P.double().cpu()
    return [float(objective(dims, acts, loss, X, Y, 1.0 / len(Xh), l)(p)) for l in (0.0, lam)]


def _form(value, forms):
    """Which of the two forms a recorded loss equals to 1e-5 (None: neither)."""
    hit = [k for k, f in enumerate(forms) if abs(value - f) <= 1e-5 * abs(f)]
    return hit[0] if hit else None


def test_slbfgs_is_plumbed(ctx, pkg):
    """S-LBFGS minimises the chosen loss: finite and descending over 3 epochs, and a recorded loss is the torch
    objective at the parameters it was recorded at. S-LBFGS records after each epoch (at the new anchor, the
    parameters a one-epoch solve returns), so the check runs one epoch; the squared error runs the same check
    and fixes the form (with or without the lambda term) the record has."""
    dims, acts = [784, 16, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(512)
    X, Y = dev(Xh), dev(Yh)
    kw = dict(M=5, L=4, b=32, b_H=16, step=0.02, tol=0.0, lam=1e-4)
    form = {}
    for loss in ("mse", XENT):
        net = pkg.Mlp(ctx, dims, acts, loss=loss)
        P = net.init_params(123, "cpu")
        hist, _ = pkg.slbfgs_solve(net, P, X, Y, max_epochs=1, **kw)
        forms = _objective_at(dims, acts, P, Xh, Yh, 1e-4, loss)
        form[loss] = _form(hist["loss"][0], forms)
        print(f"slbfgs {loss}: recorded {hist['loss'][0]:.9g}, torch {forms}")
        assert form[loss] is not None
    assert form[XENT] == form["mse"]
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    l0 = net.loss(P, X, Y)
    hist, _ = pkg.slbfgs_solve(net, P, X, Y, max_epochs=3, **kw)
    print(f"slbfgs {XENT}: start {l0:.6g}, epochs {hist['loss']}")
    # below the start point after the first epoch too: the solver's own evaluations (its twin networks on the
    # second stream included) must minimise the chosen loss, not the default one
    assert np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0] < l0


def test_slbfgs_exact_hvp_option(ctx, pkg):
    dims, acts = [784, 16, 10], ["tanh", "linear"]
    Xh, Yh = pkg.synth_mnist(512)
    X, Y = dev(Xh), dev(Yh)
    kw = dict(M=5, L=4, b=32, b_H=16, step=0.02, max_epochs=3, tol=0.0, lam=1e-4)
    res = {}
    for exact in (0, 1):
        net = pkg.Mlp(ctx, dims, acts, loss=XENT)
        P = net.init_params(123, "cpu")
        res[exact], _ = pkg.slbfgs_solve(net, P, X, Y, hvp_exact=exact, **kw)
    for h in res.values():
        assert np.all(np.isfinite(h["loss"])) and h["loss"][-1] < h["loss"][0]
    assert np.array_equal(res[0]["accepted"], res[1]["accepted"])
    r = np.abs(res[1]["loss"] - res[0]["loss"]) / np.abs(res[0]["loss"])
    print(f"xent slbfgs exact vs fd hvp: loss rel max {r.max():.2e}")
    assert r.max() <= 5e-2, r


def test_gd_and_sgd_are_plumbed(ctx, pkg):
    """GD records after each step and SGD records the start point first: the first record is the torch objective
    at the start point (SGD) or at the parameters a one-step run returns (GD), in the form the squared error
    records; 20 iterations / 3 epochs descend."""
    dims, acts = [784, 32, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(256)
    X, Y = dev(Xh), dev(Yh)
    for loss in ("mse", XENT):
        net = pkg.Mlp(ctx, dims, acts, loss=loss)
        P = net.init_params(123, "cuda")
        hist, _ = pkg.gd_solve(net, P, X, Y, lr=0.1, momentum=0.9, max_iters=1, tol=0.0)
        f = _objective_at(dims, acts, P, Xh, Yh, 0.0, loss)[0]
        print(f"gd {loss}: recorded {hist['loss'][0]:.9g}, torch {f:.9g}")
        assert abs(hist["loss"][0] - f) <= 1e-5 * abs(f)
        P = net.init_params(123, "cuda")
        f = _objective_at(dims, acts, P, Xh, Yh, 0.0, loss)[0]
        hist, _ = pkg.sgd_solve(net, P, X, Y, batch=64, lr=0.05, momentum=0.9, max_epochs=3, tol=0.0)
        print(f"sgd {loss}: recorded {hist['loss'][0]:.9g}, torch {f:.9g}")
        assert abs(hist["loss"][0] - f) <= 1e-5 * abs(f)
        assert np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cuda")
    hist, _ = pkg.gd_solve(net, P, X, Y, lr=0.1, momentum=0.9, max_iters=20, tol=0.0)
    assert len(hist["loss"]) == 20 and np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]


def test_errors_and_default(ctx, pkg):
    L = pkg.lib()
    for dims, acts in [([20, 8, 4], ["tanh", "sigmoid"]), ([20, 8, 1], ["tanh", "linear"])]:
        net = pkg.Mlp(ctx, dims, acts)
        assert L.lbf_mlp_set_loss(net.h, 1) == 1  # LBF_ERR_INVALID
        assert "invalid argument" in L.lbf_last_error().decode()
        assert net.loss_name == "mse"
        with pytest.raises(pkg.LbfError):
            pkg.Mlp(ctx, dims, acts, loss=XENT)
    assert L.lbf_mlp_set_loss(net.h, 2) == 1
    dims, acts = [784, 128, 10], ["relu", "linear"]
    X, Y, _, _ = problem(dims, 257, False, seed=2)
    plain = pkg.Mlp(ctx, dims, acts)
    P = plain.init_params(123, "cpu")
    l0, g0 = plain.loss_grad(P, dev(X), dev(Y))
    net = pkg.Mlp(ctx, dims, acts)
    assert net.loss_name == "mse"
    net.loss_name = XENT
    assert net.loss_name == XENT
    lx, _ = net.loss_grad(P, dev(X), dev(Y))
    assert lx != l0
    net.loss_name = "mse"  # takes effect from the next evaluation
    l1, g1 = net.loss_grad(P, dev(X), dev(Y))
    assert l1 == l0 and torch.equal(g1, g0)
