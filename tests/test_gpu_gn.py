"""Gauss-Newton vector product (Mlp.gnvp / lbf_mlp_gnvp, lbfgs-ffnn_amd/csrc/hvp.hip) and the
S-LBFGS curvature pairs formed with it (hvp_exact = 2).

G = J^T H_L J with the loss split from the network at the post-activation outputs A_L for the squared error
(H_L = inv_scale I) and at the logits for the cross-entropy (H_L = inv_scale Ysum (diag p - p p^T)). The
reference is torch fp64 on the CPU: J v by torch.func.jvp of the network output, H_L in closed form, J^T(.) by
torch.func.vjp, l2 v added at the end; no Jacobian is built.

Bounds: ||Gv - ref|| <= 1e-4 ||ref|| (the project's HVP bound: the same fp32 products against an fp64
reference); linearity 1e-5 and symmetry 1e-4 (test_hvp_linear_in_v_and_symmetric's); shard sums 1e-5; where
G = H, 1e-5 against the engine's own exact product (both from the same fp32 products).
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev
from ref_mlp import XENT, gap, gn_ref, hess_ref, one_hot, rel

pytestmark = pytest.mark.gpu

GN_RTOL = 1e-4
NETS = [
    ([20, 16, 3], ["tanh", "linear"]),
    ([30, 24, 12, 4], ["sigmoid", "relu", "linear"]),
    ([784, 128, 10], ["relu", "linear"]),
    ([64, 96, 33, 1], ["sigmoid", "tanh", "linear"]),
    ([40, 8], ["tanh"]),
    ([4, 6, 12], ["tanh", "linear"]),
    ([10, 5, 20], ["relu", "sigmoid"]),
]
# linear last layer and Out >= 2: those of NETS, and test_gpu_xent.py's fifth (an output wider than 16)
XENT_NETS = [(d, a) for d, a in NETS if a[-1] == "linear" and d[-1] >= 2] + [([784, 300, 20], ["relu", "linear"])]


def case_data(pkg, dims, acts, loss, gather, N=37):
    """Host inputs of one case: (P, X, Y, v, rows). The start point is the engine's seed-123 CPU-stream init
    (Mlp.init_params(123, "cpu")), at which G v and H v differ by 0.45 .. 1.03 of ||H v|| on every case."""
    rng = np.random.default_rng(len(dims) * 7 + dims[0])
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    if loss == XENT:  # one-hot rows, or (gathered case) unnormalised non-negative rows: Ysum varies
        Y = rng.random((N, dims[-1])).astype(np.float32) if gather else one_hot(rng, N, dims[-1])
    else:
        Y = rng.standard_normal((N, dims[-1])).astype(np.float32)
    P = pkg.init_params_host(dims, acts, 123, "cpu")
    v = rng.standard_normal(P.size).astype(np.float32)
    rows = rng.permutation(N)[:23] if gather else np.arange(N)
    return P, X, Y, v, rows


def references(dims, acts, loss, P, X, Y, v, rows, lam):
    B = len(rows)
    a = [torch.from_numpy(np.asarray(t)).double() for t in (P, v, X[rows], Y[rows])]
    return (gn_ref(dims, acts, loss, a[0], a[1], a[2], a[3], 1.0 / B, lam),
            hess_ref(dims, acts, loss, a[0], a[1], a[2], a[3], 1.0 / B, lam))


CASES = [("mse", d, a) for d, a in NETS] + [(XENT, d, a) for d, a in XENT_NETS]


@pytest.mark.parametrize("loss,dims,acts", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in CASES])
@pytest.mark.parametrize("lam,gather", [(0.0, False), (1e-4, True)])
def test_gnvp_matches_torch_fp64(ctx, pkg, loss, dims, acts, lam, gather):
    P, X, Y, v, rows = case_data(pkg, dims, acts, loss, gather)
    G, H = references(dims, acts, loss, P, X, Y, v, rows, lam)
    # agreement with G_ref cannot be had by calling the exact product (0.45 .. 1.03 over these cases)
    assert gap(G, H) >= 0.1, gap(G, H)
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    idx = torch.from_numpy(rows.astype(np.int32)).cuda() if gather else None
    gv = net.gnvp(dev(P), dev(v), dev(X), dev(Y), idx=idx, inv_scale=1.0 / len(rows), l2=lam)
    err = rel(gv, G)
    print(f"gnvp {loss} {dims} lam={lam} gather={gather}: rel {err:.2e}, |G-H|/|H| {gap(G, H):.2f}")
    assert err <= GN_RTOL


@pytest.mark.parametrize("loss", ["mse", XENT])
def test_gnvp_wide_split_k_route(ctx, pkg, loss):
    """cfg 4's Hessian-batch shape: 128 gathered rows through 784-512-256-10 tanh, whose forward is split-K."""
    dims, acts = [784, 512, 256, 10], ["tanh", "tanh", "linear"]
    Xh, Yh = pkg.synth_mnist(1000)
    rng = np.random.default_rng(4)
    rows = rng.permutation(1000)[:128]
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    v = rng.standard_normal(net.nparams).astype(np.float32)
    gv = net.gnvp(P, dev(v), dev(Xh), dev(Yh), idx=torch.from_numpy(rows.astype(np.int32)).cuda(), inv_scale=1.0 / 128,
                  l2=1e-4)
    a = [t.double() for t in (P.cpu(), torch.from_numpy(v), torch.from_numpy(Xh[rows]), torch.from_numpy(Yh[rows]))]
    ref = gn_ref(dims, acts, loss, a[0], a[1], a[2], a[3], 1.0 / 128, 1e-4)
    err = rel(gv, ref)
    print(f"gnvp wide {loss}: rel {err:.2e}")
    assert err <= GN_RTOL


@pytest.mark.parametrize("loss,dims,acts,zero_residual", [
    ("mse", [40, 8], ["linear"], False),
    (XENT, [50, 7], ["linear"], False),
    ("mse", [30, 24, 12, 4], ["sigmoid", "relu", "linear"], True),
    ("mse", [64, 96, 33, 1], ["sigmoid", "tanh", "linear"], True),
])
def test_gnvp_equals_hvp_where_g_is_h(ctx, pkg, loss, dims, acts, zero_residual):
    """A single linear layer has no second-order network term, and at zero residual every dropped term is a
    multiple of a residual that is zero (or zero to fp32 rounding): there G = H, checked against the engine's own
    exact product."""
    rng = np.random.default_rng(11 + dims[0])
    N = 37
    X = dev(rng.standard_normal((N, dims[0])))
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    if zero_residual:
        Y = net.forward(P, X)
    else:
        Y = dev(one_hot(rng, N, dims[-1]) if loss == XENT else rng.standard_normal((N, dims[-1])))
    v = dev(rng.standard_normal(net.nparams))
    hv = net.hvp(P, v, X, Y, l2=1e-4).clone()
    gv = net.gnvp(P, v, X, Y, l2=1e-4)
    err = rel(gv, hv)
    print(f"gnvp vs hvp {loss} {dims} zero_residual={zero_residual}: rel {err:.2e}")
    assert err <= 1e-5


@pytest.fixture(scope="module")
def mnist4096(pkg):
    Xh, Yh = pkg.synth_mnist(4096)
    return dev(Xh), dev(Yh)


@pytest.mark.parametrize("loss", ["mse", XENT])
def test_gnvp_linear_symmetric_positive(ctx, pkg, mnist4096, loss):
    dims, acts = [784, 128, 10], ["relu", "linear"]
    X, Y = mnist4096
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    g = torch.Generator(device="cuda").manual_seed(1)
    u = torch.randn(net.nparams, device="cuda", generator=g)
    w = torch.randn(net.nparams, device="cuda", generator=g)
    Gu = net.gnvp(P, u, X, Y).double()
    Gw = net.gnvp(P, w, X, Y).double()
    Gc = net.gnvp(P, 2.0 * u - 0.5 * w, X, Y).double()
    lin = float((Gc - (2.0 * Gu - 0.5 * Gw)).norm() / Gc.norm())
    a, b = float(w.double() @ Gu), float(u.double() @ Gw)
    print(f"gnvp {loss} linearity {lin:.2e}, symmetry {abs(a - b) / max(abs(a), abs(b)):.2e}")
    assert lin <= 1e-5
    assert abs(a - b) <= 1e-4 * max(abs(a), abs(b))
    for x, Gx in ((u, Gu), (w, Gw), (2.0 * u - 0.5 * w, Gc)):  # l2 = 0: the data term alone
        q = float(x.double() @ Gx)
        print(f"gnvp {loss} v.Gv {q:.4e}")
        assert q > 0.0


def test_gnvp_shard_sum_equals_full_batch(ctx, pkg, mnist4096):
    dims, acts = [784, 128, 10], ["relu", "linear"]
    X, Y = mnist4096
    N = X.shape[0]
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    v = torch.randn(net.nparams, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    full = net.gnvp(P, v, X, Y, inv_scale=1.0 / N).double()
    acc = torch.zeros_like(full)
    for r in range(8):
        lo, hi = N * r // 8, N * (r + 1) // 8
        acc += net.gnvp(P, v, X[lo:hi], Y[lo:hi], inv_scale=1.0 / N).double()
    err = float((acc - full).norm() / full.norm())
    print(f"gnvp 8 shards vs full batch: rel {err:.2e}")
    assert err <= 1e-5


def test_gnvp_dp_route_equals_single(ctx, pkg):
    dims, acts = [30, 24, 12, 4], ["sigmoid", "relu", "linear"]
    rng = np.random.default_rng(3)
    X = dev(rng.standard_normal((64, 30)))
    Y = dev(rng.standard_normal((64, 4)))
    c = pkg.Context(0)
    c.comm_init(1, 0, pkg.Context.unique_id())
    out = []
    for cc in (ctx, c):
        net = pkg.Mlp(cc, dims, acts)
        P = net.init_params(5, "cpu")
        v = torch.ones(net.nparams, device="cuda")
        out.append(net.gnvp(P, v, X, Y, l2=1e-4).clone())
    assert torch.equal(out[0], out[1])


def test_gnvp_empty_batch(ctx, pkg):
    """An empty share of the Hessian batch: G v is then the L2 term l2 v, not an error."""
    dims, acts = [30, 24, 4], ["tanh", "linear"]
    X = torch.zeros((1, 30), device="cuda")
    Y = torch.zeros((1, 4), device="cuda")
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(5, "cpu")
    v = torch.randn(net.nparams, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    idx = torch.zeros(0, dtype=torch.int32, device="cuda")
    gv = net.gnvp(P, v, X, Y, idx=idx, inv_scale=1.0, l2=1e-4)
    ref = (1e-4 * v.double()).float()
    assert torch.allclose(gv, ref, rtol=1e-6, atol=0)


def test_gnvp_shares_hvp_workspace(ctx, pkg):
    """gnvp and hvp on one network with growing and shrinking batches: each result is a fresh network's, bitwise
    (the shared R-pass workspace carries nothing from call to call)."""
    dims, acts = [30, 24, 12, 4], ["sigmoid", "relu", "linear"]
    rng = np.random.default_rng(8)
    X, Y = dev(rng.standard_normal((37, 30))), dev(rng.standard_normal((37, 4)))
    idx23 = torch.from_numpy(rng.permutation(37)[:23].astype(np.int32)).cuda()
    idx5 = torch.from_numpy(rng.permutation(37)[:5].astype(np.int32)).cuda()
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    v = dev(rng.standard_normal(net.nparams))
    for fn, idx in (("gnvp", idx23), ("hvp", None), ("gnvp", None), ("gnvp", idx5)):
        got = getattr(net, fn)(P, v, X, Y, idx=idx, l2=1e-4).clone()
        fresh = getattr(pkg.Mlp(ctx, dims, acts), fn)(P, v, X, Y, idx=idx, l2=1e-4)
        assert torch.equal(got, fresh), (fn, None if idx is None else idx.numel())


def test_gnvp_unaligned_pointers(ctx, pkg):
    """params, v and out each one float past a 16-byte boundary (4-byte alignment is the contract). Of the two
    outcomes allowed for (bitwise, or 1e-6 where the unaligned GEMM route sums in another order) the bitwise one
    holds at this shape: the GEMMs' unaligned operand route changes how a tile is loaded, not its summation."""
    dims, acts = [30, 24, 12, 4], ["sigmoid", "relu", "linear"]
    rng = np.random.default_rng(9)
    X, Y = dev(rng.standard_normal((37, 30))), dev(rng.standard_normal((37, 4)))
    net = pkg.Mlp(ctx, dims, acts)
    n = net.nparams
    P = net.init_params(123, "cpu")
    v = dev(rng.standard_normal(n))
    aligned = net.gnvp(P, v, X, Y, l2=1e-4).clone()
    bufs = [torch.full((n + 8,), 7.0, device="cuda") for _ in range(3)]
    Pv, vv, ov = (b[1:1 + n] for b in bufs)
    assert all(t.data_ptr() % 16 == 4 for t in (Pv, vv, ov))
    Pv.copy_(P)
    vv.copy_(v)
    net.gnvp(Pv, vv, X, Y, l2=1e-4, out=ov)
    err = rel(ov, aligned)
    print(f"gnvp unaligned vs aligned: rel {err:.2e}, bitwise {torch.equal(ov, aligned)}")
    assert torch.equal(ov, aligned)
    assert float(bufs[2][0]) == 7.0 and bool((bufs[2][1 + n:] == 7.0).all())  # nothing stored outside the view


SOLVER_NET = ([784, 16, 10], ["relu", "linear"])


@pytest.fixture(scope="module")
def mnist512(pkg):
    Xh, Yh = pkg.synth_mnist(512)
    return dev(Xh), dev(Yh)


def test_slbfgs_pair_is_the_gauss_newton_product(ctx, pkg, mnist512):
    """With b_H = N the Hessian batch is every row in some order, so each recorded pair's y must be gnvp on the
    whole data at the recorded u with s = u_e - u_{e-1}, up to the summation order (1e-5); the record's fourth
    block stays zero."""
    dims, acts = SOLVER_NET
    X, Y = mnist512
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    n = net.nparams
    run = pkg.SlbfgsRun(net, P, X, Y, hvp_exact=2, M=5, L=4, b=32, b_H=512, step=0.02, lam=1e-4, tol=0.0)
    rec = run.pair_io(cap=4)
    run.iterate(1)
    rec = rec[:, :, :n].clone()
    run.close()
    events = [e for e in range(4) if bool(rec[e, 1].any())]
    assert len(events) >= 3, events  # 16 inner steps, L = 4: events at t = 4, 8, 12
    net2 = pkg.Mlp(ctx, dims, acts)
    for e in events[1:]:
        u, s = rec[e, 1].contiguous(), (rec[e, 1] - rec[e - 1, 1]).contiguous()
        ref = net2.gnvp(u, s, X, Y, inv_scale=1.0 / 512, l2=1e-4)
        err = rel(rec[e, 2], ref)
        print(f"event {e}: recorded y vs gnvp rel {err:.2e}")
        assert err <= 1e-5
        assert not bool(rec[e, 3].any())


def test_slbfgs_gauss_newton_pairs_have_positive_curvature(ctx, pkg, mnist512):
    """Every Gauss-Newton pair has y.s >= lam s.s > 0 and passes the filter; the run descends at the step
    test_slbfgs_exact_hvp_option uses (0.02)."""
    dims, acts = SOLVER_NET
    X, Y = mnist512
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    lam = 1e-4
    hist, _ = pkg.slbfgs_solve(net, P, X, Y, M=5, L=4, b=32, b_H=16, step=0.02, max_epochs=3, tol=0.0, lam=lam,
                               hvp_exact="gauss_newton", pair_trace=64)
    pairs = hist["pairs"]
    assert len(pairs) > 0
    ys, ss, acc = pairs[:, 2], pairs[:, 3], pairs[:, 5]
    print(f"gauss-newton pairs: {len(pairs)}, min y.s {ys.min():.3e}, min y.s / (lam s.s) {(ys / (lam * ss)).min():.3f}; "
          f"loss {hist['loss']}")
    assert np.all(ys > 0.0) and np.all(acc == 1)
    assert np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][0]


def test_unified_curvature_member(ctx, pkg):
    """UnifiedConfig.curvature reaches the solver: Gauss-Newton pairs give another loss record than the finite
    difference, and an unknown name is an error."""
    Xh, Yh = pkg.synth_mnist(256)
    data = pkg.UnifiedDataset(train_x=Xh, train_y=Yh)
    losses = {}
    for curv in ("fd", "gauss_newton"):
        la = pkg.UnifiedLauncher(0)
        la.addLayer(784, 16, "relu")
        la.addLayer(16, 10, "linear")
        la.buildNetwork()
        la.setData(data)
        # 8 inner steps an epoch, curvature events at t = 2, 4, 6: pairs from the first epoch on
        cfg = pkg.UnifiedConfig(name="gn", max_iters=3, tolerance=0.0, learning_rate=0.02, batch_size=32, m_param=5,
                                L_param=2, write_csv=False, curvature=curv)
        la.train(pkg.UnifiedSLBFGS(), cfg)
        losses[curv] = np.array(la.last_recorder.loss)
    assert len(losses["fd"]) == len(losses["gauss_newton"]) > 0
    assert np.all(np.isfinite(losses["gauss_newton"]))
    assert not np.array_equal(losses["fd"], losses["gauss_newton"])
    la = pkg.UnifiedLauncher(0)
    la.addLayer(784, 10, "linear")
    la.buildNetwork()
    la.setData(data)
    with pytest.raises(pkg.LbfError):
        la.train(pkg.UnifiedSLBFGS(), pkg.UnifiedConfig(max_iters=1, batch_size=32, write_csv=False,
                                                         curvature="newton"))
