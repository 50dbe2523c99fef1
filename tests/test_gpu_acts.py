"""The leaky-ReLU, ELU and softplus activations on every kernel that applies an activation, against torch
fp64 on the CPU (ref_mlp.py with ref_acts.py's three entries).

Bounds, the project's existing ones: loss relative 1e-5; gradient, hvp, gnvp and grad_sq
||got - ref|| <= max(1e-4, 3 x the same torch reference run in fp32 on the CPU) ||ref||. The elementwise test of
the extremes has its own: forward |got - ref64| <= 1e-6 |ref64| + 1.2e-38 (a few ulp of expf / log1pf; 1.2e-38 is
the smallest normal fp32), bias gradient <= 1e-5 |ref| + 1.2e-38. Every test prints what it measured.

Shapes of loss_grad: those tests/test_gpu_xent.py names per output route. The fused output-layer kernels keep the
reference's four activation bodies (seven cost every network scratch and speed), so a network with one
of the three rectifiers on its last or last hidden layer runs every shape below on the unfused route: forward GEMMs
with the seven-body EPI_FWD epilogue, loss.hip, backward GEMMs with the seven-body EPI_DX epilogue. No test here
runs a head kernel.
  shapes the old activations run fused     [37, 50, 3]; [129, 130, 65, 10] with the activation on both hidden
                                           layers; [48, 200, 10] (standalone head)
  generic (loss.hip) shapes                [16, 300, 4], [32, 40, 130]; [50, 7] with the activation on the output
                                           layer under the squared error
  split forward through fwd_reduce_act     [260, 132, 70] at B = 100
  A-from-slabs prologue (a_act)            [256, 256, 132, 4] at B = 64
The last two are built under LBF_SHOW_PLAN=1 and the report must show the forward splits / the `A from slabs at`
line (on 256 compute units; elsewhere only the numbers are checked).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_acts
from gpu_helpers import dev, host, make_net, run_ranks, shard, solver_inputs
from plan_report import ASUM_RE, T32x128, lost_route, on_plan_device, planned_asum, planned_layers
from ref_acts import NEW_ACTS
from ref_mlp import (MSE, XENT, gap, gn_ref, grad_sq_ref, hess_ref, hf_ref, host_args, loss_grad, make_case, one_hot,
                     rel)

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
RTOL = 1e-4      # gradient and second-order products: max(RTOL, 3 x fp32 torch)
TINY = 1.2e-38   # the smallest normal fp32, rounded up


def data(dims, loss, N, seed, scale=1.0):
    rng = np.random.default_rng([seed, N] + list(dims))
    X = (scale * rng.standard_normal((N, dims[0]))).astype(np.float32)
    Y = one_hot(rng, N, dims[-1]) if loss == XENT else rng.standard_normal((N, dims[-1])).astype(np.float32)
    return X, Y


def check_loss_grad(net, dims, acts, loss, P, X, Y, l2=0.0, tag=""):
    """net.loss_grad on the rows X / Y against torch fp64 (inv_scale 1 / rows)."""
    B = X.shape[0]
    got_l, got_g = net.loss_grad(P, dev(X), dev(Y), l2=l2)
    Ph = P.cpu().numpy()
    l_ref, g_ref = loss_grad(dims, acts, loss, Ph, X, Y, 1.0 / B, l2)
    _, g32 = loss_grad(dims, acts, loss, Ph, X, Y, 1.0 / B, l2, torch.float32)
    dl, dg, d32 = abs(got_l - l_ref) / abs(l_ref), rel(host(got_g), g_ref), rel(g32, g_ref)
    print(f"{tag} {dims} {acts} {loss} B={B}: loss rel {dl:.2e}, grad rel {dg:.2e} (torch fp32: {d32:.2e})")
    assert np.isfinite(got_l) and bool(torch.isfinite(got_g).all())
    assert dl <= LOSS_RTOL
    assert dg <= max(RTOL, 3.0 * d32)


# ---------------------------------------------------------------- 1. every route
def hidden(n):
    return lambda a: [a] * n + ["linear"]


ROUTE_NETS = [
    # ids: the shape and the output route the old activations take on it; the rectifiers run every one of them
    # unfused (EPI_FWD, loss.hip, EPI_DX), see the module docstring
    ("37-50-3-unfused", [37, 50, 3], hidden(1), (MSE, XENT)),
    ("129-130-65-10-unfused", [129, 130, 65, 10], hidden(2), (MSE, XENT)),
    ("48-200-10-unfused", [48, 200, 10], hidden(1), (MSE, XENT)),
    ("16-300-4-generic", [16, 300, 4], hidden(1), (MSE, XENT)),
    ("32-40-130-generic", [32, 40, 130], hidden(1), (MSE, XENT)),
    ("50-7-output-layer", [50, 7], lambda a: [a], (MSE,)),
]
ROUTE_CASES = [(t, d, f, l) for t, d, f, ls in ROUTE_NETS for l in ls]


@pytest.mark.parametrize("N", [1, 31, 257])
@pytest.mark.parametrize("tag,dims,mk,loss", ROUTE_CASES, ids=[f"{t}-{l}" for t, d, f, l in ROUTE_CASES])
@pytest.mark.parametrize("act", NEW_ACTS)
def test_loss_grad_on_every_route(ctx, pkg, act, tag, dims, mk, loss, N):
    acts = mk(act)
    X, Y = data(dims, loss, N, seed=1)
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    check_loss_grad(net, dims, acts, loss, net.init_params(123, "cpu"), X, Y, tag=tag)


@pytest.mark.parametrize("loss", [MSE, XENT])
@pytest.mark.parametrize("act", NEW_ACTS)
def test_loss_grad_split_forward_reduce(ctx, pkg, monkeypatch, capfd, act, loss):
    """260-132-70 at B = 100: layer 0's forward runs in 5 splits on the 32 x 128 tile and fwd_reduce_act sums the
    slabs, adds the bias and applies the activation (no layer takes its A from slabs)."""
    dims, acts, B = [260, 132, 70], [act, "linear"], 100
    X, Y = data(dims, loss, B, seed=2)
    monkeypatch.setenv("LBF_SHOW_PLAN", "1")
    capfd.readouterr()
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    net.loss_grad(P, dev(X), dev(Y))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    got = (planned_layers(err, B, 2)[0][0], planned_asum(err, B, 2))
    print(f"split forward {act} {loss}: layer 0 forward {got[0]}, A from slabs at {got[1]}"
          f"{'' if on_plan_device() else ' (NOT asserted: the device has not 256 CUs)'}")
    if on_plan_device():
        assert got == ((T32x128, 5), ()), lost_route("split forward", got, ((T32x128, 5), ()))
    check_loss_grad(net, dims, acts, loss, P, X, Y, tag="split-forward")


@pytest.mark.parametrize("loss", [MSE, XENT])
@pytest.mark.parametrize("act", NEW_ACTS)
def test_loss_grad_a_from_slabs(ctx, pkg, monkeypatch, capfd, act, loss):
    """256-256-132-4 at B = 64: both hidden forwards run in 4 splits and layer 1's GEMM sums layer 0's slabs, adds
    the bias and applies the activation while it loads its A (gemm.hip's a_act prologue)."""
    dims, acts, B = [256, 256, 132, 4], [act, act, "linear"], 64
    X, Y = data(dims, loss, B, seed=3)
    monkeypatch.setenv("LBF_SHOW_PLAN", "1")
    capfd.readouterr()
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    net.loss_grad(P, dev(X), dev(Y))
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    plan = planned_layers(err, B, 3)
    lines = [m for m in ASUM_RE.finditer(err) if int(m[1]) == B]
    assert len(lines) == 1, err
    asum = tuple(int(t) for t in lines[0][3].split() if t != "none")
    got = (plan[0][0], plan[1][0], asum)
    print(f"A from slabs {act} {loss}: forwards {got[0]} {got[1]}, A from slabs at {asum}"
          f"{'' if on_plan_device() else ' (NOT asserted: the device has not 256 CUs)'}")
    if on_plan_device():
        want = ((T32x128, 4), (T32x128, 4), (1,))
        assert got == want, lost_route("A from slabs", got, want)
    check_loss_grad(net, dims, acts, loss, P, X, Y, tag="a-from-slabs")


# ---------------------------------------------------------------- 2. extremes, elementwise
EXTREMES = np.array([120, -120, 90, -90, 40, -40, 20, -20, 5, -5, 1, -1, 1e-3, -1e-3, 0.0, -0.0,   # the required set
                     60, -60, 30, -30, 15, -15, 10, -10, 2.5, -2.5, 0.5, -0.5, 0.1, -0.1, 88.5, -88.5],
                    np.float32).reshape(4, 8)


@pytest.mark.parametrize("act", NEW_ACTS)
def test_extremes_elementwise(ctx, pkg, act):
    """One 8-8 layer with W = I and b = 0, one row per call: the outputs are act of the inputs, and with targets
    Y = a - 1 (a the fp32 outputs) the bias gradient is act'(a) inv_scale, act' taken through a as the engine takes it
    (ref_acts.dact_y in fp64). A forward written as log(1 + exp(x)) or exp(x) - 1, or a derivative written as
    1 - exp(-y), fails here."""
    net = pkg.Mlp(ctx, [8, 8], [act])
    P = dev(np.concatenate([np.eye(8, dtype=np.float32).ravel(), np.zeros(8, np.float32)]))
    inv_scale = 0.5
    worst_f, worst_g = 0.0, 0.0
    for row in EXTREMES:
        X = dev(row[None, :])
        a = net.forward(P, X).cpu().numpy()[0]
        ref = ref_acts.act(act, row.astype(np.float64))
        assert np.all(np.isfinite(a)), (row, a)
        ef = np.abs(a.astype(np.float64) - ref)
        worst_f = max(worst_f, float((ef / np.maximum(np.abs(ref), 1e-300))[np.abs(ref) > TINY].max(initial=0.0)))
        assert np.all(ef <= 1e-6 * np.abs(ref) + TINY), (act, row, a, ref)
        Y = dev((a - np.float32(1.0))[None, :])
        _, g = net.loss_grad(P, X, Y, inv_scale=inv_scale)
        gb = host(g)[64:]
        gref = ref_acts.dact_y(act, a.astype(np.float64)) * inv_scale
        eg = np.abs(gb - gref)
        worst_g = max(worst_g, float((eg / np.maximum(np.abs(gref), 1e-300))[np.abs(gref) > TINY].max(initial=0.0)))
        assert np.all(np.isfinite(gb)) and np.all(eg <= 1e-5 * np.abs(gref) + TINY), (act, row, gb, gref)
    print(f"extremes {act}: forward worst rel {worst_f:.2e}, bias gradient worst rel {worst_g:.2e}")


@pytest.mark.parametrize("act", NEW_ACTS)
def test_extremes_through_the_backward_gemm(ctx, pkg, act):
    """8-8-8 with W = I and b = 0 in both layers, the activation on the first and a linear second layer, one row per
    call, squared error with Y = a - 1: the first layer's bias gradient is (dZ_2 W_2^T) .* act'(a) = act'(a) inv_scale,
    formed by the EPI_DX epilogue of the backward GEMM (dact_c) where the single-layer test reaches loss.hip."""
    net = pkg.Mlp(ctx, [8, 8, 8], [act, "linear"])
    eye, zero = np.eye(8, dtype=np.float32).ravel(), np.zeros(8, np.float32)
    P = dev(np.concatenate([eye, zero, eye, zero]))
    inv_scale, worst = 0.5, 0.0
    for row in EXTREMES:
        X = dev(row[None, :])
        a = net.forward(P, X).cpu().numpy()[0]
        ref = ref_acts.act(act, row.astype(np.float64))
        assert np.all(np.isfinite(a)) and np.all(np.abs(a - ref) <= 1e-6 * np.abs(ref) + TINY), (act, row, a, ref)
        _, g = net.loss_grad(P, X, dev((a - np.float32(1.0))[None, :]), inv_scale=inv_scale)
        gb = host(g)[64:72]
        gref = ref_acts.dact_y(act, a.astype(np.float64)) * inv_scale
        eg = np.abs(gb - gref)
        worst = max(worst, float((eg / np.maximum(np.abs(gref), 1e-300))[np.abs(gref) > TINY].max(initial=0.0)))
        assert np.all(np.isfinite(gb)) and np.all(eg <= 1e-5 * np.abs(gref) + TINY), (act, row, gb, gref)
    print(f"extremes through EPI_DX {act}: first-layer bias gradient worst rel {worst:.2e}")


# ---------------------------------------------------------------- 3. second order
SO_DIMS = [30, 24, 12, 4]
SO_ACTS = {"elu-softplus": ["elu", "softplus", "linear"], "leaky-elu": ["leaky_relu", "elu", "linear"]}


@pytest.mark.parametrize("scale", [1.0, 8.0], ids=["x1", "x8"])  # x8: pre-activations beyond +-20
@pytest.mark.parametrize("loss", [MSE, XENT])
@pytest.mark.parametrize("name", list(SO_ACTS))
def test_second_order_products(ctx, pkg, name, loss, scale):
    dims, acts, B, l2 = SO_DIMS, SO_ACTS[name], 37, 1e-4
    rng = np.random.default_rng([37, int(scale)] + dims)
    X = (scale * rng.standard_normal((B, dims[0]))).astype(np.float32)
    Y = (rng.random((B, dims[-1])) if loss == XENT else rng.standard_normal((B, dims[-1]))).astype(np.float32)
    P = pkg.init_params_host(dims, acts, 123, "cpu")
    v = rng.standard_normal(P.size).astype(np.float32)
    a64 = [torch.from_numpy(t).double() for t in (P, v, X, Y)]
    a32 = [t.float() for t in a64]
    G, H = (f(dims, acts, loss, *a64, 1.0 / B, l2) for f in (gn_ref, hess_ref))
    G32, H32 = (f(dims, acts, loss, *a32, 1.0 / B, l2).double() for f in (gn_ref, hess_ref))
    D = grad_sq_ref(dims, acts, loss, a64[0], a64[2], a64[3], 1.0 / B)
    D32 = grad_sq_ref(dims, acts, loss, a32[0], a32[2], a32[3], 1.0 / B).double()
    print(f"{name} {loss} x{scale:g}: |G-H|/|H| {gap(G, H):.2f}")
    assert gap(G, H) >= 0.1  # act'' matters: neither product passes by computing the other

    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    Pd, vd, Xd, Yd = dev(P), dev(v), dev(X), dev(Y)
    for what, got, ref, ref32 in (("hvp", net.hvp(Pd, vd, Xd, Yd, l2=l2), H, H32),
                                  ("gnvp", net.gnvp(Pd, vd, Xd, Yd, l2=l2), G, G32),
                                  ("grad_sq", net.grad_sq(Pd, Xd, Yd), D, D32)):
        e, e32 = rel(got, ref), rel(ref32, ref)
        print(f"    {what}: {e:.2e} (torch fp32: {e32:.2e})")
        assert bool(torch.isfinite(got).all())
        assert e <= max(RTOL, 3.0 * e32), what


# ---------------------------------------------------------------- 4. solvers
TABLE = {"elu-softplus": ([30, 24, 12, 4], ["elu", "softplus", "linear"], XENT, 37, 0)}
TRAJ_SEED = 2  # every reduction ratio of the fp64 reference is 0.18 from 0.25 and 0.75 (checked below)


@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_hf_trajectory_matches_fp64(ctx, pkg, l2):
    c = make_case(pkg, TABLE, "elu-softplus", None, TRAJ_SEED)
    ref = hf_ref(c, torch.float64, l2, 8)
    margin = min(min(abs(r - 0.25), abs(r - 0.75)) for r in ref["ratio"])
    assert margin >= 5e-3, ref["ratio"]
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=8, tol=0.0, damping0=1.0, cg_iters=10, cg_rtol=0.1)
    dl = float(np.abs(hist["loss"] - np.array(ref["loss"])).max())
    dp = rel(P, ref["P"])
    print(f"hf elu-softplus l2={l2}: loss dev {dl:.2e}, params rel {dp:.2e}, ratio margin {margin:.3f}, "
          f"cg {list(tr['cg'])}, trials {list(hist['ls_trials'])}")
    assert info.iterations == 8
    assert list(tr["cg"]) == ref["cg"]
    assert list(hist["ls_trials"]) == ref["trials"] and list(hist["accepted"]) == ref["accepted"]
    np.testing.assert_allclose(tr["damping"], ref["damping"], rtol=1e-12, atol=0)
    assert dl <= 1e-3
    assert dp <= 1e-3


@pytest.mark.parametrize("line_search", ["wolfe", "armijo"])
def test_lbfgs_descends(ctx, pkg, line_search):
    c = make_case(pkg, TABLE, "elu-softplus")
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    f0 = net.loss(P, X, Y)
    hist, info = pkg.lbfgs_solve(net, P, X, Y, line_search=line_search, m=10, max_iters=10, tol=0.0)
    print(f"lbfgs {line_search}: start {f0:.6f}, losses {hist['loss']}")
    assert len(hist["loss"]) == 10 and np.all(np.isfinite(hist["loss"]))
    assert np.all(np.diff(hist["loss"]) <= 0.0) and hist["loss"][-1] < f0
    check_loss_grad(net, c["dims"], c["acts"], c["loss"], P, c["X"], c["Y"], tag=f"after-lbfgs-{line_search}")


def test_slbfgs_exact_pairs_match_fp64(ctx, pkg):
    """One epoch with exact pairs, the curvature batch being all 37 rows (b_H = N, drawn without replacement). The
    run records every curvature event's u and y = H(u) s + lam s (pair_io), s = u - the previous event's u. Against
    H s + lam s from hess_ref at u in fp64: ||y - ref|| <= tol ||ref|| with the hvp bound tol, and the traced y.s
    within tol ||ref|| ||s|| of s.ref (Cauchy-Schwarz on the same bound)."""
    c = make_case(pkg, TABLE, "elu-softplus")
    dims, acts, loss = c["dims"], c["acts"], c["loss"]
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    lam, N, n = 1e-4, 37, P.numel()
    run = pkg.SlbfgsRun(net, P, X, Y, pair_trace=16, M=5, L=4, b=2, b_H=N, step=0.02, tol=0.0, lam=lam,
                        hvp_exact="exact")
    pio = run.pair_io(8)
    run.iterate(1)
    hist, pairs = run.hist.as_dict(), run.pairs().copy()
    pio = pio[:, :, :n].double().cpu()
    run.close()
    assert np.all(np.isfinite(hist["loss"])) and bool(torch.isfinite(P).all())
    assert len(pairs) >= 2, pairs
    _, _, X64, Y64 = host_args(c, torch.float64)
    for j, row in enumerate(pairs):
        u, s, y = pio[j + 1, 1], pio[j + 1, 1] - pio[j, 1], pio[j + 1, 2]
        ref = hess_ref(dims, acts, loss, u, s, X64, Y64, 1.0 / N, lam)
        ref32 = hess_ref(dims, acts, loss, u.float(), s.float(), X64.float(), Y64.float(), 1.0 / N, lam).double()
        tol = max(RTOL, 3.0 * rel(ref32, ref))
        ev, es = rel(y, ref), abs(row[2] - float(s @ ref)) / float(ref.norm() * s.norm())
        print(f"pair {j} (t = {int(row[1])}): y rel {ev:.2e}, y.s {row[2]:.6e} vs {float(s @ ref):.6e} "
              f"({es:.2e} of |ref||s|), tol {tol:.1e}")
        assert np.isfinite(row[2]) and ev <= tol and es <= tol


# ---------------------------------------------------------------- 5. other paths
def test_evaluate_matches_reference(ctx, pkg):
    dims, acts, N = [37, 50, 3], ["softplus", "linear"], 257
    X, Y = data(dims, XENT, N, seed=5)
    net = pkg.Mlp(ctx, dims, acts, loss=XENT)
    P = net.init_params(123, "cpu")
    r = net.evaluate(P, dev(X), dev(Y))
    P64, X64, Y64 = (torch.from_numpy(np.asarray(t)).double() for t in (P.cpu().numpy(), X, Y))
    l_ref, _ = loss_grad(dims, acts, XENT, P64, X64, Y64, 1.0 / N)
    from ref_mlp import net_out
    Z = net_out(dims, acts, X64)(P64).numpy()
    top = np.sort(Z, 1)
    assert (top[:, -1] - top[:, -2]).min() > 1e-4  # no row of the reference is near a tie
    acc = float((Z.argmax(1) == Y.argmax(1)).mean())
    print(f"evaluate: loss rel {abs(r.loss - l_ref) / abs(l_ref):.2e}, accuracy {r.accuracy} vs {acc}")
    assert r.rows == N and abs(r.loss - l_ref) <= LOSS_RTOL * abs(l_ref)
    assert r.accuracy == acc


@pytest.mark.parametrize("act", NEW_ACTS)
def test_two_ranks_loss_grad(ctx, pkg, act):
    dims, acts, N, world = [129, 130, 65, 10], [act, act, "linear"], 257, 2
    X, Y = data(dims, XENT, N, seed=6)
    P = dev(pkg.init_params_host(dims, acts, 123, "cpu"))
    shards = [shard(N, world, r) for r in range(world)]
    Xs, Ys = [dev(X[lo:hi]) for lo, hi in shards], [dev(Y[lo:hi]) for lo, hi in shards]

    def body(r, c):
        return pkg.Mlp(c, dims, acts, loss=XENT).loss_grad(P, Xs[r], Ys[r], inv_scale=1.0 / N)

    res = run_ranks(pkg, world, body)
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])  # replicated, bitwise
    l_ref, g_ref = loss_grad(dims, acts, XENT, P.cpu().numpy(), X, Y, 1.0 / N)
    _, g32 = loss_grad(dims, acts, XENT, P.cpu().numpy(), X, Y, 1.0 / N, 0.0, torch.float32)
    dl, dg, d32 = abs(res[0][0] - l_ref) / abs(l_ref), rel(host(res[0][1]), g_ref), rel(g32, g_ref)
    print(f"two ranks {act}: loss rel {dl:.2e}, grad rel {dg:.2e} (torch fp32: {d32:.2e})")
    assert dl <= LOSS_RTOL and dg <= max(RTOL, 3.0 * d32)


@pytest.mark.parametrize("act", NEW_ACTS)
def test_loss_grad_twice_is_bitwise_equal(ctx, pkg, act):
    for dims, acts in (([129, 130, 65, 10], [act, act, "linear"]), ([260, 132, 70], [act, "linear"])):
        X, Y = data(dims, XENT, 100, seed=7)
        net = pkg.Mlp(ctx, dims, acts, loss=XENT)
        P = net.init_params(123, "cpu")
        Xd, Yd = dev(X), dev(Y)
        l1, g1 = net.loss_grad(P, Xd, Yd)
        l2, g2 = net.loss_grad(P, Xd, Yd)
        assert l1 == l2 and torch.equal(g1, g2), dims


@pytest.mark.parametrize("bad", [7, -1])
def test_create_rejects_ids_out_of_range(ctx, pkg, bad):
    d, a, h = (C.c_int * 3)(4, 3, 2), (C.c_int * 2)(bad, 0), C.c_void_p()
    assert pkg.lib().lbf_mlp_create(ctx.h, 2, d, a, C.byref(h)) == 1  # LBF_ERR_INVALID
    assert not h.value
    with pytest.raises(pkg.LbfError, match="activation id"):
        pkg.Mlp(ctx, [4, 3, 2], [bad, 0])
    d1, a1 = (C.c_int * 2)(4, 3), (C.c_int * 1)(6)
    assert pkg.lib().lbf_mlp_create(ctx.h, 1, d1, a1, C.byref(h)) == 0  # 6 is the last id
    assert pkg.lib().lbf_mlp_destroy(h) == 0
