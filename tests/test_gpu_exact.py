"""Every GEMM route bit for bit: the engine on exactly representable networks (tests/exact_nets.py).

The data are small integers whose sums of absolute values stay below 2^24 (asserted when a case is built), the
kernels are true fp32 MFMA, inv_scale = 2**-floor(log2 B), l2 = 2**-6 and every grad_sq scale is a power of two:
each expected value is the fp64 numpy reference times a power of two, an fp32 number, and every comparison in this
file is an equality (exact_nets.assert_bits; the losses as fp64). There is no tolerance anywhere. All networks have
ReLU hidden layers, a linear output and the squared error; integer data sit on ReLU's kink (Z == 0) all the time,
so forward, backward and R-pass must agree on relu'(0) = 0.

Shapes: the tables of the tolerance tests, imported from them (Mlp::plan depends on dims, batch and CU count only).
Each network is built under LBF_SHOW_PLAN=1 and its route is asserted on 256 CUs (printed everywhere): the
expectation of the table's own test where it has one, else the plan pinned in PLANS below.
"""
import math

import numpy as np
import pytest
import torch

import exact_nets as en
from gpu_helpers import run_ranks
from plan_report import T32x128, T64x128, T128, lost_route, on_plan_device, planned_asum, planned_layers
from test_gpu_gemm_pipe import B_RAGGED
from test_gpu_parity import NETS as PARITY_NETS
from test_gpu_pcg import GS
from test_gpu_second_order_routes import CASES as ROUTE_CASES

pytestmark = pytest.mark.gpu

EXTRA_ROWS = 37  # a gathered case draws its B rows, with repeats, from B + 37


# ---------------------------------------------------------------- the shape tables (also read by test_exact_nets.py)

def route_none(name, plan):
    pass


# Mlp::plan on 256 CUs for the shapes whose own tests assert no route (the parity networks, the standalone head, the
# S-LBFGS minibatch, grad_sq's), as LBF_SHOW_PLAN reports it: per layer ((fwd tile, splits), (dW tile, splits,
# k chunk), dX tile).
# Among them: the forward in 13, 9 and 2 splits (784 -> 300), in 7 and 8 (784 -> 512 -> 256), dW in 1 .. 250 splits
# on 64 x 64 and 128-row tiles, dX on both tiles.
PLANS = {
    "784x128x10-B1": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "784x128x10-B31": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "784x128x10-B257": [((1, 1), (2, 5, 64), None), ((1, 1), (2, 5, 64), 1)],
    "784x128x10-B1000": [((1, 1), (2, 16, 64), None), ((1, 1), (2, 16, 64), 1)],
    "784x128x64x10-B1": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1), ((1, 1), (2, 1, 32), 0)],
    "784x128x64x10-B31": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1), ((1, 1), (2, 1, 32), 0)],
    "784x128x64x10-B257": [((1, 1), (2, 5, 64), None), ((1, 1), (2, 3, 96), 1), ((1, 1), (2, 3, 96), 0)],
    "784x128x64x10-B1000": [((1, 1), (2, 16, 64), None), ((1, 1), (2, 16, 64), 1), ((1, 1), (2, 16, 64), 0)],
    "37x50x3-B1": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 0)],
    "37x50x3-B31": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 0)],
    "37x50x3-B257": [((1, 1), (2, 3, 96), None), ((1, 1), (2, 3, 96), 0)],
    "37x50x3-B1000": [((1, 1), (2, 11, 96), None), ((1, 1), (2, 11, 96), 0)],
    "64x96x33x1-B1": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 0), ((1, 1), (2, 1, 32), 0)],
    "64x96x33x1-B31": [((1, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 0), ((1, 1), (2, 1, 32), 0)],
    "64x96x33x1-B257": [((1, 1), (2, 5, 64), None), ((1, 1), (2, 3, 96), 0), ((1, 1), (2, 3, 96), 0)],
    "64x96x33x1-B1000": [((1, 1), (2, 16, 64), None), ((1, 1), (2, 16, 64), 0), ((1, 1), (2, 11, 96), 0)],
    "129x130x65x10-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1), ((1, 1), (2, 1, 32), 0)],
    "129x130x65x10-B31": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1), ((1, 1), (2, 1, 32), 0)],
    "129x130x65x10-B257": [((0, 1), (2, 5, 64), None), ((1, 1), (2, 5, 64), 1), ((1, 1), (2, 3, 96), 0)],
    "129x130x65x10-B1000": [((0, 1), (2, 16, 64), None), ((1, 1), (2, 16, 64), 1), ((1, 1), (2, 16, 64), 0)],
    "784x300x20-B1": [((1, 13), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "784x300x20-B31": [((1, 13), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "784x300x20-B257": [((1, 9), (2, 5, 64), None), ((1, 1), (2, 5, 64), 1)],
    "784x300x20-B1000": [((1, 2), (2, 11, 96), None), ((1, 1), (2, 16, 64), 1)],
    "16x300x4-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "16x300x4-B31": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "16x300x4-B257": [((0, 1), (2, 5, 64), None), ((1, 1), (2, 5, 64), 1)],
    "16x300x4-B1000": [((0, 1), (2, 16, 64), None), ((1, 1), (2, 16, 64), 1)],
    "50x7-B1": [((1, 1), (2, 1, 32), None)],
    "50x7-B31": [((1, 1), (2, 1, 32), None)],
    "50x7-B257": [((1, 1), (2, 3, 96), None)],
    "50x7-B1000": [((1, 1), (2, 11, 96), None)],
    "48x132x10-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "48x132x10-B63": [((0, 1), (2, 1, 64), None), ((1, 1), (2, 1, 64), 1)],
    "48x132x10-B256": [((0, 1), (2, 4, 64), None), ((1, 1), (2, 4, 64), 1)],
    "48x132x10-B40000": [((0, 1), (0, 250, 160), None), ((0, 1), (0, 250, 160), 0)],
    "48x200x10-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "48x200x10-B63": [((0, 1), (2, 1, 64), None), ((1, 1), (2, 1, 64), 1)],
    "48x200x10-B256": [((0, 1), (2, 4, 64), None), ((1, 1), (2, 4, 64), 1)],
    "48x200x10-B40000": [((0, 1), (0, 250, 160), None), ((0, 1), (0, 250, 160), 0)],
    "48x255x10-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "48x255x10-B63": [((0, 1), (2, 1, 64), None), ((1, 1), (2, 1, 64), 1)],
    "48x255x10-B256": [((0, 1), (2, 4, 64), None), ((1, 1), (2, 4, 64), 1)],
    "48x255x10-B40000": [((0, 1), (0, 250, 160), None), ((0, 1), (0, 250, 160), 0)],
    "48x256x10-B1": [((0, 1), (2, 1, 32), None), ((1, 1), (2, 1, 32), 1)],
    "48x256x10-B63": [((0, 1), (2, 1, 64), None), ((1, 1), (2, 1, 64), 1)],
    "48x256x10-B256": [((0, 1), (2, 4, 64), None), ((1, 1), (2, 4, 64), 1)],
    "48x256x10-B40000": [((0, 1), (0, 250, 160), None), ((0, 1), (0, 157, 256), 0)],
    "784x512x256x10-B256": [((1, 7), (2, 4, 64), None), ((1, 8), (2, 4, 64), 1), ((1, 1), (2, 4, 64), 1)],
    # grad_sq's shapes
    "37x1-B31": [((1, 1), (2, 1, 32), None)],
    "63x3-B257": [((1, 1), (2, 3, 96), None)],
    "64x16-B1": [((1, 1), (2, 1, 32), None)],
    "129x17-B1000": [((1, 1), (2, 16, 64), None)],
    "784x130-B257": [((1, 13), (2, 5, 64), None)],
    "64x32x10-B257": [((1, 1), (2, 3, 96), None), ((1, 1), (2, 3, 96), 0)],
    "784x512x256x10-B64": [((1, 13), (2, 1, 64), None), ((1, 8), (2, 1, 64), 1), ((1, 1), (2, 1, 64), 1)],
}


def route_pinned(name, plan):
    assert plan == PLANS[name], lost_route(name, plan, PLANS[name])


def route_fwd_tile(name, plan):
    want = (T32x128 if "B8192" in name else T64x128, 1)
    assert plan[0][0] == want, lost_route(name, plan[0][0], want)


def route_head_net(name, plan):
    (fwd0, dw0, _) = plan[0]
    assert fwd0 == (T128, 1), lost_route(name + " forward", fwd0, (T128, 1))
    assert dw0[0] == T128 and dw0[1] > 1, lost_route(name + " dW", dw0, (T128, "> 1 splits"))


def route_wide(name, plan):
    dx_want = T128 if "B8100" in name else T32x128
    assert plan[0][0] == (T128, 1), lost_route(name + " forward of layer 0", plan[0][0], (T128, 1))
    assert plan[1][2] == dx_want, lost_route(name + " dX of layer 1", plan[1][2], dx_want)


def route_table(route):
    def check(name, plan):
        assert plan == list(route), lost_route(name, plan, list(route))
    return check


def uniq(cases):
    seen, out = set(), []
    for dims, B, check in cases:
        if (tuple(dims), B) not in seen:
            seen.add((tuple(dims), B))
            out.append((dims, B, check))
    return out


SECOND_ORDER = uniq([(c[0], c[3], route_table(c[6])) for c in ROUTE_CASES])
SECOND_ORDER_ASUM = {(tuple(c[0]), c[3]): tuple(c[7]) for c in ROUTE_CASES}
MINIBATCH = ([784, 512, 256, 10], 256, route_pinned)  # the S-LBFGS minibatch route: the row head, grouped dW

LOSS_GRAD = uniq(
    [(d, N, route_pinned) for d, _ in PARITY_NETS for N in (1, 31, 257, 1000)]
    + [([48, H, 10], N, route_pinned) for H in (132, 200, 255, 256) for N in (1, 63, 256, 40000)]  # standalone head
    + [(d, N, route_fwd_tile) for d in ([784, 128, 10], [784, 128, 64, 10]) for N in (8192, 8200, 15000)]
    + [([In, 128, 10], B_RAGGED, route_head_net) for In in (32, 36, 80, 96)]
    + [([144, 128, 10], 49200, route_head_net)]  # the fold
    + [([64, 256, 128, 10], B, route_wide) for B in (1000, 1100, 8100)]
    + SECOND_ORDER + [MINIBATCH])
GRAD_SQ = uniq([(c[0], c[4] or c[3], route_pinned) for c in GS.values()] + [([36, 128, 10], B_RAGGED, route_head_net)])
BATCH_GRADS = [([784, 512, 256, 10], 256, route_none), ([129, 130, 65, 10], 256, route_none)]
SHARDED = ([784, 128, 10], 1001, route_none)


def case_id(c):
    return f"{'x'.join(map(str, c[0]))}-B{c[1]}"


def all_cases():
    """Every (dims, B, rows of X) this file builds a case for."""
    out = [(d, B, B + EXTRA_ROWS) for d, B, _ in uniq(LOSS_GRAD + GRAD_SQ)]
    return out + [(d, B, B) for d, B, _ in BATCH_GRADS + [SHARDED]]


# ---------------------------------------------------------------- helpers

def dev(a):
    return torch.from_numpy(np.array(a, np.float32, order="C")).cuda()  # a copy: the cases' arrays are read-only


def host(t):
    return t.cpu().numpy()


def planned_net(pkg, ctx, monkeypatch, capfd, dims):
    monkeypatch.setenv("LBF_SHOW_PLAN", "1")
    capfd.readouterr()
    return pkg.Mlp(ctx, dims, ["relu"] * (len(dims) - 2) + ["linear"])


def check_plan(name, capfd, dims, B, check, asum=None):
    """Reads the report of the calls made so far; asserts the case's route on 256 CUs, prints it everywhere."""
    err = capfd.readouterr().err
    plan = planned_layers(err, B, len(dims) - 1)
    got_asum = planned_asum(err, B, len(dims) - 1) if asum is not None else None
    print(f"{name}: route {'asserted' if on_plan_device() else 'NOT asserted (the device has not 256 CUs)'}: "
          f"{plan}" + ("" if asum is None else f", A from slabs at {got_asum}"))
    if on_plan_device():
        check(name, plan)
        if asum is not None:
            assert got_asum == asum, lost_route(name, got_asum, asum)


def views(c, gathered):
    """Device X, Y, idx of the case's plain batch (its first B rows) or of its gathered rows (all rows + idx)."""
    if gathered:
        return dev(c["X"]), dev(c["Y"]), torch.from_numpy(c["rows"].astype(np.int32)).cuda()
    return dev(c["X"][:c["B"]]), dev(c["Y"][:c["B"]]), None


# ---------------------------------------------------------------- forward, loss, loss_grad, Mlp.loss

@pytest.mark.parametrize("case", LOSS_GRAD, ids=case_id)
def test_forward_loss_grad_exact(ctx, pkg, monkeypatch, capfd, request, case):
    dims, B, check = case
    name = request.node.callspec.id
    c = en.make_case(dims, B, B + EXTRA_ROWS)
    p, inv = c["p"], 2.0 ** -c["p"]
    net = planned_net(pkg, ctx, monkeypatch, capfd, dims)
    P, P64 = dev(c["P"]), c["P"].astype(np.float64)
    for gathered in (False, True):
        X, Y, idx = views(c, gathered)
        X64, Y64 = en.batch(c, gathered)
        tag = f"{name} {'gathered' if gathered else 'plain'}"
        if not gathered:
            en.assert_bits(host(net.forward(P, X)), en.outputs(P64, X64, dims), f"{tag} outputs")
        s, g_ref = en.sse(P64, X64, Y64, dims), en.gradient(P64, X64, Y64, dims)
        for l2 in (0.0, en.L2):
            loss, g = net.loss_grad(P, X, Y, idx=idx, inv_scale=inv, l2=l2)
            en.assert_bits(host(g), en.scaled(g_ref, p, P64, l2), f"{tag} gradient (l2 = {l2})", dims)
            en.assert_bits(np.float64(loss), en.loss_value(s, p, P64, l2), f"{tag} loss (l2 = {l2})")
            if l2 == 0.0:
                only = net.loss(P, X, Y, idx=idx, inv_scale=inv)
                assert only == loss, (tag, "Mlp.loss", only, "loss_grad", loss)
    check_plan(name, capfd, dims, B, check)


# ---------------------------------------------------------------- hvp, gnvp

@pytest.mark.parametrize("case", SECOND_ORDER, ids=case_id)
def test_hvp_gnvp_exact(ctx, pkg, monkeypatch, capfd, request, case):
    dims, B, check = case
    name = request.node.callspec.id
    c = en.make_case(dims, B, B + EXTRA_ROWS)
    p, inv = c["p"], 2.0 ** -c["p"]
    net = planned_net(pkg, ctx, monkeypatch, capfd, dims)
    P, v = dev(c["P"]), dev(c["v"])
    P64, v64 = c["P"].astype(np.float64), c["v"].astype(np.float64)
    for gathered in (False, True):
        X, Y, idx = views(c, gathered)
        X64, Y64 = en.batch(c, gathered)
        tag = f"{name} {'gathered' if gathered else 'plain'}"
        for l2 in (0.0, en.L2):
            hv = net.hvp(P, v, X, Y, idx=idx, inv_scale=inv, l2=l2)
            if not gathered and l2 == 0.0:  # the first call under this plan was the R-pass's unfused forward
                torch.cuda.synchronize()
                check_plan(name, capfd, dims, B, check, SECOND_ORDER_ASUM[(tuple(dims), B)])
            gv = net.gnvp(P, v, X, Y, idx=idx, inv_scale=inv, l2=l2)
            en.assert_bits(host(hv), en.scaled(en.hvp(P64, v64, X64, Y64, dims), p, v64, l2), f"{tag} hvp (l2 = {l2})",
                           dims)
            en.assert_bits(host(gv), en.scaled(en.gnvp(P64, v64, X64, Y64, dims), p, v64, l2),
                           f"{tag} gnvp (l2 = {l2})", dims)


# ---------------------------------------------------------------- grad_sq

@pytest.mark.parametrize("case", GRAD_SQ, ids=case_id)
def test_grad_sq_exact(ctx, pkg, monkeypatch, capfd, request, case):
    dims, B, check = case
    name = request.node.callspec.id
    c = en.make_case(dims, B, B + EXTRA_ROWS)
    net = planned_net(pkg, ctx, monkeypatch, capfd, dims)
    P, P64 = dev(c["P"]), c["P"].astype(np.float64)
    for gathered in (False, True):
        X, Y, idx = views(c, gathered)
        X64, Y64 = en.batch(c, gathered)
        ref = en.grad_sq(P64, X64, Y64, dims)
        for p in (0, c["p"]):
            d = net.grad_sq(P, X, Y, idx=idx, scale=2.0 ** -p)
            en.assert_bits(host(d), en.scaled(ref, p), f"{name} {'gathered' if gathered else 'plain'} grad_sq "
                           f"(scale 2^-{p})", dims)
    check_plan(name, capfd, dims, B, check)


# ---------------------------------------------------------------- batch_grads

@pytest.mark.parametrize("case", BATCH_GRADS, ids=case_id)
def test_batch_grads_exact(ctx, pkg, case):
    """4 minibatches of 64 rows in one evaluation: each row is loss_grad's gradient of that minibatch and the
    reference's, bit for bit."""
    dims, B, _ = case
    c = en.make_case(dims, B)
    net = pkg.Mlp(ctx, dims, ["relu"] * (len(dims) - 2) + ["linear"])
    P, X, Y, P64 = dev(c["P"]), dev(c["X"]), dev(c["Y"]), c["P"].astype(np.float64)
    X64, Y64 = en.batch(c)
    ref = en.batch_gradients(P64, X64, Y64, dims, 4)
    for l2 in (0.0, en.L2):
        got = net.batch_grads(P, X, Y, 4, inv_scale=2.0 ** -6, l2=l2)
        want = np.stack([en.scaled(ref[i], 6, P64, l2) for i in range(4)])
        en.assert_bits(host(got), want, f"batch_grads {dims} (l2 = {l2})", dims)
        for i in range(4):
            _, g = net.loss_grad(P, X[64 * i:64 * (i + 1)].contiguous(), Y[64 * i:64 * (i + 1)].contiguous(),
                                 inv_scale=2.0 ** -6, l2=l2)
            en.assert_bits(host(got[i]), host(g), f"batch_grads {dims} minibatch {i} against loss_grad (l2 = {l2})",
                           dims)


# ---------------------------------------------------------------- rank groups

@pytest.mark.parametrize("cuts", [(0, 400, 1001), (0, 200, 633, 1001)], ids=["world2", "world3"])
def test_ranks_exact(ctx, pkg, cuts):
    """Uneven shares of 1001 rows over an in-process rank group: with exact sums every rank's loss and gradient
    are the single context's, and the reference's, bit for bit."""
    dims, B, _ = SHARDED
    c = en.make_case(dims, B)
    p, inv = c["p"], 2.0 ** -c["p"]
    acts = ["relu", "linear"]
    P, P64 = dev(c["P"]), c["P"].astype(np.float64)
    X64, Y64 = en.batch(c)
    s, g_ref = en.sse(P64, X64, Y64, dims), en.gradient(P64, X64, Y64, dims)
    net1 = pkg.Mlp(ctx, dims, acts)
    single = {l2: net1.loss_grad(P, dev(c["X"]), dev(c["Y"]), inv_scale=inv, l2=l2) for l2 in (0.0, en.L2)}
    world = len(cuts) - 1
    Xs = [dev(c["X"][cuts[r]:cuts[r + 1]]) for r in range(world)]
    Ys = [dev(c["Y"][cuts[r]:cuts[r + 1]]) for r in range(world)]

    def body(r, cx):
        net = pkg.Mlp(cx, dims, acts)
        return {l2: net.loss_grad(P, Xs[r], Ys[r], inv_scale=inv, l2=l2) for l2 in (0.0, en.L2)}

    res = run_ranks(pkg, world, body)
    for l2 in (0.0, en.L2):
        l1, g1 = single[l2]
        en.assert_bits(host(g1), en.scaled(g_ref, p, P64, l2), f"single context gradient (l2 = {l2})", dims)
        en.assert_bits(np.float64(l1), en.loss_value(s, p, P64, l2), f"single context loss (l2 = {l2})")
        for r in range(world):
            lr, gr = res[r][l2]
            en.assert_bits(host(gr), host(g1), f"rank {r} of {world} gradient (l2 = {l2})", dims)
            en.assert_bits(np.float64(lr), l1, f"rank {r} of {world} loss (l2 = {l2})")


# ---------------------------------------------------------------- BLAS-1

def int_vector(n, seed):
    return np.random.default_rng(seed).integers(-2, 2, n, endpoint=True).astype(np.float32)


@pytest.mark.parametrize("n", [123457, 3_000_001])
def test_dot_nrm2_exact(ctx, n):
    """Integer vectors |x|, |y| <= 2: the dot is an integer below 2^24, exact in any precision and order; nrm2 is
    the square root of one and may round once."""
    x, y = int_vector(n, n), int_vector(n, n + 1)
    dx, dy = dev(x), dev(y)
    xy = int(np.dot(x.astype(np.int64), y.astype(np.int64)))
    xx = int(np.dot(x.astype(np.int64), x.astype(np.int64)))
    assert xx < 2 ** 24
    assert ctx.dot(dx, dy) == float(xy)
    assert ctx.dot(dx, dx) == float(xx)
    root = math.sqrt(xx)  # correctly rounded
    got = ctx.nrm2(dx)
    print(f"nrm2 n = {n}: got {got!r}, sqrt of the exact integer {root!r}")
    assert math.nextafter(root, 0.0) <= got <= math.nextafter(root, math.inf)


@pytest.mark.parametrize("alpha", [0.5, -0.5, 0.25])
def test_axpy_scal_exact(ctx, pkg, alpha):
    n = 123457
    x, y = int_vector(n, 7), int_vector(n, 8)
    dx, dy = dev(x), dev(y)
    ctx.axpy_(alpha, dx, dy)
    en.assert_bits(host(dy), y.astype(np.float64) + alpha * x.astype(np.float64), f"axpy alpha {alpha}")
    en.assert_bits(host(dx), x, "axpy leaves x")
    pkg._lib.check(pkg.lib().lbf_scal(ctx.h, n, alpha, pkg._lib.ptr(dx)), "lbf_scal")
    en.assert_bits(host(dx), alpha * x.astype(np.float64), f"scal alpha {alpha}")
