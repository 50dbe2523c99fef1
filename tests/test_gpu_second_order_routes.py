"""Mlp.hvp and Mlp.gnvp against torch fp64 on every GEMM route the R-pass takes (mlp_curvature.cpp rpass_linear_fwd,
rpass_weight_grad, rpass_back_prod, the unfused forward() with its A-from-slabs prologue; hvp.hip's row loops).

Each case names the plan it was chosen for: per layer the forward tile and splits, the dW tile, splits and k chunk,
the dX tile, and the layers whose forward GEMM takes its A from the previous layer's split-K slabs. The network is
built with LBF_SHOW_PLAN=1 and the report on stderr must equal that plan, else the case no longer covers its
route (Mlp::plan replayed for 256 CUs; on a device with another CU count only the numbers are checked).

Inputs: X ~ N(0,1) in fp32, squared-error targets N(0,1), cross-entropy targets unnormalised non-negative rows
(Ysum varies), the engine's seed-123 CPU-stream init, v ~ N(0,1), inv_scale = 1/B. References: ref_mlp.py's
gn_ref (jvp, closed-form H_L, vjp) and hess_ref (double backward), fp64 on the CPU on the selected rows.

Bounds: ||got - ref|| <= 1e-4 ||ref|| over the whole vector (the project's HVP / GN bound) and, over every
layer's weight block and every layer's bias row separately, max(1e-4, 3 x the same segment's error of the same
torch reference run in fp32 on the CPU) (test_loss_grad_matches_oracle's rule). On the references
||G - H|| >= 0.1 ||H||, so neither product passes by computing the other.

Measured with the engine's init (every figure is printed by the tests), worst segment over all cases and both
products: GPU (MI355X, 256 CUs) 6.7e-7 (1030-24-4, first layer); the fp32 torch reference on the CPU 3.1e-6
(130-36-3 at 33001 rows; it depends on the host BLAS's summation order: 6.3e-7 on another host). The whole-vector
error of the GPU is 3e-8 .. 6.6e-7, |G - H| / |H| of the references 0.44 .. 1.01. So the bound is 1e-4 on every
segment, two orders above both.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev
from plan_report import T32x128, T64x64, T64x128, T128, lost_route, on_plan_device, planned_asum, planned_layers
from ref_mlp import XENT, gap, gn_ref, hess_ref, rel

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def layer(fwd, dw, dx=None):
    """One layer's route: fwd = (tile, splits), dw = (tile, splits, k_chunk), dx = tile (None for layer 0)."""
    return (fwd, dw, dx)


TS, TL = ["tanh", "sigmoid"], ["tanh", "linear"]
STT, RTL, TTL = ["sigmoid", "tanh", "tanh"], ["relu", "tanh", "linear"], ["tanh", "tanh", "linear"]
# (dims, acts, loss, B, rows of X (> B: B of them gathered), l2, layers' routes, layers with A from slabs)
CASES = [
    # forward 32 x 128 in 5 splits with vector loads, dX 32 x 128, Out = 70 > one 64-lane stride of the xent rows
    ([260, 132, 70], TL, XENT, 100, 160, 1e-4,
     [layer((T32x128, 5), (T64x64, 2, 64)), layer((T32x128, 1), (T64x64, 2, 64), T32x128)], ()),
    # the same split forward through the guarded kernel (K = 258, K % 4 != 0); dW 64 x 64 in 5 splits, guarded
    ([258, 132, 70], TL, XENT, 301, 301, 0.0,
     [layer((T32x128, 5), (T64x64, 5, 64)), layer((T32x128, 1), (T64x64, 5, 64), T32x128)], ()),
    # forward 128 x 128 in 2 splits; dW 64 x 64 in 16 and 24 splits; dX 32 x 128
    ([300, 300, 12], TL, "mse", 1500, 1500, 1e-4,
     [layer((T128, 2), (T64x64, 16, 96)), layer((T32x128, 1), (T64x64, 24, 64), T32x128)], ()),
    # dW 128 x 128 in 17 splits, guarded (K = 2101); dW 64 x 64 with 256-row chunks
    ([300, 300, 12], TL, XENT, 2101, 2101, 0.0,
     [layer((T128, 2), (T128, 17, 128)), layer((T32x128, 1), (T64x64, 9, 256), T32x128)], ()),
    # forward 128 x 128 unsplit; dW 64 x 64 in 5 splits (LDS-DMA: K = 300); dX 32 x 128 and 128 x 128; act'' on
    # every layer, the output layer included
    ([40, 130, 66, 5], STT, "mse", 300, 300, 1e-4,
     [layer((T128, 1), (T64x64, 5, 64)), layer((T32x128, 1), (T64x64, 5, 64), T32x128),
      layer((T32x128, 1), (T64x64, 4, 96), T128)], ()),
    # the same network with dW 128 x 128 in 14 splits
    ([40, 130, 66, 5], STT, "mse", 2101, 2101, 0.0,
     [layer((T128, 1), (T128, 14, 160)), layer((T32x128, 1), (T64x64, 9, 256), T32x128),
      layer((T32x128, 1), (T64x64, 8, 288), T128)], ()),
    # odd widths everywhere; dW 128 x 128 in 17 splits
    ([129, 130, 65, 10], RTL, XENT, 2100, 2100, 1e-4,
     [layer((T128, 1), (T128, 17, 128)), layer((T32x128, 1), (T64x64, 9, 256), T32x128),
      layer((T32x128, 1), (T64x64, 8, 288), T128)], ()),
    # B > 4 x 4096: the second trip of the row loops (xent) and of every elementwise grid; dW 128 x 32 in 129
    # splits; dX 128 x 32
    ([12, 20, 5], TS, "mse", 16500, 16500, 0.0,
     [layer((T32x128, 1), (T128, 129, 128)), layer((T32x128, 1), (T128, 129, 128), T128)], ()),
    ([12, 20, 5], TL, XENT, 16500, 17000, 1e-4,
     [layer((T32x128, 1), (T128, 129, 128)), layer((T32x128, 1), (T128, 129, 128), T128)], ()),
    # forward 64 x 128; dW 64 x 64 in 29 splits of 288 rows
    ([16, 96, 6], TL, "mse", 8200, 8200, 1e-4,
     [layer((T64x128, 1), (T64x64, 29, 288)), layer((T32x128, 1), (T64x64, 29, 288), T128)], ()),
    # forward 128 x 64 and 128 x 32; dW 128 x 64 in 207 splits and 128 x 32 in 258; dX 128 x 64
    ([130, 36, 3], TL, XENT, 33001, 33001, 0.0,
     [layer((T128, 1), (T128, 207, 160)), layer((T128, 1), (T128, 258, 128), T128)], ()),
    # in + 1 > 1024: dW 128 x 32; guarded forward with K = 1030
    ([1030, 24, 4], TL, "mse", 2100, 2100, 1e-4,
     [layer((T32x128, 1), (T128, 17, 128)), layer((T32x128, 1), (T64x64, 9, 256), T128)], ()),
    # both hidden forwards in 4 splits of 64; layer 1 takes its A from layer 0's slabs
    ([256, 256, 132, 4], TTL, "mse", 64, 64, 0.0,
     [layer((T32x128, 4), (T64x64, 1, 64)), layer((T32x128, 4), (T64x64, 1, 64), T32x128),
      layer((T32x128, 1), (T64x64, 1, 64), T32x128)], (1,)),
    ([256, 256, 132, 4], TTL, "mse", 67, 67, 1e-4,
     [layer((T32x128, 4), (T64x64, 2, 64)), layer((T32x128, 4), (T64x64, 2, 64), T32x128),
      layer((T32x128, 1), (T64x64, 2, 64), T32x128)], (1,)),
]
IDS = [f"{'x'.join(map(str, c[0]))}-{c[2]}-B{c[3]}" for c in CASES]


def check_route(name, err, B, route, asum):
    got = (planned_layers(err, B, len(route)), planned_asum(err, B, len(route)))  # read on any device
    want = (list(route), tuple(asum))
    print(f"{name}: route {'asserted' if on_plan_device() else 'NOT asserted (the device has not 256 CUs)'}: {got}")
    if on_plan_device():
        assert got == want, lost_route(name, got, want)


def case_data(pkg, dims, acts, loss, B, N):
    rng = np.random.default_rng([B] + list(dims))
    X = rng.standard_normal((N, dims[0])).astype(np.float32)
    Y = (rng.random((N, dims[-1])) if loss == XENT else rng.standard_normal((N, dims[-1]))).astype(np.float32)
    P = pkg.init_params_host(dims, acts, 123, "cpu")
    v = rng.standard_normal(P.size).astype(np.float32)
    rows = rng.permutation(N)[:B] if N > B else None
    return P, X, Y, v, rows


def segments(dims):
    """(name, lo, hi) of every layer's weight block and bias row in the parameter layout."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        w = dims[l] * dims[l + 1]
        out += [(f"W{l}", off, off + w), (f"b{l}", off + w, off + w + dims[l + 1])]
        off += w + dims[l + 1]
    return out


SEGMENT_WORST = {"gpu": 0.0, "fp32": 0.0}


def check_product(name, what, got, ref, ref32, dims):
    got = got.double().cpu()
    whole = rel(got, ref)
    print(f"{name} {what}: whole {whole:.2e} (fp32-CPU {rel(ref32, ref):.2e})")
    bad = []
    for seg, lo, hi in segments(dims):
        e, e32 = rel(got[lo:hi], ref[lo:hi]), rel(ref32[lo:hi], ref[lo:hi])
        SEGMENT_WORST["gpu"], SEGMENT_WORST["fp32"] = max(SEGMENT_WORST["gpu"], e), max(SEGMENT_WORST["fp32"], e32)
        print(f"    {seg}: {e:.2e} (fp32-CPU {e32:.2e})")
        if not e <= max(RTOL, 3.0 * e32):
            bad.append((seg, e, e32))
    assert not bad, (what, "segments (name, error, fp32-CPU error) over the bound", bad)
    assert whole <= RTOL, (what, whole)


@pytest.mark.parametrize("dims,acts,loss,B,N,l2,route,asum", CASES, ids=IDS)
def test_second_order_products_on_route(ctx, pkg, monkeypatch, capfd, request, dims, acts, loss, B, N, l2, route, asum):
    name = request.node.callspec.id
    P, X, Y, v, rows = case_data(pkg, dims, acts, loss, B, N)
    sel = slice(None) if rows is None else rows
    a64 = [torch.from_numpy(t).double() for t in (P, v, X[sel], Y[sel])]
    a32 = [t.float() for t in a64]
    G, H = (f(dims, acts, loss, *a64, 1.0 / B, l2) for f in (gn_ref, hess_ref))
    G32, H32 = (f(dims, acts, loss, *a32, 1.0 / B, l2).double() for f in (gn_ref, hess_ref))
    print(f"{name}: |G-H|/|H| {gap(G, H):.2f}")
    assert gap(G, H) >= 0.1, gap(G, H)

    monkeypatch.setenv("LBF_SHOW_PLAN", "1")
    capfd.readouterr()
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    idx = None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda()
    Pd, vd, Xd, Yd = dev(P), dev(v), dev(X), dev(Y)
    hv = net.hvp(Pd, vd, Xd, Yd, idx=idx, inv_scale=1.0 / B, l2=l2)
    gv = net.gnvp(Pd, vd, Xd, Yd, idx=idx, inv_scale=1.0 / B, l2=l2)
    torch.cuda.synchronize()
    check_route(name, capfd.readouterr().err, B, route, asum)
    check_product(name, "hvp", hv, H, H32, dims)
    check_product(name, "gnvp", gv, G, G32, dims)
    print(f"worst segment so far: GPU {SEGMENT_WORST['gpu']:.2e}, fp32-CPU {SEGMENT_WORST['fp32']:.2e}")


def test_reused_network_across_split_plans(ctx, pkg):
    """One network at B = 2101, 300, 2101 (hvp, gnvp, hvp): each result is a fresh network's at that batch, bitwise
    (the re-plan, and the R-pass and slab workspaces kept from the larger batch, carry nothing over)."""
    dims, acts = [40, 130, 66, 5], STT
    P, X, Y, v, _ = case_data(pkg, dims, acts, "mse", 2101, 2101)
    Pd, vd, Xd, Yd = dev(P), dev(v), dev(X), dev(Y)
    net = pkg.Mlp(ctx, dims, acts)
    for fn, B in (("hvp", 2101), ("gnvp", 300), ("hvp", 2101)):
        got = getattr(net, fn)(Pd, vd, Xd[:B], Yd[:B], l2=1e-4)
        fresh = getattr(pkg.Mlp(ctx, dims, acts), fn)(Pd, vd, Xd[:B], Yd[:B], l2=1e-4)
        assert torch.equal(got, fresh), (fn, B)


def test_zero_direction_gives_exact_zero(ctx, pkg):
    """v = 0, l2 = 0 on the split routes of 300-300-12 at B = 1500: every entry of both products is written and is
    zero (no slab and no bias row of the products without a ones column is left undefined)."""
    dims, acts = [300, 300, 12], TL
    P, X, Y, _, _ = case_data(pkg, dims, acts, "mse", 1500, 1500)
    net = pkg.Mlp(ctx, dims, acts)
    Pd, Xd, Yd = dev(P), dev(X), dev(Y)
    zero = torch.zeros(net.nparams, device="cuda")
    for fn in ("hvp", "gnvp"):
        out = torch.full((net.nparams,), float("nan"), device="cuda")
        getattr(net, fn)(Pd, zero, Xd, Yd, l2=0.0, out=out)
        assert int(torch.count_nonzero(out)) == 0, fn  # NaN counts as nonzero
