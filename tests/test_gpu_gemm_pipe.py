"""The software-pipelined main loop of the 128 x 128 LDS-DMA GEMM tile (gemm.hip glds_body, PIPE): half k-tiles
of fragments read from LDS under the other half's MFMAs, one barrier per k-tile, the last k-tile without a
successor. loss_grad against fp64 (the CPU oracle for the squared error, the objective restated in torch for the
cross-entropy head, as tests/test_gpu_xent.py) at the loop's edge counts of k-tiles:

  B = 32900 (257 full row tiles and one of 4 rows), [In, 128, 10]: the fused-head forward GEMM runs
      nk = 1 (In = 32), 2 with a last k-tile of 4 columns (36), 3 (96), 3 with a last k-tile of 16 columns (80);
      the layer-0 dW GEMM is one 128 x 128 tile split over the batch into short chunks (EPI_STORE); gathered
      rows at In = 36 (forward only: a gathered mn-contiguous operand takes the register-staged kernel).
  B = 49200 (384 full row tiles and one of 48 rows), [144, 128, 10]: nk = 5 with the EPI_HEAD fold of 16 columns
      (144 = 128 + 16; the plan's cost model takes the 128-row tile for five k-tiles from 49153 rows).
  [64, 256, 128, 10]: the 256-wide layer's forward takes the tile at any batch (EPI_FWD, nk = 2; B = 1000, 1100,
      8100); its dX GEMM (EPI_DX, nk = 4) takes 32 x 128 tiles at 1000 / 1100 rows and the 128 x 128 tile at 8100.

Every case reads the tile of the GEMM it is about from the LBF_SHOW_PLAN report and asserts it on 256 CUs.
Tolerances: tests/test_gpu_parity.py's (loss 1e-5, gradient norm 1e-4, fp32 against fp64).
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev
from plan_report import T32x128, T128, lost_route, on_plan_device, planned_layers
from ref_mlp import XENT, loss_grad, rel

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4
B_RAGGED = 32900


def run_case(ctx, pkg, O, monkeypatch, capfd, dims, acts, loss, N, rows=None):
    """loss_grad on N synthetic rows (rows: gathered) checked against fp64; returns the plan of its batch."""
    Xh, Yh = pkg.synth_mnist(N, dims[0], dims[-1], 7)  # one-hot targets: valid for both losses
    monkeypatch.setenv("LBF_SHOW_PLAN", "1")
    capfd.readouterr()
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    idx = None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda()
    val, g = net.loss_grad(P, dev(Xh), dev(Yh), idx=idx)
    B = N if rows is None else len(rows)
    plan = planned_layers(capfd.readouterr().err, B, len(acts))
    Ph = P.double().cpu().numpy()
    if loss == XENT:
        sel = slice(None) if rows is None else rows
        l_ref, g_ref = loss_grad(dims, acts, XENT, Ph, Xh[sel], Yh[sel], 1.0 / B)
    else:
        l_ref, g_ref = O.Net(dims, acts).loss_grad(Ph, Xh.astype(np.float64), Yh.astype(np.float64), idx=rows)
    dl, dg = abs(val - l_ref) / abs(l_ref), rel(g.double().cpu().numpy(), g_ref)
    print(f"gemm pipe {dims} {loss} B={B}: loss rel {dl:.2e}, grad rel {dg:.2e}, plan {plan}")
    assert np.isfinite(val) and bool(torch.isfinite(g).all())
    assert dl <= LOSS_RTOL
    assert dg <= GRAD_RTOL
    return plan


def assert_head_net_tiles(name, plan):
    """[In, 128, 10]: the unsplit 128-row forward tile and the 128 x 128 dW tile of layer 0."""
    (fwd0, dw0, _) = plan[0]
    if on_plan_device():
        assert fwd0 == (T128, 1), lost_route(name + " forward", fwd0, (T128, 1))
        assert dw0[0] == T128 and dw0[1] > 1, lost_route(name + " dW", dw0, (T128, "> 1 splits"))


@pytest.mark.parametrize("loss", ["mse", XENT])
@pytest.mark.parametrize("In,B", [(32, B_RAGGED), (36, B_RAGGED), (96, B_RAGGED), (80, B_RAGGED), (144, 49200)])
def test_head_forward_and_dw_k_tile_counts(ctx, pkg, O, monkeypatch, capfd, In, B, loss):
    dims, acts = [In, 128, 10], ["relu", "linear"]
    plan = run_case(ctx, pkg, O, monkeypatch, capfd, dims, acts, loss, B)
    assert_head_net_tiles(f"{dims} at {B} rows", plan)


def test_head_forward_gathered_rows(ctx, pkg, O, monkeypatch, capfd):
    dims, acts = [36, 128, 10], ["relu", "linear"]
    N = B_RAGGED + 37
    rows = np.random.default_rng(N).permutation(N)[:B_RAGGED].astype(np.int64)
    plan = run_case(ctx, pkg, O, monkeypatch, capfd, dims, acts, "mse", N, rows)
    assert_head_net_tiles(f"{dims} at {B_RAGGED} gathered rows", plan)


@pytest.mark.parametrize("loss", ["mse", XENT])
@pytest.mark.parametrize("B,dx_want", [(1000, T32x128), (1100, T32x128), (8100, T128)])
def test_wide_layer_forward_and_dx(ctx, pkg, O, monkeypatch, capfd, B, dx_want, loss):
    dims, acts = [64, 256, 128, 10], ["relu", "tanh", "linear"]
    plan = run_case(ctx, pkg, O, monkeypatch, capfd, dims, acts, loss, B)
    fwd0, dx1 = plan[0][0], plan[1][2]
    if on_plan_device():
        assert fwd0 == (T128, 1), lost_route(f"{dims} at {B} rows, forward of layer 0", fwd0, (T128, 1))
        assert dx1 == dx_want, lost_route(f"{dims} at {B} rows, dX of layer 1", dx1, dx_want)
