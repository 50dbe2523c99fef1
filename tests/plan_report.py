"""Reads the LBF_SHOW_PLAN=1 report (stderr, mlp_plan.cpp plan, mlp_eval.cpp forward) so that a test can assert the
tile and split plan its shape was chosen for. The switch is read when the Mlp is constructed: set it with
monkeypatch.setenv before, and pass capfd.readouterr().err here after the first call on the network."""
import re

import torch

# GemmTile ids of the report (kernels.hpp): 0 = 128 rows x (128 | 64 | 32 by N), 1 = 32 x 128, 2 = 64 x 64, 3 = 64 x 128
T128, T32x128, T64x64, T64x128 = 0, 1, 2, 3
PLAN_CUS = 256  # the tests' expected plans are Mlp::plan's on this many compute units

LAYER_RE = re.compile(r"\[lbf plan\] B=(\d+) layer (\d+): dW tile (\d+) splits (\d+) k_chunk (\d+) \| "
                      r"fwd tile (\d+) splits (\d+)(?: \| dX tile (\d+))?\n")
ASUM_RE = re.compile(r"\[lbf plan\] B=(\d+) forward of (\d+) layers: A from slabs at layers((?: \d+)+| none)\n")


def planned_layers(err, B, nl):
    """Per layer ((fwd tile, splits), (dW tile, splits, k_chunk), dX tile or None) of batch B's plan."""
    rows = {int(m[2]): m for m in LAYER_RE.finditer(err) if int(m[1]) == B}
    assert sorted(rows) == list(range(nl)), f"no plan of B={B} for {nl} layers in the report:\n{err}"
    return [((int(m[6]), int(m[7])), (int(m[3]), int(m[4]), int(m[5])), None if m[8] is None else int(m[8]))
            for m in (rows[l] for l in range(nl))]


def planned_asum(err, B, nfwd):
    """The layers whose forward GEMM took its A from the previous layer's split-K slabs, from the line of the
    first forward pass (over nfwd layers) under batch B's plan."""
    lines = [m for m in ASUM_RE.finditer(err) if int(m[1]) == B]
    assert len(lines) == 1 and int(lines[0][2]) == nfwd, f"no forward report of B={B} over {nfwd} layers:\n{err}"
    return tuple(int(t) for t in lines[0][3].split() if t != "none")


def on_plan_device():
    """False where the device's CU count gives other plans: the caller then skips its route assertion only."""
    return torch.cuda.get_device_properties(0).multi_processor_count == PLAN_CUS


def lost_route(name, got, want):
    return (f"{name} no longer covers the route it was written for (choose another batch that reaches it; keep the "
            f"expectation): planned {got}, expected {want}")
