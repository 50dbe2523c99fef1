"""Activation microbenchmark: what the hidden activation costs in the three evaluations that apply it,
  loss_grad  Mlp.loss_grad  forward and backward pass
  hvp        Mlp.hvp        exact R-operator product (act' and, for tanh / elu / softplus, act'')
  gnvp       Mlp.gnvp       Gauss-Newton product (act' only)
for relu and tanh beside leaky_relu, elu and softplus on every hidden layer (the last layer linear, squared error),
on two shapes: 784-128-10 at N = 60000 (the headline network, full batch) and 784-512-256-10 with 128 gathered rows
of 60000 (the S-LBFGS curvature batch).

The columns of loss_grad compare two output routes: relu and tanh run the output layer fused (the
forward GEMM's EPI_HEAD epilogue on 784-128-10, the row head on 784-512-256-10), the three rectifiers run it unfused
(EPI_FWD forward GEMM of the last layer, loss.hip, EPI_DX backward GEMM), which writes and reads the last hidden
activations once more. Each line names the route per activation ("loss_grad_route"). hvp and gnvp take the same
route for all five.

Per shape one network per activation from the same seed (the rectifiers share a start point); after a
warm-up, --repeats calls of each, the activations alternating in one process so that the clock state is shared; host
clock around the call (every evaluation ends in a stream synchronise).

    python bench_act.py [--repeats 30] [--warmup 5]
Prints one JSON line per measurement (shape x evaluation), the times per activation and their ratio to relu's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

ACTS = ["relu", "tanh", "leaky_relu", "elu", "softplus"]
SHAPES = [([784, 128, 10], 60000, 0), ([784, 512, 256, 10], 60000, 128)]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats_us(v):
    return {"median": round(float(np.median(v)) * 1e3, 1), "min": round(min(v) * 1e3, 1),
            "max": round(max(v) * 1e3, 1)}


def bench_shape(pkg, ctx, a, dims, N, gathered):
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.randperm(N, device="cuda", generator=g)[:gathered].to(torch.int32) if gathered else None
    B = gathered or N
    nets = {act: pkg.Mlp(ctx, dims, [act] * (len(dims) - 2) + ["linear"]) for act in ACTS}
    P = {act: net.init_params(123, "cpu") for act, net in nets.items()}
    v = torch.randn(nets["relu"].nparams, device="cuda", generator=g)
    out = nets["relu"].new_params()
    kw = dict(idx=idx, inv_scale=1.0 / B, l2=1e-4)
    evals = {"loss_grad": lambda k: nets[k].loss_grad(P[k], X, Y, grad=out, **kw),
             "hvp": lambda k: nets[k].hvp(P[k], v, X, Y, out=out, **kw),
             "gnvp": lambda k: nets[k].gnvp(P[k], v, X, Y, out=out, **kw)}
    for what, f in evals.items():
        for _ in range(a.warmup):
            for k in ACTS:
                f(k)
        t = {k: [] for k in ACTS}
        for _ in range(a.repeats):   # alternating, so a drift of the box hits every activation alike
            for k in ACTS:
                t[k].append(host_ms(lambda: f(k)))
        med = {k: float(np.median(x)) for k, x in t.items()}
        route = ({k: "fused head" if k in ("relu", "tanh") else "unfused output layer" for k in ACTS}
                 if what == "loss_grad" else None)
        print(json.dumps({"bench": "act_call", "eval": what, "dims": dims, "rows": B, "of": N, "repeats": a.repeats,
                          "loss_grad_route": route,
                          "us": {k: stats_us(x) for k, x in t.items()},
                          "over_relu": {k: round(med[k] / med["relu"], 3) for k in ACTS}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats: at least 20")
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_act.py needs a GPU")
    ctx = pkg.Context(0)
    for dims, N, gathered in SHAPES:
        bench_shape(pkg, ctx, a, dims, N, gathered)


if __name__ == "__main__":
    main()
