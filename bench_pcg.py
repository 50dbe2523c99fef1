"""Preconditioned Hessian-free microbenchmark, with bench_hf.py's protocol.

  grad_sq  Mlp.grad_sq beside Mlp.loss_grad at the same shape: 784-128-10 relu with N = 60000 and with 4096 rows,
           784-512-256-10 tanh with 128 gathered rows of 60000. Alternating calls in one process after a warm-up,
           host clock around the call (each ends in a stream synchronise). grad_sq does a gradient's GEMM work on an
           unfused pass, once per outer iteration of the solver: the ratio is reported, there is no pass mark.
  pcg      one iteration of Mlp.gn_pcg beside one of Mlp.gn_cg at the same shapes: solves of --iters iterations
           (rtol = 0, damping 0.1, check = --iters), alternating. PCG reads minv twice more per iteration (0.8 MB at
           784-128-10). within_cg_spread: the PCG median lies no further above the CG median than the CG figure's
           own min-max spread.
  race     loss against wall time on DESIGN §15's record problem (784-128-10 cross-entropy, N = 60000, l2 = 1e-3,
           the same start): hf_solve, hf_solve(precond="grad_sq"), lbfgs_solve. For the record, no verdict.

    python bench_pcg.py [--repeats 20] [--warmup 3] [--iters 30] [--parts grad_sq,pcg,race]
Prints one JSON line per measurement.
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

SHAPES = [([784, 128, 10], ["relu", "linear"], 60000, 0), ([784, 128, 10], ["relu", "linear"], 4096, 0),
          ([784, 512, 256, 10], ["tanh", "tanh", "linear"], 60000, 128)]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats_us(v, per=1):
    return {"median": round(float(np.median(v)) * 1e3 / per, 1), "min": round(min(v) * 1e3 / per, 1),
            "max": round(max(v) * 1e3 / per, 1)}


def setup(pkg, ctx, dims, acts, N, gathered):
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    g = torch.Generator(device="cuda").manual_seed(1)
    b = torch.randn(net.nparams, device="cuda", generator=g)
    idx = torch.randperm(N, device="cuda", generator=g)[:gathered].to(torch.int32) if gathered else None
    return net, P, b, X, Y, idx, gathered or N


def alternate(fns, a):
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    t = {k: [] for k in fns}
    for _ in range(a.repeats):  # alternating, so a drift of the box hits all alike
        for k, f in fns.items():
            t[k].append(host_ms(f))
    return t


def bench_grad_sq(pkg, ctx, a):
    for dims, acts, N, gathered in SHAPES:
        net, P, b, X, Y, idx, B = setup(pkg, ctx, dims, acts, N, gathered)
        out = net.new_params()
        t = alternate({"grad_sq": lambda: net.grad_sq(P, X, Y, idx=idx, out=out),
                       "loss_grad": lambda: net.loss_grad(P, X, Y, idx=idx)}, a)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "grad_sq", "dims": dims, "rows": B, "of": N, "repeats": a.repeats,
                          "us": {k: stats_us(v) for k, v in t.items()},
                          "grad_sq_over_loss_grad": round(med["grad_sq"] / med["loss_grad"], 3)}), flush=True)


def bench_pcg(pkg, ctx, a):
    for dims, acts, N, gathered in SHAPES:
        net, P, b, X, Y, idx, B = setup(pkg, ctx, dims, acts, N, gathered)
        minv = (net.grad_sq(P, X, Y, idx=idx) + 0.1) ** -0.75
        x = net.new_params()
        kw = dict(idx=idx, inv_scale=1.0 / B, damping=0.1, max_iters=a.iters, rtol=0.0, check=a.iters, out=x)
        its = []

        def cg():
            its.append(net.gn_cg(P, b, X, Y, **kw)[1]["iterations"])

        def pcg():
            its.append(net.gn_pcg(P, b, minv, X, Y, **kw)[1]["iterations"])

        t = alternate({"cg": cg, "pcg": pcg}, a)
        assert set(its) == {a.iters}, set(its)
        s = {k: stats_us(v, a.iters) for k, v in t.items()}
        print(json.dumps({"bench": "pcg_iteration", "dims": dims, "rows": B, "of": N, "iters": a.iters,
                          "repeats": a.repeats, "us_per_iteration": s,
                          "pcg_over_cg": round(s["pcg"]["median"] / s["cg"]["median"], 3),
                          "within_cg_spread": bool(s["pcg"]["median"] - s["cg"]["median"]
                                                   <= s["cg"]["max"] - s["cg"]["min"])}), flush=True)


def race(pkg, ctx, a):
    dims, acts, N = [784, 128, 10], ["relu", "linear"], 60000
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    for name in ("hf", "hf_grad_sq", "lbfgs"):
        net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent", l2=1e-3)
        for timed in (False, True):  # the first solve warms the workspaces up
            P = net.init_params(123, "cpu")
            cg = None
            if name == "lbfgs":
                hist, info = pkg.lbfgs_solve(net, P, X, Y, m=10, max_iters=150, tol=0.0)
            else:
                hist, info, tr = pkg.hf_solve(net, P, X, Y, max_iters=30, tol=0.0,
                                              precond="grad_sq" if name == "hf_grad_sq" else None)
                cg = [int(v) for v in tr["cg"]]
        assert timed
        step = max(1, len(hist["loss"]) // 15)
        print(json.dumps({"bench": "pcg_race", "solver": name, "dims": dims, "rows": N, "l2": 1e-3,
                          "iterations": int(info.iterations), "n_evals": int(info.n_evals),
                          "n_loss_only": int(info.n_loss_only), "final_loss": float(info.final_loss),
                          "cg_iterations": cg,
                          "ms": [round(float(v), 2) for v in hist["time_ms"][::step]],
                          "loss": [round(float(v), 6) for v in hist["loss"][::step]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--parts", type=str, default="grad_sq,pcg,race")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcg.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "grad_sq" in parts:
        bench_grad_sq(pkg, ctx, a)
    if "pcg" in parts:
        bench_pcg(pkg, ctx, a)
    if "race" in parts:
        race(pkg, ctx, a)


if __name__ == "__main__":
    main()
