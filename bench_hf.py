"""Hessian-free microbenchmark.

  cg     the cost of one CG iteration inside Mlp.gn_cg against one Mlp.gnvp call, at 784-128-10 relu with
         N = 60000 and with 4096 rows and at 784-512-256-10 tanh with 128 gathered rows of 60000. A solve of
         --iters iterations (rtol = 0, damping 0.1, so none stops early) with check = --iters and with check = 1,
         and --iters gnvp calls, alternating in one process after a warm-up; host clock around the call (each
         ends in a stream synchronise). us_per_iteration is the whole solve over its iterations: the forward
         pass, the start-up and the closing dot products are spread over them. An iteration launches what gnvp
         launches minus the forward pass, plus three sweeps over the parameters, so cg_over_gnvp must stay below 1.
  race   for the record, no verdict: loss against wall time of hf_solve and lbfgs_solve on 784-128-10
         cross-entropy, N = 60000, l2 = 1e-3, from the same start.

    python bench_hf.py [--repeats 20] [--warmup 3] [--iters 30] [--parts cg,race]
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

CG_SHAPES = [([784, 128, 10], ["relu", "linear"], 60000, 0), ([784, 128, 10], ["relu", "linear"], 4096, 0),
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


def bench_cg(pkg, ctx, a):
    for dims, acts, N, gathered in CG_SHAPES:
        Xh, Yh = pkg.synth_mnist(N)
        X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
        net = pkg.Mlp(ctx, dims, acts)
        P = net.init_params(123, "cpu")
        g = torch.Generator(device="cuda").manual_seed(1)
        b = torch.randn(net.nparams, device="cuda", generator=g)
        idx = torch.randperm(N, device="cuda", generator=g)[:gathered].to(torch.int32) if gathered else None
        B = gathered or N
        x, out = net.new_params(), net.new_params()
        kw = dict(idx=idx, inv_scale=1.0 / B)
        its = []

        def solve(check):
            _, info = net.gn_cg(P, b, X, Y, damping=0.1, max_iters=a.iters, rtol=0.0, check=check, out=x, **kw)
            its.append(info["iterations"])

        def products():
            for _ in range(a.iters):
                net.gnvp(P, b, X, Y, l2=0.1, out=out, **kw)

        fns = {"cg": lambda: solve(a.iters), "cg_check1": lambda: solve(1), "gnvp": products}
        for _ in range(a.warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(a.repeats):  # alternating, so a drift of the box hits all three alike
            for k, f in fns.items():
                t[k].append(host_ms(f))
        assert set(its) == {a.iters}, set(its)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"bench": "hf_cg_iteration", "dims": dims, "rows": B, "of": N, "iters": a.iters,
                          "repeats": a.repeats, "us_per_iteration": {k: stats_us(v, a.iters) for k, v in t.items()},
                          "cg_over_gnvp": round(med["cg"] / med["gnvp"], 3),
                          "check1_over_cg": round(med["cg_check1"] / med["cg"], 3)}), flush=True)


def race(pkg, ctx, a):
    dims, acts, N = [784, 128, 10], ["relu", "linear"], 60000
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    for name in ("hf", "lbfgs"):
        net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent", l2=1e-3)
        for timed in (False, True):  # the first solve warms the workspaces up
            P = net.init_params(123, "cpu")
            if name == "hf":
                hist, info, _ = pkg.hf_solve(net, P, X, Y, max_iters=30, tol=0.0)
            else:
                hist, info = pkg.lbfgs_solve(net, P, X, Y, m=10, max_iters=150, tol=0.0)
        assert timed
        step = max(1, len(hist["loss"]) // 15)
        print(json.dumps({"bench": "hf_race", "solver": name, "dims": dims, "rows": N, "l2": 1e-3,
                          "iterations": int(info.iterations), "n_evals": int(info.n_evals),
                          "n_loss_only": int(info.n_loss_only), "final_loss": float(info.final_loss),
                          "ms": [round(float(v), 2) for v in hist["time_ms"][::step]],
                          "loss": [round(float(v), 6) for v in hist["loss"][::step]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--parts", type=str, default="cg,race")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hf.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "cg" in parts:
        bench_cg(pkg, ctx, a)
    if "race" in parts:
        race(pkg, ctx, a)


if __name__ == "__main__":
    main()
