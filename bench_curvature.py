"""Curvature-product microbenchmark: the three products S-LBFGS can take a pair's y from,
  fd_hvp  Mlp.fd_hvp  central difference of two batch gradients (the reference's, hvp_exact = 0)
  hvp     Mlp.hvp     exact R-operator product                   (hvp_exact = 1)
  gnvp    Mlp.gnvp    Gauss-Newton product                       (hvp_exact = 2)

  calls   per-call time at cfg 4's pair (784-512-256-10 tanh, 128 gathered rows of 60000) and at 784-128-10 relu
          with 4096 rows: after a warm-up, --repeats calls of each, alternating in one process so that the clock
          state is shared; host clock around the call (every product ends in a stream synchronise). gnvp launches
          a subset of hvp's GEMMs and fewer elementwise passes, so gnvp_over_hvp must not exceed 1.
  epochs  S-LBFGS epochs per second for hvp_exact 0, 1, 2 in bench.py --solver slbfgs's configuration
          (784-512-256-10 relu, N = 60000, b = 256, b_H = 128, L = M = 10, step 0.005) through SlbfgsRun, the
          three modes in turn for --rounds rounds, --epochs timed epochs each after one warm-up epoch. A pair is
          formed once in ten inner steps, so a small difference is expected.
  step02  an observation, no verdict: cfg 4's net on 8192 rows, 3 epochs at the reference's step 0.02 with
          hvp_exact 0 and 2; the loss records and the pair traces (y.s, y.y / s.s, accepted).

    python bench_curvature.py [--repeats 30] [--warmup 5] [--epochs 5] [--rounds 3] [--parts calls,epochs,step02]
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

CFG4 = [784, 512, 256, 10]
CALL_SHAPES = [(CFG4, ["tanh", "tanh", "linear"], 60000, 128), ([784, 128, 10], ["relu", "linear"], 4096, 0)]


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats_us(v):
    return {"median": round(float(np.median(v)) * 1e3, 1), "min": round(min(v) * 1e3, 1),
            "max": round(max(v) * 1e3, 1)}


def bench_calls(pkg, ctx, a):
    for dims, acts, N, gathered in CALL_SHAPES:
        Xh, Yh = pkg.synth_mnist(N)
        X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
        net = pkg.Mlp(ctx, dims, acts)
        P = net.init_params(123, "cpu")
        g = torch.Generator(device="cuda").manual_seed(1)
        v = torch.randn(net.nparams, device="cuda", generator=g)
        idx = torch.randperm(N, device="cuda", generator=g)[:gathered].to(torch.int32) if gathered else None
        B = gathered or N
        out = net.new_params()
        kw = dict(idx=idx, inv_scale=1.0 / B, l2=1e-4, out=out)
        fns = {"fd_hvp": lambda: net.fd_hvp(P, v, X, Y, **kw), "hvp": lambda: net.hvp(P, v, X, Y, **kw),
               "gnvp": lambda: net.gnvp(P, v, X, Y, **kw)}
        for _ in range(a.warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(a.repeats):   # alternating, so a drift of the box hits every product alike
            for k, f in fns.items():
                t[k].append(host_ms(f))
        med = {k: float(np.median(x)) for k, x in t.items()}
        print(json.dumps({"bench": "curvature_call", "dims": dims, "acts": acts, "rows": B, "of": N,
                          "repeats": a.repeats, "us": {k: stats_us(x) for k, x in t.items()},
                          "gnvp_over_hvp": round(med["gnvp"] / med["hvp"], 3),
                          "gnvp_over_fd_hvp": round(med["gnvp"] / med["fd_hvp"], 3)}), flush=True)


def bench_epochs(pkg, ctx, a):
    dims, acts, N = CFG4, ["relu", "relu", "linear"], 60000
    Xh, Yh = pkg.synth_mnist(N, dims[0], dims[-1], 123)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    # One solver open at a time, on a context of its own, the three modes in turn for --rounds rounds: every block
    # is the same solve from the same start (a warm-up epoch, then --epochs timed ones), so the modes differ only in
    # the pairs. (Three solvers open at once put six streams on the process's four hardware queues, and which
    # solver then shares a queue between its two streams is an accident of the creation order.)
    t, last = {m: [] for m in (0, 1, 2)}, {}
    for _ in range(a.rounds):
        for mode in t:
            net = pkg.Mlp(pkg.Context(0), dims, acts)
            P = net.init_params(123, "cpu")
            run = pkg.SlbfgsRun(net, P, X, Y, M=10, L=10, b=256, b_H=128, step=0.005, lam=1e-4, tol=0.0,
                                hvp_exact=mode)
            run.iterate(1)
            t[mode] += [host_ms(lambda: run.iterate(1)) for _ in range(a.epochs)]
            last[mode] = float(run.hist.as_dict()["loss"][-1])
            run.close()
    out = {"bench": "curvature_epochs", "dims": dims, "rows": N, "rounds": a.rounds, "epochs_per_round": a.epochs,
           "ms_per_epoch": {str(m): {"median": round(float(np.median(x)), 3), "min": round(min(x), 3),
                                     "max": round(max(x), 3)} for m, x in t.items()},
           "epochs_per_s": {str(m): round(1e3 / float(np.median(x)), 2) for m, x in t.items()},
           "last_loss": {str(m): v for m, v in last.items()}}
    print(json.dumps(out), flush=True)


def observe_step02(pkg, ctx):
    dims, acts, N = CFG4, ["relu", "relu", "linear"], 8192
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    for mode in (0, 2):
        net = pkg.Mlp(ctx, dims, acts)
        P = net.init_params(123, "cpu")
        hist, _ = pkg.slbfgs_solve(net, P, X, Y, M=10, L=10, b=256, b_H=128, step=0.02, lam=1e-4, tol=0.0,
                                   max_epochs=3, hvp_exact=mode, pair_trace=64)
        pairs = hist["pairs"]
        print(json.dumps({"bench": "curvature_step0.02", "hvp_exact": mode, "rows": N,
                          "loss": [float(x) for x in hist["loss"]],
                          "pairs": [{"epoch": int(p[0]), "t": int(p[1]), "ys": float(p[2]),
                                     "yy_over_ss": float(p[4] / p[3]) if p[3] else None, "accepted": int(p[5])}
                                    for p in pairs]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, default="calls,epochs,step02")
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats: at least 20")
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_curvature.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "calls" in parts:
        bench_calls(pkg, ctx, a)
    if "epochs" in parts:
        bench_epochs(pkg, ctx, a)
    if "step02" in parts:
        observe_step02(pkg, ctx)


if __name__ == "__main__":
    main()
