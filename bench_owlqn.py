"""OWL-QN microbenchmark.

  iteration  us per OWL-QN iteration against us per L-BFGS iteration (lbf_lbfgs_iterate, Armijo) at 784-128-10
             relu / linear cross-entropy, N = 60000, m = 10, from the same start on the same data; l1 = 1e-3 for
             OWL-QN. Both run --iters iterations per repeat, alternating in one process after a warm-up; host clock
             around calls that end in a stream synchronise. OWL-QN has no stateful form, so its iteration time is
             (solve of --iters iterations - solve of 0 iterations) / --iters: the start point's evaluation is
             taken out, as lbf_lbfgs_begin takes it out for L-BFGS. The trials per iteration of both are reported:
             an OWL-QN iteration costs what its trials cost. No verdict.
  sweeps     the two sweeps' achieved HBM bandwidth at config 5's parameter count (4096-2048-1024-1,
             n = 10,489,857) beside the Gram sweep's and the combine's in the same solve: owlqn_solve on --samples
             rows with the library's event profiler on (lbf_prof_*). Bytes: owl_pseudo 3 n floats (x, g read, pg
             written), owl_trial 4 n (x, d, pg read, x+ written), gram (2k + 7) n
             (k S + k Y + x, x_prev, g, g_prev, pg read, s, y written), combine to the direction alone
             (2k + 2) n (k S + k Y + pg read, d written).

    python bench_owlqn.py [--repeats 10] [--warmup 2] [--iters 30] [--samples 4096] [--parts iteration,sweeps]
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

HBM_PEAK_GBS = 8000.0


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats_us(v, per=1):
    return {"median": round(float(np.median(v)) * 1e3 / per, 1), "min": round(min(v) * 1e3 / per, 1),
            "max": round(max(v) * 1e3 / per, 1)}


def bench_iteration(pkg, ctx, a):
    dims, acts, N, l1, m = [784, 128, 10], ["relu", "linear"], 60000, 1e-3, 10
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    P0 = net.init_params(123, "cpu")
    seen = {}

    def owlqn(iters):
        P = P0.clone()
        return lambda: seen.__setitem__(("owlqn", iters), pkg.owlqn_solve(net, P, X, Y, m=m, max_iters=iters, tol=0.0,
                                                                          l1=l1))

    def lbfgs_ms():
        run = pkg.LbfgsRun(net, P0.clone(), X, Y, line_search="armijo", m=m, max_iters=1 << 30, tol=0.0,
                           record_cap=a.iters + 8)
        ms = host_ms(lambda: run.iterate(a.iters))
        seen["lbfgs"] = (run.hist.as_dict(), run.info)
        run.close()
        return ms

    for _ in range(a.warmup):
        owlqn(a.iters)()
        owlqn(0)()
        lbfgs_ms()
    t = {"owlqn": [], "owlqn_start": [], "lbfgs": []}
    for _ in range(a.repeats):  # alternating, so a drift of the box hits all alike
        t["owlqn"].append(host_ms(owlqn(a.iters)))
        t["owlqn_start"].append(host_ms(owlqn(0)))
        t["lbfgs"].append(lbfgs_ms())
    oh, oi, ost = seen[("owlqn", a.iters)]
    lh, li = seen["lbfgs"]
    assert int(oi.iterations) == a.iters and len(lh["loss"]) >= a.iters, (oi.iterations, len(lh["loss"]))
    it = [x - y for x, y in zip(t["owlqn"], t["owlqn_start"])]
    n = net.nparams
    print(json.dumps({"bench": "owlqn_iteration", "dims": dims, "rows": N, "l1": l1, "m": m, "iters": a.iters,
                      "repeats": a.repeats,
                      "us_per_iteration": {"owlqn": stats_us(it, a.iters), "lbfgs_armijo": stats_us(t["lbfgs"], a.iters)},
                      "owlqn_start_us": stats_us(t["owlqn_start"]),
                      "owlqn_over_lbfgs": round(float(np.median(it)) / float(np.median(t["lbfgs"])), 3),
                      "trials_per_iteration": {"owlqn": round(float(oh["ls_trials"].mean()), 2),
                                               "lbfgs_armijo": round(float(lh["ls_trials"][:a.iters].mean()), 2)},
                      "sweep_bytes_per_iteration": {"owl_pseudo": 3 * n * 4, "owl_trial_each": 4 * n * 4},
                      "final": {"owlqn_F": float(oi.final_loss), "zeros": int(ost["zeros"]),
                                "penalised": int(ost["penalised"]), "lbfgs_loss": float(li.final_loss)}}), flush=True)


def bench_sweeps(pkg, ctx, a):
    dims, acts, m = [4096, 2048, 1024, 1], ["relu", "relu", "linear"], 10
    g = torch.Generator(device="cuda").manual_seed(123)
    X = torch.randn(a.samples, dims[0], device="cuda", generator=g)
    v = torch.randn(dims[0], 1, device="cuda", generator=g)
    Y = (torch.tanh(X @ v / 64.0) + 0.01 * torch.randn(a.samples, 1, device="cuda", generator=g)).contiguous()
    net = pkg.Mlp(ctx, dims, acts)
    n = net.nparams
    iters = m + 2 + a.iters
    pkg.owlqn_solve(net, net.init_params(123, "cpu"), X, Y, m=m, max_iters=iters, tol=0.0, l1=1e-4)  # warm-up
    torch.cuda.synchronize()
    ctx.prof_select(None)
    ctx.prof_sample(1)
    ctx.prof_enable(True)
    hist, info, st = pkg.owlqn_solve(net, net.init_params(123, "cpu"), X, Y, m=m, max_iters=iters, tol=0.0, l1=1e-4)
    torch.cuda.synchronize()
    prof = ctx.prof_read()
    ctx.prof_enable(False)
    out = {"bench": "owlqn_sweeps", "dims": dims, "n": n, "m": m, "samples": a.samples,
           "iterations": int(info.iterations), "trials": int(hist["ls_trials"].sum()), "zeros": int(st["zeros"])}
    # the ring fills over the first m iterations: the Gram sweep and the combine read (k_i) live pairs at iteration i
    acc = hist["accepted"]
    ks = [min(m, int(acc[:i].sum())) for i in range(int(info.iterations))]
    bytes_of = {"owl_pseudo": lambda c: 3 * n * 4 * c, "owl_trial": lambda c: 4 * n * 4 * c,
                "gram_sweep": lambda c: sum((2 * k + 7) * n * 4 if i else n * 4 for i, k in enumerate(ks)),
                "combine_sweep": lambda c: sum((2 * k + 2) * n * 4 for k in ks)}
    for key, (ms, cnt) in sorted(prof.items()):
        kind = key.split("[")[0]
        if kind in bytes_of and cnt > 0:
            b = bytes_of[kind](cnt)
            out[kind] = {"launches": cnt, "us_mean": round(ms / cnt * 1e3, 2), "GBs": round(b / ms / 1e6, 1),
                         "hbm_frac": round(b / ms / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--parts", type=str, default="iteration,sweeps")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_owlqn.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "iteration" in parts:
        bench_iteration(pkg, ctx, a)
    if "sweeps" in parts:
        bench_sweeps(pkg, ctx, a)


if __name__ == "__main__":
    main()
