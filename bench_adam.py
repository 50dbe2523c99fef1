"""Adam microbenchmark.

  steps   steps per second of adam_solve against sgd_solve at 784-128-10 relu / linear cross-entropy, N = 60000, for
          batch 256 and batch 4096, both without the recorder (no full-batch rows): per step one fused evaluation of
          the batch and one update sweep, one synchronisation per epoch. The evaluation is the same code; what differs
          is the row gather of the shuffled batches (adam_shuffle; adam_contiguous takes the rows by pointer offset,
          as SGD does), the sweep (7 n floats against momentum SGD's 5 n) and SGD's one-thread epoch_loss_acc launch,
          which Adam's sweep absorbs. --epochs epochs per repeat, the three alternating in one process after a
          warm-up; host clock around calls that end in a stream synchronise. No verdict.
  sweep   the sweep alone at config 5's parameter count (4096-2048-1024-1, n = 10,489,857): lbf_adam_step on four
          device vectors, HIP events around --launches back-to-back launches, as GB/s of its 7 n floats (g, m, v, w
          read; m, v, w written) against the HBM peak. aligned: the float4 route; scalar: w one float off.

    python bench_adam.py [--repeats 7] [--warmup 1] [--epochs 2] [--launches 50] [--parts steps,sweep]
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


def rate(ms, steps):
    r = [steps / (t * 1e-3) for t in ms]
    return {"median": round(float(np.median(r)), 1), "min": round(min(r), 1), "max": round(max(r), 1)}


def bench_steps(pkg, ctx, a):
    dims, acts, N = [784, 128, 10], ["relu", "linear"], 60000
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    P0 = net.init_params(123, "cpu")
    for batch in (256, 4096):
        steps = a.epochs * -(-N // batch)
        runs = {
            "adam_shuffle": lambda: pkg.adam_solve(net, P0.clone(), X, Y, record=False, batch=batch,
                                                   max_epochs=a.epochs, tol=0.0),
            "adam_contiguous": lambda: pkg.adam_solve(net, P0.clone(), X, Y, record=False, batch=batch,
                                                      max_epochs=a.epochs, tol=0.0, shuffle=0),
            "sgd": lambda: pkg.sgd_solve(net, P0.clone(), X, Y, record=False, batch=batch, max_epochs=a.epochs,
                                         tol=0.0, lr=1e-3),
        }
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        t = {k: [] for k in runs}
        for _ in range(a.repeats):  # alternating, so a drift of the box hits all alike
            for k, fn in runs.items():
                t[k].append(host_ms(fn))
        out = {k: rate(v, steps) for k, v in t.items()}
        print(json.dumps({"bench": "adam_steps", "dims": dims, "rows": N, "batch": batch, "epochs": a.epochs,
                          "steps_per_run": steps, "repeats": a.repeats, "steps_per_s": out,
                          "adam_shuffle_over_sgd": round(out["adam_shuffle"]["median"] / out["sgd"]["median"], 3),
                          "adam_contiguous_over_sgd": round(out["adam_contiguous"]["median"] / out["sgd"]["median"],
                                                            3)}), flush=True)


def bench_sweep(pkg, ctx, a):
    n = 4097 * 2048 + 2049 * 1024 + 1025   # 4096-2048-1024-1
    gen = torch.Generator(device="cuda").manual_seed(123)
    base = [torch.randn(n + 4, device="cuda", generator=gen) for _ in range(4)]
    base[2].abs_()
    coef = pkg.adam_coefs(pkg.adam_params(weight_decay=1e-2), 1e-3, 10)
    out = {"bench": "adam_sweep", "n": n, "bytes": 7 * 4 * n, "launches": a.launches, "hbm_peak_GBs": HBM_PEAK_GBS}
    for route, woff in (("aligned", 0), ("scalar", 1)):
        g, m, v = (b[:n] for b in base[:3])
        w = base[3][woff:woff + n]
        us = []
        for _ in range(a.repeats + a.warmup):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                ctx.adam_step(w, m, v, g, coef)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        us = us[a.warmup:]
        gbs = [7 * 4 * n / (u * 1e-6) / 1e9 for u in us]
        out[route] = {"us": {"median": round(float(np.median(us)), 2), "min": round(min(us), 2),
                             "max": round(max(us), 2)},
                      "GBs": {"median": round(float(np.median(gbs)), 1), "min": round(min(gbs), 1),
                              "max": round(max(gbs), 1)},
                      "hbm_frac": round(float(np.median(gbs)) / HBM_PEAK_GBS, 4)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--parts", type=str, default="steps,sweep")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "steps" in parts:
        bench_steps(pkg, ctx, a)
    if "sweep" in parts:
        bench_sweep(pkg, ctx, a)


if __name__ == "__main__":
    main()
