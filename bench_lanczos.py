"""Lanczos microbenchmark, with bench_pcg.py's protocol: alternating calls in one process after a warm-up,
device events around each call, median and min..max.

  step     one Lanczos step beside one product at 784-128-10, N = 60000, both losses: runs of --steps steps with full
           re-orthogonalisation on the Gauss-Newton matrix beside one Mlp.gnvp, and on the Hessian beside one Mlp.hvp.
           A step is the product (for G on the cached forward pass) plus the sweeps over at most --steps + 1 rows.
  sweeps   the sweeps at BASELINE config 5's parameter count (4096-2048-1024-1, n = 10,489,857) on a one-row batch, for
           j = 8, 32, 64: the cost of step j as the difference of runs of j + 1 and of j steps, once with full
           re-orthogonalisation (j + 1 basis rows, two passes) and once with the three-vector recurrence (two rows,
           one pass). Both steps hold the same product on the cached forward pass, so their difference is sweeps
           alone, with no product subtracted. Bytes from the shapes: a pass is a projection (the rows, and w once per
           8 rows) and an update (the rows, w read and written), then w read and q written:
           (4 (j + 1) + 2 ceil((j + 1) / 8) + 6) n floats with full re-orthogonalisation, 9 n with three vectors. GB/s
           is the difference of the two byte counts over the difference of the two step times (the full step also has
           two launches more, which this counts as time of the sweeps).

    python bench_lanczos.py [--repeats 30] [--warmup 3] [--steps 16] [--parts step,sweeps]
Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__  # noqa: E402

PEAK_GBS = 8000.0  # MI355X HBM3E


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats_us(v, per=1):
    return {"median": round(float(np.median(v)) * 1e3 / per, 1), "min": round(min(v) * 1e3 / per, 1),
            "max": round(max(v) * 1e3 / per, 1)}


def alternate(fns, a):
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    t = {k: [] for k in fns}
    for _ in range(a.repeats):  # alternating, so a drift of the box hits all alike
        for k, f in fns.items():
            t[k].append(event_ms(f))
    return t


def bench_step(pkg, ctx, a):
    dims, acts, N = [784, 128, 10], ["relu", "linear"], 60000
    Xh, Yh = pkg.synth_mnist(N)
    X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
    for loss in ("mse", "softmax_xent"):
        net = pkg.Mlp(ctx, dims, acts, loss=loss)
        P = net.init_params(123, "cpu")
        v = torch.randn(net.nparams, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        out = net.new_params()
        done = []
        kw = dict(steps=a.steps, v0=v, check=a.steps, breakdown_rtol=0.0)
        t = alternate({"lanczos_gn": lambda: done.append(net.lanczos(P, X, Y, matrix="gauss_newton", **kw).steps),
                       "gnvp": lambda: net.gnvp(P, v, X, Y, out=out),
                       "lanczos_hessian": lambda: done.append(net.lanczos(P, X, Y, matrix="hessian", **kw).steps),
                       "hvp": lambda: net.hvp(P, v, X, Y, out=out)}, a)
        assert set(done) == {a.steps}, set(done)
        s = {k: stats_us(v_, a.steps if k.startswith("lanczos") else 1) for k, v_ in t.items()}
        print(json.dumps({"bench": "lanczos_step", "dims": dims, "rows": N, "loss": loss, "steps": a.steps,
                          "repeats": a.repeats, "us": s,
                          "gn_step_over_gnvp": round(s["lanczos_gn"]["median"] / s["gnvp"]["median"], 3),
                          "hessian_step_over_hvp": round(s["lanczos_hessian"]["median"] / s["hvp"]["median"], 3)}),
              flush=True)


def bench_sweeps(pkg, ctx, a):
    dims, acts = [4096, 2048, 1024, 1], ["tanh", "tanh", "linear"]
    net = pkg.Mlp(ctx, dims, acts)
    n = net.nparams
    P = net.init_params(123, "cpu")
    g = torch.Generator(device="cuda").manual_seed(1)
    X, Y = torch.randn((1, dims[0]), device="cuda", generator=g), torch.randn((1, 1), device="cuda", generator=g)
    v = torch.randn(n, device="cuda", generator=g)
    out = net.new_params()
    for j in (8, 32, 64):
        kw = dict(matrix="gauss_newton", v0=v, breakdown_rtol=0.0)

        def run(steps, reorth):
            return lambda: net.lanczos(P, X, Y, steps=steps, check=steps, reorth=reorth, **kw)

        t = alternate({"full_short": run(j, True), "full_long": run(j + 1, True), "three_short": run(j, False),
                       "three_long": run(j + 1, False), "gnvp": lambda: net.gnvp(P, v, X, Y, out=out)}, a)
        full = [l - s for l, s in zip(t["full_long"], t["full_short"])]
        three = [l - s for l, s in zip(t["three_long"], t["three_short"])]
        floats = 4 * (j + 1) + 2 * -(-(j + 1) // 8) + 6
        sweep_ms = float(np.median(full)) - float(np.median(three))
        gbs = (floats - 9) * n * 4 / (sweep_ms * 1e-3) / 1e9
        print(json.dumps({"bench": "lanczos_sweeps", "n": n, "basis_rows": j + 1, "repeats": a.repeats,
                          "us": {"full_step_j": stats_us(full), "three_vector_step_j": stats_us(three),
                                 "gnvp": stats_us(t["gnvp"])},
                          "bytes_full_step": floats * n * 4, "bytes_three_vector_step": 9 * n * 4,
                          "basis_bytes": (j + 1) * n * 4,
                          "basis_fits_256MB_cache": bool((j + 1) * n * 4 <= 256 * 2 ** 20),
                          "sweeps_GBs": round(gbs, 1), "share_of_peak": round(gbs / PEAK_GBS, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--parts", type=str, default="step,sweeps")
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lanczos.py needs a GPU")
    ctx = pkg.Context(0)
    parts = a.parts.split(",")
    if "step" in parts:
        bench_step(pkg, ctx, a)
    if "sweeps" in parts:
        bench_sweeps(pkg, ctx, a)


if __name__ == "__main__":
    main()
