"""Evaluation microbenchmark: the device-side Mlp.evaluate (forward + csrc/metrics.hip, one small read-back)
against the host route it complements (Mlp.forward, all N x Out outputs copied to the host, numpy metrics as in
UnifiedLauncher.evaluate), on the classifier shapes of BASELINE.md.

Per shape, after a warm-up, the median of --repeats calls of
  evaluate      Mlp.evaluate(P, X, Y): loss, correct, top-k on the device          (HIP events around the call)
  evaluate_conf the same with the confusion matrix
  metrics       the metrics kernel alone (lbf_prof_* section "metrics[0]": HIP events around its launch)
  host_route    Mlp.forward + .cpu() + the numpy loss / argmax of unified.py's evaluate()   (host clock: its
                numpy part runs on the host; the forward ends in the copy's synchronise)
and the ratio host_route / evaluate. The metrics kernel's bytes are N * Out * 8 (outputs and targets read once)
beside the HBM peak; it is latency-bound at these sizes.

    python bench_eval.py [--repeats 30] [--warmup 5]
Prints one JSON line per shape.
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
SHAPES = [([784, 128, 10], ["relu", "linear"], 10000), ([784, 128, 10], ["relu", "linear"], 60000),
          ([784, 512, 256, 10], ["relu", "relu", "linear"], 10000)]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_route(net, P, X, y64, xent):
    """unified.py UnifiedLauncher.evaluate: forward on the device, everything else on the host."""
    out = net.forward(P, X).double().cpu().numpy()
    if xent:
        m = out.max(1, keepdims=True)
        lse = m + np.log(np.exp(out - m).sum(1, keepdims=True))
        loss = float((y64 * (lse - out)).sum(1).mean())
    else:
        loss = float(((out - y64) ** 2).mean())
    acc = float((out.argmax(1) == y64.argmax(1)).mean())
    return loss, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loss", type=str, default="softmax_xent")
    a = ap.parse_args()
    if a.repeats < 20:
        raise SystemExit("--repeats: at least 20")
    pkg = __graft_entry__.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU")
    ctx = pkg.Context(0)
    xent = a.loss == "softmax_xent"
    for dims, acts, N in SHAPES:
        net = pkg.Mlp(ctx, dims, acts, loss=a.loss)
        P = net.init_params(123, "cpu")
        Xh, Yh = pkg.synth_mnist(N)
        X, Y = torch.from_numpy(Xh).cuda(), torch.from_numpy(Yh).cuda()
        y64 = Yh.astype(np.float64)
        Out = dims[-1]
        ev = lambda: net.evaluate(P, X, Y, k=2)  # noqa: E731
        evc = lambda: net.evaluate(P, X, Y, k=2, confusion=True)  # noqa: E731
        hr = lambda: host_route(net, P, X, y64, xent)  # noqa: E731
        for _ in range(a.warmup):
            ev(), evc(), hr()
        t_ev, t_evc, t_hr, t_ev_host = [], [], [], []
        for _ in range(a.repeats):   # alternating, so a drift of the box hits every variant alike
            t_ev.append(event_ms(ev))
            t_evc.append(event_ms(evc))
            t_hr.append(host_ms(hr))
            t_ev_host.append(host_ms(ev))
        # the metrics kernel alone: per-launch differences of the profiler's running total
        ctx.prof_select("metrics[0]")
        ctx.prof_sample(1)
        ctx.prof_enable(True)
        t_k, last = [], 0.0
        for _ in range(a.repeats):
            ev()
            tot = ctx.prof_read().get("metrics[0]", (0.0, 0))[0]
            t_k.append(tot - last)
            last = tot
        ctx.prof_enable(False)
        ctx.prof_select(None)
        r = ev()
        loss_h, acc_h = host_route(net, P, X, y64, xent)
        med = lambda v: float(np.median(v))  # noqa: E731
        k_ms = med(t_k)
        bytes_k = N * Out * 8
        out = {
            "bench": "eval", "dims": dims, "rows": N, "loss": a.loss, "repeats": a.repeats,
            "evaluate_us": round(med(t_ev) * 1e3, 1), "evaluate_host_clock_us": round(med(t_ev_host) * 1e3, 1),
            "evaluate_conf_us": round(med(t_evc) * 1e3, 1), "metrics_kernel_us": round(k_ms * 1e3, 2),
            "host_route_us": round(med(t_hr) * 1e3, 1),
            "ratio_host_over_device": round(med(t_hr) / med(t_ev_host), 2),
            "spread_evaluate_us": [round(min(t_ev) * 1e3, 1), round(max(t_ev) * 1e3, 1)],
            "spread_host_route_us": [round(min(t_hr) * 1e3, 1), round(max(t_hr) * 1e3, 1)],
            "metrics_bytes": bytes_k, "metrics_GBs": round(bytes_k / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None,
            "hbm_peak_GBs": HBM_PEAK_GBS,
            "check": {"accuracy_device": r.accuracy, "accuracy_host": acc_h, "loss_device": r.loss, "loss_host": loss_h},
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
