"""bench.py's rank function on the GPU, in process, on a small sample: what a plain run and a --full run
put on the result line, and what --dump-outputs writes.

The inputs are seeded (synthetic rows, seed 123; parameter init, seed 123) and every reduction in the
engine has a fixed order, so two runs with the same arguments write bitwise equal arrays; --full adds
events around launches and changes no arithmetic, so it writes the same arrays too.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["accepted", "alpha", "grad_norm", "loss", "ls_trials", "params"]
MOVED = ("roofline", "kernel_ms_per_step", "cpu_baseline")


def run(pkg, monkeypatch, out, *extra):
    lines = []
    monkeypatch.setattr(bench, "emit", lines.append)
    a = bench.parse(["--samples", "2000", "--steps", "6", "--warmup", "2", "--device-warmup", "0",
                     "--dump-outputs", str(out), *extra])
    bench.run_rank(a, 1, 0, 0, pkg)
    assert len(lines) == 1
    assert sorted(os.listdir(out)) == [n + ".npy" for n in NAMES]
    return lines[0], {n: np.load(os.path.join(out, n + ".npy")) for n in NAMES}


def check_line(line, steps, warmup=2):
    assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert np.isfinite(line["value"]) and line["value"] > 0
    # ms_per_step is the time of one timed step: value steps per second
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) <= 1e-2


def test_lbfgs_outputs(pkg, ctx, monkeypatch, tmp_path):
    line, a = run(pkg, monkeypatch, tmp_path / "a")
    check_line(line, 6)
    assert line["unit"] == "iters/s" and not any(k in line for k in MOVED)
    n_params = 785 * 128 + 129 * 10
    assert a["params"].dtype == np.float32 and a["params"].shape == (n_params,)
    for n in NAMES[:-1]:
        assert a[n].dtype == np.float64 and a[n].shape == (6,)
    assert all(np.isfinite(v).all() for v in a.values())
    assert a["loss"][-1] < a["loss"][0]

    _, b = run(pkg, monkeypatch, tmp_path / "b")
    full, c = run(pkg, monkeypatch, tmp_path / "c", "--full", "--no-cpu-baseline")
    check_line(full, 6)
    assert full["roofline"]["kernel"].startswith("gemm_") and full["kernel_ms_per_step"]
    assert "cpu_baseline" not in full
    for n in NAMES:
        print(f"{n}: max |a - b| {np.abs(a[n] - b[n]).max():.3e}, max |a - full| {np.abs(a[n] - c[n]).max():.3e}")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
        assert np.array_equal(a[n], c[n]), n


def test_slbfgs_outputs(pkg, ctx, monkeypatch, tmp_path):
    line, a = run(pkg, monkeypatch, tmp_path / "a", "--solver", "slbfgs", "--steps", "2", "--warmup", "1")
    check_line(line, 2, warmup=1)
    assert line["unit"] == "epochs/s" and not any(k in line for k in MOVED)
    assert a["params"].shape == (785 * 512 + 513 * 256 + 257 * 10,) and a["loss"].shape == (2,)
    assert all(np.isfinite(v).all() for v in a.values())
    full, c = run(pkg, monkeypatch, tmp_path / "c", "--solver", "slbfgs", "--steps", "2", "--warmup", "1", "--full",
                  "--no-cpu-baseline")
    check_line(full, 2, warmup=1)
    assert full["roofline"]["kernel"].startswith("gemm_") and full["kernel_ms_per_step"]
    for n in NAMES:
        print(f"{n}: max |a - full| {np.abs(a[n] - c[n]).max():.3e}")
    for n in NAMES:
        assert np.array_equal(a[n], c[n]), n
