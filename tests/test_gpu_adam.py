"""Adam on the GPU: the sweep (adam.hip) bit for bit against a numpy fp32 restatement on every route it takes, the
solver against the fp64 reference of ref_adam.py on the cases and settings test_ref_adam.py admits, the bitwise
equalities of the resumable form, two ranks, and the C++ classes through drivers/adam_hip.cpp.

Error metric of a trajectory: E = max |w - w64| / max |w64 - w0|, bounded by max(1e-4, 3 x E of the fp32 restatement)
(ref_adam.reference; at most 1e-3 by test_ref_adam.py). The first trace entry is a plain evaluation at w0 and is held
to the suite's 1e-5 loss tolerance; the other entries to the same max(1e-4, 3 x fp32) convention on their relative
error."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_adam
import ref_mlp
from gpu_helpers import dev, make_net, run_ranks, solver_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------- the sweep
SIZES = [1, 3, 255, 256, 257, 1023, 4099, 100003]
ALIGN = {"aligned": (0, 0, 0, 0), "all_off_by_one": (1, 1, 1, 1), "w_off_by_one": (0, 0, 0, 1)}   # g, m, v, w


def step_ref32(w, m, v, g, k, gg):
    """The sweep in numpy fp32: every operation one correctly rounded fp32 operation, in the kernel's order."""
    c = f32(1.0)
    if gg is not None and k["clip"] > 0:
        nrm = np.sqrt(f32(gg))
        if nrm > k["clip"]:
            c = k["clip"] / nrm
    gi = g * c
    m = k["b1"] * m + k["a1"] * gi
    v = k["b2"] * v + k["a2"] * (gi * gi)
    w = w * k["decay"] - k["step"] * (m / (np.sqrt(v) * k["rbc2"] + k["eps"]))
    return w, m, v


def log_uniform(rng, n, lo, hi, zeros=0.1, signed=True):
    """Exactly zero (a fraction `zeros`) or lo <= |x| <= hi, log-uniform, as fp32."""
    x = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)
    if signed:
        x *= rng.choice([-1.0, 1.0], n)
    x[rng.random(n) < zeros] = 0.0
    x = x.astype(f32)
    assert np.all((x == 0) | ((np.abs(x) >= f32(lo) * f32(0.999)) & (np.abs(x) <= f32(hi) * f32(1.001))))
    return x


def offset_view(a, off):
    """A device copy of `a` that starts `off` floats past a 256-byte boundary."""
    base = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 256 == 0
    view = base[off:off + a.size]
    view.copy_(torch.from_numpy(a))
    return base, view


@pytest.mark.parametrize("align", list(ALIGN))
@pytest.mark.parametrize("n", SIZES)
def test_sweep_bitwise(ctx, pkg, n, align):
    rng = np.random.default_rng(7 * n + len(align))
    g = log_uniform(rng, n, 1e-15, 1e3)
    m = log_uniform(rng, n, 1e-10, 1e1)
    v = log_uniform(rng, n, 1e-20, 1e2, signed=False)
    w = log_uniform(rng, n, 1e-6, 1e1, zeros=0.02)
    gg = float(np.sum(g.astype(np.float64) ** 2))
    nrm = float(np.sqrt(f32(gg)))
    # step 3 of an AdamW run; the clip at half the norm keeps c g at or above 5e-16: no subnormal square
    modes = {"gg_null": (0.5 * nrm, None), "clip_off": (0.0, gg), "clip_inactive": (2.0 * nrm + 1.0, gg),
             "clip_active": (0.5 * nrm + 1e-30, gg)}
    for mode, (clip, use_gg) in modes.items():
        p = pkg.adam_params(lr=3e-3, weight_decay=1e-2, clip_norm=clip)
        coef = pkg.adam_coefs(p, 3e-3, 3)
        k = {name: f32(getattr(coef, name)) for name, _ in pkg._lib.AdamCoef._fields_}
        want = step_ref32(w, m, v, g, k, use_gg)
        if g.any():   # the mode is what its name says
            assert (use_gg is not None and 0 < k["clip"] < np.sqrt(f32(gg))) == (mode == "clip_active")
        outs = []
        for _ in range(2):   # a second call on the same inputs gives equal bits
            keep, (dg, dm, dv, dw) = zip(*[offset_view(a, o) for a, o in zip((g, m, v, w), ALIGN[align])])
            dgg = torch.tensor([use_gg], dtype=torch.float64, device="cuda") if use_gg is not None else None
            ctx.adam_step(dw, dm, dv, dg, coef, dgg)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy() for t in (dw, dm, dv)])
            assert np.array_equal(bits(dg), bits(g))   # the gradient is read only
            for b, o, a in zip(keep, ALIGN[align], (g, m, v, w)):   # nothing outside [off, off + n) was written
                hb = b.cpu().numpy()
                assert not hb[:o].any() and not hb[o + a.size:].any()
        for name, got, again, ref in zip("wmv", outs[0], outs[1], want):
            assert np.array_equal(bits(got), bits(again)), (mode, name)
            bad = np.flatnonzero(bits(got) != bits(ref))
            assert bad.size == 0, (mode, name, bad[:5], got[bad[:5]], ref[bad[:5]])


def test_sweep_zero_state_leaves_decayed_weights(ctx, pkg):
    n = 1023
    w = log_uniform(np.random.default_rng(1), n, 1e-6, 1e1, zeros=0.0)
    coef = pkg.adam_coefs(pkg.adam_params(lr=1e-2, weight_decay=0.1), 1e-2, 1)
    dw, z = dev(w), [torch.zeros(n, device="cuda") for _ in range(3)]
    ctx.adam_step(dw, z[0], z[1], z[2], coef)
    assert np.array_equal(bits(dw), bits(w * f32(coef.decay)))   # w decay exactly: the update term is +0
    assert f32(coef.decay) == f32(1.0 - 1e-2 * 0.1) and not any(t.any() for t in z)


def test_mlp_adam_step_checks_the_length(ctx, pkg):
    c = ref_mlp.make_case(pkg, ref_mlp.NETS, "n387")
    net = make_net(pkg, ctx, c)
    P = dev(c["P"])
    coef = pkg.adam_coefs(pkg.adam_params(), 1e-3, 1)
    g = dev(c["b"])
    m, v = torch.zeros_like(P), torch.zeros_like(P)
    want = step_ref32(c["P"], np.zeros_like(c["P"]), np.zeros_like(c["P"]), c["b"],
                      {name: f32(getattr(coef, name)) for name, _ in pkg._lib.AdamCoef._fields_}, None)
    net.adam_step(P, m, v, g, coef)
    assert np.array_equal(bits(P), bits(want[0]))
    with pytest.raises(pkg.LbfError):
        net.adam_step(P[:-1], m, v, g, coef)
    with pytest.raises(pkg.LbfError):
        net.adam_step(P, m[:-1], v, g, coef)


# ---------------------------------------------------------------- the solver against fp64
def solve(pkg, ctx, r, **over):
    c, kw = r["case"], dict(r["kw"])
    l2 = kw.pop("l2", 0.0)
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    args = dict(max_epochs=ref_adam.EPOCHS, batch=ref_adam.BATCH, seed=ref_adam.SEED, tol=0.0)
    args.update(kw)
    args.update(over)
    hist, info, trace = pkg.adam_solve(net, P, X, Y, **args)
    return P, hist, info, trace


_runs = {}


def solved(pkg, ctx, name, setting):
    if (name, setting) not in _runs:
        _runs[(name, setting)] = solve(pkg, ctx, ref_adam.reference(pkg, name, setting))
    return _runs[(name, setting)]


@pytest.mark.parametrize("setting", list(ref_adam.SETTINGS))
@pytest.mark.parametrize("name", ref_adam.CASES)
def test_solver_against_fp64(ctx, pkg, name, setting):
    r = ref_adam.reference(pkg, name, setting)
    assert r["E32"] <= ref_adam.E_MAX   # the condition under which the case is used
    P, hist, info, trace = solved(pkg, ctx, name, setting)
    c = r["case"]
    N = len(c["rows"])
    E = ref_adam.travelled_error(P.cpu().numpy(), r["w64"], c["P"])
    first = abs(trace[0] - r["trace64"][0]) / abs(r["trace64"][0])
    T = ref_adam.trace_error(trace, r["trace64"])
    print(f"{name} {setting}: E {E:.2e} (fp32 {r['E32']:.2e}, bound {r['bound']:.1e}); trace first {first:.2e}, "
          f"rest {T:.2e} (fp32 {r['T32']:.2e}, bound {r['trace_bound']:.1e})")
    assert len(trace) == len(r["trace64"]) == ref_adam.EPOCHS * -(-N // ref_adam.BATCH)
    assert E <= r["bound"]
    assert first <= 1e-5
    assert T <= r["trace_bound"]
    # records and info as lbf_sgd_solve: the start row and one full-batch row per epoch
    assert info.iterations == len(hist["loss"]) == ref_adam.EPOCHS + 1
    # the rows are full-batch evaluations at the solver's own points: the suite's loss and gradient tolerances
    l2 = r["kw"].get("l2", 0.0)
    f0, _ = ref_mlp.loss_grad(c["dims"], c["acts"], c["loss"], c["P"], c["X"], c["Y"], 1.0 / N, l2)
    fN, gN = ref_mlp.loss_grad(c["dims"], c["acts"], c["loss"], P.cpu().numpy(), c["X"], c["Y"], 1.0 / N, l2)
    assert abs(hist["loss"][0] - f0) <= 1e-5 * abs(f0)
    assert abs(hist["loss"][-1] - fN) <= 1e-5 * abs(fN)
    assert float(f32(info.final_loss)) == hist["loss"][-1]   # the row holds it through float, like SGD's
    assert abs(hist["grad_norm"][-1] - np.linalg.norm(gN)) <= 1e-4 * np.linalg.norm(gN)
    assert info.n_evals == len(trace) + ref_adam.EPOCHS + 1


@pytest.mark.parametrize("name", ref_adam.CASES)
def test_shuffle_changes_the_batches(ctx, pkg, name):
    a, b = solved(pkg, ctx, name, "defaults")[3], solved(pkg, ctx, name, "noshuffle")[3]
    assert len(a) == len(b) and not np.array_equal(a, b)


# ---------------------------------------------------------------- bitwise equalities
def test_two_solves_equal_bits(ctx, pkg):
    r = ref_adam.reference(pkg, "xent10", "adamw_clip")
    a, b = solve(pkg, ctx, r), solve(pkg, ctx, r)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[3]), bits(b[3]))
    assert np.array_equal(bits(a[1]["loss"]), bits(b[1]["loss"]))
    assert np.array_equal(bits(a[0]), bits(solved(pkg, ctx, "xent10", "adamw_clip")[0]))


@pytest.mark.parametrize("name", ["n387", "xent10"])
def test_chunked_run_equals_solve(ctx, pkg, name):
    r = ref_adam.reference(pkg, name, "adamw_clip")
    P1, hist, info, trace = solved(pkg, ctx, name, "adamw_clip")
    c, kw = r["case"], dict(r["kw"])
    net = make_net(pkg, ctx, c, l2=kw.pop("l2", 0.0))
    P, X, Y = solver_inputs(c)
    run = pkg.AdamRun(net, P, X, Y, max_epochs=ref_adam.EPOCHS, batch=ref_adam.BATCH, seed=ref_adam.SEED, tol=0.0, **kw)
    for e in range(ref_adam.EPOCHS):
        assert run.iterate(1).iterations == e + 1
    run.close()
    assert np.array_equal(bits(P), bits(P1))
    assert np.array_equal(bits(run.loss_trace()), bits(trace))
    assert np.array_equal(bits(run.hist.as_dict()["loss"]), bits(hist["loss"]))
    assert run.info.iterations == info.iterations


def test_lr_decay_and_tolerance(ctx, pkg):
    """decay_rate / decay_step as lbf_sgd_params: the recorded rate halves from epoch 2 on; a huge tolerance stops
    after the second epoch, which gets no row."""
    r = ref_adam.reference(pkg, "n387", "defaults")
    _, hist, info, _ = solve(pkg, ctx, r, max_epochs=4, decay_rate=0.5, decay_step=2)
    assert list(hist["alpha"]) == [1e-3, 1e-3, 1e-3, 5e-4, 5e-4]
    _, hist, info, trace = solve(pkg, ctx, r, max_epochs=5, tol=1e9)
    assert info.iterations == len(hist["loss"]) == 2 and len(trace) == 2 * 3


def test_unified_adam_monitored_equals_plain(ctx, pkg, tmp_path, monkeypatch):
    """UnifiedAdam with eval_every = 1 runs through AdamRun and evaluates between the epochs on a network of its own:
    the parameters are bitwise those of the run without evaluations."""
    monkeypatch.chdir(tmp_path)
    Xa, Ya = pkg.synth_mnist(330)
    L = pkg.UnifiedLauncher(0)
    L.addLayer(784, 32, "relu")
    L.addLayer(32, 10, "linear")
    L.setLoss("softmax_xent")
    L.buildNetwork()
    L.setData(pkg.UnifiedDataset(train_x=Xa[:257], train_y=Ya[:257], test_x=Xa[257:], test_y=Ya[257:]))
    out = {}
    for every in (0, 1):
        opt = pkg.UnifiedAdam()
        cfg = pkg.UnifiedConfig(name=f"adam{every}", max_iters=3, batch_size=64, learning_rate=2e-3, weight_decay=1e-2,
                                clip_norm=1.0, eval_every=every, restore_best=False, write_csv=False)
        L.train(opt, cfg)
        out[every] = (L.getWrapper().params.clone(), opt)
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))
    assert np.array_equal(bits(out[0][1].trace), bits(out[1][1].trace)) and len(out[0][1].trace) == 3 * 5
    assert [e[0] for e in out[1][1].validation] == [0, 1, 2, 3]
    assert np.array_equal(bits(out[0][1].history["loss"]), bits(out[1][1].history["loss"]))
    with pytest.raises(pkg.LbfError):
        L.train(pkg.UnifiedSGD(), pkg.UnifiedConfig(eval_every=1, write_csv=False))


# ---------------------------------------------------------------- two ranks
@pytest.mark.parametrize("name,setting", [("xent10", "adamw_clip"), ("n387", "defaults"), ("xent10", "noshuffle")])
def test_two_ranks(ctx, pkg, name, setting):
    """Every rank holds all rows and takes its slice of every batch (the sliced S-LBFGS split: positions
    [rows r / 2, rows (r + 1) / 2)). N = 257 ends every epoch with a one-row batch, which that split gives to rank 1:
    rank 0's slice of it is empty."""
    r = ref_adam.reference(pkg, name, setting)
    c = r["case"]
    N = len(c["rows"])

    def body(rank, rctx):
        P, hist, info, trace = solve(pkg, rctx, r)
        return P.cpu().numpy(), hist, trace, int(info.n_rows), int(info.iterations)

    (P0, h0, t0, rows0, it0), (P1, h1, t1, rows1, it1) = run_ranks(pkg, 2, body)
    assert np.array_equal(bits(P0), bits(P1)) and np.array_equal(bits(t0), bits(t1))
    assert np.array_equal(bits(h0["loss"]), bits(h1["loss"])) and it0 == it1 == ref_adam.EPOCHS + 1
    single = solved(pkg, ctx, name, setting)
    E = ref_adam.travelled_error(P0, r["w64"], c["P"])
    Es = ref_adam.travelled_error(P0, single[0].cpu().numpy().astype(np.float64), c["P"])
    T = ref_adam.trace_error(t0, r["trace64"])
    print(f"{name} {setting} world 2: E {E:.2e} against fp64, {Es:.2e} against one rank, trace {T:.2e}")
    assert E <= r["bound"] and Es <= r["bound"] and T <= r["trace_bound"]
    # the rows each rank evaluated: its slice of every batch, and its shard of the four full-batch rows
    sizes = [min(ref_adam.BATCH, N - r0) for r0 in range(0, N, ref_adam.BATCH)]
    per_epoch = [sum(s * (k + 1) // 2 - s * k // 2 for s in sizes) for k in (0, 1)]
    shard = [N * (k + 1) // 2 - N * k // 2 for k in (0, 1)]
    want = [ref_adam.EPOCHS * per_epoch[k] + (ref_adam.EPOCHS + 1) * shard[k] for k in (0, 1)]
    assert [rows0, rows1] == want
    if N == 257:
        assert sizes[-1] == 1 and per_epoch == [128, 129]   # the one-row batch: nothing for rank 0


# ---------------------------------------------------------------- the C++ classes
EXE = os.path.join(ROOT, "lbfgs-ffnn_amd", "build", "adam_hip")


def test_cxx_driver_matches_ctypes_bitwise(ctx, pkg, tmp_path):
    """drivers/adam_hip.cpp (HipAdam, then UnifiedAdam_HIP through the launcher) in one child process, then the same
    two runs through the ctypes path; the values restate the driver's."""
    c = ref_mlp.make_case(pkg, ref_mlp.NETS, "xent10")
    c["X"].tofile(str(tmp_path / "X.f32"))
    c["Y"].tofile(str(tmp_path / "Y.f32"))
    r = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "[RESULT] ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = lambda n, t: np.fromfile(str(tmp_path / n), dtype=t)  # noqa: E731
    X, Y = dev(c["X"]), dev(c["Y"])

    net = pkg.Mlp(ctx, c["dims"], c["acts"], loss="softmax_xent", l2=1e-3)
    P = net.init_params(seed=19, mode="cuda")
    hist, info, trace = pkg.adam_solve(net, P, X, Y, lr=2e-3, weight_decay=1e-2, clip_norm=0.5, batch=16, seed=7,
                                       max_epochs=3, tol=0.0)
    assert int(open(str(tmp_path / "iterations.txt")).read()) == info.iterations == 4
    assert np.array_equal(bits(got("loss.f64", np.float64)), bits(hist["loss"]))
    assert np.array_equal(bits(got("trace.f64", np.float64)), bits(trace)) and len(trace) == 3 * 17
    assert np.array_equal(bits(got("params.f32", np.float32)), bits(P))

    net = pkg.Mlp(ctx, c["dims"], c["acts"], loss="softmax_xent")
    P = net.init_params(seed=5, mode="cuda")
    hist, info, trace = pkg.adam_solve(net, P, X, Y, lr=1e-3, batch=32, seed=5, max_epochs=2)
    assert np.array_equal(bits(got("u_loss.f64", np.float64)), bits(hist["loss"])) and len(hist["loss"]) == 3
    assert np.array_equal(bits(got("u_trace.f64", np.float64)), bits(trace)) and len(trace) == 2 * 9
    assert np.array_equal(bits(got("u_params.f32", np.float32)), bits(P))
