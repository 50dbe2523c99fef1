"""The C++ drop-in header on the real kernels: lbfgs-ffnn_amd/drivers/parity_hip.cpp runs every solver class of
include/lbfgs_amd/hip_backend.hpp once (one child process, started by the module's fixture) and dumps what came
out; each test repeats one case through the ctypes wrappers and compares.

  * bit for bit: final parameters, loss and gradient-norm histories, iteration and row counts, evaluation counts,
    confusion matrix, predictions, OWL-QN stats. Same library, same kernels; the suite already asserts bitwise
    repeatability across networks, calls and processes (test_gpu_reuse.py, test_gpu_slbfgs_run.py,
    test_gpu_rccl_procs.py). Two roundings are the C++ contract and are mirrored here: HipMinimizerBase keeps tol,
    c1 and rho as float (F32 below), and a LossGradFun returns a float loss.
  * an fp64 anchor that does not pass through the ctypes path: a recorder row against the objective in torch fp64
    at the point that row belongs to. HF, OWL-QN and SGD record an iteration's start point, so row 0 is the
    objective at the initial parameters (pkg.init_params_host); L-BFGS, GD, S-LBFGS and SGD record after the step
    (the epoch), like the reference's recorders, so their last row is the objective at the dumped final
    parameters (S-LBFGS: lambda = 1e-4 included). lastTrain() / lastTest() and EvalResult.loss against fp64 at
    the dumped final parameters. LOSS_RTOL is the suite's bound for one loss
    evaluation against fp64; the counts are exact on the rows whose fp64 top-two gap clears GAP, the bound of
    test_gpu_eval.py, and at most 1 % of the rows may miss it.
  * sensitivity: for every config field or setter that is live in a case, the same Python run with that one field
    at the library default gives other final parameters, so a field the header dropped would break the bitwise
    match. A run ends either at its tolerance or at max_iters, so each of the two is live in some cases only:
    the tolerance ends lbfgs_wolfe and hiphf, max_iters the others.

The values of every case restate those in parity_hip.cpp.
"""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from ref_mlp import XENT, bias_mask, net_out, nparams, objective

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lbfgs-ffnn_amd", "build", "parity_hip")
LOSS_RTOL = 1e-5      # test_gpu_xent.py::check_loss_grad, test_loss_grad_matches_oracle in test_gpu_parity.py
GAP = 1e-4            # test_gpu_eval.py::check_against_oracle: gap >= 1e-4 max(1, |out|max) is clear of the fp32 forward
SLBFGS_LAMBDA = 1e-4  # lbf_slbfgs_params.lambda, which the header leaves at the library's default


def F32(v):
    """What a float member of HipMinimizerBase hands the engine."""
    return float(np.float32(v))


class Problem:
    def __init__(self, tag, dims, acts, loss, n_train, n_test, rng):
        self.tag, self.dims, self.acts, self.loss = tag, dims, acts, loss
        n = n_train + n_test
        X = rng.standard_normal((n, dims[0])).astype(np.float32)
        teacher = rng.standard_normal((dims[0], dims[-1]))
        Y = np.zeros((n, dims[-1]), np.float32)
        Y[np.arange(n), np.argmax(X.astype(np.float64) @ teacher, 1)] = 1.0  # one-hot, learnable
        self.X = {"train": X[:n_train], "test": X[n_train:]}
        self.Y = {"train": Y[:n_train], "test": Y[n_train:]}
        self.nparams = nparams(dims)

    def write(self, d):
        for split in ("train", "test"):
            self.X[split].tofile(os.path.join(d, f"{self.tag}_X_{split}.f32"))
            self.Y[split].tofile(os.path.join(d, f"{self.tag}_Y_{split}.f32"))

    def weights_mask(self):
        return ~bias_mask(self.dims)


def problems():
    rng = np.random.default_rng(20261)
    p1 = Problem("p1", [20, 16, 3], ["tanh", "linear"], "mse", 37, 19, rng)
    p2 = Problem("p2", [64, 32, 10], ["relu", "linear"], XENT, 257, 63, rng)
    return p1, p2


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    """Writes the inputs and runs the driver once, as a fresh child process. Every test depends on it: after an
    abnormal exit none of them starts GPU work of its own."""
    d = str(tmp_path_factory.mktemp("dropin_parity"))
    p1, p2 = problems()
    p1.write(d)
    p2.write(d)
    r = subprocess.run([EXE, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "[RESULT] ok" in r.stdout, r.stdout[-3000:]
    return types.SimpleNamespace(dir=d, p1=p1, p2=p2)


@pytest.fixture(scope="module")
def gpu(drv, ctx):
    """The device copies of the two problems (after the driver has exited)."""
    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for p in (drv.p1, drv.p2):
        p.dX = {s: dev(p.X[s]) for s in p.X}
        p.dY = {s: dev(p.Y[s]) for s in p.Y}
    return drv


# ---- what the driver wrote ------------------------------------------------------------------------------------

def raw(drv, name, dtype):
    return np.fromfile(os.path.join(drv.dir, name), dtype=dtype)


def txt(drv, case):
    out = {}
    with open(os.path.join(drv.dir, case + ".txt")) as f:
        for line in f:
            k, v = line.split()
            out[k] = float.fromhex(v) if ("x" in v or "nan" in v or "inf" in v) else int(v)
    return out


def dumped(drv, case):
    return types.SimpleNamespace(params=raw(drv, case + ".params.f32", np.float32),
                                 loss=raw(drv, case + ".loss.f64", np.float64),
                                 gnorm=raw(drv, case + ".gnorm.f64", np.float64),
                                 time=raw(drv, case + ".time.f64", np.float64), txt=txt(drv, case))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def fbits(v):
    return np.float64(v).view(np.uint64)


# ---- fp64 references --------------------------------------------------------------------------------------------

def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def objective64(prob, P, split="train", l2=0.0, l1=0.0, l1_bias=False):
    """data loss (a mean over the rows) + 0.5 l2 |w|^2 + l1 |w|_1 over the penalised coordinates (lbfgs_amd.h)."""
    X, Y = prob.X[split], prob.Y[split]
    f = objective(prob.dims, prob.acts, prob.loss, t64(X), t64(Y), 1.0 / len(X), l2)
    v = float(f(t64(P)))
    if l1:
        w = np.asarray(P, np.float64)
        v += l1 * np.abs(w if l1_bias else w[prob.weights_mask()]).sum()
    return v


def forward64(prob, P, X):
    return net_out(prob.dims, prob.acts, t64(X))(t64(P)).numpy()


def clear_rows(z):
    s = np.sort(z, 1)
    keep = (s[:, -1] - s[:, -2]) >= GAP * np.maximum(1.0, np.abs(z).max(1))
    left_out = int((~keep).sum())
    print(f"   {left_out} of {len(z)} rows inside the fp32 forward's error")
    assert left_out <= 0.01 * len(z)
    return keep, left_out


def close(got, ref, what):
    dev = abs(got - ref) / abs(ref)
    print(f"   {what}: {got:.10g} fp64 {ref:.10g} rel {dev:.2e}")
    assert np.isfinite(got) and dev <= LOSS_RTOL, what


def check_scan_pair(prob, P, split, loss, acc, what):
    """A lastTrain() / lastTest() pair of the launcher's host scan against fp64 at P."""
    z, Y = forward64(prob, P, prob.X[split]), prob.Y[split].astype(np.float64)
    n = len(z)
    if prob.loss == XENT:
        m = z.max(1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(1, keepdims=True))
        ref = float((Y * (lse - z)).sum() / n)
    else:
        ref = float(((z - Y) ** 2).sum() / (n * prob.dims[-1]))
    close(loss, ref, what + " loss")
    keep, left_out = clear_rows(z)
    correct = acc * n / 100.0
    assert abs(correct - round(correct)) < 1e-6
    sure = int((np.argmax(z, 1) == np.argmax(Y, 1))[keep].sum())
    assert sure <= round(correct) <= sure + left_out, what


def check_launcher_pairs(prob, d, what):
    check_scan_pair(prob, d.params, "train", d.txt["train_loss"], d.txt["train_acc"], what + " lastTrain")
    check_scan_pair(prob, d.params, "test", d.txt["test_loss"], d.txt["test_acc"], what + " lastTest")


def check_history(d, hist, P, rows_key="rows"):
    """Bitwise: parameters and both histories; the time column only finite and non-decreasing."""
    assert d.txt[rows_key] == len(hist["loss"]) == len(d.loss)
    assert same_bits(d.params, P.cpu().numpy()), f"max |dP| {np.abs(d.params - P.cpu().numpy()).max():.3e}"
    assert same_bits(d.loss, hist["loss"]), (d.loss, hist["loss"])
    assert same_bits(d.gnorm, hist["grad_norm"]), (d.gnorm, hist["grad_norm"])
    assert len(d.time) == len(d.loss) and np.all(np.isfinite(d.time)) and np.all(np.diff(d.time) >= 0.0)


def check_sensitive(run, base, P_ref, fields):
    """Every field at the library default (None: the keyword left out) gives other final parameters."""
    ref = P_ref.cpu().numpy()
    for name, change in fields.items():
        P = run({**base, **change})[0].cpu().numpy()
        moved = not same_bits(P, ref)
        print(f"   without {name}: parameters {'differ' if moved else 'ARE THE SAME'}")
        assert moved, f"{name} does not reach the result: the case would not notice the header dropping it"


# ---- the Python side of each case -------------------------------------------------------------------------------

def new_net(pkg, ctx, prob, s):
    net = pkg.Mlp(ctx, prob.dims, prob.acts, loss=s.get("loss", prob.loss), l2=s.get("l2", 0.0))
    P = net.init_params(s["seed"], "cuda")  # the C++ default is LBF_INIT_CUDA
    if s.get("start") is not None:
        P.copy_(torch.from_numpy(s["start"]).cuda())
    return net, P


def solver_kw(s, drop=("seed", "loss", "l2", "start", "line_search")):
    return {k: v for k, v in s.items() if k not in drop and v is not None}


def make_run(pkg, ctx, prob, solve):
    def run(s):
        net, P = new_net(pkg, ctx, prob, s)
        out = solve(net, P, prob.dX["train"], prob.dY["train"], s)
        return (P, *out)
    return run


def test_lbfgs_armijo(gpu, pkg, ctx):
    """Case 1a: UnifiedLBFGS_HIP, Armijo, MSE, through UnifiedLauncher::train."""
    prob, d = gpu.p1, dumped(gpu, "lbfgs_armijo")
    base = dict(seed=99, line_search="armijo", m=4, max_iters=8, tol=1e-9)
    run = make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.lbfgs_solve(
        net, P, X, Y, line_search=s["line_search"], **solver_kw(s)))
    P, hist, info = run(base)
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params), "last row at the final parameters")
    check_launcher_pairs(prob, d, "lbfgs_armijo")
    check_sensitive(run, base, P, {"seed": dict(seed=123), "m_param": dict(m=None), "max_iters": dict(max_iters=None),
                                   "line_search": dict(line_search="wolfe")})


WOLFE = dict(seed=99, loss=XENT, l2=2e-3, line_search="wolfe", m=4, max_iters=60, tol=0.05)


def lbfgs_run(pkg, ctx, prob):
    return make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.lbfgs_solve(
        net, P, X, Y, line_search=s["line_search"], **solver_kw(s)))


def test_lbfgs_wolfe_xent_l2(gpu, pkg, ctx):
    """Case 1b: Wolfe on the cross-entropy loss (launcher.setLoss before buildNetwork) with config.l2; the
    tolerance ends the run before max_iters."""
    prob, d = gpu.p2, dumped(gpu, "lbfgs_wolfe")
    run = lbfgs_run(pkg, ctx, prob)
    P, hist, info = run(WOLFE)
    assert 4 < len(hist["loss"]) < WOLFE["max_iters"]  # the tolerance is live, and m_param = 4 has dropped pairs
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params, l2=2e-3), "last row at the final parameters")
    check_launcher_pairs(prob, d, "lbfgs_wolfe")
    check_sensitive(run, WOLFE, P, {"seed": dict(seed=123), "setLoss": dict(loss="mse"), "l2": dict(l2=0.0),
                                    "m_param": dict(m=None), "tolerance": dict(tol=None)})
    # On this problem every iteration's first trial passes both line searches, so the two reach the same
    # parameters (test_lbfgs_armijo is the case whose parameters depend on line_search). What a dropped
    # optimizer.line_search changes here is the record: Armijo keeps the reference's float loss.
    _, armijo, _ = run({**WOLFE, "line_search": "armijo"})
    assert not same_bits(armijo["loss"], hist["loss"])


def test_second_train_continues(gpu, pkg, ctx):
    """Case 7: reset_params = false continues from the first run's parameters, and the first run's l2 stays set
    although this config's l2 is 0 (the documented behaviour, as unified.py)."""
    prob, d, first = gpu.p2, dumped(gpu, "lbfgs_continue"), dumped(gpu, "lbfgs_wolfe")
    base = dict(seed=5, loss=XENT, l2=2e-3, line_search="wolfe", m=4, max_iters=3, tol=1e-9, start=first.params)
    run = lbfgs_run(pkg, ctx, prob)
    P, hist, info = run(base)
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params, l2=2e-3), "last row at the final parameters")
    assert d.loss[0] < first.loss[-1]  # it went on from where the first run ended
    check_launcher_pairs(prob, d, "lbfgs_continue")
    check_sensitive(run, base, P, {"reset_params": dict(start=None), "the first run's l2": dict(l2=0.0),
                                   "max_iters": dict(max_iters=None)})


def test_evaluation_of_the_trained_network(gpu, pkg, ctx):
    """Case 8: metrics(), HipNetwork::evaluate with predictions, compute_loss_and_grad, forward_only."""
    prob, t = gpu.p2, txt(gpu, "eval")
    Ph = raw(gpu, "eval.params.f32", np.float32)
    assert same_bits(Ph, dumped(gpu, "lbfgs_continue").params)  # evaluating changes nothing
    net = pkg.Mlp(ctx, prob.dims, prob.acts, loss=XENT)
    P = torch.from_numpy(Ph).cuda()
    Out = prob.dims[-1]

    def counts(key, r, k):
        assert (t[key + "_rows"], t[key + "_correct"], t[key + "_topk"], t[key + "_k"]) == (r.rows, r.correct, r.topk, k)
        assert fbits(t[key + "_loss"]) == fbits(r.loss), (t[key + "_loss"], r.loss)

    def against_fp64(key, split, k, conf, pred=None):
        z, Y = forward64(prob, Ph, prob.X[split]), prob.Y[split].astype(np.float64)
        close(t[key + "_loss"], objective64(prob, Ph, split), key + " loss")
        keep, left_out = clear_rows(z)
        tgt = np.argmax(Y, 1)
        hit = (np.argmax(z, 1) == tgt)[keep].sum()
        rank = (z > z[np.arange(len(z)), tgt][:, None]).sum(1)
        assert t[key + "_rows"] == len(z)
        assert hit <= t[key + "_correct"] <= hit + left_out
        assert (rank < k)[keep].sum() <= t[key + "_topk"] <= (rank < k)[keep].sum() + left_out
        assert conf.sum() == len(z) and np.trace(conf) == t[key + "_correct"]
        assert np.array_equal(conf.sum(1), np.bincount(tgt, minlength=Out))
        if pred is not None:
            assert np.array_equal(pred[keep], np.argmax(z, 1)[keep])

    r = net.evaluate(P, prob.dX["train"], prob.dY["train"], k=3, confusion=True)
    counts("metrics_train", r, 3)
    conf = raw(gpu, "eval.confusion_train.i64", np.int64).reshape(Out, Out)
    assert same_bits(conf, r.confusion)
    against_fp64("metrics_train", "train", 3, conf)

    r = net.evaluate(P, prob.dX["test"], prob.dY["test"], k=1)
    counts("metrics_test", r, 1)
    assert t["metrics_test_topk"] == t["metrics_test_correct"]

    r = net.evaluate(P, prob.dX["test"], prob.dY["test"], k=2, confusion=True, pred=True)
    counts("evaluate_test", r, 2)
    conf = raw(gpu, "eval.confusion_test.i64", np.int64).reshape(Out, Out)
    pred = raw(gpu, "eval.pred_test.i32", np.int32)
    assert same_bits(conf, r.confusion) and same_bits(pred, r.pred.cpu().numpy())
    against_fp64("evaluate_test", "test", 2, conf, pred)
    assert t["evaluate_test_correct"] == t["metrics_test_correct"]

    loss, g = net.loss_grad(P, prob.dX["train"], prob.dY["train"])
    assert fbits(t["loss_and_grad"]) == fbits(F32(loss))  # compute_loss_and_grad returns a float
    assert same_bits(raw(gpu, "eval.grad.f32", np.float32), g.cpu().numpy())
    close(t["loss_and_grad"], objective64(prob, Ph), "compute_loss_and_grad")
    out = net.forward(P, prob.dX["test"]).cpu().numpy()
    assert same_bits(raw(gpu, "eval.forward_test.f32", np.float32).reshape(out.shape), out)
    # the host scan and the device-side metrics see the same rows
    assert round(t["train_acc"] * len(prob.X["train"]) / 100.0) == t["metrics_train_correct"]
    assert round(t["test_acc"] * len(prob.X["test"]) / 100.0) == t["metrics_test_correct"]
    close(t["train_loss"], t["metrics_train_loss"], "host scan against the device metrics, train")
    close(t["test_loss"], t["metrics_test_loss"], "host scan against the device metrics, test")


SLBFGS = dict(seed=7, loss=XENT, M=3, L=2, b=32, b_H=20, step=0.03, max_epochs=6, tol=1e-9)


@pytest.mark.parametrize("case,mode", [("slbfgs_fd", 0), ("slbfgs_gn", 2)])
def test_slbfgs(gpu, pkg, ctx, case, mode):
    """Case 2: UnifiedSLBFGS_HIP with finite-difference and Gauss-Newton curvature pairs."""
    prob, d = gpu.p2, dumped(gpu, case)
    base = dict(SLBFGS, hvp_exact=mode)
    run = make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.slbfgs_solve(net, P, X, Y, **solver_kw(s)))
    P, hist, info = run(base)
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params, l2=SLBFGS_LAMBDA), "last row at the final parameters")
    check_launcher_pairs(prob, d, case)
    other = dumped(gpu, "slbfgs_gn" if mode == 0 else "slbfgs_fd")
    assert not same_bits(d.params, other.params)  # config.curvature reaches the solver
    fields = {"seed": dict(seed=123), "m_param": dict(M=None), "L_param": dict(L=None), "batch_size": dict(b=None),
              "b_H_param": dict(b_H=None), "learning_rate": dict(step=None)}
    if mode == 0:  # the library's 1000 epochs once only
        fields["max_iters"] = dict(max_epochs=None)
    check_sensitive(run, base, P, fields)


def test_gd_momentum_l2(gpu, pkg, ctx):
    """Case 3a: UnifiedGD_HIP."""
    prob, d = gpu.p1, dumped(gpu, "gd")
    base = dict(seed=11, l2=1e-3, lr=0.05, momentum=0.6, max_iters=7, tol=1e-9)
    run = make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.gd_solve(net, P, X, Y, **solver_kw(s)))
    P, hist, info = run(base)
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params, l2=1e-3), "last row at the final parameters")
    check_launcher_pairs(prob, d, "gd")
    check_sensitive(run, base, P, {"seed": dict(seed=123), "l2": dict(l2=0.0), "learning_rate": dict(lr=None),
                                   "momentum": dict(momentum=None), "max_iters": dict(max_iters=None)})


@pytest.mark.parametrize("case,batch", [("sgd", 64), ("sgd_b48", 48)])
def test_sgd_decay_ragged_batch(gpu, pkg, ctx, case, batch):
    """Case 3b: UnifiedSGD_HIP, 257 rows in batches of 64: a last batch of one row. The header does not pass the
    tolerance, so SGD keeps its own. 64 is also the library's default batch, so a dropped batch_size would not
    show there: the same case with batches of 48 (a last batch of 17) is the one that is sensitive to it."""
    prob, d = gpu.p2, dumped(gpu, case)
    base = dict(seed=12, loss=XENT, lr=0.02, momentum=0.5, batch=batch, decay_rate=0.7, decay_step=2, max_epochs=6)
    run = make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.sgd_solve(net, P, X, Y, **solver_kw(s)))
    P, hist, info = run(base)
    assert len(hist["loss"]) == 7  # the initial record and one per epoch
    check_history(d, hist, P)
    close(d.loss[0], objective64(prob, pkg.init_params_host(prob.dims, prob.acts, 12, "cuda")), "row 0")
    close(d.loss[-1], objective64(prob, d.params), "last row at the final parameters")
    check_launcher_pairs(prob, d, case)
    assert not same_bits(d.params, dumped(gpu, "sgd_b48" if batch == 64 else "sgd").params)
    fields = {"seed": dict(seed=123), "learning_rate": dict(lr=None), "momentum": dict(momentum=None),
              "lr_decay": dict(decay_rate=None), "lr_decay_rate": dict(decay_step=None),
              "max_iters": dict(max_epochs=None)}
    if batch != 64:
        fields["batch_size"] = dict(batch=None)
    check_sensitive(run, base, P, fields)


def hf_run(pkg, ctx, prob):
    return make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.hf_solve(net, P, X, Y, **solver_kw(s)))


def test_hf_through_the_launcher(gpu, pkg, ctx):
    """Case 4a: UnifiedHF_HIP with cg_iters, cg_rtol and damping."""
    prob, d = gpu.p2, dumped(gpu, "hf")
    base = dict(seed=13, loss=XENT, max_iters=6, tol=1e-9, cg_iters=4, cg_rtol=0.3, damping0=0.05)
    run = hf_run(pkg, ctx, prob)
    P, hist, info, traces = run(base)
    print("   CG iterations per step:", traces["cg"])
    check_history(d, hist, P)
    close(d.loss[0], objective64(prob, pkg.init_params_host(prob.dims, prob.acts, 13, "cuda")), "row 0")
    check_launcher_pairs(prob, d, "hf")
    check_sensitive(run, base, P, {"seed": dict(seed=123), "max_iters": dict(max_iters=None),
                                   "cg_iters": dict(cg_iters=None), "cg_rtol": dict(cg_rtol=None),
                                   "damping": dict(damping0=None)})


def test_hiphf_direct(gpu, pkg, ctx):
    """Case 4b: HipHF with setCG, setDamping, setCurvatureRows(16), setLineSearchParams, setTolerance and a
    recorder; the tolerance ends the run."""
    prob, d = gpu.p1, dumped(gpu, "hiphf")
    base = dict(seed=17, max_iters=12, tol=F32(0.1), cg_iters=5, cg_rtol=0.2, damping0=0.3, curv_rows=16,
                max_line_iters=6, c1=F32(0.6), rho=F32(0.4))
    run = hf_run(pkg, ctx, prob)
    P, hist, info, traces = run(base)
    print("   CG iterations per step:", traces["cg"], "trials", hist["ls_trials"], "|g|", hist["grad_norm"])
    assert d.txt["iterations"] == info.iterations
    assert 2 < info.iterations < 12  # the tolerance is live
    check_history(d, hist, P)
    close(d.loss[0], objective64(prob, pkg.init_params_host(prob.dims, prob.acts, 17, "cuda")), "row 0")
    # the members a caller leaves alone reach the engine as floats: c1 = 1e-4f, not 1e-4
    defaults = dict(max_line_iters=None, c1=F32(1e-4), rho=None)
    check_sensitive(run, base, P, {"setTolerance": dict(tol=F32(1e-6)), "setCG": dict(cg_iters=None, cg_rtol=None),
                                   "setDamping": dict(damping0=None), "setCurvatureRows": dict(curv_rows=None),
                                   "setLineSearchParams": defaults})


def owlqn_run(pkg, ctx, prob):
    return make_run(pkg, ctx, prob, lambda net, P, X, Y, s: pkg.owlqn_solve(net, P, X, Y, **solver_kw(s)))


def check_stats(d, stats):
    assert (d.txt["zeros"], d.txt["penalised"]) == (stats["zeros"], stats["penalised"])
    assert fbits(d.txt["l1_term"]) == fbits(stats["l1_term"]) and fbits(d.txt["pg_norm"]) == fbits(stats["pg_norm"])


def test_owlqn_through_the_launcher(gpu, pkg, ctx):
    """Case 5a: UnifiedOWLQN_HIP with l1 and l2, and its stats."""
    prob, d = gpu.p2, dumped(gpu, "owlqn")
    base = dict(seed=14, loss=XENT, l2=1e-3, m=2, max_iters=8, tol=1e-9, l1=2e-3)
    run = owlqn_run(pkg, ctx, prob)
    P, hist, info, stats = run(base)
    check_history(d, hist, P)
    check_stats(d, stats)
    assert d.txt["penalised"] == int(prob.weights_mask().sum())
    assert d.txt["zeros"] == int((d.params[prob.weights_mask()] == 0).sum())
    P0 = pkg.init_params_host(prob.dims, prob.acts, 14, "cuda")
    close(d.loss[0], objective64(prob, P0, l2=1e-3, l1=2e-3), "row 0")
    close(d.txt["l1_term"], 2e-3 * np.abs(d.params[prob.weights_mask()].astype(np.float64)).sum(), "l1 term")
    check_launcher_pairs(prob, d, "owlqn")
    check_sensitive(run, base, P, {"seed": dict(seed=123), "l2": dict(l2=0.0), "m_param": dict(m=None),
                                   "max_iters": dict(max_iters=None), "l1": dict(l1=None)})


def test_hipowlqn_direct(gpu, pkg, ctx):
    """Case 5b: HipOWLQN with setL1(l1, true), setHistorySize(3) and stats()."""
    prob, d = gpu.p1, dumped(gpu, "hipowlqn")
    base = dict(seed=18, m=3, max_iters=9, tol=F32(1e-9), l1=0.01, l1_bias=1, c1=F32(1e-4))
    run = owlqn_run(pkg, ctx, prob)
    P, hist, info, stats = run(base)
    assert d.txt["iterations"] == info.iterations
    check_history(d, hist, P)
    check_stats(d, stats)
    assert d.txt["penalised"] == prob.nparams  # the biases too
    assert d.txt["zeros"] == int((d.params == 0).sum())
    P0 = pkg.init_params_host(prob.dims, prob.acts, 18, "cuda")
    close(d.loss[0], objective64(prob, P0, l1=0.01, l1_bias=True), "row 0")
    check_sensitive(run, base, P, {"setL1's l1": dict(l1=None), "setL1's on_biases": dict(l1_bias=None),
                                   "setHistorySize": dict(m=None), "setMaxIterations": dict(max_iters=None)})


@pytest.mark.parametrize("ls", ["armijo", "wolfe"])
def test_hiplbfgs_on_a_network_callback(gpu, pkg, ctx, ls):
    """Case 6: HipLBFGS::solve with a LossGradFun that evaluates a HipNetwork at the trial point it is given."""
    prob, d = gpu.p1, dumped(gpu, "hiplbfgs_" + ls)
    X, Y = prob.dX["train"], prob.dY["train"]
    base = dict(seed=19, m=5, max_iters=8, tol=F32(1e-9))
    if ls == "armijo":  # setLineSearchParams is read under Armijo only; Wolfe keeps the library's values
        base.update(max_line_iters=7, c1=F32(0.5), rho=F32(0.4))

    def run(s):
        net, P = new_net(pkg, ctx, prob, s)

        def fn(p, g):
            loss, _ = net.loss_grad(p, X, Y, grad=g)
            return F32(loss)  # a LossGradFun returns a float
        return (P, *pkg.lbfgs_solve_fn(ctx, P, fn, line_search=ls, **solver_kw(s)))

    P, hist, info = run(base)
    assert d.txt["iterations"] == info.iterations
    check_history(d, hist, P)
    close(d.loss[-1], objective64(prob, d.params), "last row at the final parameters")
    other = dumped(gpu, "hiplbfgs_" + ("wolfe" if ls == "armijo" else "armijo"))
    assert not same_bits(d.params, other.params)  # setLineSearch reaches the solver
    fields = {"setMemory": dict(m=None), "setMaxIterations": dict(max_iters=None)}
    if ls == "armijo":
        fields["setLineSearchParams"] = dict(max_line_iters=None, c1=F32(1e-4), rho=None)
    check_sensitive(run, base, P, fields)
