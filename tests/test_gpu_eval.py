"""Device-side evaluation (lbf_mlp_evaluate / Mlp.evaluate, csrc/metrics.hip) and validation-monitored training.

Counts, predictions and the confusion matrix are checked for integer equality against numpy applied to the
device's own outputs (lbf_mlp_forward, which predates the metrics kernel), with the reference's scan as the argmax
rule (unified_launcher.hpp:154-199: the lowest index wins a tie, a NaN never wins, nothing above -1e20 gives 0);
the loss and the predictions against the fp64 oracle; then chunking, the in-process rank group, the isolation from
an open solver, and the validation loop of UnifiedLauncher.train.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev, run_ranks
from ref_mlp import one_hot

pytestmark = pytest.mark.gpu

# (dims, acts, losses): every output route named in tests/test_gpu_xent.py, Out = 1, both confusion paths
NETS = [
    ([784, 128, 10], ["relu", "linear"], ("mse", "softmax_xent")),
    ([37, 50, 3], ["tanh", "linear"], ("mse", "softmax_xent")),
    ([129, 130, 65, 10], ["relu", "tanh", "linear"], ("mse", "softmax_xent")),
    ([784, 512, 256, 10], ["relu", "relu", "linear"], ("mse", "softmax_xent")),
    ([20, 300, 70], ["relu", "linear"], ("mse", "softmax_xent")),   # the wide-Out confusion path
    ([16, 100], ["linear"], ("mse", "softmax_xent")),                # a single layer
    ([64, 32, 2], ["tanh", "sigmoid"], ("mse",)),
    ([33, 8, 1], ["tanh", "linear"], ("mse",)),
]
CASES = [(d, a, l) for d, a, ls in NETS for l in ls]
CASE_IDS = ["-".join(map(str, d)) + "-" + l for d, a, l in CASES]


def soft(rng, N, Out):
    Y = rng.random((N, Out)).astype(np.float32) + 1e-3
    return (Y / Y.sum(1, keepdims=True)).astype(np.float32)


def scan_argmax(Z):
    """The reference's scan, vectorised: best = 0, m = -1e20; for o: if z_o > m take it."""
    Z = np.asarray(Z, np.float64)
    with np.errstate(invalid="ignore"):
        V = np.where(Z > -1e20, Z, -np.inf)   # NaN > x is False: a NaN never wins
    return np.where(np.isneginf(V).all(1), 0, V.argmax(1)).astype(np.int64)   # argmax: the first maximum


def ranks_of(Z, tgt):
    """rank = #{o : z_o > z_t} + #{o < t : z_o == z_t}"""
    zt = Z[np.arange(len(Z)), tgt][:, None]
    o = np.arange(Z.shape[1])[None, :]
    with np.errstate(invalid="ignore"):
        return (Z > zt).sum(1) + ((Z == zt) & (o < tgt[:, None])).sum(1)


def expected(Z, Y, ks):
    pred, tgt = scan_argmax(Z), scan_argmax(Y)
    rk = ranks_of(Z, tgt)
    conf = np.zeros((Z.shape[1], Z.shape[1]), np.int64)
    np.add.at(conf, (tgt, pred), 1)
    return pred, tgt, int((pred == tgt).sum()), {k: int((rk < k).sum()) for k in ks}, conf


def check_exact(net, P, X, Y, idx=None):
    """Mlp.evaluate against numpy on lbf_mlp_forward's outputs of the same rows: integers, nothing excluded."""
    Out = net.dims[-1]
    rows = X if idx is None else X[idx.long()].contiguous()
    Z = net.forward(P, rows).cpu().numpy()
    Yh = (Y if idx is None else Y[idx.long()]).cpu().numpy()
    ks = sorted({1, min(2, Out), Out})
    pred, tgt, correct, topk, conf = expected(Z, Yh, ks)
    for k in ks:
        r = net.evaluate(P, X, Y, idx=idx, k=k, confusion=True, pred=True)
        assert r.rows == len(Z) and r.k == k
        assert r.correct == correct, (k, r.correct, correct)
        assert r.topk == topk[k], (k, r.topk, topk[k])
        assert np.array_equal(r.pred.cpu().numpy(), pred)
        assert np.array_equal(r.confusion, conf) and r.confusion.sum() == len(Z)
        assert r.accuracy == correct / len(Z)
    assert topk[1] == correct and topk[Out] == len(Z)   # finite outputs: k = 1 is `correct`, k = Out is every row
    # predictions only: no targets, the same classes, zero loss and counts
    r = net.evaluate(P, X, None, idx=idx, pred=True)
    assert np.array_equal(r.pred.cpu().numpy(), pred) and (r.loss, r.correct, r.topk, r.rows) == (0.0, 0, 0, len(Z))


@pytest.mark.parametrize("dims,acts,loss", CASES, ids=CASE_IDS)
def test_counts_equal_numpy_on_device_outputs(ctx, pkg, dims, acts, loss):
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    Out = dims[-1]
    for N in (1, 63, 257, 1000):
        rng = np.random.default_rng(1000 + N)
        X = dev(rng.standard_normal((N, dims[0])))
        for Y in (dev(one_hot(rng, N, Out)), dev(soft(rng, N, Out))):
            check_exact(net, P, X, Y)
        # gathered rows (with repeats) of a pool, targets gathered through the same list
        idx = torch.from_numpy(rng.integers(0, N, max(1, (2 * N) // 3)).astype(np.int32)).cuda()
        check_exact(net, P, X, dev(one_hot(rng, N, Out)), idx=idx)


def test_ties_follow_the_scan_rule(ctx, pkg):
    """W = 0, so every row's outputs are the biases (1,3,3,2,3,0): the first of the three maxima is predicted,
    and the rank of a target class counts the equal outputs before it."""
    b = np.array([1, 3, 3, 2, 3, 0], np.float32)
    for loss in ("mse", "softmax_xent"):
        net = pkg.Mlp(ctx, [4, 6], ["linear"], loss=loss)
        P = dev(np.concatenate([np.zeros(4 * 6, np.float32), b]))
        N = 70
        rng = np.random.default_rng(5)
        X = dev(rng.standard_normal((N, 4)))
        tgt = np.arange(N) % 6
        Y = np.zeros((N, 6), np.float32)
        Y[np.arange(N), tgt] = 1.0
        rank_of_class = np.array([4, 0, 1, 3, 2, 5])   # by the rule, for the biases above
        for k in range(1, 7):
            r = net.evaluate(P, X, dev(Y), k=k, pred=True, confusion=True)
            assert np.all(r.pred.cpu().numpy() == 1)
            assert r.correct == int((tgt == 1).sum())
            assert r.topk == int((rank_of_class[tgt] < k).sum())
            assert np.array_equal(r.confusion[:, 1], np.bincount(tgt, minlength=6)) and r.confusion.sum() == N
        check_exact(net, P, X, dev(Y))
    # all outputs equal: class 0 is predicted, the rank of class t is t
    dims, acts = [37, 50, 3], ["tanh", "linear"]
    net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    Ph = pkg.init_params_host(dims, acts, 123)
    off = (37 + 1) * 50
    Ph[off:off + 50 * 3] = 0.0
    Ph[off + 50 * 3:] = 0.25
    N = 65
    X = dev(np.random.default_rng(6).standard_normal((N, 37)))
    tgt = np.arange(N) % 3
    Y = np.zeros((N, 3), np.float32)
    Y[np.arange(N), tgt] = 1.0
    for k in (1, 2, 3):
        r = net.evaluate(dev(Ph), X, dev(Y), k=k, pred=True)
        assert np.all(r.pred.cpu().numpy() == 0) and r.correct == int((tgt == 0).sum())
        assert r.topk == int((tgt < k).sum())
    check_exact(net, dev(Ph), X, dev(Y))


@pytest.mark.parametrize("loss", ["mse", "softmax_xent"])
def test_nan_row_predicts_class_zero_and_is_counted(ctx, pkg, loss):
    dims, acts = [37, 50, 3], ["tanh", "linear"]
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    N, bad = 65, 7
    rng = np.random.default_rng(7)
    Xh = rng.standard_normal((N, 37)).astype(np.float32)
    Xh[bad] = np.nan
    Yh = one_hot(rng, N, 3)
    Yh[bad] = [0, 0, 1]
    X, Y = dev(Xh), dev(Yh)
    Z = net.forward(P, X).cpu().numpy()
    assert np.isnan(Z[bad]).all() and np.isfinite(np.delete(Z, bad, 0)).all()
    pred, tgt, correct, topk, conf = expected(Z, Yh, (1, 2, 3))
    assert pred[bad] == 0   # the scan rule (numpy.argmax would say 0 here too, but for another reason)
    fin = np.arange(N) != bad
    _, _, _, topk_fin, _ = expected(Z[fin], Yh[fin], (1, 2, 3))
    for k in (1, 2, 3):
        r = net.evaluate(P, X, Y, k=k, pred=True, confusion=True)
        assert r.rows == N and np.isnan(r.loss)
        assert np.array_equal(r.pred.cpu().numpy(), pred) and r.correct == correct
        assert np.array_equal(r.confusion, conf)
        assert r.topk - topk_fin[k] in (0, 1)   # the NaN row is outside the top-k contract; the others are exact
    # a NaN target row never wins the target scan either
    Yn = Yh.copy()
    Yn[3] = np.nan
    r = net.evaluate(P, X, dev(Yn), pred=True, confusion=True)
    assert r.confusion[0].sum() >= 1 and np.array_equal(r.confusion, expected(Z, Yn, (1,))[4])


@pytest.mark.parametrize("dims,acts", [([784, 128, 10], ["relu", "linear"]), ([37, 50, 3], ["tanh", "linear"]),
                                       ([20, 300, 70], ["relu", "linear"]), ([16, 100], ["linear"])],
                         ids=["784-128-10", "37-50-3", "20-300-70", "16-100"])
def test_proba_is_the_softmax_of_the_device_logits(ctx, pkg, dims, acts):
    """|p - softmax64(z)| <= 16 * 2^-24: an fp32 exp of 2 ulp, the sum and the division, with margin (p <= 1)."""
    net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    P = net.init_params(123, "cpu")
    N, Out = 257, dims[-1]
    rng = np.random.default_rng(11)
    X = dev(3.0 * rng.standard_normal((N, dims[0])))
    Z = net.forward(P, X).double().cpu().numpy()
    E = np.exp(Z - Z.max(1, keepdims=True))
    ref = E / E.sum(1, keepdims=True)
    for Y in (None, dev(one_hot(rng, N, Out))):
        p = net.evaluate(P, X, Y, proba=True).proba.double().cpu().numpy()
        tol = 16 * 2.0 ** -24
        print(f"{dims}: max |p - ref| = {np.abs(p - ref).max():.3e}, max |sum - 1| = {np.abs(p.sum(1) - 1).max():.3e}")
        assert np.abs(p - ref).max() <= tol
        assert np.abs(p.sum(1) - 1.0).max() <= tol * Out
    with pytest.raises(pkg.LbfError):   # MSE nets have no probabilities
        pkg.Mlp(ctx, dims, acts).evaluate(P, X, proba=True)


def oracle_reference(O, dims, acts, loss, P64, Xh, Yh):
    """fp64 loss (inv_scale = 1 / N) and outputs of the oracle; cross-entropy from its logits with logsumexp."""
    l_mse, out = O.Net(dims, acts).loss(P64, Xh.astype(np.float64), Yh.astype(np.float64), want_out=True)
    if loss == "mse":
        return l_mse, out
    m = out.max(1, keepdims=True)
    lse = m + np.log(np.exp(out - m).sum(1, keepdims=True))
    return float((Yh.astype(np.float64) * (lse - out)).sum() / len(out)), out


def check_against_oracle(O, net, P, Xh, Yh, label):
    dims, acts, loss = net.dims, net.acts, net.loss_name
    N, Out = len(Xh), dims[-1]
    X, Y = dev(Xh), dev(Yh)
    l_ref, out = oracle_reference(O, dims, acts, loss, P.double().cpu().numpy(), Xh, Yh)
    r = net.evaluate(P, X, Y, pred=True)
    l_abi = net.loss(P, X, Y)
    rel = abs(r.loss - l_ref) / abs(l_ref)
    # rows whose fp64 top-two gap is clear of the fp32 forward's error
    if Out > 1:
        s = np.sort(out, 1)
        gap = s[:, -1] - s[:, -2]
    else:
        gap = np.full(N, np.inf)
    keep = gap >= 1e-4 * np.maximum(1.0, np.abs(out).max(1))
    left_out = int((~keep).sum())
    pred64, tgt = scan_argmax(out), scan_argmax(Yh)
    acc64 = float((pred64 == tgt).mean())
    print(f"{label}: loss {r.loss:.10g} oracle {l_ref:.10g} rel {rel:.2e} | vs lbf_mlp_loss rel "
          f"{abs(r.loss - l_abi) / abs(l_abi):.2e} | accuracy {r.accuracy:.4f} (oracle {acc64:.4f}) | "
          f"{left_out} of {N} rows left out")
    assert rel <= 1e-5   # the project's loss bound
    assert left_out <= 0.01 * N
    assert np.array_equal(r.pred.cpu().numpy()[keep], pred64[keep])
    return r


@pytest.mark.parametrize("dims,acts,loss", CASES, ids=CASE_IDS)
def test_loss_and_predictions_match_the_fp64_oracle(ctx, pkg, O, dims, acts, loss):
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    N = 1000
    rng = np.random.default_rng(21)
    Xh = rng.standard_normal((N, dims[0])).astype(np.float32)
    Yh = one_hot(rng, N, dims[-1]) if dims[-1] > 1 else rng.standard_normal((N, 1)).astype(np.float32)
    check_against_oracle(O, net, P, Xh, Yh, f"{dims} {loss}")


def test_trained_net_matches_the_oracle(ctx, pkg, O):
    """After 10 L-BFGS iterations on synth_mnist(1000) the accuracy is no longer the chance level."""
    dims, acts = [784, 128, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(1000)
    for loss in ("mse", "softmax_xent"):
        net = pkg.Mlp(ctx, dims, acts, loss=loss)
        P = net.init_params(123, "cpu")
        check_against_oracle(O, net, P, Xh, Yh, f"synth_mnist start {loss}")
        pkg.lbfgs_solve(net, P, dev(Xh), dev(Yh), m=10, max_iters=10, tol=0.0)
        r = check_against_oracle(O, net, P, Xh, Yh, f"synth_mnist 10 iterations {loss}")
        assert r.accuracy > 0.2   # chance is 0.1 on ten classes


@pytest.mark.parametrize("dims,acts,loss", [([784, 128, 10], ["relu", "linear"], "softmax_xent"),
                                            ([784, 512, 256, 10], ["relu", "relu", "linear"], "softmax_xent"),
                                            ([20, 300, 70], ["relu", "linear"], "mse")],
                         ids=["784-128-10", "784-512-256-10", "20-300-70"])
def test_chunking_changes_nothing_but_the_sum_order(ctx, pkg, dims, acts, loss):
    net = pkg.Mlp(ctx, dims, acts, loss=loss)
    P = net.init_params(123, "cpu")
    N, Out = 257, dims[-1]
    rng = np.random.default_rng(31)
    X, Y = dev(rng.standard_normal((N, dims[0]))), dev(soft(rng, N, Out))
    res = {c: net.evaluate(P, X, Y, k=2, confusion=True, pred=True, chunk=c) for c in (0, 64, 100, 257)}
    base = res[0]
    again = net.evaluate(P, X, Y, k=2, confusion=True, pred=True, chunk=0)
    assert again.loss == base.loss   # bitwise: fixed summation order
    assert net.evaluate(P, X, Y, k=2, chunk=100).loss == res[100].loss
    bound = N * Out * 2.0 ** -53     # regrouping N * Out fp64 additions of same-sign terms
    for c, r in res.items():
        assert (r.rows, r.correct, r.topk) == (base.rows, base.correct, base.topk), c
        assert np.array_equal(r.confusion, base.confusion) and torch.equal(r.pred, base.pred), c
        print(f"{dims} chunk {c}: loss {r.loss:.17g} rel dev {abs(r.loss - base.loss) / abs(base.loss):.2e} (bound {bound:.2e})")
        assert abs(r.loss - base.loss) <= bound * abs(base.loss), c
    # gathered rows are chunked through the index list
    idx = torch.from_numpy(rng.integers(0, N, 200).astype(np.int32)).cuda()
    a, b = net.evaluate(P, X, Y, idx=idx, pred=True, chunk=0), net.evaluate(P, X, Y, idx=idx, pred=True, chunk=64)
    assert (a.correct, a.rows) == (b.correct, b.rows) and torch.equal(a.pred, b.pred)
    assert abs(a.loss - b.loss) <= 200 * Out * 2.0 ** -53 * abs(a.loss)


@pytest.mark.parametrize("world,N", [(2, 1001), (3, 1001), (3, 2)], ids=["w2-1001", "w3-1001", "w3-2-empty-share"])
def test_ranks_get_the_single_rank_totals(ctx, pkg, world, N):
    dims, acts = [784, 128, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(N)
    net1 = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    P = net1.init_params(123, "cpu")
    one = net1.evaluate(P, dev(Xh), dev(Yh), k=3, confusion=True)
    shards = [(N * r // world, N * (r + 1) // world) for r in range(world)]
    assert world != 3 or N != 2 or shards[0] == (0, 0)   # rank 0's share is empty
    Xs = [dev(Xh[lo:hi]) for lo, hi in shards]
    Ys = [dev(Yh[lo:hi]) for lo, hi in shards]
    torch.cuda.synchronize()

    def body(r, c):
        net = pkg.Mlp(c, dims, acts, loss="softmax_xent")
        return net.evaluate(P, Xs[r], Ys[r], k=3, confusion=True, pred=True)

    res = run_ranks(pkg, world, body)
    for r, e in enumerate(res):
        assert (e.loss, e.rows, e.correct, e.topk) == (res[0].loss, res[0].rows, res[0].correct, res[0].topk)  # bitwise
        assert np.array_equal(e.confusion, res[0].confusion)
        assert e.pred.numel() == shards[r][1] - shards[r][0]   # predictions stay local
    e = res[0]
    assert (e.rows, e.correct, e.topk) == (one.rows, one.correct, one.topk) and e.rows == N
    assert np.array_equal(e.confusion, one.confusion)
    print(f"world {world} N {N}: loss {e.loss:.12g} single {one.loss:.12g} rel {abs(e.loss - one.loss) / abs(one.loss):.2e}")
    assert abs(e.loss - one.loss) <= 1e-6 * abs(one.loss)


REC_KEYS = ("loss", "grad_norm", "alpha", "ls_trials", "accepted")


def test_evaluation_on_a_second_net_leaves_an_open_solver_alone(ctx, pkg):
    dims, acts = [784, 32, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(600)
    X, Y = dev(Xh), dev(Yh)
    Xe, Ye = pkg.synth_mnist(200, seed=77)
    Xe, Ye = dev(Xe), dev(Ye)

    def lbfgs(with_eval):
        net, ev = pkg.Mlp(ctx, dims, acts, loss="softmax_xent"), pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
        P = net.init_params(123, "cpu")
        run = pkg.LbfgsRun(net, P, X, Y, m=10, max_iters=12, tol=0.0)
        seen = []
        for _ in range(4):
            run.iterate(3)
            if with_eval:
                seen.append(ev.evaluate(P, Xe, Ye, k=2, confusion=True, pred=True, proba=True).loss)
        torch.cuda.synchronize()
        hist = run.hist.as_dict()
        run.close()
        return P.cpu().numpy(), hist, seen

    def slbfgs(with_eval):
        net, ev = pkg.Mlp(ctx, dims, acts), pkg.Mlp(ctx, dims, acts)
        P = net.init_params(123, "cpu")
        run = pkg.SlbfgsRun(net, P, X, Y, M=5, L=4, b=64, b_H=32, step=0.01, lam=1e-4, tol=0.0)
        seen = []
        for _ in range(2):
            run.iterate(1)
            if with_eval:
                seen.append(ev.evaluate(P, Xe, Ye, confusion=True).loss)
        torch.cuda.synchronize()
        hist = run.hist.as_dict()
        run.close()
        return P.cpu().numpy(), hist, seen

    for solve in (lbfgs, slbfgs):
        Pa, ha, seen = solve(True)
        Pb, hb, _ = solve(False)
        assert np.array_equal(Pa, Pb), solve.__name__
        for key in REC_KEYS:
            assert np.array_equal(ha[key], hb[key]), (solve.__name__, key)
        assert len(ha["loss"]) >= 2 and np.all(np.isfinite(seen))


def make_launcher(pkg, Xh, Yh, Xt, Yt):
    L = pkg.UnifiedLauncher(0)
    L.addLayer(784, 32, "relu")
    L.addLayer(32, 10, "linear")
    L.setLoss("softmax_xent")
    L.buildNetwork()
    L.setData(pkg.UnifiedDataset(train_x=Xh, train_y=Yh, test_x=Xt, test_y=Yt))
    return L


def replay(pkg, validation, patience, monitor="loss"):
    """The recorded entries through a fresh EarlyStopper: the stop decision after each."""
    s = pkg.EarlyStopper(patience, monitor)
    return [s.update(*e) for e in validation], s


def test_validation_monitored_training(ctx, pkg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    Xa, Ya = pkg.synth_mnist(800)   # one draw: 600 training rows, 200 held out
    Xh, Yh, Xt, Yt = Xa[:600], Ya[:600], Xa[600:], Ya[600:]
    L = make_launcher(pkg, Xh, Yh, Xt, Yt)
    every, iters = 3, 12

    def train(name, **kw):
        opt = pkg.UnifiedLBFGS()
        cfg = pkg.UnifiedConfig(name=name, max_iters=iters, tolerance=1e-9, m_param=10, log_interval=1,
                                loss="softmax_xent", eval_every=every, **kw)
        res = L.train(opt, cfg)
        return opt, res

    # restore_best=False: the last entry is the test split's metrics at the final parameters
    opt, res = train("plain", restore_best=False)
    val = opt.validation
    its = [e[0] for e in val]
    done = int(opt.info.iterations)
    assert its[0] == 0 and its[-1] == done and 0 < done <= iters
    steps = np.diff(its)
    assert np.all(steps[:-1] == every) and 0 < steps[-1] <= every   # a run that converges early ends off the grid
    assert L.last_recorder.validation == val and L.last_recorder.size() >= 1
    m = L.metrics("test")
    assert (m.loss, m.accuracy) == (val[-1][1], val[-1][2])   # bitwise
    assert m.rows == 200 and val[-1][1] < val[0][1]
    mt = L.metrics("train", k=3, confusion=True)
    assert mt.rows == 600 and mt.confusion.sum() == 600 and mt.topk >= mt.correct
    assert abs(mt.accuracy * 100.0 - res["accuracy"]) < 1e-9 and abs(mt.loss - res["mse"]) <= 1e-5 * res["mse"]
    lines = (tmp_path / "plain_validation.csv").read_text().splitlines()
    assert lines[0] == "Iteration,ValLoss,ValAccuracy" and len(lines) == 1 + len(val)
    assert [int(l.split(",")[0]) for l in lines[1:]] == its and float(lines[-1].split(",")[1]) == val[-1][1]
    assert (tmp_path / "plain_history.csv").read_text().splitlines()[0] == "Iteration,Loss,GradNorm,TimeMs"

    # restore_best=True (the default): the final parameters are those of the best entry
    opt, _ = train("best", monitor="accuracy")
    val = opt.validation
    best = max(val, key=lambda e: (e[2], -e[0]))   # the earliest of the highest accuracies
    assert opt.best_iteration == best[0]
    m = L.metrics("test")
    assert (m.loss, m.accuracy) == (best[1], best[2])   # bitwise
    stops, s = replay(pkg, val, 0, "accuracy")
    assert not any(stops) and s.best_iteration == opt.best_iteration

    # patience=1 on a validation split of random labels: whatever happens must be what the rule says
    rng = np.random.default_rng(3)
    Yr = np.zeros_like(Yt)
    Yr[np.arange(len(Yr)), rng.integers(0, 10, len(Yr))] = 1.0
    L = make_launcher(pkg, Xh, Yh, Xt, Yr)
    opt, _ = train("patience", patience=1)
    val = opt.validation
    stops, s = replay(pkg, val, 1)
    print("patience=1 validation:", val, "stops:", stops)
    assert not any(stops[:-1])                       # it did not run past a stop
    assert stops[-1] == opt.stopped_early
    assert stops[-1] or val[-1][0] == int(opt.info.iterations)   # not stopped: it ran to the end
    assert opt.best_iteration == s.best_iteration
    m = L.metrics("test")
    bi = [e for e in val if e[0] == opt.best_iteration][0]
    assert (m.loss, m.accuracy) == (bi[1], bi[2])

    # S-LBFGS: epochs for iterations
    opt = pkg.UnifiedSLBFGS()
    cfg = pkg.UnifiedConfig(name="slbfgs", max_iters=4, tolerance=0.0, m_param=5, L_param=4, batch_size=64,
                            learning_rate=0.01, eval_every=2, restore_best=False, write_csv=False)
    L.train(opt, cfg)
    assert [e[0] for e in opt.validation] == [0, 2, 4]
    m = L.metrics("test")
    assert (m.loss, m.accuracy) == (opt.validation[-1][1], opt.validation[-1][2])

    # no resumable form / no test split
    with pytest.raises(pkg.LbfError):
        L.train(pkg.UnifiedGD(), pkg.UnifiedConfig(eval_every=1, write_csv=False))
    L2 = pkg.UnifiedLauncher(0)
    L2.addLayer(784, 32, "relu")
    L2.addLayer(32, 10, "linear")
    L2.buildNetwork()
    L2.setData(pkg.UnifiedDataset(train_x=Xh, train_y=Yh))
    with pytest.raises(pkg.LbfError):
        L2.train(pkg.UnifiedLBFGS(), pkg.UnifiedConfig(eval_every=1, max_iters=2, write_csv=False))
    with pytest.raises(pkg.LbfError):
        L2.metrics("test")
