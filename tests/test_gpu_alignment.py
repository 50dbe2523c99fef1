"""Caller pointers that are only 4-byte aligned (include/lbfgs_amd.h: d_* float pointers need no more).

The engine picks between a 16-byte route and a scalar / general route from pointer alignment in many places
(gemm.hip launch() / make_gemmk / gemm_asum_ok / gemm_group_ok, Mlp::forward_phase's fold, gather_rows,
gram_update, axpy_to, combine_stream, History::update_impl); tensors fresh from the allocator are 256-byte
aligned, so only offset views reach the second kind. Every test here passes views `buf[off : off + n]` (off in
1..3 floats) of a sentinel-filled buffer and checks the result against the fp64 oracle / torch fp64 with the
bounds of the files that cover the same operation on aligned data (test_gpu_parity.py, test_gpu_hvp.py,
test_gpu_xent.py, test_gpu_dp.py, test_gpu_eval.py, test_gpu_gd.py), and that the sentinel floats around every
view are untouched (a vector store spilling past either end). The difference to the same call on aligned copies
is printed, not asserted: the routes differ.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import dev, host
from ref_mlp import MSE, hess_ref, objective, rel

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-4
DIR_RTOL = 1e-5
HVP_RTOL = 1e-4
PAD = 8
SENTINEL = 0x7FC5A5A5   # a quiet NaN: a sentinel that is read poisons the result


def raw(pkg):
    """The library, the status check and the pointer helper: for calls whose output the wrapper allocates."""
    return pkg.lib(), pkg._lib.check, pkg._lib.ptr


def view(a, off, dtype=torch.float32):
    """`a` (array or tensor) copied to buf[off : off + n] of a sentinel-filled device buffer of n + 8 elements;
    returns the view in a's shape, 4 * off bytes past a 16-byte boundary."""
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    a = a.to(dtype).cuda()
    n = a.numel()
    buf = torch.empty(n + PAD, dtype=torch.int32, device="cuda")
    buf.fill_(SENTINEL)
    buf = buf.view(dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    v.copy_(a.reshape(-1))
    v = v.view(a.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    v.guard = (buf, off, n)
    return v


def out_view(shape, off, dtype=torch.float32):
    return view(torch.zeros(shape, dtype=dtype), off, dtype)


def check_guard(*views):
    """The sentinel elements before and after each view are bit-identical to what view() wrote."""
    torch.cuda.synchronize()
    for v in views:
        buf, off, n = v.guard
        bits = buf.view(torch.int32)
        assert bool((bits[:off] == SENTINEL).all()), "store before the view"
        assert bool((bits[off + n:] == SENTINEL).all()), "store past the view"


def random_problem(dims, N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, dims[0])).astype(np.float32).astype(np.float64)
    Y = np.zeros((N, dims[-1]))
    Y[np.arange(N), rng.integers(0, dims[-1], N)] = 1.0
    return X, Y


# ------------------------------------------------------------------------------------------------
# lbf_mlp_loss_grad
# ------------------------------------------------------------------------------------------------
# (dims, acts, N): the smallest shapes whose aligned run takes each 16-byte route (Mlp::plan on 256 CUs)
A2 = ([784, 128, 10], ["relu", "linear"])
DEEP = ([784, 512, 256, 10], ["relu", "relu", "linear"])
SHAPES = [
    (*A2, 257),     # LDS-DMA 32x128 EPI_HEAD + fold of 16 columns; unaligned X: unfolded, general loads
    (*A2, 1000),
    (*A2, 8200),    # 64x128 EPI_HEAD tile
    ([784, 128, 64, 10], ["relu", "relu", "linear"], 257),   # head_in internal; unaligned P: scalar B and bias
    ([48, 200, 10], ["relu", "linear"], 256),                # standalone head
    ([784, 300, 20], ["relu", "linear"], 256),               # forward split-K on 32x128, generic output
    (*DEEP, 256),   # gemm_asum_ok prologue (off with unaligned P), rowhead, grouped dW (off with unaligned X)
]
OFFSETS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 2, 3, 1), (2, 3, 1, 2), (3, 1, 2, 3)]
OFF_IDS = ["X", "Y", "P", "G", "1231", "2312", "3123"]
_REF = {}   # (dims, N, idx) -> the problem, the oracle's result, the aligned device result


def reference(ctx, pkg, O, dims, acts, N, gathered=False):
    key = (tuple(dims), N, gathered)
    if key not in _REF:
        net = pkg.Mlp(ctx, dims, acts)
        P = net.init_params(123, "cpu")
        onet = O.Net(dims, acts)
        if gathered:   # test_loss_grad_gather_and_l2's problem
            Xh, Yh = pkg.synth_mnist(N)
            X, Y = Xh.astype(np.float64), Yh.astype(np.float64)
            idx = O.sample_indices(N, 77, seed=123, calls=1)[0]
            l_ref, g_ref = onet.loss_grad(host(P), X, Y, idx=idx, lam=1e-4)
            gtol = GRAD_RTOL
            didx = torch.from_numpy(idx.astype(np.int32)).cuda()
            la, ga = net.loss_grad(P, dev(X), dev(Y), idx=didx, l2=1e-4)
        else:
            X, Y = random_problem(dims, N, seed=N)
            idx = didx = None
            l_ref, g_ref = onet.loss_grad(host(P), X, Y)
            _, g32 = onet.loss_grad_f32(host(P), X, Y)
            gtol = max(GRAD_RTOL, 3.0 * rel(g32, g_ref))
            la, ga = net.loss_grad(P, dev(X), dev(Y))
        _REF[key] = dict(P=P, X=X, Y=Y, idx=idx, didx=didx, l_ref=l_ref, g_ref=g_ref, gtol=gtol, la=la, ga=host(ga))
    return _REF[key]


def run_loss_grad(ctx, pkg, O, dims, acts, N, offs, gathered=False):
    r = reference(ctx, pkg, O, dims, acts, N, gathered)
    ox, oy, op, og = offs
    Xv, Yv, Pv = view(r["X"], ox), view(r["Y"], oy), view(r["P"], op)
    Gv = out_view(r["P"].shape, og)
    net = pkg.Mlp(ctx, dims, acts)
    loss, g = net.loss_grad(Pv, Xv, Yv, idx=r["didx"], l2=1e-4 if gathered else 0.0, grad=Gv)
    check_guard(Xv, Yv, Pv, Gv)
    el, eg = abs(loss - r["l_ref"]) / abs(r["l_ref"]), rel(host(g), r["g_ref"])
    print(f"{dims} N={N} offs={offs}: loss rel {el:.2e}, grad rel {eg:.2e} (bound {r['gtol']:.2e}); "
          f"vs aligned: loss {abs(loss - r['la']) / abs(r['la']):.2e}, grad {rel(host(g), r['ga']):.2e}")
    assert el <= LOSS_RTOL
    assert eg <= r["gtol"]


@pytest.mark.parametrize("offs", OFFSETS, ids=OFF_IDS)
@pytest.mark.parametrize("dims,acts,N", SHAPES, ids=["-".join(map(str, d)) + f"-N{n}" for d, _, n in SHAPES])
def test_loss_grad_unaligned(ctx, pkg, O, dims, acts, N, offs):
    run_loss_grad(ctx, pkg, O, dims, acts, N, offs)


@pytest.mark.parametrize("offs", OFFSETS, ids=OFF_IDS)
def test_loss_grad_gathered_unaligned(ctx, pkg, O, offs):
    """gather_rows' vec route is the solver's; here the gathered GEMM A operand (row gather inside the loaders)."""
    run_loss_grad(ctx, pkg, O, [784, 64, 10], ["relu", "linear"], 500, offs, gathered=True)


# ------------------------------------------------------------------------------------------------
# the other network entry points: every pointer unaligned, on a fused-head net and on the split-K net
# ------------------------------------------------------------------------------------------------
ENTRY = [(*A2, 257, (1, 2, 3, 1)), (*DEEP, 256, (2, 3, 1, 2))]
ENTRY_IDS = ["784-128-10-N257", "784-512-256-10-N256"]


def entry_views(ctx, pkg, O, dims, acts, N, offs):
    r = reference(ctx, pkg, O, dims, acts, N)
    return r, view(r["X"], offs[0]), view(r["Y"], offs[1]), view(r["P"], offs[2])


def forward_into(pkg, net, Pv, Xv, off):
    L, check, ptr = raw(pkg)
    out = out_view((Xv.shape[0], net.dims[-1]), off)
    check(L.lbf_mlp_forward(net.h, ptr(Pv), ptr(Xv), Xv.shape[0], ptr(out)), "lbf_mlp_forward")
    check_guard(out)
    return out


@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_forward_unaligned(ctx, pkg, O, dims, acts, N, offs):
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    net = pkg.Mlp(ctx, dims, acts)
    out = forward_into(pkg, net, Pv, Xv, offs[3])
    _, out_ref = O.Net(dims, acts).loss(host(r["P"]), r["X"], r["Y"], want_out=True)
    aligned = net.forward(r["P"], dev(r["X"]))
    print(f"{dims}: forward rel {rel(host(out), out_ref):.2e}; vs aligned {rel(host(out), host(aligned)):.2e}")
    assert rel(host(out), out_ref) <= 1e-5


@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_loss_only_equals_fused_loss_unaligned(ctx, pkg, O, dims, acts, N, offs):
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    net = pkg.Mlp(ctx, dims, acts)
    lf = net.loss(Pv, Xv, Yv)
    lg, _ = net.loss_grad(Pv, Xv, Yv, grad=out_view(r["P"].shape, offs[3]))
    assert lf == lg
    assert abs(lf - r["l_ref"]) <= LOSS_RTOL * abs(r["l_ref"])


@pytest.mark.parametrize("lam,gather", [(0.0, False), (1e-4, True), (0.0, True), (1e-4, False)])
@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_hvp_unaligned(ctx, pkg, O, dims, acts, N, offs, lam, gather):
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    net = pkg.Mlp(ctx, dims, acts)
    rng = np.random.default_rng(N)
    vh = rng.standard_normal(net.nparams).astype(np.float32)
    rows = np.sort(rng.permutation(N)[:(2 * N) // 3]) if gather else np.arange(N)
    idx = torch.from_numpy(rows.astype(np.int32)).cuda() if gather else None
    B = len(rows)
    vv, hv = view(vh, offs[3]), out_view(vh.shape, offs[0])
    net.hvp(Pv, vv, Xv, Yv, idx=idx, inv_scale=1.0 / B, l2=lam, out=hv)
    check_guard(hv, vv, Pv, Xv, Yv)
    ref = hess_ref(dims, acts, MSE, r["P"].double().cpu(), torch.from_numpy(vh).double(),
                   torch.from_numpy(r["X"][rows]), torch.from_numpy(r["Y"][rows]), 1.0 / B, lam)
    aligned = net.hvp(r["P"], dev(vh), dev(r["X"]), dev(r["Y"]), idx=idx, inv_scale=1.0 / B, l2=lam)
    err = rel(host(hv), ref.numpy())
    print(f"{dims} lam={lam} gather={gather}: hvp rel {err:.2e}; vs aligned {rel(host(hv), host(aligned)):.2e}")
    assert err <= HVP_RTOL


@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_fd_hvp_unaligned(ctx, pkg, O, dims, acts, N, offs):
    """lbf_mlp_fd_hvp against the fp64 central difference at the same eps (test_gpu_xent.py's bound, 2e-2: fp32
    differencing of fp32 gradients)."""
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    net = pkg.Mlp(ctx, dims, acts)
    eps, lam = 1e-3, 1e-4
    vh = np.random.default_rng(9).standard_normal(net.nparams).astype(np.float32)
    vv, yv = view(vh, offs[3]), out_view(vh.shape, offs[0])
    net.fd_hvp(Pv, vv, Xv, Yv, inv_scale=1.0 / N, l2=lam, eps=eps, out=yv)
    check_guard(yv, vv, Pv, Xv, Yv)
    f = objective(dims, acts, MSE, torch.from_numpy(r["X"]), torch.from_numpy(r["Y"]), 1.0 / N, lam)
    Ph, v64 = r["P"].double().cpu(), torch.from_numpy(vh).double()
    g = [torch.autograd.grad(f(p), p)[0] for p in ((Ph + eps * v64).requires_grad_(True),
                                                   (Ph - eps * v64).requires_grad_(True))]
    ref = ((g[0] - g[1]) / (2 * eps)).numpy()
    aligned = net.fd_hvp(r["P"], dev(vh), dev(r["X"]), dev(r["Y"]), inv_scale=1.0 / N, l2=lam, eps=eps)
    err = rel(host(yv), ref)
    print(f"{dims}: fd-hvp rel {err:.2e}; vs aligned {rel(host(yv), host(aligned)):.2e}")
    assert err <= 2e-2


@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_batch_grads_unaligned(ctx, pkg, O, dims, acts, N, offs):
    """lbf_mlp_batch_grads (4 minibatches of 64 rows) against lbf_mlp_loss_grad on each minibatch through the
    same views, at test_gpu_dp.py's bound: max |diff| <= 1e-5 max |g|."""
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    nmb, cnt = 4, 64
    net = pkg.Mlp(ctx, dims, acts)
    n = net.nparams
    G = out_view((nmb, n), offs[3])
    L, check, ptr = raw(pkg)
    check(L.lbf_mlp_batch_grads(net.h, ptr(Pv), ptr(Xv), ptr(Yv), nmb, cnt, 1.0 / cnt, 1e-4, ptr(G), n),
          "lbf_mlp_batch_grads")
    check_guard(G, Pv, Xv, Yv)
    Ga = net.batch_grads(r["P"], dev(r["X"][:nmb * cnt]), dev(r["Y"][:nmb * cnt]), nmb, inv_scale=1.0 / cnt, l2=1e-4)
    print(f"{dims}: batch_grads vs aligned {rel(host(G), host(Ga)):.2e}")
    for t in range(nmb):
        _, g = net.loss_grad(Pv, Xv[t * cnt:(t + 1) * cnt], Yv[t * cnt:(t + 1) * cnt], inv_scale=1.0 / cnt, l2=1e-4)
        ref = host(g)
        err = np.abs(host(G[t]) - ref).max()
        assert err <= 1e-5 * np.abs(ref).max(), (t, err, np.abs(ref).max())


def scan_argmax(Z):
    """The reference's scan (test_gpu_eval.py): the lowest index wins a tie, nothing above -1e20 gives 0."""
    Z = np.asarray(Z, np.float64)
    with np.errstate(invalid="ignore"):
        V = np.where(Z > -1e20, Z, -np.inf)
    return np.where(np.isneginf(V).all(1), 0, V.argmax(1)).astype(np.int64)


@pytest.mark.parametrize("dims,acts,N,offs", ENTRY, ids=ENTRY_IDS)
def test_evaluate_unaligned(ctx, pkg, O, dims, acts, N, offs):
    """lbf_mlp_evaluate with confusion, pred and proba on a softmax net: integer equality with numpy on the
    device's own logits fetched through the same views (test_gpu_eval.py's check_exact), probabilities at its
    bound 16 * 2^-24."""
    r, Xv, Yv, Pv = entry_views(ctx, pkg, O, dims, acts, N, offs)
    net = pkg.Mlp(ctx, dims, acts, loss="softmax_xent")
    Out, k = dims[-1], 2
    Z = host(forward_into(pkg, net, Pv, Xv, offs[3]))
    pred_v = out_view((N,), offs[0], torch.int32)
    proba_v = out_view((N, Out), offs[1])
    res = pkg._lib.EvalResultC()
    conf = np.zeros((Out, Out), np.int64)
    L, check, ptr = raw(pkg)
    check(L.lbf_mlp_evaluate(net.h, ptr(Pv), ptr(Xv), ptr(Yv), None, N, 1.0 / N, k, 100, C.byref(res),
                             conf.ctypes.data_as(C.c_void_p), ptr(pred_v, torch.int32), ptr(proba_v)),
          "lbf_mlp_evaluate")
    check_guard(pred_v, proba_v, Pv, Xv, Yv)
    pred, tgt = scan_argmax(Z), scan_argmax(r["Y"])
    zt = Z[np.arange(N), tgt][:, None]
    rank = (Z > zt).sum(1) + ((Z == zt) & (np.arange(Out)[None, :] < tgt[:, None])).sum(1)
    want = np.zeros((Out, Out), np.int64)
    np.add.at(want, (tgt, pred), 1)
    assert res.rows == N and res.correct == int((pred == tgt).sum()) and res.topk == int((rank < k).sum())
    assert np.array_equal(pred_v.cpu().numpy(), pred)
    assert np.array_equal(conf, want)
    E = np.exp(Z - Z.max(1, keepdims=True))
    assert np.abs(host(proba_v) - E / E.sum(1, keepdims=True)).max() <= 16 * 2.0 ** -24
    lse = np.log(E.sum(1)) + Z.max(1)
    l_ref = float((r["Y"] * (lse[:, None] - Z)).sum()) / N
    assert abs(res.loss - l_ref) <= LOSS_RTOL * abs(l_ref)


# ------------------------------------------------------------------------------------------------
# lbf_two_loop
# ------------------------------------------------------------------------------------------------
def make_history(n, k, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 2.0, n)
    S = rng.standard_normal((k, n))
    Yv = S * d + 0.01 * rng.standard_normal((k, n))   # positive curvature pairs
    S = S.astype(np.float32).astype(np.float64)
    Yv = Yv.astype(np.float32).astype(np.float64)
    rho = 1.0 / np.einsum("ij,ij->i", S, Yv)
    g = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    return S, Yv, rho, g


def two_loop_into(pkg, ctx, S, Yv, rho, g, out, mode):
    k = int(S.shape[0])
    rho_arr = (C.c_double * k)(*[float(x) for x in rho])
    L, _, ptr = raw(pkg)
    rho_p = C.cast(rho_arr, C.POINTER(C.c_double))
    return L.lbf_two_loop(ctx.h, g.numel(), k, ptr(S), ptr(Yv), rho_p, ptr(g), ptr(out), mode)


_HIST = {}   # (n, k) -> history and the oracle's directions per mode


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n,k", [(1000, 5), (100003, 5), (100003, 50), (2 ** 21 + 5, 5), (2 ** 21 + 5, 20)])
def test_two_loop_unaligned(ctx, pkg, O, mode, n, k):
    """combine_small (n <= 2^21, k <= 32), the streaming combine's element-wise form through k > 32 and through
    n > 2^21, and the split Gram sweep's guard (n >= 2^21, m >= 20): S, Y, g and the output dir all off a 16-byte
    boundary."""
    if (n, k) not in _HIST:
        _HIST[(n, k)] = make_history(n, k, seed=k + n) + ({},)
    S, Yv, rho, g, refs = _HIST[(n, k)]
    if mode not in refs:
        refs[mode] = O.two_loop(mode, S, Yv, rho, g)
    Sv, Yvv, gv, out = view(S, 1), view(Yv, 2), view(g, 3), out_view((n,), 1 + mode)
    pkg._lib.check(two_loop_into(pkg, ctx, Sv, Yvv, rho, gv, out, mode), "lbf_two_loop")
    check_guard(out, Sv, Yvv, gv)
    aligned = ctx.two_loop(dev(S), dev(Yv), rho, dev(g), mode=mode)
    err = rel(host(out), refs[mode])
    print(f"two_loop n={n} k={k} mode={mode}: rel {err:.2e}; vs aligned {rel(host(out), host(aligned)):.2e}")
    assert err <= DIR_RTOL


@pytest.mark.parametrize("which", ["g", "S", "Y", "dir"])
def test_two_loop_mode3_rejects_unaligned(ctx, pkg, which):
    """Mode 3 (the S-LBFGS solver's 16-byte sweeps) is the one entry point that refuses such pointers."""
    n, k = 1000, 4
    S, Yv, rho, g = make_history(n, k, seed=1)
    Sv, Yvv, gv = view(S, int(which == "S")), view(Yv, int(which == "Y")), view(g, int(which == "g"))
    out = view(np.full(n, 7.0, np.float32), int(which == "dir"))
    assert two_loop_into(pkg, ctx, Sv, Yvv, rho, gv, out, 3) == 1   # LBF_ERR_INVALID
    assert "mode 3" in pkg.lib().lbf_last_error().decode() and "aligned" in pkg.lib().lbf_last_error().decode()
    check_guard(out)
    assert bool((out == 7.0).all())
    ok = out_view((n,), 0)
    pkg._lib.check(two_loop_into(pkg, ctx, view(S, 0), view(Yv, 0), rho, view(g, 0), ok, 3), "lbf_two_loop")
    assert torch.isfinite(ok).all() and bool(ok.any())


# ------------------------------------------------------------------------------------------------
# BLAS-1
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 257, 123457])
def test_blas1_unaligned(ctx, pkg, n):
    """test_blas1's bounds at its n = 123457, the same expressions at the smaller n."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    y = rng.standard_normal(n).astype(np.float32)
    x64, a = x.astype(np.float64), np.float32(0.5)
    for ox, oy in [(1, 2), (3, 1), (0, 1), (2, 0)]:   # both off by different offsets; y alone; x alone
        dx, dy = view(x, ox), view(y, oy)
        assert abs(ctx.dot(dx, dy) - float(np.dot(x64, y))) < 1e-9 * n
        assert abs(ctx.nrm2(dx) - float(np.linalg.norm(x64))) < 1e-9 * 400
        ctx.axpy_(0.5, dx, dy)
        check_guard(dx, dy)
        assert np.allclose(host(dy), y + a * x, rtol=1e-6, atol=1e-6)
        aligned = ctx.axpy_(0.5, dev(x), dev(y))
        print(f"axpy n={n} offs=({ox},{oy}): vs aligned max |diff| {float((dy - aligned).abs().max()):.2e}")
        pkg._lib.check(pkg.lib().lbf_scal(ctx.h, n, 0.25, pkg._lib.ptr(dx)), "lbf_scal")
        check_guard(dx)
        assert np.array_equal(dx.cpu().numpy(), np.float32(0.25) * x)


# ------------------------------------------------------------------------------------------------
# solvers: one short run each, the assertions of their aligned twins
# ------------------------------------------------------------------------------------------------
SOLVE = ([784, 32, 10], ["relu", "linear"])


def test_lbfgs_wolfe_unaligned(ctx, pkg, O):
    """test_lbfgs_wolfe_trajectory (m = 5) with X, Y and the parameters as views."""
    dims, acts = SOLVE
    Xh, Yh = pkg.synth_mnist(256)
    net = pkg.Mlp(ctx, dims, acts)
    P = view(net.init_params(123, "cpu"), 3)
    P0 = host(P)
    Xv, Yv = view(Xh, 1), view(Yh, 2)
    hist, info = pkg.lbfgs_solve(net, P, Xv, Yv, m=5, max_iters=20, tol=0.0)
    check_guard(P, Xv, Yv)
    _, rec, _ = O.Net(dims, acts).lbfgs_wolfe(P0, Xh.astype(np.float64), Yh.astype(np.float64), m=5, max_iters=20)
    assert len(hist["loss"]) == 20
    r = np.abs(hist["loss"][:10] - rec[:10, 0]) / np.abs(rec[:10, 0])
    assert r.max() <= 1e-3, r
    assert np.array_equal(hist["ls_trials"][:10], rec[:10, 4].astype(int))
    assert np.array_equal(hist["accepted"][:9], rec[:9, 3].astype(int))
    assert np.all(np.diff(hist["loss"]) <= 1e-7)


def test_lbfgs_armijo_long_history_unaligned(ctx, pkg, O):
    """test_gram_fin_route_matches_oracle's Armijo run (m = 40: the unfused history route) with the same views."""
    dims, acts = SOLVE
    Xh, Yh = pkg.synth_mnist(256)
    net = pkg.Mlp(ctx, dims, acts)
    P = view(net.init_params(123, "cuda"), 3)
    P0 = host(P)
    Xv, Yv = view(Xh, 1), view(Yh, 2)
    hist, _ = pkg.lbfgs_solve(net, P, Xv, Yv, line_search="armijo", m=40, max_iters=25, tol=0.0)
    check_guard(P, Xv, Yv)
    _, rec = O.Net(dims, acts).lbfgs_armijo(P0, Xh.astype(np.float64), Yh.astype(np.float64), m=40, max_iters=25,
                                            fp32=True)
    r = np.abs(hist["loss"][:10] - rec[:10, 0]) / np.abs(rec[:10, 0])
    assert r.max() <= 1e-3, r
    assert np.array_equal(hist["ls_trials"][:8], rec[:8, 4].astype(int))


SLBFGS_KW = dict(M=5, L=4, b=32, b_H=16, step=0.02)


def check_slbfgs(pkg, O, net, dims, acts, P, Xh, Yh, Xd, Yd):
    P0 = host(P)
    hist, info = pkg.slbfgs_solve(net, P, Xd, Yd, max_epochs=2, tol=0.0, lam=1e-4, **SLBFGS_KW)
    _, rec, _ = O.Net(dims, acts).slbfgs(P0, Xh.astype(np.float64), Yh.astype(np.float64), epochs=2, tol=0.0,
                                         M=5, L=4, b=32, bH=16, step=0.02, lam=1e-4)
    assert len(hist["loss"]) == 2
    r = np.abs(hist["loss"] - rec[:, 0]) / np.abs(rec[:, 0])
    print(f"slbfgs {dims}: loss rel {r}, accepted {hist['accepted']}")
    assert r.max() <= 1e-3, r
    assert np.array_equal(hist["accepted"], rec[:, 3].astype(int))


def test_slbfgs_unaligned(ctx, pkg, O):
    """test_slbfgs_matches_oracle with X and Y as views: gather_rows' element-wise route, the minibatch GEMMs'
    general loaders."""
    dims, acts = [784, 16, 10], ["relu", "linear"]
    Xh, Yh = pkg.synth_mnist(512)
    net = pkg.Mlp(ctx, dims, acts)
    Xv, Yv = view(Xh, 1), view(Yh, 3)
    check_slbfgs(pkg, O, net, dims, acts, net.init_params(123, "cpu"), Xh, Yh, Xv, Yv)
    check_guard(Xv, Yv)


# Data seed 0: the fp64 and the fp32 oracle agree on `accepted` ([2, 5]) and every pair's y.s is 5e-3 .. 2e-2,
# eight orders above the acceptance threshold 1e-10, so the comparison does not hang on a near-threshold pair.
SEG_SEED = 0


def test_slbfgs_segment_offset_not_a_multiple_of_four(ctx, pkg, O):
    """37-51-3: layer 1 starts at 38 * 51 = 1938 floats, 1938 % 4 = 2, so the deferred gradient's segments do not
    start on a quad and History::update_impl finishes them with reduce_all instead of inside the sweep."""
    dims, acts = [37, 51, 3], ["tanh", "linear"]
    X, Y = random_problem(dims, 512, seed=SEG_SEED)
    net = pkg.Mlp(ctx, dims, acts)
    check_slbfgs(pkg, O, net, dims, acts, net.init_params(123, "cpu"), X, Y, dev(X), dev(Y))


def test_gd_unaligned(ctx, pkg, O):
    """test_gd_matches_oracle (momentum 0.9) with the parameters, updated in place, as a view."""
    dims, acts = SOLVE
    Xh, Yh = pkg.synth_mnist(256)
    net = pkg.Mlp(ctx, dims, acts)
    P = view(net.init_params(123, "cuda"), 1)
    P0 = host(P)
    hist, info = pkg.gd_solve(net, P, dev(Xh), dev(Yh), lr=0.1, momentum=0.9, max_iters=15, tol=1e-6)
    check_guard(P)
    Pr, rec = O.Net(dims, acts).gd(P0, Xh.astype(np.float64), Yh.astype(np.float64), lr=0.1, momentum=0.9,
                                   max_iters=15, tol=1e-6, fp32=True)
    assert info.iterations == len(rec) == 15
    r = np.abs(hist["loss"] - rec[:, 0]) / np.abs(rec[:, 0])
    assert r.max() <= 1e-3, r
    assert np.linalg.norm(host(P) - Pr) <= 1e-3 * np.linalg.norm(Pr)
