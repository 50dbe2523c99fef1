"""Device-side Lanczos (lbf_mlp_lanczos) on the MI355X against the fp64 reference of ref_lanczos.py.

Every bound is either the project's product bound max(1e-4, 3 x the fp32 restatement's figure) or, for the basis'
orthonormality, which no product enters, 3 x the restatement's figure alone; the restatement is ref_lanczos.lanczos_ref
in fp32 on the same case and start vector. The fp64 references are made once per module and shared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_lanczos as RL
from gpu_helpers import dev, gpu_args, make_net, run_ranks, shard
from ref_mlp import SMALL, make_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GN, HESS = "gauss_newton", "hessian"
KMAX = {"n387": 24, "xent4": 32, "xent10": 32, "mnist": 32, "wide": 4, "elu": 24}
CHUNK = 8  # lanczos.hip kLzChunk: steps 8 and 9 end with 8 and 9 rows in the projection


def case(pkg, name):
    return make_case(pkg, RL.TABLE, name)


_nets, _ref = {}, {}


def device_run(pkg, ctx, c, **kw):
    """Mlp.lanczos on the case's batch (its own P, X, Y, gathered rows) with the default start vector."""
    key = (c["name"], c["loss"])
    if key not in _nets:
        _nets[key] = (make_net(pkg, ctx, c), gpu_args(c))
    net, (P, _, X, Y, idx) = _nets[key]
    return net.lanczos(P, X, Y, idx=idx, **kw)


def reference(c, matrix, dtype, steps, reorth=True, l2=0.0, rtol=0.0):
    """lanczos_ref of the case from the default start vector, made once per argument set."""
    key = (c["name"], matrix, dtype, steps, reorth, l2, rtol)
    if key not in _ref:
        v0 = RL.start_vector(len(c["P"])).to(dtype)
        _ref[key] = RL.lanczos_ref(RL.matvec(c, matrix, dtype, l2), v0, steps, reorth, rtol)
    return _ref[key]


def norm_of(c, matrix):
    """|A|_2: of the dense matrix on the small cases, else the fp64 reference's largest |Ritz value| (a lower bound of
    |A|, so the figures divided by it are upper bounds)."""
    if len(c["P"]) <= 4096:
        return float(np.abs(np.linalg.eigvalsh(RL.dense_matrix(c, matrix).numpy())).max())
    k = KMAX[c["name"]] if c["name"] == "wide" else 8
    r = reference(c, matrix, torch.float64, k)
    return float(np.abs(RL.ritz(r["alpha"], r["beta"], r["steps"])[0]).max())


def products(c, matrix, Q, l2=0.0):
    """A q_j in fp64 for the rows of Q (any dtype or device): by the dense matrix on the small cases."""
    Q = torch.as_tensor(Q).double().cpu()
    if len(c["P"]) <= 4096:
        A = RL.dense_matrix(c, matrix)
        return [A @ q + l2 * q for q in Q]
    A = RL.matvec(c, matrix, torch.float64, l2)
    return [A(q) for q in Q]


def relation(c, matrix, r, l2=0.0):
    """The Lanczos relation's figure of a run (a LanczosResult or lanczos_ref's dict)."""
    get = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, {"Q": "basis"}.get(k, k)))
    m = get("steps")
    return RL.relation_figure(products(c, matrix, get("Q")[:m], l2), get("Q"), get("alpha"), get("beta"), m,
                              norm_of(c, matrix))


# ---------------------------------------------------------------- 1. orthonormality
ORTH = [(n, k) for n in ("n387", "xent4", "xent10", "mnist") for k in (1, 2, 3, CHUNK, CHUNK + 1, KMAX[n])]
ORTH.append(("wide", 4))


@pytest.mark.parametrize("name,k", ORTH)
def test_basis_is_orthonormal(ctx, pkg, name, k):
    c = case(pkg, name)
    r = device_run(pkg, ctx, c, steps=k, basis=True)
    assert (r.status, r.steps) == (0, k) and tuple(r.basis.shape) == (k + 1, len(c["P"]))
    own = RL.orth_figure(reference(c, GN, torch.float32, KMAX[name])["Q"][:k + 1])  # a prefix of the longest run
    got = RL.orth_figure(r.basis)
    print(f"orthonormality {name} k={k}: device {got:.2e}, cpu fp32 {own:.2e}")
    assert got <= 3 * own


# ---------------------------------------------------------------- 2. the Lanczos relation
RELATION = [(n, KMAX[n]) for n in SMALL] + [("mnist", 8), ("wide", 4)]


@pytest.mark.parametrize("reorth", [True, False], ids=["reorth", "three-term"])
@pytest.mark.parametrize("matrix", [GN, HESS])
@pytest.mark.parametrize("name,k", RELATION + [("elu", KMAX["elu"])])
def test_lanczos_relation(ctx, pkg, name, k, matrix, reorth):
    """n387 has tanh, xent10 and mnist relu, elu its namesake in the hidden layers."""
    c = case(pkg, name)
    r = device_run(pkg, ctx, c, steps=k, matrix=matrix, reorth=reorth, basis=True)
    assert (r.status, r.steps) == (0, k)
    own = relation(c, matrix, reference(c, matrix, torch.float32, k, reorth))
    got = relation(c, matrix, r)
    print(f"relation {name} {matrix} reorth={reorth} k={k}: device {got:.2e}, cpu fp32 {own:.2e}")
    assert got <= max(1e-4, 3 * own)


# ---------------------------------------------------------------- 3. extreme Ritz values
@pytest.mark.parametrize("matrix", [GN, HESS])
@pytest.mark.parametrize("name", SMALL)
def test_extreme_ritz_values(ctx, pkg, name, matrix):
    c = case(pkg, name)
    k = KMAX[name]
    ev = np.linalg.eigvalsh(RL.dense_matrix(c, matrix).numpy())
    norm_A = float(np.abs(ev).max())
    ref = reference(c, matrix, torch.float64, k)
    th64 = RL.ritz(ref["alpha"], ref["beta"], k)[0]
    assert abs(th64[-1] - ev[-1]) <= 1e-8 * ev[-1]  # the condition: the reference itself has converged at this k
    own = reference(c, matrix, torch.float32, k)
    th32 = RL.ritz(own["alpha"], own["beta"], k)[0]
    r = device_run(pkg, ctx, c, steps=k, matrix=matrix)
    got, fig = abs(r.ritz[-1] - ev[-1]) / ev[-1], abs(th32[-1] - ev[-1]) / ev[-1]
    print(f"theta_max {name} {matrix}: lambda_max {ev[-1]:.6e}, device {got:.2e}, cpu fp32 {fig:.2e}")
    assert got <= max(1e-4, 3 * fig)
    assert abs(r.weights.sum() - 1.0) <= 1e-12
    if name == "xent4" and matrix == HESS:
        assert ev[0] < 0.0 and abs(th64[0] - ev[0]) <= 1e-8 * norm_A
        got, fig = abs(r.ritz[0] - ev[0]) / norm_A, abs(th32[0] - ev[0]) / norm_A
        print(f"theta_min xent4 hessian: lambda_min {ev[0]:.6e}, device {got:.2e}, cpu fp32 {fig:.2e}")
        assert got <= max(1e-4, 3 * fig)


# ---------------------------------------------------------------- 4. invariant subspace
def test_single_layer_exhausts_its_krylov_space(ctx, pkg):
    """[6, 3] linear, squared error: 7 distinct eigenvalues among 21. The run stops at the default breakdown_rtol."""
    c = case(pkg, "lin63")
    ev = np.linalg.eigvalsh(RL.dense_matrix(c, GN).numpy())
    distinct = ev.reshape(7, 3).mean(1)
    r = device_run(pkg, ctx, c, steps=12, basis=True)
    scale = np.maximum.accumulate(np.maximum(np.abs(r.alpha), np.concatenate([[0.0], r.beta[:-1]])))
    print(f"lin63 device: beta / scale {r.beta[:7] / scale[:7]}")
    assert (r.status, r.steps) == (1, 7)
    assert np.all(r.alpha[7:] == 0.0) and np.all(r.beta[7:] == 0.0) and r.basis.shape[0] == 7
    p = pkg._lib.LanczosParams()
    pkg.lib().lbf_lanczos_default_params(C.byref(p))
    own = reference(c, GN, torch.float32, 12, rtol=p.breakdown_rtol)
    assert (own["status"], own["steps"]) == (1, 7)
    fig = np.abs(RL.ritz(own["alpha"], own["beta"], 7)[0] - distinct).max() / ev[-1]
    got = np.abs(r.ritz - distinct).max() / ev[-1]
    print(f"lin63 Ritz values: device {got:.2e}, cpu fp32 {fig:.2e}")
    assert got <= max(1e-4, 3 * fig)


def test_two_parameters_stop_at_two(ctx, pkg):
    r = device_run(pkg, ctx, case(pkg, "n2"), steps=4)
    print(f"n2 device: beta / |alpha|max {r.beta[:2] / np.abs(r.alpha[:2]).max()}")
    assert (r.status, r.steps) == (1, 2)


# ---------------------------------------------------------------- 5. reproducibility
def same_bits(a, b):
    return (a.steps, a.status) == (b.steps, b.status) and np.array_equal(a.alpha.view(np.uint64), b.alpha.view(np.uint64)) \
        and np.array_equal(a.beta.view(np.uint64), b.beta.view(np.uint64))


@pytest.mark.parametrize("name,matrix,reorth", [("mnist", GN, True), ("xent4", HESS, True), ("n387", GN, False),
                                                ("lin63", GN, True)])
def test_bitwise_reproducible_whatever_check_is(ctx, pkg, name, matrix, reorth):
    c = case(pkg, name)
    k = 12
    a = device_run(pkg, ctx, c, steps=k, matrix=matrix, reorth=reorth)
    assert same_bits(a, device_run(pkg, ctx, c, steps=k, matrix=matrix, reorth=reorth))
    for every in (1, 8, k):
        assert same_bits(a, device_run(pkg, ctx, c, steps=k, matrix=matrix, reorth=reorth, check=every)), every
    b = device_run(pkg, ctx, c, steps=k, matrix=matrix, reorth=reorth, basis=True)
    assert same_bits(a, b)
    assert b.basis.shape[0] == (k + 1 if a.status == 0 else a.steps)


@pytest.mark.parametrize("name,k", [("n387", CHUNK + 1), ("xent10", 12)])
def test_unaligned_pointers(ctx, pkg, name, k):
    """v0, P and the basis one float off a 16-byte boundary (the basis' rows then alternate their offsets unless the
    stride is a multiple of four): orthonormality and the relation hold as they do aligned."""
    c = case(pkg, name)
    P, _, X, Y, idx = gpu_args(c)
    n = P.numel()
    net = make_net(pkg, ctx, c)
    for ld in (n, (n + 3) // 4 * 4):
        bufs = [torch.full((n + 8,), 1234.5, device="cuda") for _ in range(2)]
        Pu, vu = (t[1:n + 1] for t in bufs)
        Pu.copy_(P)
        vu.copy_(RL.start_vector(n).cuda())
        qbuf = torch.full(((k + 1) * ld + 8,), 1234.5, device="cuda")
        Q = qbuf[1:(k + 1) * ld + 1].view(k + 1, ld)
        assert Pu.data_ptr() % 16 == 4 and vu.data_ptr() % 16 == 4 and Q.data_ptr() % 16 == 4
        for matrix, reorth in ((GN, True), (HESS, False)):
            r = net.lanczos(Pu, X, Y, idx=idx, steps=k, matrix=matrix, reorth=reorth, v0=vu, basis=Q)
            assert (r.status, r.steps) == (0, k)
            assert bool((qbuf[:1] == 1234.5).all()) and bool((qbuf[(k + 1) * ld + 1:] == 1234.5).all())
            if ld > n:
                assert bool((Q[:, n:] == 1234.5).all())
            own = reference(c, matrix, torch.float32, k, reorth)
            got, fig = relation(c, matrix, r), relation(c, matrix, own)
            print(f"unaligned {name} ld={ld} {matrix}: relation device {got:.2e}, cpu fp32 {fig:.2e}")
            assert got <= max(1e-4, 3 * fig)
            if reorth:
                got, fig = RL.orth_figure(r.basis), RL.orth_figure(own["Q"])
                print(f"unaligned {name} ld={ld}: orthonormality device {got:.2e}, cpu fp32 {fig:.2e}")
                assert got <= 3 * fig
        assert bool((bufs[0][:1] == 1234.5).all()) and torch.equal(Pu, P)


# ---------------------------------------------------------------- 6. two ranks
@pytest.mark.parametrize("split", [100, 0], ids=["unequal", "empty-shard"])
@pytest.mark.parametrize("matrix", [GN, HESS])
def test_world2(ctx, pkg, matrix, split):
    c = case(pkg, "xent10")
    P, _, X, Y, _ = gpu_args(c)
    N, k = X.shape[0], 12
    bounds = [(0, split), (split, N)]

    def body(r, cx):
        lo, hi = bounds[r]
        return make_net(pkg, cx, c).lanczos(P.clone(), X[lo:hi].contiguous(), Y[lo:hi].contiguous(), steps=k,
                                            matrix=matrix, inv_scale=1.0 / N)

    out = run_ranks(pkg, 2, body)
    assert same_bits(out[0], out[1])
    one = device_run(pkg, ctx, c, steps=k, matrix=matrix)
    own, ref = reference(c, matrix, torch.float32, k), reference(c, matrix, torch.float64, k)
    nA = norm_of(c, matrix)
    dist = lambda a, b: max(np.abs(a["alpha"] - b["alpha"]).max(), np.abs(a["beta"] - b["beta"]).max()) / nA  # noqa: E731
    as_dict = lambda r: dict(alpha=r.alpha, beta=r.beta)  # noqa: E731
    got, fig = dist(as_dict(out[0]), as_dict(one)), dist(own, ref)
    print(f"world 2 {matrix} split {split}: |T - one rank's| / |A| {got:.2e}, cpu fp32 against fp64 {fig:.2e}")
    assert out[0].status == 0 and got <= max(1e-4, 3 * fig)


@pytest.mark.parametrize("matrix", [GN, HESS])
def test_world2_stop_with_steps_enqueued_behind_it(ctx, pkg, matrix):
    """lin63 on two ranks: the run stops after 7 of 12 steps with one more step already enqueued, whose product and
    all-reduce still run on both ranks. Both ranks report the stop with equal bits, whatever check is, and the
    network is usable afterwards. (For one linear layer H = G.)"""
    c = case(pkg, "lin63")
    P, _, X, Y, _ = gpu_args(c)
    N = X.shape[0]

    def body(r, cx):
        lo, hi = shard(N, 2, r)
        net = make_net(pkg, cx, c)
        kw = dict(steps=12, matrix=matrix, inv_scale=1.0 / N)
        runs = [net.lanczos(P.clone(), X[lo:hi].contiguous(), Y[lo:hi].contiguous(), check=every, **kw)
                for every in (8, 1, 12)]
        after = net.lanczos(P.clone(), X[lo:hi].contiguous(), Y[lo:hi].contiguous(), steps=5, matrix=matrix,
                            inv_scale=1.0 / N)
        return runs, after

    out = run_ranks(pkg, 2, body)
    for (runs, after), (runs1, after1) in [(out[0], out[1])]:
        for a, b in zip(runs, runs1):
            assert same_bits(a, b) and same_bits(a, runs[0])
            assert (a.status, a.steps) == (1, 7)
        assert same_bits(after, after1) and (after.status, after.steps) == (0, 5)
        assert np.array_equal(after.alpha[:5].view(np.uint64), runs[0].alpha[:5].view(np.uint64))
    ev = np.linalg.eigvalsh(RL.dense_matrix(c, GN).numpy())
    got = np.abs(out[0][0][0].ritz - ev.reshape(7, 3).mean(1)).max() / ev[-1]
    print(f"world 2 lin63 {matrix}: Ritz values against the distinct eigenvalues {got:.2e}")
    assert got <= 1e-4


# ---------------------------------------------------------------- 7. consistency with the existing products
@pytest.mark.parametrize("matrix", [GN, HESS])
@pytest.mark.parametrize("name", ["xent4", "mnist"])
def test_alpha0_is_the_rayleigh_quotient_and_l2_shifts(ctx, pkg, name, matrix):
    c = case(pkg, name)
    net, (P, _, X, Y, idx) = (make_net(pkg, ctx, c), gpu_args(c))
    k = 8
    v0 = RL.start_vector(P.numel()).cuda()
    Av = (net.gnvp if matrix == GN else net.hvp)(P, v0, X, Y, idx=idx)
    rq = float(v0.double() @ Av.double()) / float(v0.double() @ v0.double())
    r0 = net.lanczos(P, X, Y, idx=idx, steps=k, matrix=matrix)
    nA = norm_of(c, matrix)
    own, ref = reference(c, matrix, torch.float32, k), reference(c, matrix, torch.float64, k)
    fig = abs(own["alpha"][0] - ref["alpha"][0]) / nA
    got = abs(r0.alpha[0] - rq) / nA
    print(f"alpha_0 {name} {matrix}: |alpha_0 - v.Av / v.v| / |A| {got:.2e}, cpu fp32 {fig:.2e}")
    assert got <= max(1e-4, 3 * fig)
    r1 = net.lanczos(P, X, Y, idx=idx, steps=k, matrix=matrix, l2=0.1)
    th32 = RL.ritz(own["alpha"], own["beta"], k)[0]
    th64 = RL.ritz(ref["alpha"], ref["beta"], k)[0]
    got, fig = np.abs(r1.ritz - r0.ritz - 0.1).max() / nA, np.abs(th32 - th64).max() / nA
    print(f"l2 shift {name} {matrix}: {got:.2e}, cpu fp32 Ritz error {fig:.2e}")
    assert got <= max(1e-4, 3 * fig)


# ---------------------------------------------------------------- 8. bad input
@pytest.mark.parametrize("matrix", [GN, HESS])
def test_non_finite_input_returns_status_2(ctx, pkg, matrix):
    c = case(pkg, "xent10")
    net, (P, _, X, Y, idx) = (make_net(pkg, ctx, c), gpu_args(c))
    bad = P.clone()
    bad[-1] = float("nan")  # an output bias: every logit (a hidden ReLU unit would turn a NaN weight into 0)
    r = net.lanczos(bad, X, Y, steps=6, matrix=matrix, check=2)
    assert (r.status, r.steps) == (2, 0) and np.all(r.alpha == 0.0) and np.all(r.beta == 0.0) and r.ritz.size == 0
    r = net.lanczos(P, X, Y, steps=6, matrix=matrix, v0=torch.zeros_like(P))
    assert (r.status, r.steps, r.v0_norm) == (2, 0, 0.0)
    v = RL.start_vector(P.numel()).cuda()
    v[7] = float("inf")
    assert net.lanczos(P, X, Y, steps=6, matrix=matrix, v0=v).status == 2
    good = net.lanczos(P, X, Y, steps=6, matrix=matrix)  # the network is usable afterwards
    assert (good.status, good.steps) == (0, 6)
    # the arguments that need a network to be told apart from a null handle
    Q = torch.empty((7, P.numel() - 1), device="cuda")
    with pytest.raises(pkg.LbfError, match="basis must be"):
        net.lanczos(P, X, Y, steps=6, basis=Q)
    p = pkg._lib.LanczosParams()
    pkg.lib().lbf_lanczos_default_params(C.byref(p))
    p.steps = 6
    a, info = (C.c_double * 6)(), pkg._lib.LanczosInfo()
    rc = pkg.lib().lbf_mlp_lanczos(net.h, P.data_ptr(), v.data_ptr(), X.data_ptr(), Y.data_ptr(), None, X.shape[0], 1.0,
                                   C.byref(p), a, a, Q.data_ptr(), P.numel() - 1, C.byref(info))
    assert rc == 1 and "ld" in pkg.lib().lbf_last_error().decode()


# ---------------------------------------------------------------- 9. the C++ route
EXE = os.path.join(ROOT, "lbfgs-ffnn_amd", "build", "lanczos_hip")


@pytest.mark.parametrize("which", ["gn", "hessian"])
def test_cxx_driver_matches_ctypes_bitwise(ctx, pkg, tmp_path, which):
    """drivers/lanczos_hip.cpp (HipSpectrum) in a child process, then the same case through the ctypes path."""
    c = case(pkg, "xent10")
    c["X"].tofile(str(tmp_path / "X.f32"))
    c["Y"].tofile(str(tmp_path / "Y.f32"))
    v0 = RL.start_vector(len(c["P"]), seed=3)
    v0.numpy().tofile(str(tmp_path / "v0.f32"))
    r = subprocess.run([EXE, str(tmp_path), which], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "[RESULT] ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    net = pkg.Mlp(ctx, c["dims"], c["acts"], loss=c["loss"])
    P = net.init_params(seed=19, mode="cuda")
    res = net.lanczos(P, dev(c["X"]), dev(c["Y"]), steps=12, matrix=GN if which == "gn" else HESS, l2=1e-3,
                      v0=v0.cuda())
    got = lambda n, t: np.fromfile(str(tmp_path / n), dtype=t)  # noqa: E731
    assert np.array_equal(got("params.f32", np.float32).view(np.uint32), P.cpu().numpy().view(np.uint32))
    assert open(str(tmp_path / "info.txt")).read().split() == [str(res.steps), str(res.status)] == ["12", "0"]
    for name, arr in (("alpha", res.alpha), ("beta", res.beta), ("ritz", res.ritz), ("weights", res.weights)):
        assert np.array_equal(got(name + ".f64", np.float64).view(np.uint64), arr.view(np.uint64)), name


# ---------------------------------------------------------------- the layers above
def test_unified_launcher_spectrum(ctx, pkg):
    """UnifiedLauncher.spectrum on both splits: a network of its own, inv_scale 1 / rows of the split, the launcher's
    l2; equal bits to Mlp.lanczos with those arguments."""
    c = case(pkg, "xent10")
    data = pkg.UnifiedDataset(train_x=c["X"], train_y=c["Y"], test_x=c["X"][:32], test_y=c["Y"][:32])
    launcher = pkg.UnifiedLauncher()
    for i in range(len(c["acts"])):
        launcher.addLayer(c["dims"][i], c["dims"][i + 1], c["acts"][i])
    launcher.setLoss(c["loss"])
    launcher.setL2(1e-2)
    launcher.buildNetwork()
    with pytest.raises(pkg.LbfError, match="no train split"):
        launcher.spectrum()
    launcher.setData(data)
    with pytest.raises(pkg.LbfError, match="split must be"):
        launcher.spectrum("validation")
    P = launcher.getWrapper().params
    net = pkg.Mlp(ctx, c["dims"], c["acts"], loss=c["loss"])
    for split, rows in (("train", slice(None)), ("test", slice(0, 32))):
        X, Y = dev(c["X"][rows]), dev(c["Y"][rows])
        for matrix in (GN, HESS):
            r = launcher.spectrum(split, steps=10, matrix=matrix, seed=4)
            want = net.lanczos(P, X, Y, steps=10, matrix=matrix, l2=1e-2, inv_scale=1.0 / X.shape[0], seed=4)
            assert same_bits(r, want) and (r.status, r.steps) == (0, 10)
            assert r.ritz[0] >= 1e-2 - 1e-6 or matrix == HESS  # G + l2 I is bounded below by l2
def test_spectral_density_and_ritz_vectors(ctx, pkg):
    c = case(pkg, "xent4")
    net, (P, _, X, Y, idx) = (make_net(pkg, ctx, c), gpu_args(c))
    grid, dens, runs = pkg.spectral_density(net, P, X, Y, probes=3, steps=16, matrix=HESS)
    assert len(runs) == 3 and abs(float(((dens[1:] + dens[:-1]) * 0.5 * np.diff(grid)).sum()) - 1.0) <= 1e-6
    assert not same_bits(runs[0], runs[1])  # one start vector per probe
    r = net.lanczos(P, X, Y, steps=32, matrix=HESS, basis=True)
    y = r.ritz_vectors([0, -1])
    A = RL.dense_matrix(c, HESS)
    for vec, th in zip(y.double().cpu(), (r.ritz[0], r.ritz[-1])):
        assert abs(float(vec @ vec) - 1.0) <= 1e-5
        assert abs(float(vec @ (A @ vec)) - th) <= 1e-4 * norm_of(c, HESS)
