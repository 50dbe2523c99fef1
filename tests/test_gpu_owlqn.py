"""OWL-QN: the orthant-wise sweeps (Mlp.l1_pseudo_grad / Mlp.l1_trial, lbfgs-ffnn_amd/csrc/owlqn.hip)
and the solver built on them (engine.owlqn_solve / lbf_owlqn_solve).

The sweeps are compared bitwise with numpy fp32 restatements of lbfgs_amd.h's rules on crafted vectors that hold
every branch; their sums with fp64 sums of the same fp32 values (1e-12 relative: both sides sum in fp64, only the
order differs). The solver's reference is the algorithm of lbfgs_amd.h restated in torch fp64 on the CPU; the same
code in fp32 gives the deviation an fp32 implementation is allowed.

Bounds. Trajectories: line-search decisions equal, F and parameters within max(1e-3, 3 x the CPU fp32 restatement's
deviation), the project's trajectory rule; the zero pattern may differ from fp64 on max(2, 3 x the fp32
restatement's count) coordinates. The reference is first shown to keep every Armijo test 1e-4 |F| away from
equality and every pair's y.s ten times above the storing threshold, so an fp32 evaluation cannot flip a decision.
LASSO: 1e-4 against fp64 coordinate descent (the fp64 restatement reaches 5.9e-9, the fp32 one 5.8e-6).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import dev, make_net, run_ranks, solver_inputs
from ref_mlp import NETS, SMALL, XENT, bias_mask, make_case, nparams, objective, rel

pytestmark = pytest.mark.gpu

F32 = np.float32


def case(pkg, name, loss=None, seed=0):
    """The sweeps read only the shapes of `wide`; the solver cases are the ungathered ones."""
    return make_case(pkg, NETS, name, loss, seed)


# ---------------------------------------------------------------- the sweeps in numpy fp32
def pseudo_np(x, g, cv):
    """lbfgs_amd.h step 1; cv = c_i as fp32. Every value is one fp32 add."""
    gp, gm = (g + cv).astype(F32), (g - cv).astype(F32)
    at0 = np.where(gm > 0, gm, np.where(gp < 0, gp, F32(0.0)))
    return np.where(x > 0, gp, np.where(x < 0, gm, at0)).astype(F32)


def trial_np(x, d, pg, alpha, pen):
    """Steps 2 to 4: alpha is a power of two, so alpha * d is exact and x + alpha * d rounds once, like fmaf. The
    sign test and the projection are the penalised coordinates'; the free ones take the plain step."""
    keep = ~pen | ((d > 0) & (pg < 0)) | ((d < 0) & (pg > 0))
    t = (x + (F32(alpha) * np.where(keep, d, F32(0.0))).astype(F32)).astype(F32)
    xi = np.where(x != 0, np.sign(x), np.sign(-pg))
    return np.where(~pen | ((t != 0) & (np.sign(t) == xi)), t, F32(0.0)).astype(F32)


def crafted(dims, seed, l1):
    """x, g, d with every branch of both sweeps, biases included: x positive, negative and zero; at zero g > c,
    g < -c and |g| <= c; d with and against pg; steps that cross zero and steps that land exactly on it."""
    n = nparams(dims)
    rng = np.random.default_rng(seed)
    c = F32(l1)
    x = rng.standard_normal(n).astype(F32)
    x[rng.random(n) < 0.35] = 0.0
    x[rng.random(n) < 0.02] = -0.0
    g = (rng.standard_normal(n) * 2.0 * c).astype(F32)          # |g| <= c on about 38 % of the coordinates
    d = (rng.standard_normal(n) * 2.0).astype(F32)              # |alpha d| > |x| often: many crossings
    hit = (rng.random(n) < 0.1) & (x != 0)                      # land on zero at alpha = 0.5: pg has the sign of x,
    g[hit] = (np.sign(x[hit]) * (np.abs(g[hit]) + 2 * c)).astype(F32)   # d = -2 x opposes it, fmaf gives 0 exactly
    d[hit] = -2.0 * x[hit]
    b = bias_mask(dims)
    for arr in (x, g, d):                                       # the few biases hold the branches too
        assert np.isfinite(arr).all()
    x[np.flatnonzero(b)[::3]] = 0.0
    return x, g, d


def sweep_sums(x, pg, xn, pen, l1):
    x64, p64, n64 = x.astype(np.float64), pg.astype(np.float64), xn.astype(np.float64)
    return dict(pg_norm=float(np.sqrt((p64 * p64).sum())), l1_x=l1 * float(np.abs(x64[pen]).sum()),
                zeros_x=int((x[pen] == 0).sum()), l1_term=l1 * float(np.abs(n64[pen]).sum()),
                ww=float((n64 * n64).sum()), dec=float((p64 * (n64 - x64)).sum()), zeros=int((xn[pen] == 0).sum()))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("l1_bias", [False, True], ids=["weights", "weights+biases"])
@pytest.mark.parametrize("name", ["n387", "xent10", "wide"])
def test_sweeps_bitwise_against_numpy(ctx, pkg, name, l1_bias):
    dims, l1 = NETS[name][0], 0.1
    net = pkg.Mlp(ctx, dims, NETS[name][1])
    x, g, d = crafted(dims, 11, l1)
    pen = np.ones(x.size, bool) if l1_bias else ~bias_mask(dims)
    cv = np.where(pen, F32(l1), F32(0.0)).astype(F32)
    want_pg = pseudo_np(x, g, cv)
    at0 = x == 0
    assert (at0 & (g - cv > 0)).any() and (at0 & (g + cv < 0)).any() and (at0 & (want_pg == 0) & (g != 0)).any()
    xd, gd, dd = dev(x), dev(g), dev(d)
    pg, st = net.l1_pseudo_grad(xd, gd, l1, l1_bias)
    got_pg = pg.cpu().numpy()
    assert np.array_equal(bits(got_pg), bits(want_pg))
    assert st["penalised"] == int(pen.sum())
    for alpha in (1.0, 0.5, 0.125):
        want = trial_np(x, d, want_pg, alpha, pen)
        assert np.array_equal(bits(want[~pen]), bits((x + F32(alpha) * d).astype(F32)[~pen]))  # the biases, when free
        keep = pen & (((d > 0) & (want_pg < 0)) | ((d < 0) & (want_pg > 0)))
        t = (x + (F32(alpha) * np.where(keep, d, F32(0.0))).astype(F32)).astype(F32)
        assert (pen & ~keep & (d != 0)).any() and (keep & (x != 0) & (t != 0) & (np.sign(t) != np.sign(x))).any()  # crossings
        if alpha == 0.5:
            assert (keep & (x != 0) & (t == 0)).sum() > x.size // 40                               # exact landings
        xn, sm = net.l1_trial(xd, dd, pg, l1, alpha, l1_bias)
        got = xn.cpu().numpy()
        assert np.array_equal(bits(got), bits(want))                   # the sign bit too: every clipped value is +0.0
        assert not np.signbit(got[pen & (got == 0)]).any()
        ref = sweep_sums(x, want_pg, want, pen, l1)
        assert st["zeros"] == ref["zeros_x"] and sm["zeros"] == ref["zeros"]
        assert close(st["pg_norm"], ref["pg_norm"]) and close(st["l1_term"], ref["l1_x"])
        for k in ("l1_term", "ww", "dec"):
            assert close(sm[k], ref[k]), (k, sm[k], ref[k])
        xn2, sm2 = net.l1_trial(xd, dd, pg, l1, alpha, l1_bias)        # run to run
        assert torch.equal(xn, xn2) and sm == sm2
    pg2, st2 = net.l1_pseudo_grad(xd, gd, l1, l1_bias)
    assert torch.equal(pg, pg2) and st == st2


@pytest.mark.parametrize("mixed", [False, True], ids=["all-offset", "mixed-offsets"])
@pytest.mark.parametrize("name", ["n387", "xent10", "wide"])
def test_sweeps_unaligned_pointers(ctx, pkg, name, mixed):
    """Every vector one float off a 16-byte boundary (the float4 body behind a scalar head), and only some of them
    (the all-scalar sweep): the same bits, and the words around the outputs untouched."""
    dims, l1, alpha = NETS[name][0], 0.1, 0.5
    net = pkg.Mlp(ctx, dims, NETS[name][1])
    x, g, d = crafted(dims, 12, l1)
    n = x.size
    xd, gd, dd = dev(x), dev(g), dev(d)
    pg, st = net.l1_pseudo_grad(xd, gd, l1)
    xn, sm = net.l1_trial(xd, dd, pg, l1, alpha)
    bufs = [torch.full((n + 8,), 1234.5, device="cuda") for _ in range(5)]
    offs = [1, 0, 1, 0, 1] if mixed else [1] * 5
    xu, gu, du, pu, ou = (t[o:n + o] for t, o in zip(bufs, offs))
    assert xu.data_ptr() % 16 == 4
    xu.copy_(xd)
    gu.copy_(gd)
    du.copy_(dd)
    keep = [t.clone() for t in bufs[:3]]
    pg_u, st_u = net.l1_pseudo_grad(xu, gu, l1, out=pu)
    xn_u, sm_u = net.l1_trial(xu, du, pu, l1, alpha, out=ou)
    assert pg_u.data_ptr() == pu.data_ptr() and xn_u.data_ptr() == ou.data_ptr()
    assert torch.equal(pg_u, pg) and torch.equal(xn_u, xn)
    assert st_u["zeros"] == st["zeros"] and sm_u["zeros"] == sm["zeros"]
    assert close(st_u["pg_norm"], st["pg_norm"]) and close(st_u["l1_term"], st["l1_term"])
    for k in ("l1_term", "ww", "dec"):
        assert close(sm_u[k], sm[k]), k
    for t, k in zip(bufs[:3], keep):
        assert torch.equal(t, k)
    for t, o in zip(bufs[3:], offs[3:]):
        assert bool((t[:o] == 1234.5).all()) and bool((t[n + o:] == 1234.5).all())


def test_trial_ww_is_the_point_s_own(ctx, pkg):
    """The trial's x+.x+ and the data loss of x+ add up to what a full evaluation of x+ reports under weight decay."""
    c = case(pkg, "xent10")
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    _, g = net.loss_grad(P, X, Y)
    pg, _ = net.l1_pseudo_grad(P, g, 1e-2)
    xn, sm = net.l1_trial(P, -pg, pg, 1e-2, 0.5)
    f, _ = net.loss_grad(xn, X, Y, l2=1e-3)
    assert abs(net.loss(xn, X, Y) + 0.5e-3 * sm["ww"] - f) <= 1e-6 * abs(f)


# ---------------------------------------------------------------- the reference (any dtype, CPU)
def owlqn_ref(c, dtype, l1, l2, iters, m=10, l1_bias=False, c1=1e-4, rho=0.5, max_line_iters=20, tol=0.0):
    """lbf_owlqn_solve's iteration (lbfgs_amd.h) in `dtype` on the CPU. Also returns the smallest Armijo slack
    |F(x+) - (F + c1 dec)| / |F| over all trials and the smallest y.s over all pairs."""
    P, X, Y = (torch.from_numpy(np.asarray(t)).to(dtype) for t in (c["P"], c["X"], c["Y"]))
    dims = c["dims"]
    obj = objective(dims, c["acts"], c["loss"], X, Y, 1.0 / X.shape[0], l2)
    pen = torch.from_numpy(np.ones(P.numel(), bool) if l1_bias else ~bias_mask(dims))
    cv = torch.where(pen, torch.tensor(l1, dtype=dtype), torch.tensor(0.0, dtype=dtype))
    zero = torch.zeros((), dtype=dtype)

    def fg(x):
        xg = x.clone().requires_grad_(True)
        fv = obj(xg)
        g, = torch.autograd.grad(fv, xg)
        return float(fv.detach()), g

    def pseudo(x, g):
        gp, gm = g + cv, g - cv
        at0 = torch.where(gm > 0, gm, torch.where(gp < 0, gp, zero))
        return torch.where(x > 0, gp, torch.where(x < 0, gm, at0))

    def penalty(x):
        return float((cv.double() * x.double().abs()).sum())

    x = P.clone()
    f, g = fg(x)
    F = f + penalty(x)
    pg = pseudo(x, g)
    S, Yl = [], []
    out = dict(loss=[], trials=[], accepted=[], alpha=[], slack=np.inf, ys=np.inf)
    for k in range(iters):
        pgn = float(pg.double().norm())
        if pgn < tol or pgn == 0.0:
            break
        q = pg.clone()
        al = []
        for s, y in zip(reversed(S), reversed(Yl)):
            a = float(s @ q) / float(y @ s)
            al.append(a)
            q = q - a * y
        if S:
            q = q * (float(S[-1] @ Yl[-1]) / float(Yl[-1] @ Yl[-1]))
        for (s, y), a in zip(zip(S, Yl), reversed(al)):
            b = float(y @ q) / float(y @ s)
            q = q + (a - b) * s
        d = -q
        d = torch.where(~pen | ((d > 0) & (pg < 0)) | ((d < 0) & (pg > 0)), d, zero)
        xi = torch.where(x != 0, torch.sign(x), torch.sign(-pg))
        alpha = min(1.0, 1.0 / pgn) if k == 0 else 1.0
        trials, accepted = 0, 0
        for _ in range(max_line_iters):
            t = x + alpha * d
            xn = torch.where(~pen | ((t != 0) & (torch.sign(t) == xi)), t, zero)
            dec = float((pg.double() * (xn.double() - x.double())).sum())
            Ft = float(obj(xn)) + penalty(xn)
            trials += 1
            out["slack"] = min(out["slack"], abs(Ft - (F + c1 * dec)) / abs(F))
            if Ft <= F + c1 * dec:
                accepted = 1
                break
            alpha *= rho
        for key, val in zip(("loss", "trials", "accepted", "alpha"), (F, trials, accepted, alpha if accepted else 0.0)):
            out[key].append(val)
        if not accepted:
            break
        _, gn = fg(xn)
        s, y = xn - x, gn - g
        ys = float(y.double() @ s.double())
        out["ys"] = min(out["ys"], ys)
        if ys > 1e-10 and m > 0:
            S.append(s)
            Yl.append(y)
            if len(S) > m:
                S.pop(0)
                Yl.pop(0)
        x, g, F = xn, gn, Ft
        pg = pseudo(x, g)
    out["P"], out["F"], out["pg_norm"] = x, F, float(pg.double().norm())
    return out


# ---------------------------------------------------------------- trajectories
TRAJ = [(n, l, l1, l2) for n in SMALL for l in ("mse", XENT) for l1 in (1e-3, 1e-2) for l2 in (0.0, 1e-3)]
# Data seed picked on the CPU (seed 0 fails with an Armijo slack of 6.5e-7 |F| on one case, seed 1 with 3.2e-5): on
# all 24 cases the fp64 reference accepts all 20 iterations, its smallest Armijo slack is 1.40e-4 |F| and its
# smallest y.s 7.6e-4, and the fp32 restatement takes the same decisions with the same zero pattern.
TRAJ_SEED = 2
TRAJ_ITERS = 20


@pytest.mark.parametrize("name,loss,l1,l2", TRAJ, ids=[f"{n}-{l}-l1={a}-l2={b}" for n, l, a, b in TRAJ])
def test_owlqn_trajectory_matches_fp64(ctx, pkg, name, loss, l1, l2):
    c = case(pkg, name, loss, TRAJ_SEED)
    ref = owlqn_ref(c, torch.float64, l1, l2, TRAJ_ITERS)
    assert len(ref["loss"]) == TRAJ_ITERS and all(ref["accepted"])
    assert ref["slack"] >= 1e-4, ref["slack"]
    assert ref["ys"] >= 1e-9, ref["ys"]
    r32 = owlqn_ref(c, torch.float32, l1, l2, TRAJ_ITERS)
    own_f = float(np.abs(np.array(r32["loss"]) - np.array(ref["loss"])).max()) if len(r32["loss"]) == TRAJ_ITERS else 0.0
    own_p = rel(r32["P"], ref["P"])
    own_z = int(((r32["P"] == 0) != (ref["P"] == 0)).sum())
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    hist, info, stats = pkg.owlqn_solve(net, P, X, Y, max_iters=TRAJ_ITERS, tol=0.0, m=10, l1=l1)
    df = float(np.abs(hist["loss"] - np.array(ref["loss"])).max())
    dp = rel(P, ref["P"])
    dz = int(((P.cpu() == 0) != (ref["P"] == 0)).sum())
    print(f"owlqn {name} {loss} l1={l1} l2={l2}: F dev {df:.2e} (cpu fp32 {own_f:.2e}), params rel {dp:.2e} "
          f"({own_p:.2e}), pattern {dz} ({own_z}), zeros {stats['zeros']}/{stats['penalised']}, "
          f"slack {ref['slack']:.1e}, min y.s {ref['ys']:.1e}, trials {list(hist['ls_trials'])}")
    assert info.iterations == TRAJ_ITERS
    assert list(hist["ls_trials"]) == ref["trials"] and list(hist["accepted"]) == ref["accepted"]
    assert df <= max(1e-3, 3 * own_f)
    assert abs(info.final_loss - ref["F"]) <= max(1e-3, 3 * own_f)
    assert dp <= max(1e-3, 3 * own_p)
    assert dz <= max(2, 3 * own_z)


def test_owlqn_without_history(ctx, pkg):
    """m = 0: projected steepest descent on the pseudo-gradient, against the same restatement."""
    c = case(pkg, "xent10")
    ref = owlqn_ref(c, torch.float64, 1e-2, 0.0, 6, m=0)
    assert ref["slack"] >= 1e-4
    P, X, Y = solver_inputs(c)
    hist, info, _ = pkg.owlqn_solve(make_net(pkg, ctx, c), P, X, Y, max_iters=6, tol=0.0, m=0, l1=1e-2)
    assert list(hist["ls_trials"]) == ref["trials"] and list(hist["accepted"]) == ref["accepted"]
    assert float(np.abs(hist["loss"] - np.array(ref["loss"])).max()) <= 1e-3 and rel(P, ref["P"]) <= 1e-3


# ---------------------------------------------------------------- LASSO known answer
def lasso_cd(X, Y, l1, sweeps=400):
    """min over (W, b) of 0.5 / N |X W + b - Y|^2 + l1 |W|_1 by cyclic coordinate descent in fp64."""
    N, In = X.shape
    W, b = np.zeros((In, Y.shape[1])), Y.mean(0)
    R = Y - b
    cn = (X * X).sum(0) / N
    for _ in range(sweeps):
        for j in range(In):
            rho = X[:, j] @ R / N + cn[j] * W[j]
            wj = np.sign(rho) * np.maximum(np.abs(rho) - l1, 0.0) / cn[j]
            R += np.outer(X[:, j], W[j] - wj)
            W[j] = wj
        db = R.mean(0)
        b += db
        R -= db
    return np.concatenate([W.ravel(), b])


def test_owlqn_lasso_known_answer(ctx, pkg):
    dims, acts, N, l1 = [40, 8], ["linear"], 257, 0.05
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 40)).astype(np.float32)
    Y = rng.standard_normal((N, 8)).astype(np.float32)
    want = lasso_cd(X.astype(np.float64), Y.astype(np.float64), l1)
    c = dict(dims=dims, acts=acts, loss="mse", P=pkg.init_params_host(dims, acts, 123, "cpu"), X=X, Y=Y,
             rows=np.arange(N))
    r64 = owlqn_ref(c, torch.float64, l1, 0.0, 20)
    r32 = owlqn_ref(c, torch.float32, l1, 0.0, 20)
    e64, e32 = float(np.abs(r64["P"].numpy() - want).max()), float(np.abs(r32["P"].double().numpy() - want).max())
    net = pkg.Mlp(ctx, dims, acts)
    P, Xd, Yd = solver_inputs(c)
    hist, info, stats = pkg.owlqn_solve(net, P, Xd, Yd, max_iters=20, tol=0.0, l1=l1)
    got = P.double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"lasso: max abs {err:.2e} (restatement fp64 {e64:.2e}, fp32 {e32:.2e}), zeros {stats['zeros']} of "
          f"{stats['penalised']}, {info.iterations} iterations")
    assert err <= 1e-4
    assert np.array_equal(got == 0, want == 0)
    assert stats["zeros"] == int((want[:320] == 0).sum()) and stats["penalised"] == 320


# ---------------------------------------------------------------- properties
def test_owlqn_properties(ctx, pkg):
    c = case(pkg, "mnist")
    l1, l2 = 1e-3, 1e-3
    net = make_net(pkg, ctx, c, l2=l2)
    P, X, Y = solver_inputs(c)
    P0 = P.clone()
    hist, info, stats = pkg.owlqn_solve(net, P, X, Y, max_iters=15, tol=0.0, l1=l1)
    assert info.iterations == 15 and len(hist["loss"]) == 15
    assert np.all(np.diff(hist["loss"]) <= 0.0), hist["loss"]
    assert info.final_loss <= hist["loss"][-1]
    b = torch.from_numpy(bias_mask(c["dims"])).cuda()
    zeros = int((P[~b] == 0).sum())
    assert stats["zeros"] > 0 and stats["zeros"] == zeros and stats["penalised"] == int((~b).sum())
    assert not bool(((P[b] == 0) & (P0[b] != 0)).any())  # l1_bias = 0: no bias is zeroed
    assert stats["zeros_trace"][-1] == zeros and len(stats["zeros_trace"]) == 15
    assert info.n_evals == 1 + int(hist["accepted"].sum())
    assert info.n_loss_only == int(hist["ls_trials"].sum())
    assert info.n_grad_after_loss == int(hist["accepted"].sum())
    Pd = P.double()
    F = net.loss(P, X, Y) + 0.5 * l2 * float(Pd @ Pd) + l1 * float(Pd[~b].abs().sum())
    assert abs(info.final_loss - F) <= 1e-6 * abs(F)
    assert abs(stats["l1_term"] - l1 * float(Pd[~b].abs().sum())) <= 1e-12 * stats["l1_term"]
    _, g = net.loss_grad(P, X, Y, l2=l2)
    _, st = net.l1_pseudo_grad(P, g, l1)
    assert abs(st["pg_norm"] - info.final_grad_norm) <= 1e-5 * st["pg_norm"] and st["zeros"] == zeros
    # the penalty on the biases too: they are counted, and they may become zero
    Pb = P0.clone()
    _, _, sb = pkg.owlqn_solve(make_net(pkg, ctx, c, l2=l2), Pb, X, Y, max_iters=5, tol=0.0, l1=l1, l1_bias=True)
    assert sb["penalised"] == P.numel() and sb["zeros"] == int((Pb == 0).sum())
    # run to run
    P2 = P0.clone()
    h2, i2, s2 = pkg.owlqn_solve(make_net(pkg, ctx, c, l2=l2), P2, X, Y, max_iters=15, tol=0.0, l1=l1)
    assert torch.equal(P, P2) and np.array_equal(hist["loss"], h2["loss"])


def test_owlqn_invalid_parameters(ctx, pkg):
    c = case(pkg, "n387")
    net = make_net(pkg, ctx, c)
    P, X, Y = solver_inputs(c)
    for kw in (dict(l1=-1.0), dict(l1=float("nan")), dict(l1=float("inf")), dict(m=129), dict(m=-1),
               dict(max_iters=-1), dict(rho=1.0), dict(rho=0.0), dict(max_line_iters=0)):
        with pytest.raises(pkg.LbfError, match="status 1"):
            pkg.owlqn_solve(net, P, X, Y, **{**dict(max_iters=2), **kw})
    assert torch.equal(P, dev(c["P"]))
    with pytest.raises(pkg.LbfError, match="status 1"):
        net.l1_pseudo_grad(P, P, -0.5)
    hist, info, _ = pkg.owlqn_solve(net, P, X, Y, max_iters=0)
    assert info.iterations == 0 and len(hist["loss"]) == 0 and torch.equal(P, dev(c["P"]))
    L = pkg.lib()
    p = pkg.engine.owlqn_params(max_iters=1)
    assert L.lbf_owlqn_solve(net.h, C.byref(p), None, None, None, 0, 1, None, None, None) == 1  # null parameters


# ---------------------------------------------------------------- two ranks
@pytest.mark.parametrize("split", [100, 0], ids=["unequal", "empty-shard"])
def test_world2_owlqn(ctx, pkg, split):
    c = case(pkg, "xent10")
    N = len(c["X"])
    kw = dict(max_iters=8, tol=0.0, l1=1e-2)
    P, X, Y = solver_inputs(c)
    h1, i1, s1 = pkg.owlqn_solve(make_net(pkg, ctx, c, l2=1e-3), P, X, Y, **kw)
    bounds = [(0, split), (split, N)]

    def body(r, cx):
        lo, hi = bounds[r]
        Pr = dev(c["P"])
        h, i, s = pkg.owlqn_solve(make_net(pkg, cx, c, l2=1e-3), Pr, X[lo:hi].contiguous(), Y[lo:hi].contiguous(),
                                  n_global=N, **kw)
        return Pr, h, s

    out = run_ranks(pkg, 2, body)
    assert torch.equal(out[0][0], out[1][0])
    for k in ("loss", "grad_norm", "ls_trials", "accepted", "alpha"):
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    assert np.array_equal(out[0][2]["zeros_trace"], out[1][2]["zeros_trace"])
    for k in ("ls_trials", "accepted"):
        assert np.array_equal(out[0][1][k], h1[k]), k
    # the first step is min(1, 1 / |pg|) of a gradient summed over the shards in another order: equal to rounding
    np.testing.assert_allclose(out[0][1]["alpha"], h1["alpha"], rtol=1e-5, atol=0)
    err = rel(out[0][0], P)
    print(f"world 2 owlqn (split {split}): params against one rank rel {err:.2e}")
    assert err <= 1e-5


# ---------------------------------------------------------------- unified layer
def test_unified_owlqn(ctx, pkg, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    c = case(pkg, "xent10")
    data = pkg.UnifiedDataset(train_x=c["X"], train_y=c["Y"], test_x=c["X"][:32], test_y=c["Y"][:32])
    cfg = pkg.UnifiedConfig(name="owlqn_test", max_iters=6, tolerance=0.0, l1=1e-3, loss=XENT)
    launcher = pkg.UnifiedLauncher()
    for i in range(len(c["acts"])):
        launcher.addLayer(c["dims"][i], c["dims"][i + 1], c["acts"][i])
    launcher.buildNetwork()
    launcher.setData(data)
    opt = pkg.UnifiedOWLQN()
    launcher.train(opt, cfg)
    assert opt.info.iterations == 6 and opt.stats["zeros"] > 0
    P, X, Y = solver_inputs(c)
    hist, info, stats = pkg.owlqn_solve(make_net(pkg, ctx, c), P, X, Y, max_iters=6, tol=0.0, m=10, l1=1e-3)
    assert torch.equal(launcher.net_wrapper_.params, P)
    assert np.array_equal(opt.history["loss"], hist["loss"]) and opt.stats["zeros"] == stats["zeros"]
    csvs = list(tmp_path.rglob("*.csv"))
    assert csvs and any("owlqn_test" in p.name for p in csvs)
