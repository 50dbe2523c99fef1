"""The one torch reference of the network, its objective and its second-order products, for every test that compares
the engine with fp64. CPU only: nothing here imports the package or touches the GPU.

Everything works in the dtype of its arguments, so the same code gives the fp64 reference and the fp32 restatement
whose error sets the max(1e-4, 3 x fp32) bounds.

The rule for what lives here: a helper that two or more test files would define or import. What one file alone uses
(owlqn_ref, the alignment views, a file's own shape tables) stays in that file.

Parameter layout: the layers one after another, each layer its weights W as [In][Out] (row-major, In rows) followed
by its Out biases; a layer computes act(a @ W + b).
"""
import numpy as np
import torch
from torch.func import grad, jacrev, jvp, vjp, vmap

XENT, MSE = "softmax_xent", "mse"
ACTS = {"linear": lambda z: z, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}

# The solver tests' cases. name: dims, acts, loss, rows (N), gathered rows (0: all)
NETS = {
    "n387": ([20, 16, 3], ["tanh", "linear"], MSE, 37, 0),              # n % 4 != 0, n < one CG sweep workgroup
    "xent4": ([30, 24, 12, 4], ["sigmoid", "relu", "linear"], XENT, 37, 0),
    "xent10": ([64, 32, 10], ["relu", "linear"], XENT, 257, 0),
    "mnist": ([784, 128, 10], ["relu", "linear"], XENT, 257, 0),
    "wide": ([784, 512, 256, 10], ["tanh", "tanh", "linear"], MSE, 1000, 64),  # n = 535818: hundreds of workgroups
}
SMALL = ["n387", "xent4", "xent10"]


# ---------------------------------------------------------------- layout
def nparams(dims):
    return sum((dims[i] + 1) * dims[i + 1] for i in range(len(dims) - 1))


def unpack(P, dims):
    """(W [In][Out], b [Out]) of every layer, as views of the flat parameters (a tensor or an array)."""
    off = 0
    for i, o in zip(dims[:-1], dims[1:]):
        yield P[off:off + i * o].reshape(i, o), P[off + i * o:off + (i + 1) * o]
        off += (i + 1) * o


def bias_mask(dims):
    """True on the bias coordinates of the flat parameters."""
    m, off = np.zeros(nparams(dims), bool), 0
    for i, o in zip(dims[:-1], dims[1:]):
        m[off + i * o:off + (i + 1) * o] = True
        off += (i + 1) * o
    return m


# ---------------------------------------------------------------- the network and its objective
def net_out(dims, acts, X):
    """f(P): the network's output on the rows X."""
    def f(P):
        a = X
        for act, (W, b) in zip(acts, unpack(P, dims)):
            a = ACTS[act](a @ W + b)
        return a
    return f


def objective(dims, acts, loss, X, Y, inv_scale, l2):
    """obj(P) = inv_scale * data loss + 0.5 l2 |P|^2; the data loss is 0.5 |a - Y|^2 or sum_o y_o (lse - z_o)."""
    f = net_out(dims, acts, X)

    def obj(P):
        a = f(P)
        data = (Y * (torch.logsumexp(a, 1, keepdim=True) - a)).sum() if loss == XENT else 0.5 * ((a - Y) ** 2).sum()
        return inv_scale * data + 0.5 * l2 * (P * P).sum()
    return obj


def loss_grad(dims, acts, loss, P, X, Y, inv_scale, l2=0.0, dtype=torch.float64):
    """(objective, its gradient as an fp64 array) at P by autograd, computed in `dtype`; arrays or tensors."""
    P, X, Y = (torch.as_tensor(np.asarray(t)).to(dtype) for t in (P, X, Y))
    p = P.clone().requires_grad_(True)
    val = objective(dims, acts, loss, X, Y, inv_scale, l2)(p)
    (g,) = torch.autograd.grad(val, p)
    return float(val.detach()), g.double().numpy()


# ---------------------------------------------------------------- second-order products
def hess_ref(dims, acts, loss, P, v, X, Y, inv_scale, lam):
    """H(P) v + lam v by double backward."""
    return torch.autograd.functional.hvp(objective(dims, acts, loss, X, Y, inv_scale, lam), P, v)[1]


def gn_ref(dims, acts, loss, P, v, X, Y, inv_scale, lam):
    """G(P) v + lam v: J v by jvp of the network output, the loss's Hessian in closed form, J^T(.) by vjp."""
    f = net_out(dims, acts, X)
    out, Jv = jvp(f, (P,), (v,))
    if loss == XENT:
        p = torch.softmax(out, 1)
        HJv = inv_scale * Y.sum(1, keepdim=True) * p * (Jv - (p * Jv).sum(1, keepdim=True))
    else:
        HJv = inv_scale * Jv
    _, pull = vjp(f, P)
    return pull(HJv)[0] + lam * v


def gap(G, H):
    return float((G - H).norm() / H.norm())


def gn_matrix(dims, acts, loss, P, X, Y, inv_scale):
    """The explicit Gauss-Newton matrix from the network's Jacobian (small nets only)."""
    f = net_out(dims, acts, X)
    J = jacrev(f)(P)  # [B, Out, n]
    if loss == XENT:
        p = torch.softmax(f(P), 1)[:, :, None]
        HJ = inv_scale * Y.sum(1)[:, None, None] * p * (J - (p * J).sum(1, keepdim=True))
    else:
        HJ = inv_scale * J
    return torch.einsum("bon,bom->nm", J, HJ)


def grad_sq_ref(dims, acts, loss, P, X, Y, scale, chunk=64):
    """scale * sum_b (d l_b / d P)^2 from per-example gradients, l_b the row's data loss at inv_scale = 1."""
    def row_loss(p, x, y):
        a = net_out(dims, acts, x[None])(p)[0]
        return (y * (torch.logsumexp(a, 0) - a)).sum() if loss == XENT else 0.5 * ((a - y) ** 2).sum()
    per_row = vmap(grad(row_loss), in_dims=(None, 0, 0))
    acc = torch.zeros_like(P)
    for s in range(0, X.shape[0], chunk):
        g = per_row(P, X[s:s + chunk], Y[s:s + chunk])
        acc = acc + (g * g).sum(0)
    return scale * acc


# ---------------------------------------------------------------- CG and the Hessian-free iteration
def pcg_ref(A, b, minv, max_iters, rtol):
    """Preconditioned CG from x = 0 with the engine's rules (minv None: plain CG); (x, r, iterations, status, rrs),
    rrs[k] = r.r / rr0 after iteration k + 1."""
    x, r = torch.zeros_like(b), b.clone()
    z = r if minv is None else minv * r
    p = z.clone()
    rr0 = float(r @ r)
    rz = float(r @ z)
    rrs = []
    if rr0 == 0.0:
        return x, r, 0, 0, rrs
    for k in range(max_iters):
        Ap = A(p)
        pAp = float(p @ Ap)
        if not (pAp > 0.0) or not np.isfinite(pAp) or not (rz > 0.0):
            return x, r, k, 2, rrs
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        rrn = float(r @ r)
        rrs.append(rrn / rr0)
        if rrn <= rtol * rtol * rr0:
            return x, r, k + 1, 0, rrs
        z = r if minv is None else minv * r
        rzn = float(r @ z)
        p = z + (rzn / rz) * p
        rz = rzn
    return x, r, max_iters, 1, rrs


def hf_ref(c, dtype, l2, iters, grad_sq=False, exponent=0.75, refresh=1, damping0=1.0, cg_iters=10, cg_rtol=0.1,
           c1=1e-4, rho=0.5, max_line_iters=20, up=1.5, down=2.0 / 3.0, lo=0.25, hi=0.75):
    """The outer iteration of lbf_hf_solve (lbfgs_amd.h) in `dtype` on the CPU: Armijo backtracking from alpha = 1,
    Levenberg-Marquardt damping from the first trial's reduction ratio. grad_sq: lbf_hf_solve_pc's mode
    LBF_PRECOND_GRAD_SQ, CG preconditioned with M = (D + l2 + lambda)^exponent, D refreshed every `refresh`
    iterations."""
    P, _, X, Y = host_args(c, dtype)
    dims, acts, loss = c["dims"], c["acts"], c["loss"]
    inv = 1.0 / X.shape[0]
    obj = objective(dims, acts, loss, X, Y, inv, l2)
    lam = damping0
    out = dict(loss=[], cg=[], trials=[], accepted=[], alpha=[], damping=[], ratio=[])
    D, minv = None, None
    for it in range(iters):
        Pg = P.clone().requires_grad_(True)
        fv = obj(Pg)
        g, = torch.autograd.grad(fv, Pg)
        f = float(fv.detach())
        b = -g
        if grad_sq:
            if it % refresh == 0:
                D = grad_sq_ref(dims, acts, loss, P, X, Y, inv)
            minv = (D + (l2 + lam)) ** (-exponent)
        x, r, k, _, _ = pcg_ref(lambda v: gn_ref(dims, acts, loss, P, v, X, Y, inv, l2 + lam), b, minv, cg_iters,
                                cg_rtol)
        q = -0.5 * float(x @ (b + r)) - 0.5 * lam * float(x @ x)
        gp = float(g @ x)
        alpha, trials, accepted, f1 = 1.0, 0, 0, f
        for t in range(max_line_iters):
            ft = float(obj(P + alpha * x))
            if t == 0:
                f1 = ft
            trials += 1
            if ft <= f + c1 * alpha * gp:
                accepted = 1
                break
            alpha *= rho
        if accepted:
            P = P + alpha * x
        ratio = (f1 - f) / q
        if ratio < lo:
            lam *= up
        elif ratio > hi:
            lam *= down
        for key, val in zip(("loss", "cg", "trials", "accepted", "alpha", "damping", "ratio"),
                            (f, k, trials, accepted, alpha if accepted else 0.0, lam, ratio)):
            out[key].append(val)
    out["P"] = P
    return out


# ---------------------------------------------------------------- errors and cases
def rel(a, b):
    """|a - b| / |b| in fp64, of arrays or tensors (on any device)."""
    a, b = (t.detach().double().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64) for t in (a, b))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def one_hot(rng, N, Out):
    Y = np.zeros((N, Out), np.float32)
    Y[np.arange(N), rng.integers(0, Out, N)] = 1.0
    return Y


_cases = {}


def make_case(pkg, table, name, loss=None, seed=0, keep_labels=False):
    """Host inputs of a case of `table`, made once: dict(name, dims, acts, loss, P, X, Y, rows, b). The start point is
    the engine's seed-123 CPU-stream init; b is a random right-hand side. A 784-input case takes synth_mnist's rows
    and, for the cross-entropy on ten outputs, its labels; otherwise it draws its targets, unless keep_labels leaves
    the ten one-hot labels in place whatever the loss."""
    key = (name, loss, seed, keep_labels, repr(table[name]))
    if key in _cases:
        return _cases[key]
    dims, acts, dloss, N, gathered = table[name]
    loss = loss or dloss
    rng = np.random.default_rng(1000 * seed + len(dims) * 7 + dims[0])
    if dims[0] == 784:
        X, Y = pkg.synth_mnist(N)
        if not keep_labels and (dims[-1] != 10 or loss != XENT):
            Y = one_hot(rng, N, dims[-1]) if loss == XENT else rng.standard_normal((N, dims[-1])).astype(np.float32)
    else:
        X = rng.standard_normal((N, dims[0])).astype(np.float32)
        Y = one_hot(rng, N, dims[-1]) if loss == XENT else rng.standard_normal((N, dims[-1])).astype(np.float32)
    P = pkg.init_params_host(dims, acts, 123, "cpu")
    rows = rng.permutation(N)[:gathered] if gathered else np.arange(N)
    b = rng.standard_normal(P.size).astype(np.float32)
    _cases[key] = dict(name=name, dims=dims, acts=acts, loss=loss, P=P, X=X, Y=Y, rows=rows, b=b)
    return _cases[key]


def host_args(c, dtype):
    """(P, b, X, Y) of the batch rows as CPU tensors of dtype."""
    r = c["rows"]
    return tuple(torch.from_numpy(np.asarray(t)).to(dtype) for t in (c["P"], c["b"], c["X"][r], c["Y"][r]))
