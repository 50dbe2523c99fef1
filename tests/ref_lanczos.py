"""The Lanczos iteration of lbf_mlp_lanczos (include/lbfgs_amd.h) in torch, and the dense matrices it is
checked against. CPU only: nothing here imports the package or touches the GPU.

lanczos_ref works in the dtype of its start vector, so the same code is the fp64 reference and the fp32 restatement
whose figures set the 3 x fp32 bounds. Dots and norms are fp64 in both, as on the device.
"""
import numpy as np
import torch

import ref_acts  # noqa: F401  (registers leaky_relu, elu and softplus with ref_mlp.ACTS)
import ref_mlp
from ref_mlp import MSE, gn_matrix, gn_ref, hess_ref, host_args, objective

# Cases beside ref_mlp.NETS. lin63: one linear layer, squared error: G = ([X 1]^T [X 1] / N) (x) I_3 has 7 distinct
# eigenvalues among 21, so every Krylov space is exhausted after 7 steps. n2: two parameters. elu: act'' != 0.
EXTRA = {
    "lin63": ([6, 3], ["linear"], MSE, 37, 0),
    "n2": ([1, 1], ["linear"], MSE, 37, 0),
    "elu": ([20, 16, 3], ["elu", "linear"], MSE, 37, 0),
}
TABLE = dict(ref_mlp.NETS, **EXTRA)


def start_vector(n, seed=0):
    """Mlp.lanczos's default start vector: torch.randn from a CPU generator."""
    return torch.randn(n, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def matvec(c, matrix, dtype, l2=0.0):
    """v -> (G + l2 I) v ("gauss_newton") or (H + l2 I) v ("hessian") of the case's mean batch loss, in dtype."""
    P, _, X, Y = host_args(c, dtype)
    prod = gn_ref if matrix == "gauss_newton" else hess_ref
    return lambda v: prod(c["dims"], c["acts"], c["loss"], P, v, X, Y, 1.0 / X.shape[0], l2)


def hess_matrix(c, l2=0.0):
    """The dense fp64 Hessian of the case's mean batch loss (+ l2 I) by autograd (small nets only)."""
    P, _, X, Y = host_args(c, torch.float64)
    obj = objective(c["dims"], c["acts"], c["loss"], X, Y, 1.0 / X.shape[0], l2)
    H = torch.autograd.functional.hessian(obj, P, vectorize=True)
    return 0.5 * (H + H.T)


_dense = {}


def dense_matrix(c, matrix):
    """The dense fp64 G or H of a case at l2 = 0, made once."""
    key = (c["name"], c["loss"], matrix)
    if key not in _dense:
        if matrix == "gauss_newton":
            P, _, X, Y = host_args(c, torch.float64)
            _dense[key] = gn_matrix(c["dims"], c["acts"], c["loss"], P, X, Y, 1.0 / X.shape[0])
        else:
            _dense[key] = hess_matrix(c)
    return _dense[key]


def lanczos_ref(A, v0, steps, reorth=True, breakdown_rtol=0.0):
    """The iteration on the symmetric operator A (a function of a vector) from v0, in v0's dtype. Returns
    dict(alpha, beta, steps, status, Q): alpha and beta have `steps` entries (the argument), zeros from the returned
    steps on; Q holds the rows q_0 .. that were formed."""
    dt = v0.dtype
    alpha, beta = np.zeros(steps), np.zeros(steps)
    nrm = float(v0.double().norm())
    if not np.isfinite(nrm) or nrm == 0.0:
        return dict(alpha=alpha, beta=beta, steps=0, status=2, Q=torch.zeros((0, v0.numel()), dtype=dt))
    Q = [v0 * torch.tensor(1.0 / nrm, dtype=dt)]
    status, done, scale = 0, steps, 0.0
    for j in range(steps):
        w = A(Q[j])
        rows = torch.stack(Q if reorth else Q[max(0, j - 1):j + 1])
        a = 0.0
        for _ in range(2 if reorth else 1):
            c = rows.double() @ w.double()
            w = w - rows.T @ c.to(dt)
            a += float(c[-1])
        b = float(w.double().norm())
        if not (np.isfinite(a) and np.isfinite(b)):
            status, done = 2, j
            break
        alpha[j], beta[j] = a, b
        scale = max(scale, abs(a))
        if b <= breakdown_rtol * scale:
            status, done = 1, j + 1
            break
        scale = max(scale, b)
        Q.append(w * torch.tensor(1.0 / b, dtype=dt))
    return dict(alpha=alpha, beta=beta, steps=done, status=status, Q=torch.stack(Q))


def ritz(alpha, beta, m):
    """The eigenvalues (ascending) and squared first eigenvector components of T_m by numpy."""
    T = np.diag(alpha[:m]) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    th, S = np.linalg.eigh(T)
    return th, S[0] ** 2


# ---------------------------------------------------------------- the figures the tests bound
def orth_figure(Q):
    """max |Q Q^T - I| of the rows Q, in fp64."""
    Q = torch.as_tensor(Q).double().cpu()
    return float((Q @ Q.T - torch.eye(Q.shape[0], dtype=torch.float64)).abs().max())


def relation_figure(Aq, Q, alpha, beta, steps, norm_A):
    """max_j |A q_j - beta_{j-1} q_{j-1} - alpha_j q_j - beta_j q_{j+1}| / |A| over the steps taken; Aq[j] = A q_j in
    fp64, Q the rows formed (a missing q_steps, after a breakdown, counts as beta_j q_{j+1} = 0)."""
    Q = torch.as_tensor(Q).double().cpu()
    worst = 0.0
    for j in range(steps):
        r = Aq[j] - alpha[j] * Q[j]
        if j > 0:
            r = r - beta[j - 1] * Q[j - 1]
        if j + 1 < Q.shape[0]:
            r = r - beta[j] * Q[j + 1]
        worst = max(worst, float(r.norm()) / norm_A)
    return worst
