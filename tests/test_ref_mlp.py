"""ref_mlp.py, the reference every GPU tolerance test is measured against, pinned once on the CPU: against the C oracle
(squared error), against torch's own cross-entropy, its products against each other, its CG against a textbook CG,
and its parameter layout against itself."""
import numpy as np
import pytest
import torch

import ref_mlp as R

ORACLE_NETS = [([784, 128, 10], ["relu", "linear"]),            # test_oracle_vs_torch_autograd's four
               ([20, 30, 40, 5], ["tanh", "sigmoid", "linear"]),
               ([7, 3], ["sigmoid"]),
               ([16, 8, 8, 1], ["relu", "tanh", "linear"]),
               ([64, 48, 16, 1], ["relu", "tanh", "linear"])]
XENT_NETS = [([30, 24, 12, 4], ["sigmoid", "relu", "linear"]), ([64, 32, 10], ["relu", "linear"])]
SMALL_NETS = [([20, 16, 3], ["tanh", "linear"]), ([30, 24, 12, 4], ["sigmoid", "relu", "linear"])]


def problem(dims, N, seed):
    """fp64 tensors (P, v, X, Y) with P at a tenth of N(0,1): activations stay out of saturation."""
    rng = np.random.default_rng(seed)
    n = R.nparams(dims)
    return [torch.from_numpy(a) for a in (0.1 * rng.standard_normal(n), rng.standard_normal(n),
                                          rng.standard_normal((N, dims[0])), rng.standard_normal((N, dims[-1])))]


@pytest.mark.parametrize("N", [97, 257])
@pytest.mark.parametrize("dims,acts", ORACLE_NETS)
def test_loss_grad_matches_the_c_oracle(O, dims, acts, N):
    """test_oracle_vs_torch_autograd's data and bounds."""
    rng = np.random.default_rng(len(dims))
    X = rng.standard_normal((N, dims[0]))
    Y = rng.standard_normal((N, dims[-1]))
    net = O.Net(dims, acts)
    P = net.init_cpu(5)
    l, g = net.loss_grad(P, X, Y)
    lt, gt = R.loss_grad(dims, acts, R.MSE, P, X, Y, 1.0 / N)
    assert abs(l - lt) <= 1e-12 * abs(lt)
    assert np.linalg.norm(g - gt) <= 1e-11 * np.linalg.norm(gt)


@pytest.mark.parametrize("dims,acts", XENT_NETS)
def test_cross_entropy_objective(dims, acts):
    """One-hot targets against torch.nn.functional.cross_entropy, soft targets against -(Y log_softmax).sum(): the same
    <= 37 x 10 fp64 terms summed in another order, so 1e-14 relative."""
    N, inv = 37, 1.0 / 37
    P, _, X, _ = problem(dims, N, 1)
    rng = np.random.default_rng(2)
    z = R.net_out(dims, acts, X)(P)
    labels = torch.from_numpy(rng.integers(0, dims[-1], N))
    hard = torch.nn.functional.one_hot(labels, dims[-1]).double()
    soft = torch.from_numpy(rng.random((N, dims[-1])))
    soft = soft / soft.sum(1, keepdim=True)
    for Y, want in ((hard, torch.nn.functional.cross_entropy(z, labels, reduction="sum") * inv),
                    (soft, -(soft * torch.log_softmax(z, 1)).sum() * inv)):
        got = float(R.objective(dims, acts, R.XENT, X, Y, inv, 0.0)(P))
        assert abs(got - float(want)) <= 1e-14 * abs(float(want)), (got, float(want))
    with_l2 = float(R.objective(dims, acts, R.XENT, X, hard, inv, 1e-2)(P))
    assert with_l2 == float(inv * (hard * (torch.logsumexp(z, 1, keepdim=True) - z)).sum() + 0.5 * 1e-2 * (P * P).sum())


@pytest.mark.parametrize("loss", [R.MSE, R.XENT])
@pytest.mark.parametrize("dims,acts", SMALL_NETS)
def test_gn_ref_is_the_gauss_newton_matrix(dims, acts, loss):
    N, lam = 37, 1e-2
    P, v, X, Y = problem(dims, N, 3)
    Y = Y.abs() if loss == R.XENT else Y   # unnormalised non-negative rows: Ysum varies
    G = R.gn_matrix(dims, acts, loss, P, X, Y, 1.0 / N)
    assert torch.equal(G, G.T) or R.rel(G, G.T) <= 1e-14
    assert R.rel(R.gn_ref(dims, acts, loss, P, v, X, Y, 1.0 / N, lam), G @ v + lam * v) <= 1e-12


def test_hess_ref_is_gn_ref_where_g_is_h():
    """All-linear activations and the squared error. One layer is linear in P, so G = H at any residual; a product of
    layers is not, and there the term G drops is a multiple of the residual: G = H at targets equal to the output."""
    for dims, acts, fitted in (([40, 8], ["linear"], False), ([20, 16, 3], ["linear", "linear"], True)):
        P, v, X, Y = problem(dims, 37, 4)
        if fitted:
            Y = R.net_out(dims, acts, X)(P)
        H = R.hess_ref(dims, acts, R.MSE, P, v, X, Y, 1.0 / 37, 1e-3)
        assert R.rel(H, R.gn_ref(dims, acts, R.MSE, P, v, X, Y, 1.0 / 37, 1e-3)) <= 1e-12


def spd(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return torch.from_numpy(M @ M.T + n * np.eye(n)), torch.from_numpy(rng.standard_normal(n))


def test_pcg_ref_is_textbook_cg_bit_for_bit():
    A, b = spd(50, 6)
    x, r = torch.zeros_like(b), b.clone()
    p, rr = r.clone(), float(r @ r)
    for _ in range(12):
        Ap = A @ p
        alpha = rr / float(p @ Ap)
        x, r = x + alpha * p, r - alpha * Ap
        p, rr = r + (float(r @ r) / rr) * p, float(r @ r)
    got = R.pcg_ref(lambda u: A @ u, b, None, 12, 0.0)
    assert torch.equal(got[0], x) and torch.equal(got[1], r) and got[2:4] == (12, 1)
    ones = R.pcg_ref(lambda u: A @ u, b, torch.ones_like(b), 12, 0.0)
    assert torch.equal(ones[0], x) and torch.equal(ones[1], r) and ones[2:] == got[2:]
    # the stopping rule, and x = 0 for b = 0
    k = R.pcg_ref(lambda u: A @ u, b, None, 200, 1e-6)
    assert k[3] == 0 and k[2] < 200 and k[4][-1] <= 1e-12 < k[4][-2]
    assert R.pcg_ref(lambda u: A @ u, torch.zeros_like(b), None, 5, 0.0)[2:4] == (0, 0)


@pytest.mark.parametrize("dims", [[7, 3], [129, 130, 65, 10]])
def test_layout(dims):
    n = R.nparams(dims)
    P = np.arange(n, dtype=np.float64)
    layers = list(R.unpack(P, dims))
    assert [W.shape for W, _ in layers] == [(i, o) for i, o in zip(dims[:-1], dims[1:])]
    assert [b.shape for _, b in layers] == [(o,) for o in dims[1:]]
    flat = np.concatenate([np.concatenate([W.ravel(), b]) for W, b in layers])
    assert np.array_equal(flat, P)                                   # every coordinate once, in order
    assert np.array_equal(np.concatenate([b for _, b in layers]), P[R.bias_mask(dims)])
    assert int(R.bias_mask(dims).sum()) == sum(dims[1:])
    assert len(list(R.unpack(torch.from_numpy(P), dims))) == len(dims) - 1
