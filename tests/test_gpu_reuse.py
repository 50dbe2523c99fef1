"""One network, many calls: every result of a reused Mlp is bitwise the result of a fresh Mlp.

Callers keep one network and change the batch between calls (S-LBFGS alternates b, b_H and N; a validation
split follows a training evaluation), so whatever an Mlp carries from one call to the next (its plan for the last
batch size, the capacity of its activation buffers, the forward state kept for the backward phase, the slabs, the
plan pinned by evaluate) must not change a later result. Evaluations are bitwise reproducible
(test_gpu_parity.py::test_eval_is_deterministic), so the check has no tolerance and needs no oracle: each step of
one sequence on one network equals the same single call on a network created for it.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import dev

pytestmark = pytest.mark.gpu

NETS = [
    ([784, 128, 10], ["relu", "linear"]),
    ([48, 200, 10], ["relu", "linear"]),
    ([784, 300, 20], ["relu", "linear"]),
    ([784, 512, 256, 10], ["relu", "relu", "linear"]),
]
ROWS = 2048


def steps(X, Y, v, idx, empty):
    """(name, loss of the network for the call or None to keep it, call) in the order of the sequence."""
    def lg(n):
        return lambda net, P: net.loss_grad(P, X[:n], Y[:n])

    def ev(net, P):
        r = net.evaluate(P, X, Y, k=2, confusion=True, pred=True, chunk=300)
        return (r.loss, r.rows, r.correct, r.topk, torch.from_numpy(r.confusion), r.pred)

    return [
        ("loss_grad 1000", None, lg(1000)),
        ("loss_grad 31", None, lg(31)),
        ("loss_grad 1000 again", None, lg(1000)),
        ("loss_grad 257 gathered", None, lambda net, P: net.loss_grad(P, X, Y, idx=idx)),
        ("loss 257 gathered", None, lambda net, P: (net.loss(P, X, Y, idx=idx),)),
        ("evaluate 2048 chunk 300", None, ev),
        ("loss_grad 256 (7)", None, lg(256)),
        ("hvp 128", None, lambda net, P: (net.hvp(P, v, X[:128], Y[:128]),)),
        ("loss_grad 256 (9)", None, lg(256)),
        ("loss_grad 0", None, lambda net, P: net.loss_grad(P, X, Y, idx=empty)),
        ("loss_grad 2048", None, lg(2048)),
        ("softmax_xent loss_grad 256", "softmax_xent", lg(256)),
        ("mse loss_grad 256 (13)", "mse", lg(256)),
    ]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            if not torch.equal(x, y):
                return False
        elif x != y:
            return False
    return True


@pytest.mark.parametrize("dims,acts", NETS, ids=["-".join(map(str, d)) for d, _ in NETS])
def test_reused_network_equals_fresh_network_bitwise(ctx, pkg, dims, acts):
    Xh, Yh = pkg.synth_mnist(ROWS, dims[0], dims[-1], 7)
    X, Y = dev(Xh), dev(Yh)
    rng = np.random.default_rng(5)
    idx = torch.from_numpy(rng.permutation(ROWS)[:257].astype(np.int32)).cuda()
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")   # B = 0: a data-parallel rank's empty share
    net = pkg.Mlp(ctx, dims, acts)
    P = net.init_params(123, "cpu")
    v = torch.randn(net.nparams, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    kept, bad = {}, []
    for name, loss, call in steps(X, Y, v, idx, empty):
        if loss is not None:
            net.loss_name = loss
        got = call(net, P)
        fresh = pkg.Mlp(ctx, dims, acts, loss=net.loss_name)
        want = call(fresh, P)
        kept[name] = got
        if not same(got, want):
            bad.append(name)
    assert not bad, f"steps that differ from a fresh network: {bad}"
    l0, g0 = kept["loss_grad 0"]
    assert l0 == 0.0 and not g0.any()
    a, b, c = kept["loss_grad 256 (7)"], kept["loss_grad 256 (9)"], kept["mse loss_grad 256 (13)"]
    assert same(a, b) and same(a, c)
    assert not same(a, kept["softmax_xent loss_grad 256"])   # the loss switch did take effect
