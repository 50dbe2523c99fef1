"""exact_nets.py on the CPU: the cases of test_gpu_exact.py keep the 2^24 rule and exercise what they are for, fp32
sums of such data do not depend on their order, and assert_bits sees the defects the relative bounds let through.
Run with -s for the per-case table (largest sum of absolute values / 2^24, non-zero share) and the mutation
figures recorded in DESIGN.md §18."""
import numpy as np
import pytest
import torch

import exact_nets as en
import test_gpu_exact as ge
from ref_mlp import gn_ref, hess_ref

CASES = ge.all_cases()


def ident(c):
    return f"{'x'.join(map(str, c[0]))}-B{c[1]}"


def dw_blocks(g, dims):
    return [g[w:b] for w, b, _ in en.layout(dims)]


# dW[i][j] = sum_b a[b][i] delta[b][j] can be non-zero only if some row has both factors non-zero. With the inputs at
# density 48 / 784 and ReLU leaving about half of the deltas, 256 rows reach 1 - (1 - 0.03)^256 > 99.9 % of a block,
# 31 rows 62 %, one row 3 %: the 75 % bound on the block holds from 256 rows; below, it is on the reachable entries
# (at most a quarter of them may cancel to zero).
DENSE_FROM = 256


# ---------------------------------------------------------------- a. range and density

@pytest.mark.parametrize("case", CASES, ids=ident)
def test_case_is_exact_and_dense(case):
    """The range assertion holds (make_case raises otherwise). Every batch row has a residual, every hidden layer
    has Z == 0 entries, and at least 75 % of every weight-gradient block is non-zero (of its reachable entries
    below DENSE_FROM rows, see there)."""
    dims, B, N = case
    c = en.make_case(dims, B, N)
    assert c["worst"] and max(c["worst"].values()) < en.LIMIT
    P64 = c["P"].astype(np.float64)
    shares = []
    for gathered in ([False, True] if c["rows"] is not None else [False]):
        X, Y = en.batch(c, gathered)
        A, Z = en.forward(P64, X, dims)
        assert (A[-1] - Y).any(1).all(), "a batch row without a residual"
        for l in range(1, len(dims) - 1):
            assert (Z[l] == 0).any(), f"hidden layer {l} never sits on the kink"
        g, deltas = en.backward(en.unpack(P64, dims), A, A[-1] - Y)
        for l, blk in enumerate(dw_blocks(g, dims)):
            share = float(np.count_nonzero(blk)) / blk.size
            reach = float(np.count_nonzero(np.abs(A[l]).T @ np.abs(deltas[l]))) / blk.size
            need = 0.75 * (1.0 if B >= DENSE_FROM else reach)
            shares.append(share)
            assert share >= need, f"layer {l} dW: {share:.2f} non-zero, need {need:.2f} (reachable {reach:.2f})"
    name, val = max(c["worst"].items(), key=lambda kv: kv[1])
    print(f"\n| {dims} | {B} | {val / en.LIMIT:.4f} ({name}) | {min(shares):.2f} | "
          f"v {c['thin']['v']} X {c['thin']['X']} W {c['thin']['W']} |")


def test_references_equal_torch_autograd():
    """The numpy references are torch's fp64 autograd results (double backward, jvp / vjp) on integer data, where
    both are exact: equal, not close. relu'(0) = 0 in both."""
    dims, B = [40, 130, 66, 5], 300
    c = en.make_case(dims, B)
    acts = ["relu", "relu", "linear"]
    X, Y = en.batch(c)
    P, v = c["P"].astype(np.float64), c["v"].astype(np.float64)
    t = [torch.from_numpy(a) for a in (P, v, X, Y)]
    assert np.array_equal(en.hvp(P, v, X, Y, dims), hess_ref(dims, acts, "mse", *t, 1.0, 0.0).numpy())
    assert np.array_equal(en.gnvp(P, v, X, Y, dims), gn_ref(dims, acts, "mse", *t, 1.0, 0.0).numpy())
    p = t[0].clone().requires_grad_(True)
    a, off = t[2], 0
    for l in range(3):
        i, o = dims[l], dims[l + 1]
        a = a @ p[off:off + i * o].reshape(i, o) + p[off + i * o:off + (i + 1) * o]
        a = torch.relu(a) if l < 2 else a
        off += (i + 1) * o
    rowloss = 0.5 * ((a - t[3]) ** 2).sum(1)
    (g,) = torch.autograd.grad(rowloss.sum(), p, retain_graph=True)
    assert np.array_equal(en.gradient(P, X, Y, dims), g.numpy())
    assert en.sse(P, X, Y, dims) == 2.0 * rowloss.sum().item()
    per_row = torch.stack([torch.autograd.grad(rowloss[b], p, retain_graph=True)[0] for b in range(40)])
    assert np.array_equal(en.grad_sq(P, X[:40], Y[:40], dims), (per_row ** 2).sum(0).numpy())
    bg = en.batch_gradients(P, X[:256], Y[:256], dims, 4)
    assert np.array_equal(bg.sum(0), en.gradient(P, X[:256], Y[:256], dims))


# ---------------------------------------------------------------- b. order independence

def chunks(n, fracs=(0.0, 0.13, 0.5, 0.51, 1.0)):
    cuts = sorted({int(round(f * n)) for f in fracs})
    return [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]


def mm32(A, B):
    """A @ B in fp32 with the k dimension cut into unequal chunks, each summed on its own."""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for lo, hi in chunks(A.shape[1]):
        acc = acc + (A[:, lo:hi] @ B[lo:hi]).astype(np.float32)
    return acc


def gradient_f32_reordered(c, perm):
    """The gradient in numpy fp32 with the batch rows in the order `perm` and every GEMM's k cut in chunks."""
    dims, B = c["dims"], c["B"]
    layers = en.unpack(c["P"], dims)
    X, Y = c["X"][:B][perm], c["Y"][:B][perm]
    A = [X]
    for l, (W, b) in enumerate(layers):
        z = mm32(A[-1], W) + b
        A.append(z if l == len(layers) - 1 else np.maximum(z, np.float32(0)))
    delta, parts = A[-1] - Y, [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        parts[l] = (mm32(np.ascontiguousarray(A[l].T), delta), mm32(np.ones((1, B), np.float32), delta))
        if l:
            delta = mm32(delta, np.ascontiguousarray(layers[l][0].T)) * (A[l] > 0)
    g = en.pack(parts, np.float32)
    assert g.dtype == np.float32 and all(a.dtype == np.float32 for a in A)
    return g


@pytest.mark.parametrize("case", [([36, 128, 10], 32900), ([129, 130, 65, 10], 2100), ([784, 128, 10], 1000)],
                         ids=ident)
def test_fp32_sums_do_not_depend_on_order(case):
    dims, B = case
    c = en.make_case(dims, B, B + ge.EXTRA_ROWS)
    X, Y = en.batch(c)
    want = en.gradient(c["P"].astype(np.float64), X, Y, dims)
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(B)
        en.assert_bits(gradient_f32_reordered(c, perm), want, f"fp32 gradient, batch order {seed}", dims)


# ---------------------------------------------------------------- c. mutations

def test_assert_bits_catches_what_the_relative_bounds_pass(capsys):
    dims, B = [36, 128, 10], 32900
    c = en.make_case(dims, B, B + ge.EXTRA_ROWS)
    X, Y = en.batch(c)
    P64 = c["P"].astype(np.float64)
    g = en.gradient(P64, X, Y, dims)
    layers = en.unpack(P64, dims)
    A, _ = en.forward(P64, X, dims)
    _, deltas = en.backward(layers, A, A[-1] - Y)
    w0 = dims[0] * dims[1]
    row = int(np.flatnonzero(X.any(1) & deltas[0].any(1))[0])
    one = np.outer(X[row], deltas[0][row]).reshape(-1)
    assert one.any()
    shifted = g.copy()
    shifted[32 * dims[1]:w0] = (np.roll(X[:, 32:], 1, axis=0).T @ deltas[0]).reshape(-1)
    bias = g.copy()
    bias[w0 + 5] += 1.0
    mutants = {"one batch row left out of dW0": np.concatenate([g[:w0] - one, g[w0:]]),
               "one batch row counted twice in dW0": np.concatenate([g[:w0] + one, g[w0:]]),
               "the last 4 input columns' rows shifted by one": shifted,
               "one bias entry off by one unit": bias}
    en.assert_bits(g.astype(np.float32), g, "the reference itself", dims)
    with capsys.disabled():
        print()
        for name, m in mutants.items():
            with pytest.raises(AssertionError) as e:
                en.assert_bits(m.astype(np.float32), g, name, dims)
            rel = np.linalg.norm(m - g) / np.linalg.norm(g)
            print(f"mutation: {name}: |dg| / |g| = {rel:.2e} (the 1e-4 rule "
                  f"{'passes' if rel <= 1e-4 else 'catches'} it); assert_bits: {str(e.value).splitlines()[0]}")
            assert "layer 0" in str(e.value) and "row tile" in str(e.value)
    msg = ""
    try:
        en.assert_bits(shifted.astype(np.float32), g, "shifted", dims, show=10 ** 6)
    except AssertionError as e:
        msg = str(e)
    # the report points at the rows of the last k-tile: inputs 32..35 of layer 0, all in the second 32-row tile
    assert "layer 0 W row 32" in msg and "row 31 " not in msg and "32-row tiles touched: [(0, 1)]" in msg
