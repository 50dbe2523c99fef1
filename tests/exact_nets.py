"""Exactly representable networks: data on which every GEMM route must give the fp64 result bit for bit.

If every operand of a sum of products is a small integer and the sum of the absolute values of the products stays
below 2^24, then every product and every partial sum is an integer of at most 24 bits and so an fp32 number: the
fp32 result is the exact one in any order, tiling or split, with or without fused multiply-adds. The
engine's GEMMs are true fp32 MFMA, so on such data one dropped, doubled or misplaced element is a difference of at
least one unit, where the suite's relative bounds (1e-4, 1e-5) let it pass.

make_case() builds such a problem for a ReLU / linear-output network under the squared error and asserts the 2^24
rule on every sum any kernel may form; the references below are plain fp64 numpy at inv_scale = 1 (the tests scale
by powers of two, which is exact); assert_bits() compares and says where in which GEMM tile a difference lies.

Parameter layout: the engine's, per layer [W (in x out, row-major) | b (out)].
"""
import functools

import numpy as np

LIMIT = float(2 ** 24)
L2 = 2.0 ** -6  # the tests' weight decay: a power of two, so l2 * w is exact


# ---------------------------------------------------------------- layout

def layout(dims):
    """Per layer (offset of W, offset of b, end) in the flat parameter vector."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        w = dims[l] * dims[l + 1]
        out.append((off, off + w, off + w + dims[l + 1]))
        off += w + dims[l + 1]
    return out


def unpack(P, dims):
    """[(W (in x out), b (out))] views of the flat vector P."""
    return [(P[w:b].reshape(dims[l], dims[l + 1]), P[b:e]) for l, (w, b, e) in enumerate(layout(dims))]


def pack(parts, dtype=np.float64):
    return np.concatenate([np.concatenate([W.reshape(-1), b.reshape(-1)]) for W, b in parts]).astype(dtype)


def log2_floor(B):
    """p of the tests' inv_scale = 2**-p."""
    return int(B).bit_length() - 1


# ---------------------------------------------------------------- fp64 references (inv_scale = 1) with their ranges

class Range:
    """The largest sum of absolute values met, by name of the sum."""

    def __init__(self):
        self.worst = {}

    def see(self, name, bound):
        v = float(np.max(bound)) if np.size(bound) else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), v)

    def over(self):
        return {k: v for k, v in self.worst.items() if not v < LIMIT}


def forward(P, X, dims, rng=None):
    """Activations A[0..nl] (A[0] = X, A[nl] the linear outputs) and pre-activations Z[1..nl] (Z[0] unused)."""
    A, Z = [np.asarray(X, np.float64)], [None]
    layers = unpack(np.asarray(P, np.float64), dims)
    for l, (W, b) in enumerate(layers):
        z = A[-1] @ W + b
        if rng is not None:
            rng.see("forward GEMM", np.abs(A[-1]) @ np.abs(W) + np.abs(b))
        Z.append(z)
        A.append(z if l == len(layers) - 1 else np.maximum(z, 0.0))
    return A, Z


def outputs(P, X, dims):
    return forward(P, X, dims)[0][-1]


def sse(P, X, Y, dims, rng=None):
    """sum (out - Y)^2; the loss at inv_scale s and weight decay l2 is 0.5 s sse + 0.5 l2 |P|^2."""
    d = outputs(P, X, dims) - Y
    if rng is not None:
        rng.see("sum (out - Y)^2", (d * d).sum())
        rng.see("sum P^2", float(np.dot(P.astype(np.float64), P.astype(np.float64))))
    return float((d * d).sum())


def backward(layers, A, delta, rng=None, tag="d"):
    """[dW | db] of every layer for the output-layer delta; returns the packed vector and the deltas."""
    nl = len(layers)
    parts, deltas = [None] * nl, [None] * nl
    for l in range(nl - 1, -1, -1):
        deltas[l] = delta
        parts[l] = (A[l].T @ delta, delta.sum(0))
        if rng is not None:
            rng.see(f"{tag}W / {tag}b sum", np.abs(A[l]).T @ np.abs(delta))
            rng.see(f"{tag}W / {tag}b sum", np.abs(delta).sum(0))
        if l:
            if rng is not None:
                rng.see(f"{tag}X GEMM", np.abs(delta) @ np.abs(layers[l][0]).T)
            delta = (delta @ layers[l][0].T) * (A[l] > 0)  # relu'(y) = [y > 0]: 0 at the kink
    return pack(parts), deltas


def gradient(P, X, Y, dims, rng=None):
    """d/dP of 0.5 sum (out - Y)^2."""
    A, _ = forward(P, X, dims, rng)
    return backward(unpack(np.asarray(P, np.float64), dims), A, A[-1] - Y, rng)[0]


def r_forward(layers, vl, A, rng=None):
    """R{A[l]} along v (R{X} = 0) and R{out}."""
    RA = [np.zeros_like(A[0])]
    for l, ((W, b), (V, vb)) in enumerate(zip(layers, vl)):
        rz = RA[-1] @ W + A[l] @ V + vb
        if rng is not None:
            rng.see("R-forward GEMMs", np.abs(RA[-1]) @ np.abs(W) + np.abs(A[l]) @ np.abs(V) + np.abs(vb))
        RA.append(rz if l == len(layers) - 1 else rz * (A[l + 1] > 0))
    return RA


def hvp(P, v, X, Y, dims, rng=None):
    """Exact Hessian-vector product of 0.5 sum (out - Y)^2 (R-operator; relu'' = 0, so no curvature term)."""
    P, v = np.asarray(P, np.float64), np.asarray(v, np.float64)
    layers, vl = unpack(P, dims), unpack(v, dims)
    nl = len(layers)
    A, _ = forward(P, X, dims)  # rng: the first-order sums are gradient()'s and grad_sq()'s to report
    _, deltas = backward(layers, A, A[-1] - Y)
    RA = r_forward(layers, vl, A, rng)
    parts, rd = [None] * nl, RA[-1]
    for l in range(nl - 1, -1, -1):
        parts[l] = (RA[l].T @ deltas[l] + A[l].T @ rd, rd.sum(0))
        if rng is not None:
            rng.see("R-pass dW / db sum", np.abs(RA[l]).T @ np.abs(deltas[l]) + np.abs(A[l]).T @ np.abs(rd))
            rng.see("R-pass dW / db sum", np.abs(rd).sum(0))
        if l:
            if rng is not None:
                rng.see("R-pass dX GEMMs", np.abs(rd) @ np.abs(layers[l][0]).T + np.abs(deltas[l]) @ np.abs(vl[l][0]).T)
            rd = (rd @ layers[l][0].T + deltas[l] @ vl[l][0].T) * (A[l] > 0)
    return pack(parts)


def gnvp(P, v, X, Y, dims, rng=None):
    """Gauss-Newton product J^T J v of 0.5 sum (out - Y)^2 (H_L = I at the outputs)."""
    P, v = np.asarray(P, np.float64), np.asarray(v, np.float64)
    layers = unpack(P, dims)
    A, _ = forward(P, X, dims)
    RA = r_forward(layers, unpack(v, dims), A)  # rng: hvp() reports the R-forward sums
    return backward(layers, A, RA[-1], rng, tag="G")[0]


def grad_sq(P, X, Y, dims, rng=None):
    """sum_b (d l_b / dP)^2, l_b = 0.5 |out_b - Y_b|^2: every term is non-negative, the sum is its own bound."""
    P = np.asarray(P, np.float64)
    layers = unpack(P, dims)
    A, _ = forward(P, X, dims, rng)
    _, deltas = backward(layers, A, A[-1] - Y, rng)
    out = pack([((A[l] ** 2).T @ (deltas[l] ** 2), (deltas[l] ** 2).sum(0)) for l in range(len(layers))])
    if rng is not None:
        rng.see("squared-gradient sum", out)
    return out


def batch_gradients(P, X, Y, dims, nmb):
    """Gradients of nmb consecutive equal minibatches, (nmb, nparams)."""
    cnt = X.shape[0] // nmb
    return np.stack([gradient(P, X[i * cnt:(i + 1) * cnt], Y[i * cnt:(i + 1) * cnt], dims) for i in range(nmb)])


def scaled(ref, p, P=None, l2=0.0):
    """ref * 2**-p + l2 * P as fp32, asserting that the cast loses nothing."""
    want = np.asarray(ref, np.float64) * 2.0 ** -p
    if l2:
        want = want + l2 * np.asarray(P, np.float64)
    w32 = want.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), want), "the expected value is no fp32 number"
    return w32


def loss_value(s, p, P=None, l2=0.0):
    """0.5 * 2**-p * sse + 0.5 * l2 * |P|^2, exact in fp64 (every term a dyadic rational of few bits)."""
    val = 0.5 * 2.0 ** -p * s
    if l2:
        val += 0.5 * l2 * float(np.dot(np.asarray(P, np.float64), np.asarray(P, np.float64)))
    return val


# ---------------------------------------------------------------- the generator

def sparse_ints(rng, shape, lo, hi, density):
    """Integers lo..hi without 0 at `density` of the entries, 0 elsewhere."""
    vals = rng.integers(lo, hi, shape, endpoint=True)
    vals = np.where(vals == 0, rng.choice([lo, hi], shape), vals)
    return np.where(rng.random(shape) < density, vals, 0).astype(np.float64)


def build(dims, B, N, seed, thin, draw=0):
    """Draw number `draw` at the densities thinned by 2**-thin[k] (k = 'v', 'X', 'W')."""
    rng = np.random.default_rng([seed, draw, B, N] + list(dims))
    dX = min(1.0, 48.0 / dims[0]) / 2 ** thin["X"]
    X = sparse_ints(rng, (N, dims[0]), -2, 2, dX)
    parts, vparts = [], []
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        dW = min(1.0, max(6.0 / i, 4.0 / o)) / 2 ** thin["W"]
        parts.append((sparse_ints(rng, (i, o), -1, 1, dW), rng.integers(0, 2, o, endpoint=True).astype(np.float64)))
        dv = 0.25 * dW / 2 ** thin["v"]
        vparts.append((sparse_ints(rng, (i, o), -1, 1, dv), sparse_ints(rng, (o,), -1, 1, 0.25 / 2 ** thin["v"])))
    P, v = pack(parts), pack(vparts)
    noise = rng.integers(-1, 1, (N, dims[-1]), endpoint=True).astype(np.float64)
    dead = np.flatnonzero(~noise.any(1))  # every row keeps a residual
    noise[dead, rng.integers(0, dims[-1], dead.size)] = rng.choice([-1.0, 1.0], dead.size)
    Y = outputs(P, X, dims) + noise
    rows = rng.integers(0, N, B) if N > B else None  # with repeats
    return P, v, X, Y, rows


def ranges(dims, P, v, X, Y):
    first, second = Range(), Range()
    sse(P, X, Y, dims, first)
    grad_sq(P, X, Y, dims, first)  # forward, backward and the squared sums
    hvp(P, v, X, Y, dims, second)
    gnvp(P, v, X, Y, dims, second)
    return first, second


@functools.lru_cache(maxsize=None)
def _make_case(dims, B, N, seed):
    thin, draw = {"v": 0, "X": 0, "W": 0}, 0
    for _ in range(48):
        P, v, X, Y, rows = build(dims, B, N, seed, thin, draw)
        sels = [slice(0, B)] + ([rows] if rows is not None else [])
        # a batch of a few rows may miss ReLU's kink in a narrow layer: then the next draw (of the same densities)
        if not all((z == 0).any() for sel in sels for z in forward(P, X[sel], dims)[1][1:-1]):
            draw += 1
            continue
        first, second = Range(), Range()
        for sel in sels:
            f, s = ranges(dims, P, v, X[sel], Y[sel])
            for dst, src in ((first, f), (second, s)):
                for k, val in src.worst.items():
                    dst.see(k, val)
        # what does not fit is thinned in the order v, X, W (never B or the widths: those select the route)
        if not first.over() and not second.over():
            break
        only_v = not first.over() and not any(k in first.worst for k in second.over())
        key = "v" if only_v and thin["v"] < 3 else ("X" if thin["X"] < 3 else "W")
        thin[key] += 1
    worst = dict(second.worst)
    worst.update(first.worst)
    over = {k: val for k, val in worst.items() if not val < LIMIT}
    assert not over, f"{dims} at {B} rows: sums of absolute values not below 2^24 at any density tried: {over}"
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    case = dict(dims=list(dims), B=B, N=N, p=log2_floor(B), thin=dict(thin), draw=draw, worst=worst,
                P=f32(P), v=f32(v), X=f32(X), Y=f32(Y), rows=rows)
    for k in ("P", "v", "X", "Y"):
        case[k].setflags(write=False)
    return case


def make_case(dims, B, N=None, seed=0):
    """Integer-valued fp32 P, v, X (N rows), Y and, when N > B, `rows`: B gathered indices with repeats. Every sum
    of absolute values on the first B rows and on the gathered rows is asserted below 2^24; `worst` maps each sum's
    name to its largest value, `thin` gives the halvings of the densities of v, X and W that this took, `p` is
    floor(log2 B). Every hidden layer has Z == 0 entries on both selections (`draw` draws were skipped for that).
    The arrays are shared between callers and read-only."""
    N = B if N is None else N
    assert N >= B >= 1
    return _make_case(tuple(int(d) for d in dims), int(B), int(N), int(seed))


def batch(case, gathered=False):
    """(X, Y) fp64 of the case's batch: its first B rows, or its gathered rows."""
    sel = case["rows"] if gathered else slice(0, case["B"])
    return case["X"][sel].astype(np.float64), case["Y"][sel].astype(np.float64)


# ---------------------------------------------------------------- the comparison

def tiles(i):
    return "/".join(f"{i // t}" for t in (32, 64, 128))


def locate(i, dims):
    """Flat parameter index -> (layer, 'W' | 'b', row = input, col = output)."""
    for l, (w, b, e) in enumerate(layout(dims)):
        if i < b:
            return l, "W", (i - w) // dims[l + 1], (i - w) % dims[l + 1]
        if i < e:
            return l, "b", dims[l], i - b  # the bias row is row `in` of the layer's [in + 1] x out dW GEMM
    raise IndexError(i)


def assert_bits(got, want, what, dims=None, show=8):
    """got == want bit for bit (np.array_equal in got's dtype; want must be representable in it). On a difference:
    how many entries differ, the first few with their place and the 32 / 64 / 128-aligned row and column tile of
    the GEMM that wrote them (dims given: a flat parameter vector, or rows of them; else a [rows][cols] array)."""
    got = np.asarray(got)
    want = np.asarray(want, np.float64)
    w = want.astype(got.dtype)
    assert np.array_equal(w.astype(np.float64), want), f"{what}: the reference is not representable in {got.dtype}"
    assert got.shape == w.shape, f"{what}: shape {got.shape}, expected {w.shape}"
    if np.array_equal(got, w):
        return
    g2, w2 = np.atleast_1d(got), np.atleast_1d(w)
    bad = np.argwhere(g2 != w2)
    lines = [f"{what}: {len(bad)} of {g2.size} entries differ from the exact result"]
    rows_seen, cols_seen = set(), set()
    for k, ix in enumerate(bad):
        ix = tuple(int(t) for t in ix)
        if dims is not None:
            l, kind, r, c = locate(ix[-1], dims)
            where = f"layer {l} {kind} row {r} col {c}" + (f" (vector {ix[0]})" if len(ix) > 1 else "")
            rows_seen.add((l, r // 32))
            cols_seen.add((l, c // 32))
        else:
            r, c = (ix + (0,))[:2] if len(ix) < 2 else ix[-2:]
            where = f"row {r} col {c}"
            rows_seen.add(r // 32)
            cols_seen.add(c // 32)
        if k < show:
            lines.append(f"  {where}: got {g2[ix]!r}, want {w2[ix]!r}, diff {float(g2[ix]) - float(w2[ix]):g}; "
                         f"row tile (32/64/128) {tiles(r)} at offsets {r % 32}/{r % 64}/{r % 128}, "
                         f"col tile {tiles(c)} at offsets {c % 32}/{c % 64}/{c % 128}")
    lines.append(f"  32-row tiles touched: {sorted(rows_seen)[:16]}; 32-column tiles touched: {sorted(cols_seen)[:16]}")
    raise AssertionError("\n".join(lines))
