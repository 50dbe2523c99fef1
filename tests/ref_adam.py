"""The torch / numpy reference of the Adam solver (lbf_adam_solve in include/lbfgs_amd.h), for test_ref_adam.py,
test_adam_api.py and test_gpu_adam.py. CPU only: nothing here touches the GPU, and only reference() (its start point
and data) needs the package.

adam_ref works in the dtype it is given, like ref_mlp: fp64 is the reference, fp32 the restatement whose own error sets
the max(1e-4, 3 x fp32) bounds. The epoch orders are an input; epoch_orders_ref restates lbf_adam_epoch_orders on
numpy's MT19937, whose legacy seeding gives the raw stream of std::mt19937(seed).
"""
import numpy as np
import torch

import ref_mlp

EPOCHS, BATCH, SEED = 3, 16, 123
CASES = ["n387", "xent4", "xent10"]   # of ref_mlp.NETS: N = 37 gives batches of 16, 16, 5; N = 257 ends with one row
SETTINGS = {
    "defaults": {},
    "adamw_clip": dict(weight_decay=1e-2, l2=1e-3, clip_norm=0.5),
    "lr1e-2": dict(lr=1e-2),
    "noshuffle": dict(shuffle=0),
}
E_MAX = 3e-4   # a case is used only while the fp32 restatement stays below this (test_ref_adam.py asserts it)


# ---------------------------------------------------------------- epoch orders
def epoch_orders_ref(N, seed, epochs):
    """int32 [epochs][N]: every epoch the identity shuffled by Fisher-Yates downward, for i = N - 1 .. 1:
    j = (draw * (i + 1)) >> 32 with the next raw 32-bit draw of one mt19937(seed), swap positions i and j."""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    out = np.empty((epochs, N), np.int32)
    for e in range(epochs):
        o = list(range(N))
        draws = bg.random_raw(N - 1) if N > 1 else []
        for k, i in enumerate(range(N - 1, 0, -1)):
            j = (int(draws[k]) * (i + 1)) >> 32
            o[i], o[j] = o[j], o[i]
        out[e] = o
    return out


# ---------------------------------------------------------------- coefficients
def coefs_ref(t, lr_now, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, clip_norm=0.0):
    """The nine coefficients of step t as fp64 numbers, in lbf_adam_coef's field order; beta^t by t multiplications."""
    p1 = p2 = 1.0
    for _ in range(t):
        p1 *= beta1
        p2 *= beta2
    return dict(b1=beta1, a1=1.0 - beta1, b2=beta2, a2=1.0 - beta2, step=lr_now / (1.0 - p1),
                rbc2=1.0 / np.sqrt(1.0 - p2), eps=eps, decay=1.0 - lr_now * weight_decay, clip=clip_norm)


def clip_coef(g, clip_norm):
    """c of the step, in g's dtype: 1, or clip_norm / |g| where |g| > clip_norm (no + 1e-6: not torch's rule)."""
    one = torch.ones((), dtype=g.dtype)
    if clip_norm <= 0.0:
        return one
    nrm = torch.sqrt((g * g).sum())
    clip = torch.tensor(clip_norm, dtype=g.dtype)
    return clip / nrm if nrm > clip else one


# ---------------------------------------------------------------- the solver
def adam_ref(c, dtype, orders, epochs=EPOCHS, batch=BATCH, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=0.0, clip_norm=0.0, l2=0.0, decay_rate=1.0, decay_step=0, shuffle=1, seed=None):
    """lbf_adam_solve on the case's rows in `dtype`: (final parameters as an fp64 array, the batch objectives).
    orders: [epochs][N] row orders (ignored with shuffle = 0: the identity). The evaluation is ref_mlp.loss_grad in
    `dtype`; the coefficients are fp64 values cast to `dtype`; m, v, w and every product stay in `dtype`."""
    dims, acts, loss = c["dims"], c["acts"], c["loss"]
    X, Y = c["X"][c["rows"]], c["Y"][c["rows"]]
    N = X.shape[0]
    w = torch.from_numpy(np.asarray(c["P"])).to(dtype)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    trace, t, lr_e = [], 0, lr
    for e in range(epochs):
        if decay_step > 0 and e > 0 and e % decay_step == 0:
            lr_e *= decay_rate
        order = np.asarray(orders[e]) if shuffle else np.arange(N)
        for r0 in range(0, N, batch):
            rows = order[r0:r0 + batch]
            f, g = ref_mlp.loss_grad(dims, acts, loss, w, X[rows], Y[rows], 1.0 / len(rows), l2, dtype)
            trace.append(f)
            t += 1
            k = {n: torch.tensor(x, dtype=dtype) for n, x in
                 coefs_ref(t, lr_e, beta1, beta2, eps, weight_decay, clip_norm).items()}
            g = torch.from_numpy(g).to(dtype)
            gi = g * clip_coef(g, clip_norm)
            m = k["b1"] * m + k["a1"] * gi
            v = k["b2"] * v + k["a2"] * (gi * gi)
            w = w * k["decay"] - k["step"] * (m / (torch.sqrt(v) * k["rbc2"] + k["eps"]))
    return w.double().numpy(), np.asarray(trace, np.float64)


def travelled_error(w, w64, w0):
    """E = max |w - w64| / max |w64 - w0|: the deviation relative to the distance travelled."""
    w, w64, w0 = (np.asarray(a, np.float64) for a in (w, w64, w0))
    return float(np.max(np.abs(w - w64)) / np.max(np.abs(w64 - w0)))


def trace_error(tr, tr64):
    """max_t |tr_t - tr64_t| / |tr64_t| over the batch objectives (all positive)."""
    tr, tr64 = np.asarray(tr, np.float64), np.asarray(tr64, np.float64)
    return float(np.max(np.abs(tr - tr64) / np.abs(tr64)))


_refs = {}


def reference(pkg, name, setting):
    """The fp64 run and the fp32 restatement of a case under a setting, computed once and left unchanged:
    dict(case, kw, orders, w64, trace64, E32, T32, bound, trace_bound)."""
    key = (name, setting)
    if key not in _refs:
        c = ref_mlp.make_case(pkg, ref_mlp.NETS, name)
        kw = SETTINGS[setting]
        orders = epoch_orders_ref(len(c["rows"]), SEED, EPOCHS)
        w64, tr64 = adam_ref(c, torch.float64, orders, **kw)
        w32, tr32 = adam_ref(c, torch.float32, orders, **kw)
        E32, T32 = travelled_error(w32, w64, c["P"]), trace_error(tr32, tr64)
        _refs[key] = dict(case=c, kw=kw, orders=orders, w64=w64, trace64=tr64, E32=E32, T32=T32,
                          bound=max(1e-4, 3.0 * E32), trace_bound=max(1e-4, 3.0 * T32))
    return _refs[key]
