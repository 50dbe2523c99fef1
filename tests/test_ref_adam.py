"""The Adam reference (ref_adam.py) checked on the CPU before the GPU tests rely on it: adam_ref in fp64 is
torch.optim.AdamW's trajectory, its clip coefficient brings the gradient to clip_norm exactly, and on every case and
setting of the GPU tests the fp32 restatement stays within ref_adam.E_MAX of the fp64 run, so the bounds
max(1e-4, 3 x fp32) never exceed 1e-3."""
import numpy as np
import pytest
import torch

import ref_adam
import ref_mlp


def test_fp64_reference_is_torch_adamw(pkg):
    """One case, unclipped (torch's clip_grad_norm_ divides by norm + 1e-6, which is not the solver's rule): the same
    batches through torch.optim.AdamW with decoupled decay, the coupled l2 inside the objective."""
    c = ref_mlp.make_case(pkg, ref_mlp.NETS, "xent4")
    kw = dict(lr=2e-3, weight_decay=1e-2, l2=1e-3, beta1=0.8, beta2=0.99, eps=1e-7)
    N = len(c["rows"])
    orders = ref_adam.epoch_orders_ref(N, 5, 2)
    w, trace = ref_adam.adam_ref(c, torch.float64, orders, epochs=2, batch=16, **kw)
    P, _, X, Y = ref_mlp.host_args(c, torch.float64)
    p = P.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=kw["lr"], betas=(kw["beta1"], kw["beta2"]), eps=kw["eps"],
                            weight_decay=kw["weight_decay"])
    losses = []
    for e in range(2):
        for r0 in range(0, N, 16):
            rows = torch.from_numpy(orders[e][r0:r0 + 16].astype(np.int64))
            opt.zero_grad()
            f = ref_mlp.objective(c["dims"], c["acts"], c["loss"], X[rows], Y[rows], 1.0 / len(rows), kw["l2"])(p)
            f.backward()
            opt.step()
            losses.append(float(f.detach()))
    E = ref_adam.travelled_error(w, p.detach().numpy(), c["P"])
    print("adam_ref fp64 against torch.optim.AdamW: E", E)
    assert E < 1e-10
    assert np.allclose(trace, losses, rtol=1e-11, atol=0.0)
    assert float(np.max(np.abs(w - np.asarray(c["P"], np.float64)))) > 1e-3   # it moved


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_clip_coefficient(dtype):
    g = torch.from_numpy(np.random.default_rng(3).standard_normal(1000)).to(dtype)
    nrm = float(torch.sqrt((g * g).sum()))
    eps = 1e-14 if dtype == torch.float64 else 1e-6
    for clip in (0.25, 0.5 * nrm):
        cg = g * ref_adam.clip_coef(g, clip)
        assert abs(float(torch.sqrt((cg * cg).sum())) / clip - 1.0) < eps   # |c g| = clip_norm
    assert float(ref_adam.clip_coef(g, 2.0 * nrm)) == 1.0    # below the bound: untouched
    assert float(ref_adam.clip_coef(g, 0.0)) == 1.0          # off


def test_clipping_changes_the_trajectory(pkg):
    r0, r1 = ref_adam.reference(pkg, "n387", "defaults"), ref_adam.reference(pkg, "n387", "adamw_clip")
    assert not np.array_equal(r0["w64"], r1["w64"])


def test_epoch_orders_are_permutations_of_one_stream():
    o = ref_adam.epoch_orders_ref(37, 123, 3)
    assert all(np.array_equal(np.sort(r), np.arange(37)) for r in o)
    assert not np.array_equal(o[0], o[1]) and not np.array_equal(o[1], o[2])
    assert np.array_equal(ref_adam.epoch_orders_ref(37, 123, 2), o[:2])


@pytest.mark.parametrize("setting", list(ref_adam.SETTINGS))
@pytest.mark.parametrize("name", ref_adam.CASES)
def test_fp32_restatement_within_the_condition(pkg, name, setting):
    r = ref_adam.reference(pkg, name, setting)
    print(f"{name} {setting}: E32 {r['E32']:.2e}, trace {r['T32']:.2e}, bounds {r['bound']:.1e} {r['trace_bound']:.1e}")
    assert r["E32"] <= ref_adam.E_MAX
    assert r["bound"] <= 1e-3
    assert len(r["trace64"]) == ref_adam.EPOCHS * -(-len(r["case"]["rows"]) // ref_adam.BATCH)
