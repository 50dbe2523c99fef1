"""Pins the torch restatement of the Lanczos iteration (ref_lanczos.py) that the GPU tests compare the engine with:
its extreme Ritz values are the dense matrices' eigenvalues, its recurrence holds, and it finds the invariant
subspace of the single-layer case. CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from ref_lanczos import (TABLE, dense_matrix, lanczos_ref, matvec, orth_figure, relation_figure, ritz, start_vector)
from ref_mlp import SMALL, make_case

STEPS = {"n387": 24, "xent4": 32, "xent10": 32}


@pytest.mark.parametrize("matrix", ["gauss_newton", "hessian"])
@pytest.mark.parametrize("name", SMALL)
def test_extreme_ritz_values_are_eigenvalues(pkg, name, matrix):
    c = make_case(pkg, TABLE, name)
    A = dense_matrix(c, matrix)
    ev = np.linalg.eigvalsh(A.numpy())
    k = STEPS[name]
    v0 = start_vector(A.shape[0]).double()
    r = lanczos_ref(lambda v: A @ v, v0, k)
    assert r["status"] == 0 and r["steps"] == k
    th, w = ritz(r["alpha"], r["beta"], k)
    norm_A = max(abs(ev[0]), abs(ev[-1]))
    print(f"{name} {matrix}: lambda_max {ev[-1]:.6e} theta_max err {abs(th[-1] - ev[-1]) / ev[-1]:.1e}, "
          f"lambda_min {ev[0]:.3e} theta_min err {abs(th[0] - ev[0]) / norm_A:.1e}")
    assert abs(th[-1] - ev[-1]) <= 1e-8 * ev[-1]
    if name == "xent4" and matrix == "hessian":
        assert ev[0] < 0.0 and abs(th[0] - ev[0]) <= 1e-8 * norm_A
    assert abs(w.sum() - 1.0) <= 1e-12
    assert orth_figure(r["Q"]) <= 1e-12
    Aq = [A @ q for q in r["Q"][:k]]
    assert relation_figure(Aq, r["Q"], r["alpha"], r["beta"], k, norm_A) <= 1e-13
    # the products and the dense matrix are one operator
    prod = matvec(c, matrix, torch.float64)(v0)
    assert float((prod - A @ v0).norm() / (A @ v0).norm()) <= 1e-10


@pytest.mark.parametrize("reorth", [True, False])
def test_three_vector_recurrence_agrees_while_orthogonal(pkg, reorth):
    c = make_case(pkg, TABLE, "n387")
    A = dense_matrix(c, "gauss_newton")
    v0 = start_vector(A.shape[0]).double()
    full = lanczos_ref(lambda v: A @ v, v0, 6)
    r = lanczos_ref(lambda v: A @ v, v0, 6, reorth=reorth)
    assert np.allclose(r["alpha"], full["alpha"], rtol=1e-9) and np.allclose(r["beta"], full["beta"], rtol=1e-9)


def test_single_layer_krylov_space_is_exhausted_after_seven_steps(pkg):
    c = make_case(pkg, TABLE, "lin63")
    A = dense_matrix(c, "gauss_newton")
    ev = np.linalg.eigvalsh(A.numpy())
    distinct = ev.reshape(7, 3).mean(1)
    assert np.abs(ev.reshape(7, 3) - distinct[:, None]).max() <= 1e-12 * ev[-1]
    v0 = start_vector(21)
    prm = pkg._lib.LanczosParams()
    pkg.lib().lbf_lanczos_default_params(ctypes.byref(prm))
    # fp32 stops at the library's default tolerance, which lies between its noise-level and its healthy betas
    for dtype, rtol, tol in ((torch.float64, 1e-10, 1e-9), (torch.float32, prm.breakdown_rtol, 1e-4)):
        r = lanczos_ref(matvec(c, "gauss_newton", dtype), v0.to(dtype), 12, breakdown_rtol=rtol)
        assert (r["status"], r["steps"]) == (1, 7)
        th, _ = ritz(r["alpha"], r["beta"], 7)
        scale = np.abs(r["alpha"][:7]).max()
        print(f"lin63 {dtype}: beta/|A| {r['beta'][:7] / ev[-1]}, ritz err {np.abs(th - distinct).max() / ev[-1]:.1e}")
        assert r["beta"][6] <= rtol * scale and r["beta"][:6].min() >= 0.01 * ev[-1]
        assert np.abs(th - distinct).max() <= tol * ev[-1]
        assert np.all(r["alpha"][7:] == 0.0) and np.all(r["beta"][7:] == 0.0) and r["Q"].shape[0] == 7


def test_two_parameters_stop_at_two(pkg):
    c = make_case(pkg, TABLE, "n2")
    r = lanczos_ref(matvec(c, "gauss_newton", torch.float64), start_vector(2).double(), 4, breakdown_rtol=1e-10)
    assert (r["status"], r["steps"]) == (1, 2)


def test_bad_start_vectors():
    A = torch.eye(5, dtype=torch.float64)
    assert lanczos_ref(lambda v: A @ v, torch.zeros(5, dtype=torch.float64), 3)["status"] == 2
    bad = torch.ones(5, dtype=torch.float64)
    bad[2] = float("nan")
    r = lanczos_ref(lambda v: A @ v, bad, 3)
    assert (r["status"], r["steps"]) == (2, 0)
