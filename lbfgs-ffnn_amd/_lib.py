"""ctypes binding of ``build/liblbfgs_amd_abi3.so`` (C ABI: ``include/lbfgs_amd.h``).

The shared library is the product: every numeric operation below runs in its HIP kernels. There is
no CPU fallback; a missing or unloadable library raises :class:`LbfError` immediately.
torch is imported first so that the HIP runtime torch loaded (SONAME ``libamdhip64.so.7``) is the
one the library binds to, and torch tensors are used purely as device allocations.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ABI_VERSION = 3  # include/lbfgs_amd.h LBF_ABI_VERSION (also in the library's file name)
LIB_PATH = os.environ.get("LBF_LIB_PATH") or os.path.join(_HERE, "build", f"liblbfgs_amd_abi{ABI_VERSION}.so")
SLBFGS_DP_REPLICATED, SLBFGS_DP_SLICED = 0, 1
HVP_MODES = {"fd": 0, "exact": 1, "gauss_newton": 2}  # LBF_HVP_FD, LBF_HVP_EXACT, LBF_HVP_GAUSS_NEWTON
LS_WOLFE, LS_ARMIJO = 0, 1
INIT_CPU, INIT_CUDA = 0, 1
# LBF_ACT_* of include/lbfgs_amd.h (leaky_relu: slope 0.01, elu: alpha 1; fixed, as torch's defaults)
ACTS = {"linear": 0, "tanh": 1, "relu": 2, "sigmoid": 3, "leaky_relu": 4, "elu": 5, "softplus": 6}
LOSSES = {"mse": 0, "softmax_xent": 1}  # LBF_LOSS_MSE, LBF_LOSS_SOFTMAX_XENT
LANCZOS_MATRICES = {"hessian": 1, "gauss_newton": 2}  # LBF_HVP_EXACT, LBF_HVP_GAUSS_NEWTON (lbf_mlp_lanczos)
PRECONDS = {"none": 0, "grad_sq": 1}  # LBF_PRECOND_NONE, LBF_PRECOND_GRAD_SQ


class LbfError(RuntimeError):
    pass


class LbfgsParams(C.Structure):
    _fields_ = [("m", C.c_int), ("max_iters", C.c_int), ("tol", C.c_double), ("line_search", C.c_int),
                ("max_line_iters", C.c_int), ("c1", C.c_double), ("c2", C.c_double), ("rho", C.c_double)]


class SlbfgsParams(C.Structure):
    _fields_ = [("max_epochs", C.c_int), ("tol", C.c_double), ("M", C.c_int), ("L", C.c_int), ("b", C.c_int),
                ("b_H", C.c_int), ("step", C.c_double), ("reg", C.c_double), ("seed", C.c_uint),
                ("fd_eps", C.c_double), ("hvp_exact", C.c_int), ("pair_trace", C.POINTER(C.c_double)),
                ("pair_trace_cap", C.c_int), ("dp_mode", C.c_int)]


class GdParams(C.Structure):
    _fields_ = [("lr", C.c_double), ("momentum", C.c_double), ("max_iters", C.c_int), ("tol", C.c_double)]


class SgdParams(C.Structure):
    _fields_ = [("lr", C.c_double), ("momentum", C.c_double), ("batch", C.c_int), ("decay_rate", C.c_double),
                ("decay_step", C.c_int), ("max_epochs", C.c_int), ("tol", C.c_double)]


class CgParams(C.Structure):  # lbf_cg_params
    _fields_ = [("max_iters", C.c_int), ("rtol", C.c_double), ("damping", C.c_double), ("check", C.c_int)]


class CgInfo(C.Structure):  # lbf_cg_info
    _fields_ = [("iterations", C.c_int), ("status", C.c_int), ("rr0", C.c_double), ("rr", C.c_double),
                ("xb", C.c_double), ("xr", C.c_double), ("xx", C.c_double)]


class LanczosParams(C.Structure):  # lbf_lanczos_params
    _fields_ = [("steps", C.c_int), ("matrix", C.c_int), ("reorth", C.c_int), ("check", C.c_int),
                ("l2", C.c_double), ("breakdown_rtol", C.c_double)]


class LanczosInfo(C.Structure):  # lbf_lanczos_info
    _fields_ = [("steps", C.c_int), ("status", C.c_int), ("v0_norm", C.c_double)]


class HfParams(C.Structure):  # lbf_hf_params
    _fields_ = [("max_iters", C.c_int), ("tol", C.c_double), ("cg_iters", C.c_int), ("cg_rtol", C.c_double),
                ("cg_check", C.c_int), ("damping0", C.c_double), ("damp_up", C.c_double), ("damp_down", C.c_double),
                ("ratio_lo", C.c_double), ("ratio_hi", C.c_double), ("c1", C.c_double), ("rho", C.c_double),
                ("max_line_iters", C.c_int), ("curv_rows", C.c_longlong), ("damping_trace", C.POINTER(C.c_double)),
                ("ratio_trace", C.POINTER(C.c_double)), ("cg_trace", C.POINTER(C.c_int)), ("trace_cap", C.c_int)]


class HfPrecond(C.Structure):  # lbf_hf_precond
    _fields_ = [("mode", C.c_int), ("exponent", C.c_double), ("refresh", C.c_int)]


class OwlqnParams(C.Structure):  # lbf_owlqn_params
    _fields_ = [("m", C.c_int), ("max_iters", C.c_int), ("tol", C.c_double), ("l1", C.c_double),
                ("l1_bias", C.c_int), ("c1", C.c_double), ("rho", C.c_double), ("max_line_iters", C.c_int),
                ("zeros_trace", C.POINTER(C.c_longlong)), ("trace_cap", C.c_int)]


class OwlqnStats(C.Structure):  # lbf_owlqn_stats
    _fields_ = [("zeros", C.c_longlong), ("penalised", C.c_longlong), ("l1_term", C.c_double),
                ("pg_norm", C.c_double)]


class AdamParams(C.Structure):  # lbf_adam_params
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("clip_norm", C.c_double), ("batch", C.c_int), ("shuffle", C.c_int),
                ("seed", C.c_uint), ("decay_rate", C.c_double), ("decay_step", C.c_int), ("max_epochs", C.c_int),
                ("tol", C.c_double), ("loss_trace", C.POINTER(C.c_double)), ("trace_cap", C.c_int)]


class AdamCoef(C.Structure):  # lbf_adam_coef
    _fields_ = [(k, C.c_float) for k in ("b1", "a1", "b2", "a2", "step", "rbc2", "eps", "decay", "clip")]


class Record(C.Structure):
    _fields_ = [("loss", C.POINTER(C.c_double)), ("grad_norm", C.POINTER(C.c_double)),
                ("time_ms", C.POINTER(C.c_double)), ("alpha", C.POINTER(C.c_double)),
                ("ls_trials", C.POINTER(C.c_int)), ("accepted", C.POINTER(C.c_int)), ("cap", C.c_int),
                ("size", C.c_int)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int), ("n_evals", C.c_longlong), ("final_loss", C.c_double),
                ("final_grad_norm", C.c_double), ("n_rows", C.c_longlong), ("n_loss_only", C.c_longlong),
                ("n_grad_after_loss", C.c_longlong)]


class EvalResultC(C.Structure):  # lbf_eval_result
    _fields_ = [("loss", C.c_double), ("rows", C.c_longlong), ("correct", C.c_longlong), ("topk", C.c_longlong),
                ("k", C.c_int), ("reserved", C.c_int)]


_lib = None
_vp, _ip, _dp, _fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)

# (restype, argtypes) of every function include/lbfgs_amd.h declares: the one place a new entry point is named
_SIG = {
    "lbf_last_error": (C.c_char_p, []),
    "lbf_version": (C.c_char_p, []),
    "lbf_abi_version": (C.c_int, []),
    "lbf_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "lbf_ctx_destroy": (C.c_int, [_vp]),
    "lbf_ctx_sync": (C.c_int, [_vp]),
    "lbf_ctx_stream": (_vp, [_vp]),
    "lbf_comm_unique_id": (C.c_int, [C.c_char_p]),
    "lbf_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "lbf_comm_init_local": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "lbf_comm_rank": (C.c_int, [_vp, _ip, _ip]),
    "lbf_allreduce_sum": (C.c_int, [_vp, _vp, C.c_size_t]),
    "lbf_mlp_create": (C.c_int, [_vp, C.c_int, _ip, _ip, C.POINTER(_vp)]),
    "lbf_mlp_destroy": (C.c_int, [_vp]),
    "lbf_mlp_param_count": (C.c_longlong, [_vp]),
    "lbf_mlp_init_params": (C.c_int, [_vp, C.c_uint, C.c_int, _vp]),
    "lbf_init_params_host": (C.c_int, [C.c_int, _ip, _ip, C.c_uint, C.c_int, _vp]),
    "lbf_mlp_forward": (C.c_int, [_vp, _vp, _vp, C.c_longlong, _vp]),
    "lbf_mlp_loss_grad": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.c_double, _dp]),
    "lbf_mlp_batch_grads": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_longlong, C.c_double, C.c_double, _vp,
                                      C.c_longlong]),
    "lbf_two_loop": (C.c_int, [_vp, C.c_longlong, C.c_int, _vp, _vp, _dp, _vp, _vp, C.c_int]),
    "lbf_dot": (C.c_int, [_vp, C.c_longlong, _vp, _vp, _dp]),
    "lbf_nrm2": (C.c_int, [_vp, C.c_longlong, _vp, _dp]),
    "lbf_axpy": (C.c_int, [_vp, C.c_longlong, C.c_float, _vp, _vp]),
    "lbf_scal": (C.c_int, [_vp, C.c_longlong, C.c_float, _vp]),
    "lbf_lbfgs_default_params": (None, [C.POINTER(LbfgsParams), C.c_int]),
    "lbf_slbfgs_default_params": (None, [C.POINTER(SlbfgsParams)]),
    "lbf_lbfgs_solve": (C.c_int, [_vp, C.POINTER(LbfgsParams), _vp, _vp, _vp, C.c_longlong, C.c_longlong,
                                  C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_lbfgs_begin": (C.c_int, [_vp, C.POINTER(LbfgsParams), _vp, _vp, _vp, C.c_longlong, C.c_longlong,
                                  C.POINTER(_vp)]),
    "lbf_lbfgs_iterate": (C.c_int, [_vp, C.c_int, C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_lbfgs_end": (C.c_int, [_vp]),
    "lbf_lbfgs_solve_fn": (C.c_int, [_vp, C.POINTER(LbfgsParams), C.c_longlong, _vp, _vp, _vp,
                                     C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_device_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "lbf_device_free": (C.c_int, [_vp, _vp]),
    "lbf_memcpy": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int]),
    "lbf_slbfgs_solve": (C.c_int, [_vp, C.POINTER(SlbfgsParams), _vp, _vp, _vp, C.c_longlong, C.POINTER(Record),
                                   C.POINTER(SolveInfo)]),
    "lbf_slbfgs_begin": (C.c_int, [_vp, C.POINTER(SlbfgsParams), _vp, _vp, _vp, C.c_longlong, C.POINTER(_vp)]),
    "lbf_slbfgs_iterate": (C.c_int, [_vp, C.c_int, C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_slbfgs_end": (C.c_int, [_vp]),
    "lbf_slbfgs_pair0": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "lbf_slbfgs_pair_io": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "lbf_prof_enable": (C.c_int, [_vp, C.c_int]),
    "lbf_prof_select": (C.c_int, [_vp, C.c_int]),
    "lbf_prof_sample": (C.c_int, [_vp, C.c_int]),
    "lbf_prof_read": (C.c_int, [_vp, C.c_int, _ip, _dp, C.POINTER(C.c_longlong), _ip]),
    "lbf_prof_read_work": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip]),
    "lbf_synth_mnist": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_uint, _vp, _vp]),
    "lbf_sample_indices": (C.c_int, [C.c_longlong, C.c_int, C.c_uint, C.c_int, _vp]),
    "lbf_idx_read_images": (C.c_int, [C.c_char_p, C.c_longlong, _vp, C.POINTER(C.c_longlong), _ip, _ip]),
    "lbf_idx_read_labels": (C.c_int, [C.c_char_p, C.c_longlong, C.c_int, _vp, C.POINTER(C.c_longlong)]),
    "lbf_mlp_hvp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.c_double, _vp]),
    "lbf_mlp_gnvp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.c_double, _vp]),
    "lbf_mlp_loss": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, _dp]),
    "lbf_mlp_fd_hvp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.c_double,
                                 C.c_double, _vp]),
    "lbf_gd_default_params": (None, [C.POINTER(GdParams)]),
    "lbf_sgd_default_params": (None, [C.POINTER(SgdParams)]),
    "lbf_gd_solve": (C.c_int, [_vp, C.POINTER(GdParams), _vp, _vp, _vp, C.c_longlong, C.c_longlong,
                               C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_sgd_solve": (C.c_int, [_vp, C.POINTER(SgdParams), _vp, _vp, _vp, C.c_longlong, C.POINTER(Record),
                                C.POINTER(SolveInfo)]),
    "lbf_synth_regression": (C.c_int, [_vp, C.c_longlong, C.c_longlong, C.c_int, C.c_uint, C.c_uint, _vp, _vp]),
    "lbf_mlp_set_loss": (C.c_int, [_vp, C.c_int]),
    "lbf_mlp_get_loss": (C.c_int, [_vp, _ip]),
    "lbf_mlp_set_l2": (C.c_int, [_vp, C.c_double]),
    "lbf_mlp_get_l2": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "lbf_cg_default_params": (None, [C.POINTER(CgParams)]),
    "lbf_mlp_gn_cg": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.POINTER(CgParams), _vp,
                                C.POINTER(CgInfo)]),
    "lbf_mlp_gn_cg_residual": (C.c_int, [_vp, _vp]),
    "lbf_hf_default_params": (None, [C.POINTER(HfParams)]),
    "lbf_hf_solve": (C.c_int, [_vp, C.POINTER(HfParams), _vp, _vp, _vp, C.c_longlong, C.c_longlong,
                               C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_mlp_grad_sq": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, _vp]),
    "lbf_mlp_gn_pcg": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.POINTER(CgParams),
                                 _vp, C.POINTER(CgInfo)]),
    "lbf_hf_precond_default": (None, [C.POINTER(HfPrecond)]),
    "lbf_hf_solve_pc": (C.c_int, [_vp, C.POINTER(HfParams), C.POINTER(HfPrecond), _vp, _vp, _vp, C.c_longlong,
                                  C.c_longlong, C.POINTER(Record), C.POINTER(SolveInfo)]),
    "lbf_lanczos_default_params": (None, [C.POINTER(LanczosParams)]),
    "lbf_mlp_lanczos": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.POINTER(LanczosParams),
                                  _dp, _dp, _vp, C.c_longlong, C.POINTER(LanczosInfo)]),
    "lbf_tridiag_eig": (C.c_int, [C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "lbf_owlqn_default_params": (None, [C.POINTER(OwlqnParams)]),
    "lbf_owlqn_solve": (C.c_int, [_vp, C.POINTER(OwlqnParams), _vp, _vp, _vp, C.c_longlong, C.c_longlong,
                                  C.POINTER(Record), C.POINTER(SolveInfo), C.POINTER(OwlqnStats)]),
    "lbf_mlp_l1_pseudo_grad": (C.c_int, [_vp, _vp, _vp, C.c_double, C.c_int, _vp, C.POINTER(OwlqnStats)]),
    "lbf_mlp_l1_trial": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_float, _vp, _dp, _dp, _dp,
                                   C.POINTER(C.c_longlong)]),
    "lbf_adam_default_params": (None, [C.POINTER(AdamParams)]),
    "lbf_adam_coefs": (C.c_int, [C.POINTER(AdamParams), C.c_double, C.c_longlong, C.POINTER(AdamCoef)]),
    "lbf_adam_epoch_orders": (C.c_int, [C.c_longlong, C.c_uint, C.c_int, _vp]),
    "lbf_adam_step": (C.c_int, [_vp, C.c_longlong, C.POINTER(AdamCoef), _vp, _vp, _vp, _vp, _vp]),
    "lbf_adam_solve": (C.c_int, [_vp, C.POINTER(AdamParams), _vp, _vp, _vp, C.c_longlong, C.POINTER(Record),
                                 C.POINTER(SolveInfo)]),
    "lbf_adam_begin": (C.c_int, [_vp, C.POINTER(AdamParams), _vp, _vp, _vp, C.c_longlong, C.POINTER(_vp)]),
    "lbf_adam_iterate": (C.c_int, [_vp, C.c_int, C.POINTER(Record), C.POINTER(SolveInfo), _ip]),
    "lbf_adam_end": (C.c_int, [_vp]),
    "lbf_mlp_evaluate": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_longlong, C.c_double, C.c_int, C.c_longlong,
                                   C.POINTER(EvalResultC), _vp, _vp, _vp]),
}
EXPORTS = tuple(_SIG)


def lib():
    """Load the HIP library (raises LbfError if it is missing: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbfError(f"{os.path.basename(LIB_PATH)} not built ({LIB_PATH}); run `make -C lbfgs-ffnn_amd` or "
                       "__graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIG.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.lbf_abi_version() != ABI_VERSION:
        raise LbfError(f"{LIB_PATH} implements ABI {L.lbf_abi_version()}, this binding needs {ABI_VERSION}: rebuild it")
    _lib = L
    return L


def act_ids(acts) -> list:
    """Activation names (or LBF_ACT_* ids, which lbf_mlp_create range-checks) as ids."""
    out = []
    for a in acts:
        if isinstance(a, str):
            if a not in ACTS:
                raise LbfError(f"unknown activation {a!r} (known: {', '.join(sorted(ACTS))})")
            out.append(ACTS[a])
        else:
            out.append(int(a))
    return out


def check_precond(name) -> int:
    """A preconditioner name of hf_solve ("none", "grad_sq") as its LBF_PRECOND_* code (checked before anything
    touches the device)."""
    if name not in PRECONDS:
        raise LbfError(f"unknown preconditioner {name!r} (known: {', '.join(sorted(PRECONDS))})")
    return PRECONDS[name]


def check_l2(l2) -> float:
    """A weight-decay coefficient: a finite number >= 0 (checked before anything touches the device)."""
    try:
        v = float(l2)
    except (TypeError, ValueError):
        raise LbfError(f"l2 must be a number, got {l2!r}") from None
    if not (v >= 0.0) or v == float("inf"):
        raise LbfError(f"l2 must be finite and >= 0, got {l2!r}")
    return v


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().lbf_last_error().decode(errors="replace")
        raise LbfError(f"{what} failed (status {rc}): {msg}")


def ptr(t: Optional[torch.Tensor], dtype: torch.dtype = torch.float32, numel: Optional[int] = None):
    """Device pointer of a contiguous tensor of `dtype` (and exactly `numel` elements when given): the
    kernels read raw memory, so an int64 index list or a float64 matrix would be silently misread."""
    if t is None:
        return None
    if not t.is_cuda:
        raise LbfError("expected a device (cuda/hip) tensor")
    if not t.is_contiguous():
        raise LbfError("expected a contiguous tensor")
    if t.dtype != dtype:
        raise LbfError(f"expected a {dtype} tensor, got {t.dtype}")
    if numel is not None and t.numel() != numel:
        raise LbfError(f"expected {numel} elements, got {t.numel()}")
    return C.c_void_p(t.data_ptr())
