"""Object layer over the C ABI: context, MLP, solvers (all compute in liblbfgs_amd_abi3.so).

Mirrors the reference's GPU-side pieces: ``CublasHandle`` -> :class:`Context`,
``CudaNetwork`` -> :class:`Mlp` (src/cuda/network.cuh), ``CudaLBFGS::solve`` -> :func:`lbfgs_solve`
(src/cuda/lbfgs.cuh:39-194, plus the CPU semantics of src/minimizer/lbfgs.hpp:38-100), and the S-LBFGS
of src/minimizer/s_lbfgs.hpp:165-290 -> :func:`slbfgs_solve`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import (HVP_MODES, INIT_CPU, INIT_CUDA, LANCZOS_MATRICES, LOSSES, LS_ARMIJO, LS_WOLFE, SLBFGS_DP_REPLICATED,
                   SLBFGS_DP_SLICED, AdamCoef, AdamParams, CgInfo, CgParams, EvalResultC, GdParams, HfParams,
                   HfPrecond, LanczosInfo, LanczosParams, LbfError, LbfgsParams, OwlqnParams, OwlqnStats, Record,
                   SgdParams, SlbfgsParams, SolveInfo, act_ids, check, check_l2, check_precond, lib, ptr)

_check = check  # for the methods that have an argument of their own named `check`


def _dptr(a: np.ndarray):
    """A float64 host array as the double * of a C call."""
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Context:
    """One per GPU: device, stream (torch's current stream), optional RCCL communicator."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        if not torch.cuda.is_available():
            raise LbfError("no HIP device visible: the MI355X engine has no CPU fallback")
        self.device = device
        torch.cuda.set_device(device)
        stream = torch.cuda.current_stream(device).cuda_stream if use_torch_stream else 0
        h = C.c_void_p()
        check(lib().lbf_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)), "lbf_ctx_create")
        self.h = h
        self.rank, self.world = 0, 1

    def sync(self):
        check(lib().lbf_ctx_sync(self.h), "lbf_ctx_sync")

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib().lbf_comm_unique_id(buf), "lbf_comm_unique_id")
        return buf.raw

    def comm_init(self, world: int, rank: int, uid: bytes):
        check(lib().lbf_comm_init(self.h, world, rank, uid), "lbf_comm_init")
        self.rank, self.world = rank, world

    @staticmethod
    def comm_init_local(ctxs: Sequence["Context"]):
        """In-process rank group (lbf_comm_init_local): ctxs[r] becomes rank r. The contexts share one device
        and each must then be driven by its own thread with the same call sequence."""
        arr = (C.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])
        check(lib().lbf_comm_init_local(arr, len(ctxs)), "lbf_comm_init_local")
        for r, c in enumerate(ctxs):
            c.rank, c.world = r, len(ctxs)

    def allreduce_(self, t: torch.Tensor):
        check(lib().lbf_allreduce_sum(self.h, ptr(t), t.numel()), "lbf_allreduce_sum")
        return t

    def dot(self, x: torch.Tensor, y: torch.Tensor) -> float:
        out = C.c_double()
        check(lib().lbf_dot(self.h, x.numel(), ptr(x), ptr(y), C.byref(out)), "lbf_dot")
        return out.value

    def nrm2(self, x: torch.Tensor) -> float:
        out = C.c_double()
        check(lib().lbf_nrm2(self.h, x.numel(), ptr(x), C.byref(out)), "lbf_nrm2")
        return out.value

    def axpy_(self, alpha: float, x: torch.Tensor, y: torch.Tensor):
        check(lib().lbf_axpy(self.h, x.numel(), alpha, ptr(x), ptr(y)), "lbf_axpy")
        return y

    def two_loop(self, S: Optional[torch.Tensor], Y: Optional[torch.Tensor], rho: Sequence[float],
                 g: torch.Tensor, mode: int = 0) -> torch.Tensor:
        """Two-loop recursion on an explicit history (logical order, oldest first).
        mode 0: CPU semantics (returns -Hg), 1: S-LBFGS (+Hg), 2: CUDA (-Hg), 3: S-LBFGS through the solver's pair
        updates and direction-only step (rho computed on the device, `rho` ignored)."""
        k = 0 if S is None else int(S.shape[0])
        out = torch.empty_like(g)
        rho_arr = (C.c_double * max(k, 1))(*[float(r) for r in rho]) if k else None
        check(lib().lbf_two_loop(self.h, g.numel(), k, ptr(S) if k else None, ptr(Y) if k else None,
                                 C.cast(rho_arr, C.POINTER(C.c_double)) if k else None, ptr(g), ptr(out), mode),
              "lbf_two_loop")
        return out

    def adam_step(self, w: torch.Tensor, m: torch.Tensor, v: torch.Tensor, g: torch.Tensor, coef: AdamCoef,
                  gg: Optional[torch.Tensor] = None):
        """One Adam / AdamW step in place on w, m, v with gradient g (lbf_adam_step): float32 vectors of one length,
        coef from adam_coefs. gg (a float64 device tensor of one element holding g.g) clips g to the global norm
        coef.clip; None or coef.clip == 0: no clipping. Asynchronous on the context stream."""
        n = int(w.numel())
        check(lib().lbf_adam_step(self.h, n, C.byref(coef), ptr(w), ptr(m, numel=n), ptr(v, numel=n), ptr(g, numel=n),
                                  ptr(gg, torch.float64, 1)), "lbf_adam_step")
        return w

    PROF_KINDS = ["gemm_fwd", "gemm_dw", "gemm_dx", "loss", "splitk_reduce", "finalize", "gram_sweep",
                  "hist_coef", "combine_sweep", "ls_axpy", "allreduce", "metrics", "owl_pseudo", "owl_trial"]

    def prof_enable(self, on: bool = True):
        check(lib().lbf_prof_enable(self.h, int(on)), "lbf_prof_enable")

    def prof_select(self, section=None):
        """Time only `section` ("kind[layer]"), or every section when None."""
        sid = -1
        if section is not None:
            kind, layer = section.split("[")
            sid = self.PROF_KINDS.index(kind) * 16 + int(layer.rstrip("]"))
        check(lib().lbf_prof_select(self.h, sid), "lbf_prof_select")

    def prof_sample(self, every: int = 1):
        """Time only every `every`-th launch of the selected sections."""
        check(lib().lbf_prof_sample(self.h, int(every)), "lbf_prof_sample")

    def _prof_read(self, name, *ctypes):
        """[(section name, values...)] of lbf_prof_read / lbf_prof_read_work: one output array per ctype."""
        fn, n = getattr(lib(), name), C.c_int(0)
        check(fn(self.h, 0, None, *[None] * len(ctypes), C.byref(n)), name)
        cap = n.value
        ids = (C.c_int * max(cap, 1))()
        cols = [(t * max(cap, 1))() for t in ctypes]
        check(fn(self.h, cap, ids, *cols, C.byref(n)), name)
        out = []
        for i in range(min(cap, n.value)):
            kind, layer = divmod(ids[i], 16)
            kname = self.PROF_KINDS[kind] if kind < len(self.PROF_KINDS) else f"k{kind}"
            out.append((f"{kname}[{layer}]", *[c[i] for c in cols]))
        return out

    def prof_read_work(self):
        """{section name: work units of the timed launches} (GEMM sections: batch rows)."""
        return dict(self._prof_read("lbf_prof_read_work", C.c_double))

    def prof_read(self):
        """{section name: (total ms, launches)}; section = kind[layer]."""
        return {k: (ms, int(cnt)) for k, ms, cnt in self._prof_read("lbf_prof_read", C.c_double, C.c_longlong)}

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lbf_ctx_destroy(self.h)
                self.h = None
        except Exception:
            pass


@dataclass
class EvalResult:
    """What Mlp.evaluate returns (lbf_eval_result + the optional outputs). accuracy = correct / rows in [0, 1]."""
    loss: float
    rows: int
    correct: int
    topk: int
    k: int
    accuracy: float
    confusion: Optional[np.ndarray] = None   # [target][predicted] int64
    pred: Optional[torch.Tensor] = None      # int32 [rows of this rank], batch order
    proba: Optional[torch.Tensor] = None     # float32 [rows of this rank][Out]


class Mlp:
    """Dense MLP; flat fp32 params in the reference layout [W (Out x In col-major) | b] per layer."""

    def __init__(self, ctx: Context, dims: Sequence[int], acts: Sequence, loss: str = "mse", l2: float = 0.0):
        """loss: "mse" (0.5 inv_scale ||net(X) - Y||^2, the reference's) or "softmax_xent" (softmax
        cross-entropy on the logits of a linear last layer; lbf_mlp_set_loss). l2: weight decay of lbfgs_solve,
        LbfgsRun, gd_solve and sgd_solve on this network (see the l2 property)."""
        if loss not in LOSSES:  # before anything touches the device
            raise LbfError(f"unknown loss {loss!r}: expected one of {sorted(LOSSES)}")
        l2 = check_l2(l2)
        self.ctx = ctx
        self.dims = [int(d) for d in dims]
        self.acts = act_ids(acts)
        assert len(self.dims) == len(self.acts) + 1
        d = (C.c_int * len(self.dims))(*self.dims)
        a = (C.c_int * len(self.acts))(*self.acts)
        h = C.c_void_p()
        check(lib().lbf_mlp_create(ctx.h, len(self.acts), d, a, C.byref(h)), "lbf_mlp_create")
        self.h = h
        self.nparams = int(lib().lbf_mlp_param_count(h))
        if loss != "mse":
            self.loss_name = loss
        if l2 != 0.0:
            self.l2 = l2

    @property
    def l2(self) -> float:
        """L2 weight decay (lbf_mlp_set_l2): lbfgs_solve, LbfgsRun, gd_solve and sgd_solve minimise and report
        data loss + 0.5 l2 |w|^2. Read when a solve begins. Not used by loss_grad / hvp / fd_hvp / batch_grads
        (their own l2 argument), slbfgs_solve (lam), loss() and lbfgs_solve_fn."""
        v = C.c_double(-1.0)
        check(lib().lbf_mlp_get_l2(self.h, C.byref(v)), "lbf_mlp_get_l2")
        return v.value

    @l2.setter
    def l2(self, l2: float):
        check(lib().lbf_mlp_set_l2(self.h, check_l2(l2)), "lbf_mlp_set_l2")

    @property
    def loss_name(self) -> str:
        """The loss every evaluation and solver on this network minimises ("mse" or "softmax_xent")."""
        v = C.c_int(-1)
        check(lib().lbf_mlp_get_loss(self.h, C.byref(v)), "lbf_mlp_get_loss")
        return next(k for k, c in LOSSES.items() if c == v.value)

    @loss_name.setter
    def loss_name(self, loss: str):
        if loss not in LOSSES:
            raise LbfError(f"unknown loss {loss!r}: expected one of {sorted(LOSSES)}")
        check(lib().lbf_mlp_set_loss(self.h, LOSSES[loss]), "lbf_mlp_set_loss")

    def _check_data(self, X: torch.Tensor, Y: Optional[torch.Tensor]):
        """X [rows][In], Y [rows][Out] (the reference's column-major In x N / Out x N)."""
        if X is not None and (X.dim() != 2 or X.shape[1] != self.dims[0]):
            raise LbfError(f"X must be [rows][{self.dims[0]}], got {tuple(X.shape)}")
        if Y is not None and (Y.dim() != 2 or Y.shape[1] != self.dims[-1] or Y.shape[0] != X.shape[0]):
            raise LbfError(f"Y must be [{X.shape[0]}][{self.dims[-1]}], got {tuple(Y.shape)}")

    def _batch(self, X, Y, idx, scale, out=False):
        """The prologue of a batch evaluation: (rows, `scale` or 1 / rows, `out` or, for None, a new parameter-sized
        tensor), after the shape check of X / Y."""
        B = int(idx.numel()) if idx is not None else int(X.shape[0])
        if scale is None:
            scale = 1.0 / max(B, 1)
        if out is None:
            out = self.new_params()
        self._check_data(X, Y)
        return B, scale, out

    def new_params(self) -> torch.Tensor:
        return torch.empty(self.nparams, dtype=torch.float32, device=f"cuda:{self.ctx.device}")

    def init_params(self, seed: int = 123, mode: str = "cpu", out: Optional[torch.Tensor] = None):
        out = self.new_params() if out is None else out
        check(lib().lbf_mlp_init_params(self.h, seed, INIT_CPU if mode == "cpu" else INIT_CUDA, ptr(out)),
              "lbf_mlp_init_params")
        return out

    def forward(self, params: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
        out = torch.empty((X.shape[0], self.dims[-1]), dtype=torch.float32, device=X.device)
        self._check_data(X, None)
        check(lib().lbf_mlp_forward(self.h, ptr(params, numel=self.nparams), ptr(X), X.shape[0], ptr(out)),
              "lbf_mlp_forward")
        return out

    def loss_grad(self, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, idx: Optional[torch.Tensor] = None,
                  inv_scale: Optional[float] = None, l2: float = 0.0, grad: Optional[torch.Tensor] = None):
        """LossGradFun (src/cuda/minimizer_base.cuh:15-16): returns (loss, grad)."""
        B, inv_scale, grad = self._batch(X, Y, idx, inv_scale, grad)
        loss = C.c_double()
        check(lib().lbf_mlp_loss_grad(self.h, ptr(params, numel=self.nparams), ptr(grad, numel=self.nparams), ptr(X),
                                      ptr(Y), ptr(idx, torch.int32), B, inv_scale, l2, C.byref(loss)),
              "lbf_mlp_loss_grad")
        return loss.value, grad

    def batch_grads(self, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, nmb: int,
                    inv_scale: Optional[float] = None, l2: float = 0.0) -> torch.Tensor:
        """Gradients of nmb consecutive minibatches of X / Y (X.shape[0] // nmb rows each, a multiple of 32) at
        one point, in one evaluation (lbf_mlp_batch_grads): returns an (nmb, nparams) tensor."""
        rows = int(X.shape[0])
        if nmb <= 0 or rows % nmb:
            raise LbfError(f"batch_grads: {rows} rows do not split into {nmb} equal minibatches")
        cnt = rows // nmb
        if cnt % 32:
            raise LbfError(f"batch_grads: {cnt} rows per minibatch, need a multiple of 32")
        if inv_scale is None:
            inv_scale = 1.0 / cnt
        self._check_data(X, Y)
        out = torch.empty((nmb, self.nparams), dtype=torch.float32, device=params.device)
        check(lib().lbf_mlp_batch_grads(self.h, ptr(params, numel=self.nparams), ptr(X), ptr(Y), nmb, cnt, inv_scale,
                                        l2, ptr(out), self.nparams), "lbf_mlp_batch_grads")
        return out

    def loss(self, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, idx: Optional[torch.Tensor] = None,
             inv_scale: Optional[float] = None) -> float:
        """Forward + MSE only (lbf_mlp_loss): the f of a line-search trial."""
        B, inv_scale, _ = self._batch(X, Y, idx, inv_scale)
        out = C.c_double()
        check(lib().lbf_mlp_loss(self.h, ptr(params, numel=self.nparams), ptr(X), ptr(Y), ptr(idx, torch.int32), B,
                                 inv_scale, C.byref(out)), "lbf_mlp_loss")
        return out.value

    def evaluate(self, params: torch.Tensor, X: torch.Tensor, Y: Optional[torch.Tensor] = None,
                 idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, k: int = 1,
                 confusion: bool = False, pred: bool = False, proba: bool = False, chunk: int = 0) -> "EvalResult":
        """Device-side evaluation (lbf_mlp_evaluate): data loss, accuracy, top-k, and on request the confusion
        matrix [target][predicted], the predicted class per row (batch order) and the softmax probabilities
        (cross-entropy networks). Y None: predictions only. With a communicator X / Y are this rank's rows (an
        empty share is legal) and the counts and the loss are the totals over all ranks; inv_scale then defaults
        to 1 / total rows. chunk: rows per forward pass (0: 65536). The argmax and top-k rules are those of
        include/lbfgs_amd.h. To evaluate while an LbfgsRun / SlbfgsRun is open, use a second Mlp of the same shape."""
        B = int(idx.numel()) if idx is not None else int(X.shape[0])
        Out = self.dims[-1]
        if not 1 <= int(k) <= Out:
            raise LbfError(f"k must be in 1..{Out}, got {k}")
        if confusion and Y is None:
            raise LbfError("a confusion matrix needs targets")
        if proba and self.loss_name != "softmax_xent":
            raise LbfError("probabilities need the softmax_xent loss")
        if Y is not None and idx is None:
            self._check_data(X, Y)
        else:
            self._check_data(X, None)
        dev = X.device
        res = EvalResultC()
        conf = np.zeros((Out, Out), np.int64) if confusion else None
        d_pred = torch.empty(B, dtype=torch.int32, device=dev) if pred else None
        d_proba = torch.empty((B, Out), dtype=torch.float32, device=dev) if proba else None
        # the loss is linear in inv_scale: evaluate with 1 and scale by the default once the total rows are known
        check(lib().lbf_mlp_evaluate(self.h, ptr(params, numel=self.nparams), ptr(X), ptr(Y), ptr(idx, torch.int32), B,
                                     1.0 if inv_scale is None else float(inv_scale), int(k), int(chunk), C.byref(res),
                                     conf.ctypes.data_as(C.c_void_p) if confusion else None,
                                     ptr(d_pred, torch.int32), ptr(d_proba)), "lbf_mlp_evaluate")
        rows = int(res.rows)
        loss = float(res.loss) if inv_scale is not None else float(res.loss) * (1.0 / max(rows, 1))
        return EvalResult(loss=loss, rows=rows, correct=int(res.correct), topk=int(res.topk), k=int(k),
                          accuracy=(int(res.correct) / rows if rows and Y is not None else 0.0), confusion=conf,
                          pred=d_pred, proba=d_proba)

    def hvp(self, params: torch.Tensor, v: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
            idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, l2: float = 0.0,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Exact H(params) v of the loss_grad batch loss (R-operator, lbf_mlp_hvp)."""
        return self._product("lbf_mlp_hvp", params, v, X, Y, idx, inv_scale, l2, out)

    def _product(self, name, params, v, X, Y, idx, inv_scale, l2, out, *eps):
        """hvp, gnvp and fd_hvp (whose eps follows l2): one call shape, `name` the entry point."""
        B, inv_scale, out = self._batch(X, Y, idx, inv_scale, out)
        n = self.nparams
        check(getattr(lib(), name)(self.h, ptr(params, numel=n), ptr(v, numel=n), ptr(X), ptr(Y),
                                   ptr(idx, torch.int32), B, inv_scale, l2, *eps, ptr(out, numel=n)), name)
        return out

    def gnvp(self, params: torch.Tensor, v: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
             idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, l2: float = 0.0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Gauss-Newton product G(params) v + l2 v of the loss_grad batch loss (lbf_mlp_gnvp): G = J^T H_L J,
        positive semi-definite, split at the outputs for "mse" and at the logits for "softmax_xent"."""
        return self._product("lbf_mlp_gnvp", params, v, X, Y, idx, inv_scale, l2, out)

    def gn_cg(self, params: torch.Tensor, b: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
              idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, l2: float = 0.0,
              damping: Optional[float] = None, max_iters: Optional[int] = None, rtol: Optional[float] = None,
              check: Optional[int] = None, out: Optional[torch.Tensor] = None, residual: bool = False):
        """Conjugate gradients on (G(params) + damping I) x = b from x = 0 (lbf_mlp_gn_cg), G as in gnvp on the same
        batch; `l2` is another name for the damping (the two add). One forward pass for the whole solve, every CG
        scalar on the device; `check` iterations are enqueued between two status reads and the result does not
        depend on it. Returns (x, info): info has iterations, status (0 converged to rtol, 1 max_iters, 2 p.Ap <= 0),
        rr0, rr, xb, xr, xx and, with residual=True, "r": the recurrence residual as a tensor."""
        return self._gn_cg(params, b, None, X, Y, idx, inv_scale, l2, damping, max_iters, rtol, check, out, residual)

    def _gn_cg(self, params, b, minv, X, Y, idx, inv_scale, l2, damping, max_iters, rtol, every, out, residual):
        """gn_cg (minv None: lbf_mlp_gn_cg) and gn_pcg (lbf_mlp_gn_pcg); `every` is their `check`."""
        B, inv_scale, out = self._batch(X, Y, idx, inv_scale, out)
        n = self.nparams
        p = CgParams()
        lib().lbf_cg_default_params(C.byref(p))
        p.damping = float(l2) + (0.0 if damping is None else float(damping))
        for k, v in (("max_iters", max_iters), ("rtol", rtol), ("check", every)):
            if v is not None:
                setattr(p, k, v)
        ci = CgInfo()
        name = "lbf_mlp_gn_cg" if minv is None else "lbf_mlp_gn_pcg"
        mp = () if minv is None else (ptr(minv, numel=n),)
        check(getattr(lib(), name)(self.h, ptr(params, numel=n), ptr(b, numel=n), *mp, ptr(X), ptr(Y),
                                   ptr(idx, torch.int32), B, inv_scale, C.byref(p), ptr(out, numel=n), C.byref(ci)),
              name)
        info = {k: getattr(ci, k) for k, _ in CgInfo._fields_}
        if residual:
            r = torch.empty(n, dtype=torch.float32, device=out.device)
            check(lib().lbf_mlp_gn_cg_residual(self.h, ptr(r, numel=n)), "lbf_mlp_gn_cg_residual")
            info["r"] = r
        return out, info

    def gn_pcg(self, params: torch.Tensor, b: torch.Tensor, minv: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
               idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, l2: float = 0.0,
               damping: Optional[float] = None, max_iters: Optional[int] = None, rtol: Optional[float] = None,
               check: Optional[int] = None, out: Optional[torch.Tensor] = None, residual: bool = False):
        """gn_cg preconditioned with a diagonal (lbf_mlp_gn_pcg): `minv` holds the inverse of the preconditioner's
        diagonal, one entry > 0 per parameter. z = minv * r is never stored; the stopping test stays on r.r; status 2
        also covers a non-positive r.z. With minv all ones the result is bitwise gn_cg's. Other arguments and the
        return value as gn_cg."""
        return self._gn_cg(params, b, minv, X, Y, idx, inv_scale, l2, damping, max_iters, rtol, check, out, residual)

    def grad_sq(self, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, idx: Optional[torch.Tensor] = None,
                scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """scale * sum_b (d l_b / d w)^2 over the batch rows (lbf_mlp_grad_sq): the sum of the squared per-example
        gradients of the data loss (l_b at inv_scale = 1, no l2 term), i.e. the diagonal of the empirical Fisher
        matrix, formed on the device without materialising a per-example gradient. scale defaults to 1 / rows.
        Bitwise reproducible; with a communicator the ranks' scaled sums are all-reduced."""
        B, scale, out = self._batch(X, Y, idx, scale, out)
        n = self.nparams
        check(lib().lbf_mlp_grad_sq(self.h, ptr(params, numel=n), ptr(X), ptr(Y), ptr(idx, torch.int32), B,
                                        float(scale), ptr(out, numel=n)), "lbf_mlp_grad_sq")
        return out

    def l1_pseudo_grad(self, x: torch.Tensor, g: torch.Tensor, l1: float, l1_bias: bool = False,
                       out: Optional[torch.Tensor] = None):
        """OWL-QN's pseudo-gradient of f + l1 |w|_1 at x with smooth gradient g (lbf_mlp_l1_pseudo_grad): the
        penalty is on the weights, and on the biases too with l1_bias. Returns (pg, stats): stats has zeros,
        penalised, l1_term = l1 sum |x_i| and pg_norm, fp64 sums in a fixed order."""
        n = self.nparams
        out = self.new_params() if out is None else out
        st = OwlqnStats()
        check(lib().lbf_mlp_l1_pseudo_grad(self.h, ptr(x, numel=n), ptr(g, numel=n), float(l1), int(bool(l1_bias)),
                                               ptr(out, numel=n), C.byref(st)), "lbf_mlp_l1_pseudo_grad")
        return out, {k: getattr(st, k) for k, _ in OwlqnStats._fields_}

    def l1_trial(self, x: torch.Tensor, d: torch.Tensor, pg: torch.Tensor, l1: float, alpha: float = 1.0,
                 l1_bias: bool = False, out: Optional[torch.Tensor] = None):
        """OWL-QN's trial point from x along the raw direction d (lbf_mlp_l1_trial): d counts only where it opposes
        pg, the step fmaf(alpha, d, x) is clipped to +0 where it leaves the orthant of x (of -pg where x is zero).
        Returns (xnew, sums): sums has l1_term, ww = xnew.xnew, dec = pg.(xnew - x) and zeros."""
        n = self.nparams
        out = self.new_params() if out is None else out
        l1t, ww, dec, zeros = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_longlong(0)
        check(lib().lbf_mlp_l1_trial(self.h, ptr(x, numel=n), ptr(d, numel=n), ptr(pg, numel=n), float(l1),
                                         int(bool(l1_bias)), float(alpha), ptr(out, numel=n), C.byref(l1t),
                                         C.byref(ww), C.byref(dec), C.byref(zeros)), "lbf_mlp_l1_trial")
        return out, {"l1_term": l1t.value, "ww": ww.value, "dec": dec.value, "zeros": zeros.value}

    def adam_step(self, params: torch.Tensor, m: torch.Tensor, v: torch.Tensor, g: torch.Tensor, coef: AdamCoef,
                  gg: Optional[torch.Tensor] = None):
        """Context.adam_step on this network's parameters: for callers that evaluate with loss_grad and keep
        their own m and v (nparams floats each)."""
        ptr(params, numel=self.nparams)   # the length check; the vectors must match it
        return self.ctx.adam_step(params, m, v, g, coef, gg)

    def fd_hvp(self, params: torch.Tensor, v: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
               idx: Optional[torch.Tensor] = None, inv_scale: Optional[float] = None, l2: float = 0.0,
               eps: float = 1e-4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """finite_difference_hvp_batch (s_lbfgs.hpp:88-101), the S-LBFGS curvature pair's y."""
        return self._product("lbf_mlp_fd_hvp", params, v, X, Y, idx, inv_scale, l2, out, eps)

    def lanczos(self, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, steps: int = 32,
                matrix: str = "gauss_newton", l2: float = 0.0, idx: Optional[torch.Tensor] = None,
                inv_scale: Optional[float] = None, v0: Optional[torch.Tensor] = None, seed: int = 0,
                reorth: bool = True, basis=False, check: int = 8,
                breakdown_rtol: Optional[float] = None) -> "LanczosResult":
        """`steps` steps of device-side Lanczos (lbf_mlp_lanczos) on the Gauss-Newton matrix ("gauss_newton") or the
        exact Hessian ("hessian") of the loss_grad batch loss at params, plus l2 I. v0 None: the start vector is
        torch.randn from a CPU generator seeded with `seed`, so it is reproducible and the same on every rank.
        reorth: full re-orthogonalisation (steps + 1 vectors kept) or the three-vector recurrence. basis: True
        returns the Lanczos vectors; a float32 device tensor [>= steps + 1][ld >= nparams] receives them in place.
        The Ritz values (ascending) and quadrature weights come from lbf_tridiag_eig on the host."""
        if matrix not in LANCZOS_MATRICES:
            raise LbfError(f"unknown matrix {matrix!r}: expected one of {sorted(LANCZOS_MATRICES)}")
        B, inv_scale, _ = self._batch(X, Y, idx, inv_scale)
        n, steps = self.nparams, int(steps)
        p = LanczosParams()
        lib().lbf_lanczos_default_params(C.byref(p))
        p.steps, p.matrix, p.reorth, p.check, p.l2 = steps, LANCZOS_MATRICES[matrix], int(bool(reorth)), int(check), l2
        if breakdown_rtol is not None:
            p.breakdown_rtol = breakdown_rtol
        if v0 is None:
            v0 = torch.randn(n, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32).to(params.device)
        Q, ld = None, 0
        if torch.is_tensor(basis):
            if basis.dim() != 2 or basis.shape[0] < steps + 1 or basis.shape[1] < n:
                raise LbfError(f"basis must be [>= {steps + 1}][>= {n}], got {tuple(basis.shape)}")
            Q, ld = basis, int(basis.shape[1])
        elif basis:
            ld = (n + 3) // 4 * 4  # the row stride of the network's own workspace: the same float4 routes, the same bits
            Q = torch.empty((max(steps, 0) + 1, ld), dtype=torch.float32, device=params.device)
        alpha, beta = np.zeros(max(steps, 1)), np.zeros(max(steps, 1))
        info = LanczosInfo()
        _check(lib().lbf_mlp_lanczos(self.h, ptr(params, numel=n), ptr(v0, numel=n), ptr(X), ptr(Y),
                                     ptr(idx, torch.int32), B, inv_scale, C.byref(p), _dptr(alpha), _dptr(beta),
                                     ptr(Q), ld, C.byref(info)), "lbf_mlp_lanczos")
        m = int(info.steps)
        rows = m + 1 if info.status == 0 else m  # an exhausted or failed run has no q_m
        return LanczosResult(alpha=alpha[:steps], beta=beta[:steps], steps=m, status=int(info.status),
                             v0_norm=float(info.v0_norm), basis=None if Q is None else Q[:rows, :n])

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().lbf_mlp_destroy(self.h)
                self.h = None
        except Exception:
            pass


def tridiag_eig(alpha, beta, vectors: bool = False):
    """Eigenvalues (ascending) of the symmetric tridiagonal matrix with diagonal alpha[0..m-1] and off-diagonal
    beta[0..m-2] (lbf_tridiag_eig: implicit QL in fp64 on the host; entries of beta past m - 1 are ignored), and the
    squared first components of its eigenvectors. Returns (theta, weights), and with vectors also the m x m matrix
    whose column k is theta[k]'s eigenvector."""
    a = np.ascontiguousarray(alpha, np.float64)
    m = int(a.size)
    b = np.ascontiguousarray(np.asarray(beta, np.float64)[:max(m - 1, 0)])
    if m < 1 or b.size < m - 1:
        raise LbfError(f"tridiag_eig: {m} diagonal entries need {max(m - 1, 0)} off-diagonal ones, got {b.size}")
    b = np.concatenate([b, np.zeros(1)])  # never a null pointer, also for m == 1
    theta, w = np.zeros(m), np.zeros(m)
    vecs = np.zeros((m, m)) if vectors else None
    check(lib().lbf_tridiag_eig(m, _dptr(a), _dptr(b), _dptr(theta), _dptr(w), _dptr(vecs) if vectors else None),
          "lbf_tridiag_eig")
    return (theta, w, vecs) if vectors else (theta, w)


@dataclass
class LanczosResult:
    """What Mlp.lanczos returns. alpha, beta: the recurrence's coefficients (length = the steps asked for, zeros from
    `steps` on); T = tridiag(beta[:steps-1]; alpha[:steps]). status 0: every step ran; 1: the Krylov space of the
    start vector was exhausted after `steps` steps (the Ritz values are then eigenvalues); 2: a non-finite product
    or start vector. ritz (ascending) and weights (the squared first components of T's eigenvectors: the Gauss
    quadrature of the start vector's spectral measure, summing to 1) are empty when steps == 0."""
    alpha: np.ndarray
    beta: np.ndarray
    steps: int
    status: int
    v0_norm: float
    basis: Optional[torch.Tensor] = None  # rows q_0 .. (q_steps when status == 0), when asked for
    ritz: Optional[np.ndarray] = None
    weights: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.steps > 0:
            self.ritz, self.weights = tridiag_eig(self.alpha[:self.steps], self.beta[:self.steps])
        else:
            self.ritz, self.weights = np.zeros(0), np.zeros(0)

    def ritz_vectors(self, which=None) -> torch.Tensor:
        """The Ritz vectors Q s_k of ritz[which] (an index, a list of them, None: all) as rows of a float32 device
        tensor; needs the basis."""
        if self.basis is None:
            raise LbfError("ritz_vectors needs the Lanczos vectors: call lanczos(..., basis=True)")
        if self.steps == 0:
            raise LbfError("ritz_vectors: the run took no step")
        _, _, S = tridiag_eig(self.alpha[:self.steps], self.beta[:self.steps], vectors=True)
        sel = np.arange(self.steps) if which is None else np.atleast_1d(np.asarray(which, np.int64))
        coef = torch.from_numpy(np.ascontiguousarray(S[:, sel].T, np.float32)).to(self.basis.device)
        return coef @ self.basis[:self.steps]


def slq_density(ritz_list, weight_list, grid, sigma: float) -> np.ndarray:
    """Stochastic Lanczos quadrature: the eigenvalue density on `grid`, each probe's Ritz values broadened by a
    Gaussian of width sigma and weighted by its quadrature weights, averaged over the probes. Pure host arithmetic;
    integrates to 1 on a grid that covers the spectrum."""
    grid = np.asarray(grid, np.float64)
    if len(ritz_list) == 0 or len(ritz_list) != len(weight_list) or not sigma > 0.0:
        raise LbfError("slq_density: one weight list per Ritz list, at least one probe, sigma > 0")
    dens = np.zeros_like(grid)
    for theta, w in zip(ritz_list, weight_list):
        theta, w = np.asarray(theta, np.float64), np.asarray(w, np.float64)
        z = (grid[:, None] - theta[None, :]) / sigma
        dens += (np.exp(-0.5 * z * z) * w[None, :]).sum(1) / (sigma * np.sqrt(2.0 * np.pi))
    return dens / len(ritz_list)


def spectral_density(net: "Mlp", params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, probes: int = 4,
                     steps: int = 32, grid=None, sigma: Optional[float] = None, seed: int = 0, **kw):
    """The eigenvalue density of the curvature matrix by stochastic Lanczos quadrature: `probes` runs of Mlp.lanczos
    from the start vectors of seeds seed, seed + 1, .. (kw goes to lanczos: matrix, l2, idx, inv_scale, reorth,
    check), then slq_density. grid None: 512 points over the Ritz values' range widened by 5 sigma; sigma None: 1 %
    of that range. Returns (grid, density, results)."""
    runs = [net.lanczos(params, X, Y, steps=steps, seed=seed + p, **kw) for p in range(int(probes))]
    runs = [r for r in runs if r.steps > 0]
    if not runs:
        raise LbfError("spectral_density: no probe took a step")
    lo, hi = min(r.ritz[0] for r in runs), max(r.ritz[-1] for r in runs)
    if sigma is None:
        sigma = 0.01 * max(hi - lo, abs(hi), 1e-30)
    if grid is None:
        grid = np.linspace(lo - 5.0 * sigma, hi + 5.0 * sigma, 512)
    return np.asarray(grid, np.float64), slq_density([r.ritz for r in runs], [r.weights for r in runs], grid, sigma), runs


class History:
    """Host arrays receiving the per-iteration record (IterationRecorder, src/iteration_recorder.hpp)."""

    def __init__(self, cap: int):
        self.cap = max(int(cap), 1)
        self.loss = np.zeros(self.cap)
        self.grad_norm = np.zeros(self.cap)
        self.time_ms = np.zeros(self.cap)
        self.alpha = np.zeros(self.cap)
        self.ls_trials = np.zeros(self.cap, np.int32)
        self.accepted = np.full(self.cap, -1, np.int32)
        self.rec = Record(self.loss.ctypes.data_as(C.POINTER(C.c_double)),
                          self.grad_norm.ctypes.data_as(C.POINTER(C.c_double)),
                          self.time_ms.ctypes.data_as(C.POINTER(C.c_double)),
                          self.alpha.ctypes.data_as(C.POINTER(C.c_double)),
                          self.ls_trials.ctypes.data_as(C.POINTER(C.c_int)),
                          self.accepted.ctypes.data_as(C.POINTER(C.c_int)), self.cap, 0)

    @property
    def size(self) -> int:
        return int(self.rec.size)

    def as_dict(self):
        n = self.size
        return dict(loss=self.loss[:n].copy(), grad_norm=self.grad_norm[:n].copy(), time_ms=self.time_ms[:n].copy(),
                    alpha=self.alpha[:n].copy(), ls_trials=self.ls_trials[:n].copy(),
                    accepted=self.accepted[:n].copy())


def _params(what, struct, defaults, kw, reserved=(), aliases=(), ints=()):
    """The parameter struct of a solver: `struct` with the library's defaults (defaults(pointer)) and the fields that
    kw names; a None keeps the default. reserved: the fields the solve function owns (trace pointers and capacities);
    aliases: {keyword: field}; ints: fields that take a bool. An unknown keyword raises LbfError naming the known
    ones, before the library is touched: a ctypes Structure would take any attribute and ignore it."""
    aliases = dict(aliases)
    settable = {k for k, _ in struct._fields_} - set(reserved)
    for k in kw:
        if k not in settable and k not in aliases:
            known = ", ".join(sorted(settable | set(aliases)))
            raise LbfError(f"{what}: unknown parameter {k!r} (known: {known})")
    p = struct()
    defaults(C.byref(p))
    for k, v in kw.items():
        if v is not None:
            k = aliases.get(k, k)
            setattr(p, k, int(v) if k in ints else v)
    return p


def lbfgs_params(line_search: str = "wolfe", **kw) -> LbfgsParams:
    """lbf_lbfgs_params with the defaults of the line search ("wolfe" or "armijo") and the given fields (m, max_iters,
    tol, max_line_iters, c1, c2, rho). An unknown keyword raises LbfError, here and in the builders below."""
    ls = LS_ARMIJO if line_search == "armijo" else LS_WOLFE
    return _params("lbfgs_params", LbfgsParams, lambda p: lib().lbf_lbfgs_default_params(p, ls), kw,
                   reserved=("line_search",))


def slbfgs_params(**kw) -> SlbfgsParams:
    """lbf_slbfgs_params with the library's defaults and the given fields (max_epochs, tol, M, L, b, b_H, step, reg or
    lam, seed, fd_eps, hvp_exact, dp_mode); the pair trace is slbfgs_solve's."""
    if isinstance(kw.get("dp_mode"), str):
        kw["dp_mode"] = {"replicated": SLBFGS_DP_REPLICATED, "sliced": SLBFGS_DP_SLICED}[kw["dp_mode"]]
    if isinstance(kw.get("hvp_exact"), str):  # "fd", "exact" or "gauss_newton" (LBF_HVP_*); an int passes through
        if kw["hvp_exact"] not in HVP_MODES:
            raise LbfError(f"unknown curvature {kw['hvp_exact']!r}: expected one of {sorted(HVP_MODES)}")
        kw["hvp_exact"] = HVP_MODES[kw["hvp_exact"]]
    return _params("slbfgs_params", SlbfgsParams, lambda p: lib().lbf_slbfgs_default_params(p), kw,
                   reserved=("pair_trace", "pair_trace_cap"), aliases={"lam": "reg"})


def gd_params(**kw) -> GdParams:
    """lbf_gd_params with the library's defaults and the given fields (lr, momentum, max_iters, tol)."""
    return _params("gd_params", GdParams, lambda p: lib().lbf_gd_default_params(p), kw)


def sgd_params(**kw) -> SgdParams:
    """lbf_sgd_params with the library's defaults and the given fields (lr, momentum, batch, decay_rate, decay_step,
    max_epochs, tol)."""
    return _params("sgd_params", SgdParams, lambda p: lib().lbf_sgd_default_params(p), kw)


def _pair_trace(p: SlbfgsParams, cap: int):
    """Points p at a new curvature-pair trace of `cap` rows (NaN until written); None for cap <= 0."""
    if cap <= 0:
        return None
    trace = np.full((int(cap), 8), np.nan)
    p.pair_trace = trace.ctypes.data_as(C.POINTER(C.c_double))
    p.pair_trace_cap = int(cap)
    return trace


class _Run:
    """What LbfgsRun, SlbfgsRun and AdamRun share: the record, the solve info, the handle from lbf_*_begin, iterate
    and close. _keep holds the tensors the solver reads and writes for as long as the handle lives."""
    _name = None   # "lbf_lbfgs": the prefix of _begin / _iterate / _end
    h = None

    def _begin(self, record_cap, keep, *args):
        self.hist = History(record_cap)
        self.info = SolveInfo()
        self._keep = keep
        h = C.c_void_p()
        check(getattr(lib(), self._name + "_begin")(*args, C.byref(h)), self._name + "_begin")
        self.h = h

    def iterate(self, iters: int, *extra):
        check(getattr(lib(), self._name + "_iterate")(self.h, int(iters), C.byref(self.hist.rec), C.byref(self.info),
                                                      *extra), self._name + "_iterate")
        return self.info

    def close(self):
        if self.h:
            getattr(lib(), self._name + "_end")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lbfgs_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, n_global: Optional[int] = None,
                line_search: str = "wolfe", **kw):
    """Full-batch L-BFGS; params updated in place. Returns (history dict, SolveInfo)."""
    p = lbfgs_params(line_search, **kw)
    hist = History(p.max_iters)
    info = SolveInfo()
    n_local = int(X.shape[0])
    check(lib().lbf_lbfgs_solve(net.h, C.byref(p), ptr(params), ptr(X), ptr(Y), n_local,
                                int(n_global or n_local), C.byref(hist.rec), C.byref(info)), "lbf_lbfgs_solve")
    return hist.as_dict(), info


_LOSS_GRAD_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p, C.c_void_p)  # lbf_loss_grad_fn


def lbfgs_solve_fn(ctx: Context, params: torch.Tensor, fn, line_search: str = "wolfe", **kw):
    """L-BFGS on an arbitrary objective (lbf_lbfgs_solve_fn): ``loss = fn(p, g)`` is called once per trial with
    the trial point ``p`` (a device tensor, read-only) and must write the gradient into the device tensor ``g``
    and return the loss. params updated in place. Returns (history dict, SolveInfo). The engine hands the
    callback raw device pointers; they are copied to and from the two tensors (device to device)."""
    p = lbfgs_params(line_search, **kw)
    hist = History(p.max_iters)
    info = SolveInfo()
    n = int(params.numel())
    pt, gt = torch.empty_like(params), torch.empty_like(params)
    nbytes = 4 * n
    failed = []

    def trampoline(_user, d_params, d_grad):
        try:
            check(lib().lbf_memcpy(ctx.h, ptr(pt), C.c_void_p(d_params), nbytes, 2), "lbf_memcpy")
            loss = float(fn(pt, gt))
            torch.cuda.synchronize(ctx.device)
            check(lib().lbf_memcpy(ctx.h, C.c_void_p(d_grad), ptr(gt), nbytes, 2), "lbf_memcpy")
            return loss
        except BaseException as e:  # an exception cannot cross the C frames: reported after the solve returns
            failed.append(e)
            return float("nan")

    cb = _LOSS_GRAD_FN(trampoline)
    rc = lib().lbf_lbfgs_solve_fn(ctx.h, C.byref(p), n, ptr(params, numel=n), C.cast(cb, C.c_void_p), None,
                                  C.byref(hist.rec), C.byref(info))
    if failed:
        raise failed[0]
    check(rc, "lbf_lbfgs_solve_fn")
    return hist.as_dict(), info


class LbfgsRun(_Run):
    """Stateful L-BFGS (begin / iterate / end) used by the benchmark."""
    _name = "lbf_lbfgs"

    def __init__(self, net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor,
                 n_global: Optional[int] = None, line_search: str = "wolfe", record_cap: int = 100000, **kw):
        self.p = lbfgs_params(line_search, **kw)
        self._begin(record_cap, (net, params, X, Y), net.h, C.byref(self.p), ptr(params), ptr(X), ptr(Y),
                    int(X.shape[0]), int(n_global or X.shape[0]))


def slbfgs_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, pair_trace: int = 0, **kw):
    """S-LBFGS (SVRG + FD-HVP curvature pairs; hvp_exact="exact" / "gauss_newton" or 1 / 2 takes the pairs' y from
    Mlp.hvp / Mlp.gnvp instead); X/Y hold all N rows on every rank. pair_trace > 0 records up
    to that many curvature-pair candidates (diagnostics, synchronous) into hist["pairs"]: rows of (epoch, t,
    y.s, s.s, y.y, accepted, live pairs, 0)."""
    p = slbfgs_params(**kw)
    trace = _pair_trace(p, pair_trace)
    hist = History(p.max_epochs)
    info = SolveInfo()
    check(lib().lbf_slbfgs_solve(net.h, C.byref(p), ptr(params), ptr(X), ptr(Y), int(X.shape[0]),
                                 C.byref(hist.rec), C.byref(info)), "lbf_slbfgs_solve")
    out = hist.as_dict()
    if trace is not None:
        out["pairs"] = trace[~np.isnan(trace[:, 0])]
    return out, info


class SlbfgsRun(_Run):
    """Stateful S-LBFGS (begin / iterate / end) used by the benchmark: the epochs of one solve across several
    iterate() calls (the breakdown, warmup and timed epochs), bitwise one lbf_slbfgs_solve."""
    _name = "lbf_slbfgs"

    def __init__(self, net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, record_cap: int = 100000,
                 pair_trace: int = 0, **kw):
        self.p = slbfgs_params(**kw)
        self.p.max_epochs = max(int(self.p.max_epochs), 1 << 30)
        self.trace = _pair_trace(self.p, pair_trace)   # diagnostics: rows as slbfgs_solve's hist["pairs"], and pair0()
        self._begin(record_cap, (net, params, X, Y), net.h, C.byref(self.p), ptr(params), ptr(X), ptr(Y),
                    int(X.shape[0]))

    def pairs(self):
        return None if self.trace is None else self.trace[~np.isnan(self.trace[:, 0])]

    def pair0(self):
        """The first traced curvature-pair candidate's (w_t, u, s, y) as device tensors (lbf_slbfgs_pair0)."""
        n = int(self._keep[1].numel())
        out = [torch.empty(n, dtype=torch.float32, device=self._keep[1].device) for _ in range(4)]
        check(lib().lbf_slbfgs_pair0(self.h, *[ptr(t) for t in out]), "lbf_slbfgs_pair0")
        return out

    def pair_io(self, cap: int, record: bool = True, force: Optional[torch.Tensor] = None):
        """Teacher forcing of the curvature pairs (lbf_slbfgs_pair_io; call before iterate). Returns the record
        tensor [cap, 4, ld] ([w_{t+1} | u | g(u + eps s) | g(u - eps s)] per curvature event; with hvp_exact 1 / 2
        the third block is H(u) s + lam s / G(u) s + lam s and the fourth is zero) or None; `force`
        (same shape, e.g. another run's record) replaces u and the two gradients of each event."""
        n = int(self._keep[1].numel())
        ld = (n + 3) & ~3
        dev = self._keep[1].device
        rec = torch.zeros((int(cap), 4, ld), dtype=torch.float32, device=dev) if record else None
        if force is not None:
            if tuple(force.shape) != (int(cap), 4, ld):
                raise LbfError(f"force: expected shape {(int(cap), 4, ld)}, got {tuple(force.shape)}")
        self._pio = (rec, force)  # kept alive while the solver may write / read them
        check(lib().lbf_slbfgs_pair_io(self.h, int(cap), ptr(rec), ptr(force)), "lbf_slbfgs_pair_io")
        return rec


def gd_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, n_global: Optional[int] = None,
             **kw):
    """CudaGD::solve (src/cuda/gd.cuh:38-106); params updated in place. kw: see gd_params."""
    p = gd_params(**kw)
    hist = History(max(p.max_iters, 1))
    info = SolveInfo()
    n_local = int(X.shape[0])
    check(lib().lbf_gd_solve(net.h, C.byref(p), ptr(params), ptr(X), ptr(Y), n_local, int(n_global or n_local),
                             C.byref(hist.rec), C.byref(info)), "lbf_gd_solve")
    return hist.as_dict(), info


def hf_params(**kw) -> HfParams:
    """lbf_hf_params with the library's defaults and the given fields (max_iters, tol, cg_iters, cg_rtol, cg_check,
    damping0, damp_up, damp_down, ratio_lo, ratio_hi, c1, rho, max_line_iters, curv_rows); the trace pointers are
    hf_solve's. An unknown keyword raises LbfError."""
    return _params("hf_params", HfParams, lambda p: lib().lbf_hf_default_params(p), kw,
                   reserved=("damping_trace", "ratio_trace", "cg_trace", "trace_cap"))


def hf_precond(precond: str = "none", exponent: float = 0.75, refresh: int = 1) -> HfPrecond:
    """lbf_hf_precond from a preconditioner name ("none", "grad_sq"), its exponent in [0, 1] and the outer iterations
    between two evaluations of the squared-gradient diagonal. Raises LbfError without touching the library."""
    pc = HfPrecond()
    pc.mode = check_precond(precond)
    if not (0.0 <= float(exponent) <= 1.0):
        raise LbfError(f"precond_exponent must lie in [0, 1], got {exponent!r}")
    if int(refresh) < 1:
        raise LbfError(f"precond_refresh must be >= 1, got {refresh!r}")
    pc.exponent = float(exponent)
    pc.refresh = int(refresh)
    return pc


def hf_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, n_global: Optional[int] = None,
             precond: Optional[str] = None, precond_exponent: float = 0.75, precond_refresh: int = 1, **kw):
    """Hessian-free solver (lbf_hf_solve): Gauss-Newton CG steps with Levenberg-Marquardt damping and a
    backtracking line search on the network's loss + its l2; params updated in place. kw: see hf_params.
    precond="grad_sq" (lbf_hf_solve_pc): the CG is preconditioned with M = (D / rows + l2 + damping)^precond_exponent,
    D the sum of squared per-example gradients of the curvature rows (Mlp.grad_sq), re-evaluated every
    precond_refresh outer iterations; precond="none" goes through lbf_hf_solve_pc too and gives the bits of the
    default (None: lbf_hf_solve itself). An unknown name raises LbfError before the device is touched.
    Returns (hist, info, traces): traces = {"damping", "ratio", "cg"}, one entry per outer iteration."""
    pc = None if precond is None else hf_precond(precond, precond_exponent, precond_refresh)
    p = hf_params(**kw)
    cap = max(int(p.max_iters), 1)
    damping, ratio, cg = np.full(cap, np.nan), np.full(cap, np.nan), np.zeros(cap, np.int32)
    p.damping_trace = damping.ctypes.data_as(C.POINTER(C.c_double))
    p.ratio_trace = ratio.ctypes.data_as(C.POINTER(C.c_double))
    p.cg_trace = cg.ctypes.data_as(C.POINTER(C.c_int))
    p.trace_cap = cap
    hist = History(cap)
    info = SolveInfo()
    n_local = int(X.shape[0])
    if pc is None:
        check(lib().lbf_hf_solve(net.h, C.byref(p), ptr(params), ptr(X), ptr(Y), n_local, int(n_global or n_local),
                                 C.byref(hist.rec), C.byref(info)), "lbf_hf_solve")
    else:
        check(lib().lbf_hf_solve_pc(net.h, C.byref(p), C.byref(pc), ptr(params), ptr(X), ptr(Y), n_local,
                                    int(n_global or n_local), C.byref(hist.rec), C.byref(info)), "lbf_hf_solve_pc")
    k = int(info.iterations)
    return hist.as_dict(), info, {"damping": damping[:k], "ratio": ratio[:k], "cg": cg[:k]}


def owlqn_params(**kw) -> OwlqnParams:
    """lbf_owlqn_params with the library's defaults and the given fields (m, max_iters, tol, l1, l1_bias, c1, rho,
    max_line_iters); the trace pointer is owlqn_solve's. An unknown keyword raises LbfError."""
    return _params("owlqn_params", OwlqnParams, lambda p: lib().lbf_owlqn_default_params(p), kw,
                   reserved=("zeros_trace", "trace_cap"), ints=("l1_bias",))


def owlqn_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, n_global: Optional[int] = None,
                **kw):
    """OWL-QN (lbf_owlqn_solve): L-BFGS on the network's loss + its l2 + l1 |w|_1 with the orthant-wise
    pseudo-gradient, direction and projection, so weights become exactly zero; params updated in place. kw: see
    owlqn_params. l1 = 0 is still orthant-wise (steps are clipped at sign changes), not lbfgs_solve.
    Returns (hist, info, stats): hist["loss"] is the penalised objective and hist["grad_norm"] the pseudo-gradient
    norm; stats = {"zeros", "penalised", "l1_term", "pg_norm"} of the final point and "zeros_trace", the zero
    count after each iteration."""
    p = owlqn_params(**kw)
    cap = max(int(p.max_iters), 1)
    trace = np.zeros(cap, np.int64)
    p.zeros_trace = trace.ctypes.data_as(C.POINTER(C.c_longlong))
    p.trace_cap = cap
    hist = History(cap)
    info = SolveInfo()
    st = OwlqnStats()
    n_local = int(X.shape[0])
    check(lib().lbf_owlqn_solve(net.h, C.byref(p), ptr(params, numel=net.nparams), ptr(X), ptr(Y), n_local,
                                int(n_global or n_local), C.byref(hist.rec), C.byref(info), C.byref(st)),
          "lbf_owlqn_solve")
    stats = {k: getattr(st, k) for k, _ in OwlqnStats._fields_}
    stats["zeros_trace"] = trace[:int(info.iterations)]
    return hist.as_dict(), info, stats


def adam_params(**kw) -> AdamParams:
    """lbf_adam_params with the library's defaults and the given fields (lr, beta1, beta2, eps, weight_decay,
    clip_norm, batch, shuffle, seed, decay_rate, decay_step, max_epochs, tol); the trace pointer is adam_solve's.
    An unknown keyword raises LbfError."""
    return _params("adam_params", AdamParams, lambda p: lib().lbf_adam_default_params(p), kw,
                   reserved=("loss_trace", "trace_cap"), ints=("shuffle",))


def adam_coefs(p: AdamParams, lr_now: float, t: int) -> AdamCoef:
    """The nine fp32 coefficients of step t at learning rate lr_now (lbf_adam_coefs; host only)."""
    k = AdamCoef()
    check(lib().lbf_adam_coefs(C.byref(p), float(lr_now), int(t), C.byref(k)), "lbf_adam_coefs")
    return k


def adam_epoch_orders(N: int, seed: int = 123, epochs: int = 1) -> np.ndarray:
    """The row orders of epochs 0 .. epochs - 1 as adam_solve draws them with shuffle=1 (lbf_adam_epoch_orders; host
    only): int32 [epochs][N], each row a permutation of 0 .. N - 1."""
    out = np.empty((int(epochs), int(N)), np.int32)
    check(lib().lbf_adam_epoch_orders(int(N), int(seed), int(epochs), out.ctypes.data_as(C.c_void_p)),
          "lbf_adam_epoch_orders")
    return out


def _adam_trace(p: AdamParams, N: int, epochs: int):
    steps = max(1, int(epochs) * -(-int(N) // max(int(p.batch), 1)))
    trace = np.full(steps, np.nan)
    p.loss_trace = trace.ctypes.data_as(C.POINTER(C.c_double))
    p.trace_cap = steps
    return trace


def adam_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, record: bool = True, **kw):
    """Adam / AdamW over shuffled minibatches (lbf_adam_solve) on the network's loss + its l2; params updated in
    place, X / Y hold all N rows on every rank. kw: see adam_params (weight_decay > 0 is AdamW's decoupled decay,
    clip_norm > 0 clips each batch gradient to that global norm). record=False runs without the full-batch rows.
    Returns (hist, info, trace): trace[t] is the batch objective evaluated before step t + 1."""
    p = adam_params(**kw)
    net._check_data(X, Y)
    N = int(X.shape[0])
    trace = _adam_trace(p, N, p.max_epochs)
    hist = History(p.max_epochs + 1)
    info = SolveInfo()
    check(lib().lbf_adam_solve(net.h, C.byref(p), ptr(params, numel=net.nparams), ptr(X), ptr(Y), N,
                               C.byref(hist.rec) if record else None, C.byref(info)), "lbf_adam_solve")
    return hist.as_dict(), info, trace[~np.isnan(trace)]


class _Epochs:
    """What AdamRun.iterate returns: `iterations` counts epochs, as LbfgsRun / SlbfgsRun count their iterations
    (lbf_solve_info.iterations of the Adam solver counts record rows, like lbf_sgd_solve's)."""

    def __init__(self, iterations: int):
        self.iterations = int(iterations)


class AdamRun(_Run):
    """Stateful Adam (lbf_adam_begin / iterate / end): the epochs of one solve across several iterate() calls,
    bitwise one adam_solve. max_epochs bounds the loss trace only; iterate() decides how many epochs run."""
    _name = "lbf_adam"

    def __init__(self, net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, record_cap: int = 100000,
                 **kw):
        self.p = adam_params(**kw)
        net._check_data(X, Y)
        N = int(X.shape[0])
        self.trace = _adam_trace(self.p, N, self.p.max_epochs)
        self.epochs = 0
        self._begin(record_cap, (net, params, X, Y), net.h, C.byref(self.p), ptr(params, numel=net.nparams), ptr(X),
                    ptr(Y), N)

    def iterate(self, epochs: int):
        done = C.c_int(0)
        super().iterate(epochs, C.byref(done))
        self.epochs = int(done.value)
        return _Epochs(self.epochs)

    def loss_trace(self):
        return self.trace[~np.isnan(self.trace)]

def sgd_solve(net: Mlp, params: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, record: bool = True, **kw):
    """CudaSGD::solve (src/cuda/sgd.cuh:50-153). kw: see sgd_params. record=False runs without the recorder (no
    full-batch evaluations)."""
    p = sgd_params(**kw)
    hist = History(p.max_epochs + 1)
    info = SolveInfo()
    check(lib().lbf_sgd_solve(net.h, C.byref(p), ptr(params), ptr(X), ptr(Y), int(X.shape[0]),
                              C.byref(hist.rec) if record else None, C.byref(info)), "lbf_sgd_solve")
    return hist.as_dict(), info


def init_params_host(dims: Sequence[int], acts: Sequence, seed: int = 123, mode: str = "cpu") -> np.ndarray:
    """Host-side copy of the init stream (for tests; the device path is Mlp.init_params)."""
    a = act_ids(acts)
    d = (C.c_int * len(dims))(*[int(x) for x in dims])
    ac = (C.c_int * len(a))(*a)
    n = sum((dims[i] + 1) * dims[i + 1] for i in range(len(a)))
    out = np.empty(n, np.float32)
    check(lib().lbf_init_params_host(len(a), d, ac, seed, INIT_CPU if mode == "cpu" else INIT_CUDA,
                                     out.ctypes.data_as(C.c_void_p)), "lbf_init_params_host")
    return out


def synth_mnist(N: int, In: int = 784, classes: int = 10, seed: int = 123):
    """Synthetic MNIST-shaped data; host float32 arrays [N][In], [N][classes]."""
    X = np.empty((N, In), np.float32)
    Y = np.empty((N, classes), np.float32)
    check(lib().lbf_synth_mnist(N, In, classes, seed, X.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p)),
          "lbf_synth_mnist")
    return X, Y


def synth_regression(ctx: Context, N: int, In: int = 4096, seed_x: int = 123, seed_t: int = 124, row0: int = 0):
    """BASELINE config 5 data on the device: rows [row0, row0+N) of X ~ N(0,1) [.][In] and
    y = tanh(v.x/64) + 0.01 e [.][1]."""
    X = torch.empty((N, In), dtype=torch.float32, device=f"cuda:{ctx.device}")
    Y = torch.empty((N, 1), dtype=torch.float32, device=f"cuda:{ctx.device}")
    check(lib().lbf_synth_regression(ctx.h, row0, N, In, seed_x, seed_t, ptr(X), ptr(Y)), "lbf_synth_regression")
    return X, Y


def load_idx_images(path: str, max_images: int = 0) -> np.ndarray:
    """MNISTLoader::loadImages (tests/mnist/mnist_loader.hpp:21-61): [N][rows*cols] float32 in [0, 1]."""
    n, r, c = C.c_longlong(0), C.c_int(0), C.c_int(0)
    check(lib().lbf_idx_read_images(path.encode(), max_images, None, C.byref(n), C.byref(r), C.byref(c)),
          "lbf_idx_read_images")
    out = np.empty((n.value, r.value * c.value), np.float32)
    check(lib().lbf_idx_read_images(path.encode(), max_images, out.ctypes.data_as(C.c_void_p), C.byref(n),
                                    C.byref(r), C.byref(c)), "lbf_idx_read_images")
    return out


def load_idx_labels(path: str, max_labels: int = 0, classes: int = 10) -> np.ndarray:
    """MNISTLoader::loadLabels (tests/mnist/mnist_loader.hpp:63-100): one-hot [N][classes] float32."""
    n = C.c_longlong(0)
    check(lib().lbf_idx_read_labels(path.encode(), max_labels, classes, None, C.byref(n)), "lbf_idx_read_labels")
    out = np.empty((n.value, classes), np.float32)
    check(lib().lbf_idx_read_labels(path.encode(), max_labels, classes, out.ctypes.data_as(C.c_void_p), C.byref(n)),
          "lbf_idx_read_labels")
    return out


def sample_indices(N: int, b: int, seed: int = 123, calls: int = 1) -> np.ndarray:
    out = np.empty(calls * b, np.int64)
    check(lib().lbf_sample_indices(N, b, seed, calls, out.ctypes.data_as(C.c_void_p)), "lbf_sample_indices")
    return out.reshape(calls, b)


def grad_flops_per_sample(dims: Sequence[int]) -> int:
    """Algorithmic flops of one loss+grad per sample: fwd + dW + dX (layer 0 has no dX)."""
    f = 0
    for l in range(len(dims) - 1):
        io = dims[l] * dims[l + 1]
        f += 2 * io + 2 * io + (2 * io if l > 0 else 0)
    return f
