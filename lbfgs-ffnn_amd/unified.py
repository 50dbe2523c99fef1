"""Host-side mirror of the reference's unified API for the HIP backend.

Same names, argument meaning and defaults as src/unified_optimization.hpp / src/unified_launcher.hpp /
src/iteration_recorder.hpp, so a driver like tests/mnist/main-gpu.cpp reads the same:

    launcher = UnifiedLauncher()                     # UnifiedLauncher<HipBackend>
    launcher.addLayer(784, 128, "relu"); launcher.addLayer(128, 10, "linear"); launcher.buildNetwork()
    launcher.setData(dataset)                        # UnifiedDataset (numpy, [N][In] == In x N col-major)
    cfg = UnifiedConfig(name="MNIST_LBFGS_m10", max_iters=1000, tolerance=1e-3, m_param=10, log_interval=1)
    launcher.train(UnifiedLBFGS(), cfg); launcher.test()

Data parallelism: if torch.distributed is initialised, each rank holds its contiguous shard of the
training rows for full-batch L-BFGS (one RCCL all-reduce of [grad | loss] per evaluation) and all rows
for S-LBFGS (minibatch index lists are sliced across ranks).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import engine
from ._lib import LOSSES, LbfError, act_ids, check_l2


@dataclass
class UnifiedConfig:
    """src/unified_optimization.hpp:26-48 (+ HIP extensions: line_search, init)."""
    name: str = "Experiment"
    max_iters: int = 100
    tolerance: float = 1e-4
    learning_rate: float = 0.01
    momentum: float = 0.0
    lr_decay: float = 0.0
    lr_decay_rate: int = 1
    batch_size: int = 128
    m_param: int = 10
    L_param: int = 10
    b_H_param: int = 0
    log_interval: int = 10
    reset_params: bool = True
    seed: int = 123
    line_search: str = "wolfe"   # "wolfe" = CPU semantics (parity target), "armijo" = CUDA semantics
    init: str = "cpu"            # "cpu" (network.hpp:45-71) or "cuda" (network.cuh:36-59) init stream
    write_csv: bool = True
    loss: str = "mse"            # "mse" or "softmax_xent" (HIP extension; train() applies a non-default choice
                                 # like UnifiedLauncher.setLoss, and it then stays the network's loss)
    l2: float = 0.0              # weight decay of UnifiedLBFGS / UnifiedGD / UnifiedSGD (HIP extension; train()
                                 # applies a non-zero value like UnifiedLauncher.setL2, and it then stays)
    l1: float = 0.0              # L1 penalty on the weights, UnifiedOWLQN only (HIP extension): the other optimisers
                                 # do not read it
    curvature: str = "fd"        # UnifiedSLBFGS's curvature pairs (HIP extension): "fd" (the reference's finite
                                 # difference), "exact" (R-operator H s) or "gauss_newton" (G s, always y.s > 0)
    # UnifiedHF (HIP extension): CG iterations and relative residual per step, the initial damping, and the rows of
    # the curvature window (0: all local rows; > 0 is single rank, like UnifiedSGD)
    cg_iters: int = 50
    cg_rtol: float = 0.1
    damping: float = 1.0
    curv_rows: int = 0
    precond: str = "none"        # UnifiedHF's CG preconditioner: "none" or "grad_sq" (the squared-gradient diagonal)
    precond_exponent: float = 0.75
    # Validation-monitored training (HIP extension; UnifiedLBFGS, UnifiedSLBFGS and UnifiedAdam). eval_every > 0: the test split
    # is evaluated on the device at iteration 0, every eval_every iterations (epochs for S-LBFGS) and at the end.
    eval_every: int = 0          # 0: off (the unmonitored code path)
    patience: int = 0            # stop after this many evaluations in a row without a strict improvement; 0: never
    monitor: str = "loss"        # "loss" (lower is better) or "accuracy" (higher is better)
    restore_best: bool = True    # finish with the parameters of the best evaluation
    # UnifiedAdam (HIP extension): it also reads learning_rate, batch_size, max_iters (epochs), seed (the shuffle's),
    # lr_decay / lr_decay_rate (applied only when lr_decay > 0) and the network's l2 (the coupled penalty)
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    weight_decay: float = 0.0    # AdamW's decoupled decay
    clip_norm: float = 0.0       # clip each batch gradient to this global norm; 0: off
    shuffle: bool = True         # a fresh row order per epoch; False: contiguous batches like UnifiedSGD


@dataclass
class UnifiedDataset:
    """src/unified_optimization.hpp:54-59; arrays are [N][features] (== the reference's column-major)."""
    train_x: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))
    train_y: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))
    test_x: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))
    test_y: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))


class IterationRecorder:
    """src/iteration_recorder.hpp:13-146 (loss, grad-norm, cumulative ms per iteration)."""

    def __init__(self):
        self.loss, self.grad_norm, self.time_ms = [], [], []
        self.validation = []   # (iteration, val_loss, val_accuracy) of a validation-monitored run

    def init(self, capacity: int):
        self.reset()

    def reset(self):
        self.loss, self.grad_norm, self.time_ms = [], [], []
        self.validation = []

    def record(self, idx: int, loss: float, grad_norm: float, time_ms: float = 0.0):
        while len(self.loss) <= idx:
            self.loss.append(0.0)
            self.grad_norm.append(0.0)
            self.time_ms.append(0.0)
        self.loss[idx], self.grad_norm[idx], self.time_ms[idx] = loss, grad_norm, time_ms

    def copy_to_host(self):
        return list(self.loss), list(self.grad_norm), list(self.time_ms)

    def size(self) -> int:
        return len(self.loss)


def log_filename(config: UnifiedConfig) -> str:
    return (config.name or "run") + "_history.csv"   # unified_optimization.hpp:61-64


def write_history_csv(filename: str, recorder: IterationRecorder, log_interval: int) -> None:
    """unified_optimization.hpp:66-85 / :446-465: `Iteration,Loss,GradNorm,TimeMs`, strided."""
    if log_interval <= 0 or recorder.size() == 0:
        return
    loss, grad, tms = recorder.copy_to_host()
    with open(filename, "w") as f:
        f.write("Iteration,Loss,GradNorm,TimeMs\n")
        for i in range(0, len(loss), max(1, log_interval)):
            f.write(f"{i},{loss[i]:g},{grad[i]:g},{tms[i]:g}\n")


class _DeviceNet:
    """What NetworkWrapper<HipBackend> wraps: the HIP MLP and its flat parameter tensor."""

    def __init__(self, ctx: engine.Context):
        self.ctx = ctx
        self.layers = []
        self.mlp: Optional[engine.Mlp] = None
        self.params: Optional[torch.Tensor] = None
        self.loss = "mse"
        self.l2 = 0.0

    def setL2(self, l2: float):
        l2 = check_l2(l2)
        if self.mlp is not None:
            self.mlp.l2 = l2
        self.l2 = l2

    def setLoss(self, loss: str):
        if loss not in LOSSES:
            raise LbfError(f"unknown loss {loss!r}: expected one of {sorted(LOSSES)}")
        if self.mlp is not None:
            self.mlp.loss_name = loss
        self.loss = loss

    def addLayer(self, In: int, Out: int, act):
        if self.layers and self.layers[-1][1] != In:
            raise LbfError(f"layer input {In} does not match previous output {self.layers[-1][1]}")
        act_ids([act])  # an unknown name fails here, not at bindParams
        self.layers.append((int(In), int(Out), act))

    def bindParams(self, seed: int = 123, mode: str = "cpu"):
        dims = [self.layers[0][0]] + [l[1] for l in self.layers]
        if self.mlp is None:
            self.mlp = engine.Mlp(self.ctx, dims, [l[2] for l in self.layers], loss=self.loss, l2=self.l2)
            self.params = self.mlp.new_params()
        self.mlp.init_params(seed, mode, self.params)

    def getParamsSize(self) -> int:
        return self.mlp.nparams if self.mlp else 0


class UnifiedOptimizer:
    def optimize(self, net: _DeviceNet, data: "_DeviceData", config: UnifiedConfig) -> IterationRecorder:
        raise NotImplementedError


def _recorded(optimizer: UnifiedOptimizer, hist, info) -> IterationRecorder:
    """What every optimize() ends with: the solver's history dict and solve info kept as optimizer.history and
    optimizer.info, and the history's loss, gradient norm and time as the IterationRecorder that train() writes."""
    rec = IterationRecorder()
    for i in range(len(hist["loss"])):
        rec.record(i, float(hist["loss"][i]), float(hist["grad_norm"][i]), float(hist["time_ms"][i]))
    optimizer.info = info
    optimizer.history = hist
    return rec


class EarlyStopper:
    """Decides when validation-monitored training stops: after `patience` evaluations in a row that bring no
    strict improvement of the monitored value ("loss": lower is better, "accuracy": higher is better). A tie is
    not an improvement, neither is a NaN; the first evaluation always counts as one. patience == 0 never stops.
    Pure Python: update(iteration, loss, accuracy) returns True when training should stop; best_iteration,
    best_loss and best_accuracy name the best evaluation so far."""

    def __init__(self, patience: int = 0, monitor: str = "loss"):
        if monitor not in ("loss", "accuracy"):
            raise LbfError(f"monitor must be 'loss' or 'accuracy', got {monitor!r}")
        if int(patience) < 0:
            raise LbfError(f"patience must be >= 0, got {patience!r}")
        self.patience, self.monitor = int(patience), monitor
        self.best_iteration: Optional[int] = None
        self.best_loss = self.best_accuracy = None
        self.stale = 0   # evaluations since the best one

    def improved(self, loss: float, accuracy: float) -> bool:
        if self.best_iteration is None:
            return True
        return accuracy > self.best_accuracy if self.monitor == "accuracy" else loss < self.best_loss

    def update(self, iteration: int, loss: float, accuracy: float) -> bool:
        if self.improved(loss, accuracy):
            self.best_iteration, self.best_loss, self.best_accuracy = int(iteration), loss, accuracy
            self.stale = 0
        else:
            self.stale += 1
        return self.patience > 0 and self.stale >= self.patience


def validation_filename(config: UnifiedConfig) -> str:
    return (config.name or "run") + "_validation.csv"


def write_validation_csv(filename: str, validation) -> None:
    """`Iteration,ValLoss,ValAccuracy`, one line per evaluation of the monitored run."""
    with open(filename, "w") as f:
        f.write("Iteration,ValLoss,ValAccuracy\n")
        for it, loss, acc in validation:
            f.write(f"{it},{loss:.17g},{acc:.17g}\n")


def _check_monitored(config: UnifiedConfig, data: "_DeviceData") -> None:
    if config.monitor not in ("loss", "accuracy"):
        raise LbfError(f"monitor must be 'loss' or 'accuracy', got {config.monitor!r}")
    if data is None or data.test_xs is None or data.n_test == 0:
        raise LbfError("eval_every > 0 needs a test split (UnifiedDataset.test_x / test_y)")


def _assert_ranks_agree(entry) -> None:
    """Every rank must hold bitwise the same validation entry, or the ranks would stop at different iterations."""
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return
    world = torch.distributed.get_world_size()
    if world == 1:
        return
    mine = (int(entry[0]), float(entry[1]).hex(), float(entry[2]).hex())
    seen = [None] * world
    torch.distributed.all_gather_object(seen, mine)
    if any(s != mine for s in seen):
        raise LbfError(f"validation metrics differ between ranks: {seen}")


def _monitored_run(optimizer: "UnifiedOptimizer", net: _DeviceNet, data: "_DeviceData", config: UnifiedConfig, run):
    """Drive a resumable solver (`run`: LbfgsRun / SlbfgsRun / AdamRun on net.mlp) in chunks of config.eval_every iterations,
    evaluating the test split between the chunks on a second Mlp of the same shape (the solver's own network and
    workspace are never touched). Sets optimizer.validation = [(iteration, val_loss, val_accuracy)],
    optimizer.best_iteration and optimizer.stopped_early; with restore_best the best parameters are copied back."""
    ev_net = engine.Mlp(net.ctx, net.mlp.dims, net.mlp.acts, loss=net.loss)
    stopper = EarlyStopper(config.patience, config.monitor)
    best = torch.empty_like(net.params) if config.restore_best else None
    validation = []

    def observe(it: int) -> bool:
        r = ev_net.evaluate(net.params, data.test_xs, data.test_ys)
        entry = (it, r.loss, r.accuracy)
        _assert_ranks_agree(entry)
        validation.append(entry)
        stop = stopper.update(*entry)
        if best is not None and stopper.best_iteration == it:
            best.copy_(net.params)
        return stop

    it = 0
    try:
        stop = observe(0)
        while not stop and it < config.max_iters:
            n = min(int(config.eval_every), config.max_iters - it)
            now = int(run.iterate(n).iterations)
            if now == it:   # converged on entry: the last evaluation is the final one
                break
            ended = now - it < n
            it = now
            stop = observe(it) or ended
    finally:
        run.close()
    if best is not None and stopper.best_iteration != it:
        net.params.copy_(best)
    torch.cuda.synchronize(net.ctx.device)
    optimizer.validation = validation
    optimizer.best_iteration = stopper.best_iteration
    optimizer.stopped_early = bool(stopper.patience > 0 and stopper.stale >= stopper.patience)
    rec = _recorded(optimizer, run.hist.as_dict(), run.info)
    rec.validation = list(validation)
    return rec


class UnifiedLBFGS(UnifiedOptimizer):
    """UnifiedLBFGS<HipBackend> (unified_optimization.hpp:191-214 / 560-592). config.eval_every > 0: the same solve
    through LbfgsRun in chunks, with validation, early stopping and restore_best (_monitored_run)."""

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            _check_monitored(config, data)
            run = engine.LbfgsRun(net.mlp, net.params, data.x, data.y, n_global=data.n_global,
                                  line_search=config.line_search, record_cap=max(config.max_iters, 1),
                                  m=config.m_param if config.m_param > 0 else 10, max_iters=config.max_iters,
                                  tol=config.tolerance)
            return _monitored_run(self, net, data, config, run)
        hist, info = engine.lbfgs_solve(net.mlp, net.params, data.x, data.y, n_global=data.n_global,
                                        line_search=config.line_search, m=config.m_param if config.m_param > 0 else 10,
                                        max_iters=config.max_iters, tol=config.tolerance)
        return _recorded(self, hist, info)


class UnifiedSLBFGS(UnifiedOptimizer):
    """UnifiedSLBFGS<HipBackend>: the reference has it CPU-only (static_assert for CUDA,
    unified_optimization.hpp:635-641, 688-696); here it runs on the GPU with the CPU semantics of
    UnifiedSLBFGS_CPU (unified_optimization.hpp:306-408)."""

    def optimize(self, net, data, config):
        b_H = config.b_H_param if config.b_H_param > 0 else config.batch_size // 2   # :325
        if config.eval_every > 0:   # the same solve through SlbfgsRun, an epoch per iteration (_monitored_run)
            _check_monitored(config, data)
            run = engine.SlbfgsRun(net.mlp, net.params, data.x_full, data.y_full, record_cap=max(config.max_iters, 1),
                                   tol=config.tolerance, M=config.m_param, L=config.L_param, b=config.batch_size,
                                   b_H=b_H, step=config.learning_rate, lam=1e-4, seed=123,
                                   hvp_exact=config.curvature)
            return _monitored_run(self, net, data, config, run)
        hist, info = engine.slbfgs_solve(net.mlp, net.params, data.x_full, data.y_full, max_epochs=config.max_iters,
                                         tol=config.tolerance, M=config.m_param, L=config.L_param,
                                         b=config.batch_size, b_H=b_H, step=config.learning_rate, lam=1e-4,
                                         seed=123, hvp_exact=config.curvature)
        return _recorded(self, hist, info)


class UnifiedGD(UnifiedOptimizer):
    """UnifiedGD<HipBackend> (unified_optimization.hpp:518-554: CudaGD with the config's learning_rate,
    momentum, max_iters, tolerance)."""

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            raise LbfError("UnifiedGD has no resumable form: eval_every > 0 needs UnifiedLBFGS, UnifiedSLBFGS or UnifiedAdam")
        hist, info = engine.gd_solve(net.mlp, net.params, data.x, data.y, n_global=data.n_global,
                                     lr=config.learning_rate, momentum=config.momentum, max_iters=config.max_iters,
                                     tol=config.tolerance)
        return _recorded(self, hist, info)


class UnifiedHF(UnifiedOptimizer):
    """Hessian-free (truncated Newton) training (HIP extension, no reference counterpart): engine.hf_solve with the
    config's max_iters, tolerance, cg_iters, cg_rtol, damping (the initial one), curv_rows, precond and
    precond_exponent; the loss and l2 are the network's. The damping, reduction-ratio and CG-iteration traces are
    kept in self.traces."""

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            raise LbfError("UnifiedHF has no resumable form: eval_every > 0 needs UnifiedLBFGS, UnifiedSLBFGS or UnifiedAdam")
        engine.hf_precond(config.precond, config.precond_exponent)   # an unknown name fails here, before the device
        precond = None if config.precond == "none" else config.precond   # "none": lbf_hf_solve itself
        hist, info, traces = engine.hf_solve(net.mlp, net.params, data.x, data.y, n_global=data.n_global,
                                             precond=precond, precond_exponent=config.precond_exponent,
                                             max_iters=config.max_iters, tol=config.tolerance,
                                             cg_iters=config.cg_iters, cg_rtol=config.cg_rtol,
                                             damping0=config.damping, curv_rows=config.curv_rows)
        self.traces = traces
        return _recorded(self, hist, info)


class UnifiedOWLQN(UnifiedOptimizer):
    """L1-regularised L-BFGS (HIP extension, no reference counterpart): engine.owlqn_solve with the config's l1,
    m_param, max_iters and tolerance; the loss and l2 are the network's. The recorded loss includes the penalties;
    the zero counts are kept in self.stats."""

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            raise LbfError("UnifiedOWLQN has no resumable form: eval_every > 0 needs UnifiedLBFGS, UnifiedSLBFGS or UnifiedAdam")
        hist, info, stats = engine.owlqn_solve(net.mlp, net.params, data.x, data.y, n_global=data.n_global,
                                               m=config.m_param, max_iters=config.max_iters, tol=config.tolerance,
                                               l1=config.l1)
        self.stats = stats
        return _recorded(self, hist, info)


class UnifiedSGD(UnifiedOptimizer):
    """UnifiedSGD<HipBackend> (unified_optimization.hpp:595-632: CudaSGD with learning_rate, momentum,
    batch_size, max_iters epochs and setLearningRateDecay(lr_decay, lr_decay_rate); the tolerance is
    not passed, so CudaSGD's default 1e-6 applies). Single rank."""

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            raise LbfError("UnifiedSGD has no resumable form: eval_every > 0 needs UnifiedLBFGS, UnifiedSLBFGS or UnifiedAdam")
        hist, info = engine.sgd_solve(net.mlp, net.params, data.x_full, data.y_full, lr=config.learning_rate,
                                      momentum=config.momentum, batch=config.batch_size, max_epochs=config.max_iters,
                                      decay_rate=config.lr_decay, decay_step=config.lr_decay_rate)
        return _recorded(self, hist, info)


class UnifiedAdam(UnifiedOptimizer):
    """Adam / AdamW over shuffled minibatches (HIP extension, no reference counterpart): engine.adam_solve with the
    config's learning_rate, beta1, beta2, adam_eps, weight_decay, clip_norm, batch_size, shuffle, seed and max_iters
    epochs; lr_decay / lr_decay_rate as UnifiedSGD reads them, but only when lr_decay > 0. The loss and l2 are the
    network's; the stopping tolerance stays the solver's 1e-6, as for UnifiedSGD. Every rank holds all rows and takes
    its slice of every batch. config.eval_every > 0: the same solve through AdamRun, an epoch per iteration, with
    validation, early stopping and restore_best (_monitored_run). The batch objectives are kept in self.trace."""

    @staticmethod
    def _kw(config):
        decay = config.lr_decay > 0
        return dict(lr=config.learning_rate, beta1=config.beta1, beta2=config.beta2, eps=config.adam_eps,
                    weight_decay=config.weight_decay, clip_norm=config.clip_norm, batch=config.batch_size,
                    shuffle=config.shuffle, seed=config.seed, max_epochs=config.max_iters,
                    decay_rate=config.lr_decay if decay else 1.0, decay_step=config.lr_decay_rate if decay else 0)

    def optimize(self, net, data, config):
        if config.eval_every > 0:
            _check_monitored(config, data)
            run = engine.AdamRun(net.mlp, net.params, data.x_full, data.y_full,
                                 record_cap=max(config.max_iters, 1) + 1, **self._kw(config))
            rec = _monitored_run(self, net, data, config, run)
            self.trace = run.loss_trace()
            return rec
        hist, info, trace = engine.adam_solve(net.mlp, net.params, data.x_full, data.y_full, **self._kw(config))
        self.trace = trace
        return _recorded(self, hist, info)


class _DeviceData:
    def __init__(self, dataset: UnifiedDataset, device: str, rank: int, world: int, need_full: bool = True):
        tx = np.ascontiguousarray(dataset.train_x, np.float32)   # fp64 -> fp32 upload (unified_launcher.hpp:105-128)
        ty = np.ascontiguousarray(dataset.train_y, np.float32)
        N = tx.shape[0]
        lo, hi = N * rank // world, N * (rank + 1) // world
        self.n_global = N
        self.x = torch.from_numpy(tx[lo:hi]).to(device)
        self.y = torch.from_numpy(ty[lo:hi]).to(device)
        if world == 1:
            self.x_full, self.y_full = self.x, self.y
        elif need_full:
            self.x_full = torch.from_numpy(tx).to(device)
            self.y_full = torch.from_numpy(ty).to(device)
        self.test_x = torch.from_numpy(np.ascontiguousarray(dataset.test_x, np.float32)).to(device) \
            if dataset.test_x.size else None
        self.test_y = np.asarray(dataset.test_y, np.float64)
        self.train_y_host = np.asarray(dataset.train_y, np.float64)
        # this rank's contiguous shard of the test split and its targets, device-resident (metrics(), validation)
        self.n_test = int(dataset.test_x.shape[0]) if dataset.test_x.size else 0
        self.test_xs = self.test_ys = None
        if self.n_test:
            ey = np.ascontiguousarray(dataset.test_y, np.float32)
            tlo, thi = self.n_test * rank // world, self.n_test * (rank + 1) // world
            self.test_xs = self.test_x if world == 1 else self.test_x[tlo:thi].contiguous()
            self.test_ys = torch.from_numpy(ey[tlo:thi]).to(device)
        torch.cuda.synchronize()


class UnifiedLauncher:
    """UnifiedLauncher<HipBackend> (src/unified_launcher.hpp:83-205)."""

    def __init__(self, device: Optional[int] = None):
        rank, world = 0, 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", rank)) % max(1, torch.cuda.device_count())
        self.ctx = engine.Context(device)
        if world > 1:
            uid = [engine.Context.unique_id() if rank == 0 else None]
            torch.distributed.broadcast_object_list(uid, src=0)
            self.ctx.comm_init(world, rank, uid[0])
        self.rank, self.world = rank, world
        self.net_wrapper_ = _DeviceNet(self.ctx)
        self.data_: Optional[_DeviceData] = None
        self.dataset_ = None

    def addLayer(self, In: int, Out: int, act="linear"):
        self.net_wrapper_.addLayer(In, Out, act)

    def buildNetwork(self):
        self.net_wrapper_.bindParams()

    def setLoss(self, loss: str):
        """The loss the optimizers minimise and evaluate() reports: "mse" (default) or "softmax_xent" (softmax
        cross-entropy on the logits; the last layer must be linear). Before or after buildNetwork()."""
        self.net_wrapper_.setLoss(loss)

    def setL2(self, l2: float):
        """L2 weight decay of UnifiedLBFGS, UnifiedGD and UnifiedSGD: they minimise and record
        data loss + 0.5 l2 |w|^2 (UnifiedSLBFGS keeps its own lambda). evaluate() reports the data term only.
        Before or after buildNetwork()."""
        self.net_wrapper_.setL2(l2)

    def setData(self, data: UnifiedDataset):
        self.dataset_ = data
        self.data_ = _DeviceData(data, f"cuda:{self.ctx.device}", self.rank, self.world)

    def train(self, optimizer: UnifiedOptimizer, config: UnifiedConfig):
        if self.rank == 0:
            print(f">>> Running HIP Experiment: {config.name}")
        if config.loss != "mse":
            self.setLoss(config.loss)
        if check_l2(config.l2) != 0.0:
            self.setL2(config.l2)
        if config.reset_params:
            self.net_wrapper_.bindParams(config.seed, config.init)
        recorder = optimizer.optimize(self.net_wrapper_, self.data_, config)
        if config.write_csv and self.rank == 0:
            write_history_csv(log_filename(config), recorder, config.log_interval)
        if config.eval_every > 0 and config.write_csv and self.rank == 0:
            write_validation_csv(validation_filename(config), recorder.validation)
        self.last_recorder = recorder
        return self.evaluate(self.data_.x_full if self.world == 1 else self.data_.x_full,
                             self.data_.train_y_host, "Training Results")

    def test(self):
        if self.data_ is None or self.data_.test_x is None:
            return None
        return self.evaluate(self.data_.test_x, self.data_.test_y, "Test Results")

    def evaluate(self, x: torch.Tensor, y: np.ndarray, label: str):
        """unified_launcher.hpp:154-199: forward on the device, accuracy + mean MSE on the host. With the
        cross-entropy loss the outputs are logits and the mean cross-entropy per sample is reported in the MSE's
        place (same label and key); the argmax is the same."""
        out = self.net_wrapper_.mlp.forward(self.net_wrapper_.params, x).double().cpu().numpy()
        if self.net_wrapper_.loss == "softmax_xent" and out.size:
            m = out.max(1, keepdims=True)
            lse = m + np.log(np.exp(out - m).sum(1, keepdims=True))
            mse = float((y * (lse - out)).sum(1).mean())
        else:
            mse = float(((out - y) ** 2).mean()) if out.size else 0.0
        acc = float((out.argmax(1) == y.argmax(1)).mean() * 100.0) if out.size else 0.0
        if self.rank == 0:
            print(f"{label}: MSE={mse:g}, Accuracy={acc:g}%")
        return dict(mse=mse, accuracy=acc)

    def metrics(self, split: str = "train", k: int = 1, confusion: bool = False):
        """Device-side evaluation of a split (engine.Mlp.evaluate): loss, accuracy, top-k and optionally the
        confusion matrix, as an engine.EvalResult. Under data parallelism each rank evaluates its contiguous shard
        and every rank gets the same totals. Prints nothing. It runs on a network of its own, so it may be called
        while a solver is open on the launcher's network."""
        if split not in ("train", "test"):
            raise LbfError(f"split must be 'train' or 'test', got {split!r}")
        d = self.data_
        if d is None or (split == "test" and d.test_xs is None):
            raise LbfError(f"no {split} split: call setData() with one first")
        nw = self.net_wrapper_
        if getattr(self, "eval_mlp_", None) is None:
            self.eval_mlp_ = engine.Mlp(self.ctx, nw.mlp.dims, nw.mlp.acts, loss=nw.loss)
        elif self.eval_mlp_.loss_name != nw.loss:
            self.eval_mlp_.loss_name = nw.loss
        x, y = (d.x, d.y) if split == "train" else (d.test_xs, d.test_ys)
        return self.eval_mlp_.evaluate(nw.params, x, y, k=k, confusion=confusion)

    def spectrum(self, split: str = "train", steps: int = 32, matrix: str = "gauss_newton", **kw):
        """The curvature spectrum at the current parameters (engine.Mlp.lanczos, an engine.LanczosResult): `steps`
        steps of Lanczos on the Gauss-Newton matrix or the exact Hessian ("hessian") of the mean loss over a split,
        plus the network's l2. Under data parallelism each rank passes its shard and every rank gets the same bits.
        kw: seed, v0, reorth, basis, check. Like metrics() it runs on a network of its own."""
        if split not in ("train", "test"):
            raise LbfError(f"split must be 'train' or 'test', got {split!r}")
        d = self.data_
        if d is None or (split == "test" and d.test_xs is None):
            raise LbfError(f"no {split} split: call setData() with one first")
        nw = self.net_wrapper_
        if getattr(self, "spec_mlp_", None) is None:
            self.spec_mlp_ = engine.Mlp(self.ctx, nw.mlp.dims, nw.mlp.acts, loss=nw.loss)
        elif self.spec_mlp_.loss_name != nw.loss:
            self.spec_mlp_.loss_name = nw.loss
        x, y, rows = (d.x, d.y, d.n_global) if split == "train" else (d.test_xs, d.test_ys, d.n_test)
        return self.spec_mlp_.lanczos(nw.params, x, y, steps=steps, matrix=matrix, l2=nw.mlp.l2,
                                      inv_scale=1.0 / max(rows, 1), **kw)

    def getWrapper(self):
        return self.net_wrapper_
