"""lbfgs-ffnn_amd — MI355X-native L-BFGS / S-LBFGS engine for dense FFNNs.

Compute lives in ``build/liblbfgs_amd_abi3.so`` (hand-written HIP kernels for gfx950 behind the C ABI
``include/lbfgs_amd.h``). This package is the host-side mirror of the reference's unified API.
The directory name contains a hyphen, so load it with :func:`load` from the repo root helpers
(``tests/conftest.py``, ``bench.py``, ``__graft_entry__.py``) under the module name ``lbfgs_ffnn_amd``.
"""
from ._lib import LIB_PATH, LbfError, lib  # noqa: F401
from .engine import (AdamRun, Context, EvalResult, History, LanczosResult, LbfgsRun, Mlp, SlbfgsRun,  # noqa: F401
                     adam_coefs, adam_epoch_orders, adam_params, adam_solve, gd_params, gd_solve,
                     grad_flops_per_sample, hf_params, hf_solve, init_params_host, lbfgs_params, lbfgs_solve,
                     lbfgs_solve_fn, load_idx_images, load_idx_labels, owlqn_params, owlqn_solve, sample_indices,
                     sgd_params, sgd_solve, slbfgs_params, slbfgs_solve, slq_density, spectral_density, synth_mnist,
                     synth_regression, tridiag_eig)
from .unified import (EarlyStopper, UnifiedAdam, IterationRecorder, UnifiedConfig, UnifiedDataset, UnifiedGD, UnifiedHF, UnifiedLauncher, UnifiedOWLQN,  # noqa: F401
                      UnifiedLBFGS, UnifiedSGD, UnifiedSLBFGS, write_history_csv, write_validation_csv)
