/* include/lbfgs_amd.h — C ABI of the MI355X-native L-BFGS / S-LBFGS engine (liblbfgs_amd_abi3.so).
 *
 * Plain pointers and sizes only (no torch / HIP types in the signatures; a stream is passed as void*).
 * Every entry point names the reference interface it replaces (paths relative to SignorB/lbfgs-FFNN).
 * Conventions:
 *   - return value: LBF_OK (0) or an error code; lbf_last_error() gives the message (thread-local).
 *   - d_* arguments are device pointers (hipMalloc'd or torch tensors' data_ptr), h_* are host pointers.
 *   - d_* float pointers need 4-byte alignment only; 16-byte-aligned ones take faster routes; lbf_two_loop
 *     mode 3 is the exception (it returns LBF_ERR_INVALID unless d_S, d_Y, d_g and d_dir are 16-byte aligned).
 *   - calls are asynchronous on the context stream unless they return a host value.
 *   - parameter layout is the reference's flat vector: per layer [W (Out x In, column-major) | b (Out)]
 *     (src/network.hpp:45-71, src/cuda/network.cuh:36-59); data X is In x N column-major and Y is
 *     Out x N column-major, i.e. one sample per contiguous row of In (resp. Out) floats.
 *   - one context per GPU, one host thread per context (the reference is single-threaded too,
 *     src/cuda/common.cuh).
 */
#ifndef LBFGS_AMD_H
#define LBFGS_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBF_OK 0
#define LBF_ERR_INVALID 1 /* bad argument (reference: early return in lbfgs.cuh:45-48)          */
#define LBF_ERR_HIP 2     /* HIP runtime error (reference: cuda_check abort, common.cuh:18-23)  */
#define LBF_ERR_COMM 3    /* RCCL error                                                         */
#define LBF_ERR_STATE 4   /* call out of order                                                  */

/* Activation ids == the reference's ActivationType (src/cuda/kernels.cuh:53-58). */
#define LBF_ACT_LINEAR 0
#define LBF_ACT_TANH 1
#define LBF_ACT_RELU 2
#define LBF_ACT_SIGMOID 3
/* Rectifiers with curvature (an extension: the reference has the four above). Constants are fixed. */
#define LBF_ACT_LEAKY_RELU 4 /* x > 0 ? x : 0.01 x                          */
#define LBF_ACT_ELU 5        /* x > 0 ? x : expm1(x)             (alpha 1)  */
#define LBF_ACT_SOFTPLUS 6   /* max(x, 0) + log1p(exp(-|x|)) = log(1 + e^x) */

/* Line-search / two-loop policies.
 * WOLFE  = CPU semantics: src/minimizer/lbfgs.hpp:38-139 + full_batch_minimizer.hpp:126-157.
 * ARMIJO = CUDA semantics: src/cuda/lbfgs.cuh:39-261. */
#define LBF_LS_WOLFE 0
#define LBF_LS_ARMIJO 1

/* Parameter-initialisation streams (both libstdc++ mt19937, seed = UnifiedConfig::seed):
 * CPU  = normal_distribution<double> over all params (src/network.hpp:45-71);
 * CUDA = normal_distribution<float> over weights, zero biases (src/cuda/network.cuh:36-59). */
#define LBF_INIT_CPU 0
#define LBF_INIT_CUDA 1

typedef struct lbf_ctx lbf_ctx;
typedef struct lbf_mlp lbf_mlp;
typedef struct lbf_lbfgs lbf_lbfgs;

/* ABI revision of this header. The library's file name and SONAME carry it (liblbfgs_amd_abi3.so), so a
 * binary linked against another revision fails to load instead of handing this library structs of a
 * different size: ABI 1 had no lbf_abi_version() to check, and lbf_solve_info / lbf_slbfgs_params have
 * grown since. Within one revision structs never change. A caller that loads the library by path (dlopen,
 * ctypes) checks lbf_abi_version() == LBF_ABI_VERSION before passing any struct.
 * 2: lbf_solve_info.n_grad_after_loss; lbf_comm_init_local (in-process rank group).
 * 3: lbf_slbfgs_params.dp_mode; the revision in the library name. */
#define LBF_ABI_VERSION 3

const char *lbf_last_error(void);
const char *lbf_version(void);
int lbf_abi_version(void);

/* ---- context: device, stream, workspace, optional communicator --------------------------------
 * Replaces CublasHandle (src/cuda/cublas_handle.cuh:22-39) + the implicit legacy stream. */
int lbf_ctx_create(int device, void *stream /* hipStream_t or NULL = own stream */, lbf_ctx **out);
int lbf_ctx_destroy(lbf_ctx *ctx);
int lbf_ctx_sync(lbf_ctx *ctx);
void *lbf_ctx_stream(lbf_ctx *ctx);

/* ---- data-parallel communicator (RCCL over xGMI). New in this engine: the reference has no
 * collective. One all-reduce of [grad | loss] per loss+grad evaluation. */
int lbf_comm_unique_id(char out[128]);
int lbf_comm_init(lbf_ctx *ctx, int nranks, int rank, const char id[128]);
/* In-process rank group: ctxs[r] becomes rank r of an nranks-rank group whose all-reduce sums every rank's
 * buffer on the device in rank order (HIP events + a host barrier; no RCCL). All contexts must live on one
 * device and each rank must then be driven by its own host thread, calling the same sequence of
 * evaluations as the others (exactly as one process per GPU would). RCCL refuses two ranks on one GPU,
 * so this is how the multi-rank path (shard offsets, n_global scaling, minibatch slices, replicated
 * line-search decisions over summed data) runs on a single GPU; the product route is lbf_comm_init.
 * ABI 2. */
int lbf_comm_init_local(lbf_ctx **ctxs, int nranks);
int lbf_comm_rank(lbf_ctx *ctx, int *rank, int *nranks);
int lbf_allreduce_sum(lbf_ctx *ctx, float *d_buf, size_t count);

/* ---- dense MLP --------------------------------------------------------------------------------
 * Replaces CudaNetwork (src/cuda/network.cuh:21-158) / CudaDenseLayer (src/cuda/layer.cuh).
 * acts[l] is an LBF_ACT_* id, 0..6 (else LBF_ERR_INVALID). Only the post-activation values y are stored, and
 * act' and act'' are taken through them:
 *   linear      y = x                               act' = 1                    act'' = 0
 *   tanh        y = tanh x                          act' = 1 - y^2              act'' = -2 y (1 - y^2)
 *   relu        y = max(x, 0)                       act' = [y > 0]              act'' = 0
 *   sigmoid     y = 1 / (1 + e^-x)                  act' = y (1 - y)            act'' = y (1 - y) (1 - 2 y)
 *   leaky_relu  y = x > 0 ? x : 0.01 x              act' = y > 0 ? 1 : 0.01     act'' = 0
 *   elu         y = x > 0 ? x : expm1(x)            act' = y > 0 ? 1 : y + 1    act'' = y > 0 ? 0 : y + 1
 *   softplus    y = max(x, 0) + log1p(e^-|x|)       act' = -expm1(-y)           act'' = e^-y (-expm1(-y))
 * The slope 0.01 and alpha 1 are fixed (torch's defaults); there is no per-layer parameter. The three new ones
 * are strictly increasing, so y determines x and the identities are exact. Any of them may sit on the output
 * layer under LBF_LOSS_MSE; LBF_LOSS_SOFTMAX_XENT keeps its linear last layer. The fused output-layer kernels carry
 * the first four only: with one of the three on the last or the last hidden layer, the output layer runs as a forward
 * GEMM, the loss kernel and a backward GEMM (same results, one more pass over the last activations).
 * lbf_mlp_init_params and lbf_init_params_host give relu, leaky_relu, elu and softplus the same sqrt(2) gain in
 * both init modes, so exchanging one for another keeps a seed's start point bit for bit. */
int lbf_mlp_create(lbf_ctx *ctx, int nlayers, const int *dims /* nlayers+1 */, const int *acts /* nlayers */,
                   lbf_mlp **out);
int lbf_mlp_destroy(lbf_mlp *net);
long long lbf_mlp_param_count(const lbf_mlp *net);
/* bindParams(seed) (network.cuh:36-59 / network.hpp:45-71): host libstdc++ RNG, upload to d_params. */
int lbf_mlp_init_params(lbf_mlp *net, unsigned seed, int init_mode, float *d_params);
/* Host-only form of the same draws (h_out holds lbf count of params); no device needed. */
int lbf_init_params_host(int nlayers, const int *dims, const int *acts, unsigned seed, int init_mode, float *h_out);
/* forward_only (network.cuh:79-88): d_out is batch x Out row-major (== Out x batch column-major). */
int lbf_mlp_forward(lbf_mlp *net, const float *d_params, const float *d_X, long long batch, float *d_out);
/* compute_loss_and_grad (network.cuh:97-119) == the LossGradFun of minimizer_base.cuh:15-16:
 *   loss = 0.5*||net(X)-Y||^2 * inv_scale + 0.5*l2*||w||^2,  grad = dloss/dw (written to d_grad).
 * inv_scale is 1/batch in the reference; under data parallelism pass 1/global_batch and the
 * context's communicator sums the shards. d_idx (nullable) gathers rows of X/Y (S-LBFGS minibatches,
 * unified_optimization.hpp:361-364). h_loss receives the loss (synchronises). */
int lbf_mlp_loss_grad(lbf_mlp *net, const float *d_params, float *d_grad, const float *d_X, const float *d_Y,
                      const int *d_idx, long long batch, double inv_scale, double l2, double *h_loss);

/* ---- two-loop recursion (src/minimizer/lbfgs.hpp:106-139 / s_lbfgs.hpp:106-136 /
 * lbfgs.cuh:206-261) on an explicit history given in logical order (oldest first):
 * d_S, d_Y are k x n row-major, h_rho[k]. mode: 0 = CPU (returns -Hg), 1 = S-LBFGS (returns +Hg,
 * gamma guarded and clamped), 2 = CUDA (returns -Hg, gamma guarded), 3 = S-LBFGS as the S-LBFGS solver computes
 * it: each pair offered through the solver's pair update (kept when |y.s| > 1e-10, rho = 1 / y.s on the device,
 * h_rho ignored; s_lbfgs.hpp:245-256), then one direction-only step (the coefficients from the pairs' map K;
 * k <= 16, n % 4 == 0). */
/* Exact Hessian-vector product of the batch loss of lbf_mlp_loss_grad (same inv_scale / l2 / d_idx
 * meaning): d_hv = H(params) d_v, computed with Pearlmutter's R-operator on the device (one forward
 * and backward R-pass; no finite differences). With a communicator the shards' products are summed.
 * Replaces, as an option, the finite-difference HVP of s_lbfgs.hpp:88-101. */
int lbf_mlp_hvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                const int *d_idx, long long batch, double inv_scale, double l2, float *d_hv);
/* Generalized Gauss-Newton vector product of the same batch loss (extension; same inv_scale / l2 / d_idx meaning,
 * argument checks, 4-byte pointer alignment and error codes as lbf_mlp_hvp): d_gv = J^T H_L J d_v + l2 d_v, with
 * J the Jacobian of the network up to where the convex loss begins and H_L that loss's Hessian. The split is at
 * the post-activation outputs A_L for LBF_LOSS_MSE (H_L = inv_scale I) and at the logits for
 * LBF_LOSS_SOFTMAX_XENT (H_L = inv_scale Ysum (diag p - p p^T), p = softmax). With Z_l = A_{l-1} W_l + b_l,
 * A_l = act_l(Z_l), s = inv_scale and d_v = [V_l ; v_l] in the parameter layout:
 *   R-forward   T_l     = A_{l-1} V_l + v_l                  (l = 0: X V_0 + v_0, rows gathered by d_idx)
 *               R{Z_l}  = T_l + R{A_{l-1}} W_l               (l >= 1; the second product has no bias)
 *               R{A_l}  = act'_l(A_l) .* R{Z_l}              (hidden layers)
 *   output      M_L     = s act'_L(A_L)^2 .* R{Z_L}                          (LBF_LOSS_MSE)
 *               M_L     = s Ysum p .* (R{Z_L} - sum_k p_k R{Z_L}_k)          (LBF_LOSS_SOFTMAX_XENT)
 *   backward    (G v)_l = [A_{l-1} | 1]^T M_l,   M_{l-1} = (M_l W_l^T) .* act'_{l-1}(A_{l-1})
 * act' is taken through the post-activation value (ReLU: [a > 0]). G is positive semi-definite for both losses
 * and has no term from an activation's kink or curvature: v.Gv >= l2 v.v. It is the exact product without
 * (A_L - y) act''_L, [R{A_{l-1}} | 0]^T dZ_l, dZ_l V_l^T and delta act'' R{Z}; the two agree for a single linear
 * layer and at zero residual. One forward, the R-forward and one backward pass; no finite differences. With a
 * communicator the shards' products are summed (one all-reduce, before the l2 term); batch == 0 gives l2 d_v. */
int lbf_mlp_gnvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                 const int *d_idx, long long batch, double inv_scale, double l2, float *d_gv);
/* Per-minibatch gradients at one point (extension; the reference evaluates them one step at a time:
 * SLBFGS::stochastic_solve's batch_g(w) of every inner step, s_lbfgs.hpp:218-230, at the epoch's fixed anchor
 * w): rows [t cnt, (t+1) cnt) of d_X / d_Y are minibatch t, t < nmb; its gradient of
 * 0.5 inv_scale ||net - Y||^2 + 0.5 l2 ||w||^2 is written to d_grads + t ld (ld >= param count). One
 * evaluation over nmb cnt rows whose dW GEMMs split K at the minibatch boundaries. cnt % 32 == 0.
 * Single rank only (a communicator's ranks would each hold partial sums). */
int lbf_mlp_batch_grads(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, int nmb,
                        long long cnt, double inv_scale, double l2, float *d_grads, long long ld);
/* Loss only (CudaNetwork::forward_only, network.cuh:79-88, + the MSE of network.cuh:105; the CPU f closure of
 * unified_optimization.hpp:101-108): forward pass and 0.5 * inv_scale * ||out - Y||^2 (summed over ranks with a
 * communicator), bitwise the loss lbf_mlp_loss_grad reports for the same point. */
int lbf_mlp_loss(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                 long long batch, double inv_scale, double *h_loss);
/* finite_difference_hvp_batch (src/minimizer/s_lbfgs.hpp:88-101): y = (g(w + eps v) - g(w - eps v)) / (2 eps)
 * of the batch loss (inv_scale, + l2 w), computed exactly as the S-LBFGS solver's curvature pair does
 * (two fused batch evaluations; the fp32 difference times the once-rounded 1/(2 eps)). */
int lbf_mlp_fd_hvp(lbf_mlp *net, const float *d_params, const float *d_v, const float *d_X, const float *d_Y,
                   const int *d_idx, long long batch, double inv_scale, double l2, double eps, float *d_y);
/* The loss of the network (extension; the reference has the squared error only). LBF_LOSS_MSE (the default) is
 * the loss documented above. LBF_LOSS_SOFTMAX_XENT: the network's outputs z are logits (the last layer's
 * activation must be LBF_ACT_LINEAR and it must have at least two outputs, else LBF_ERR_INVALID), and with
 * lse_b = log sum_o exp(z_bo)
 *   loss = inv_scale * sum_b sum_o y_bo (lse_b - z_bo) + 0.5*l2*||w||^2        (no factor 0.5)
 * for target rows y_b >= 0 (one-hot or soft; not validated). inv_scale, l2, d_idx, sharding and n_global keep
 * their meaning. It is a property of the network: lbf_mlp_loss_grad, lbf_mlp_loss, lbf_mlp_hvp, lbf_mlp_fd_hvp,
 * lbf_mlp_batch_grads and every solver created on the network minimise it; lbf_mlp_forward returns the logits.
 * Takes effect from the next evaluation / solve. Must not be changed between *_begin and *_end of a stateful
 * solver (its history and recorded losses would mix two objectives). */
#define LBF_LOSS_MSE 0
#define LBF_LOSS_SOFTMAX_XENT 1
int lbf_mlp_set_loss(lbf_mlp *net, int loss);
int lbf_mlp_get_loss(const lbf_mlp *net, int *loss);
/* L2 weight decay of the solvers that take no lambda of their own (extension; the reference's full-batch
 * solvers have none). lbf_lbfgs_solve, lbf_lbfgs_begin / iterate / end, lbf_gd_solve and lbf_sgd_solve on the
 * network minimise
 *   data loss + 0.5*l2*||w||^2
 * with either loss, and everything they report includes the penalty: lbf_record.loss and grad_norm, the line
 * search's f, final_loss and final_grad_norm (gradient: data gradient + l2*w). SGD's epoch loss is then the
 * row-weighted mean of the batch objectives, penalty included. Default 0; l2 < 0 or a non-finite value returns
 * LBF_ERR_INVALID. A property of the network, like the loss: read at *_begin / at the start of a solve, and it
 * must not be changed between *_begin and *_end. NOT affected: the functions with an l2 argument of their own
 * (lbf_mlp_loss_grad, lbf_mlp_hvp, lbf_mlp_fd_hvp, lbf_mlp_batch_grads), lbf_slbfgs_* (lbf_slbfgs_params.lambda),
 * lbf_mlp_loss (the data term) and lbf_lbfgs_solve_fn (the callback is the whole objective). */
int lbf_mlp_set_l2(lbf_mlp *net, double l2);
int lbf_mlp_get_l2(const lbf_mlp *net, double *l2);
/* Device-side evaluation (extension; replaces the host scan of UnifiedLauncher::evaluate,
 * src/unified_launcher.hpp:154-199, which copies every output to the host): forward pass and one metrics kernel
 * per chunk of chunk_rows rows (0: 65536, or the batch if smaller; the activation workspace is bounded by the
 * chunk, and no result depends on the chunking beyond the regrouping of the loss's fp64 sum).
 *   predicted class of a row: the reference's scan: best = 0, m = -1e20; for o = 0..Out-1: if z_o > m take it.
 *     The lowest index wins a tie, a NaN never wins, a row with nothing above -1e20 gives 0 (numpy.argmax differs
 *     on NaN rows). z = what lbf_mlp_forward returns: the outputs of an MSE net, the logits of a cross-entropy net.
 *   target class: the same scan over the target row (one-hot or soft); d_idx gathers target and input rows.
 *   correct: rows with predicted == target class.
 *   topk:    rows whose target class t has rank < k, rank = #{o : z_o > z_t} + #{o < t : z_o == z_t}, 1 <= k <= Out;
 *            for finite outputs k = 1 gives correct. Rows holding a non-finite output are outside this contract;
 *            they are counted in rows and never fault.
 *   loss:    the network's data loss with the caller's inv_scale, as lbf_mlp_loss defines it (no l2 term),
 *            accumulated in fp64 in a fixed order: a second call gives the bitwise same value.
 *   h_confusion (nullable, needs d_Y): Out*Out counts, [target * Out + predicted].
 *   d_pred (nullable): batch ints, the predicted class per row, in batch (gathered) order.
 *   d_proba (nullable): batch*Out floats, softmax of the logits; LBF_LOSS_SOFTMAX_XENT nets only.
 * d_Y NULL: predictions only; loss, correct and topk are 0. With a communicator every rank passes its own
 * batch local rows (0 is legal: an empty share) and receives the totals over all ranks, bitwise the same on every
 * rank (world <= 256); d_pred and d_proba stay local. Synchronous: it returns host values.
 * LBF_ERR_INVALID: null handles, k outside 1..Out, h_confusion without d_Y, d_proba on an MSE net.
 * All state is the network's own: no other network's evaluation and no solver of another network is disturbed.
 * To evaluate while a stateful solver (lbf_lbfgs_begin / lbf_slbfgs_begin .. *_end) is open, use a second
 * lbf_mlp of the same shape between two *_iterate calls: the parameters live outside the networks, so the second
 * one costs only workspace. On the solver's own network this call overwrites the activations, exactly as
 * lbf_mlp_forward does. */
typedef struct lbf_eval_result {
  double loss;
  long long rows, correct, topk;
  int k, reserved;
} lbf_eval_result;
int lbf_mlp_evaluate(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                     long long batch, double inv_scale, int k, long long chunk_rows, lbf_eval_result *h_res,
                     long long *h_confusion, int *d_pred, float *d_proba);
int lbf_two_loop(lbf_ctx *ctx, long long n, int k, const float *d_S, const float *d_Y, const double *h_rho,
                 const float *d_g, float *d_dir, int mode);

/* ---- BLAS-1 with device-side deterministic fp64 reductions (replace kernels.cuh:14-50). */
int lbf_dot(lbf_ctx *ctx, long long n, const float *d_x, const float *d_y, double *h_out);
int lbf_nrm2(lbf_ctx *ctx, long long n, const float *d_x, double *h_out);
int lbf_axpy(lbf_ctx *ctx, long long n, float alpha, const float *d_x, float *d_y);
int lbf_scal(lbf_ctx *ctx, long long n, float alpha, float *d_x);

/* ---- solvers --------------------------------------------------------------------------------- */
typedef struct lbf_lbfgs_params {
  int m;              /* history size (UnifiedConfig::m_param; LBFGS::setHistorySize lbfgs.hpp:29) */
  int max_iters;      /* setMaxIterations                                                         */
  double tol;         /* setTolerance: stop when ||g|| < tol                                      */
  int line_search;    /* LBF_LS_WOLFE | LBF_LS_ARMIJO                                             */
  int max_line_iters; /* 50 (full_batch_minimizer.hpp:116) | 20 (minimizer_base.cuh:63)           */
  double c1, c2, rho; /* 1e-4, 0.9, 0.5 (full_batch_minimizer.hpp:113-115; minimizer_base.cuh:64)  */
} lbf_lbfgs_params;

typedef struct lbf_slbfgs_params {
  int max_epochs;     /* UnifiedConfig::max_iters (outer iterations)                  */
  double tol;         /* full-gradient norm tolerance (s_lbfgs.hpp:208)              */
  int M, L, b, b_H;   /* m_param, L_param, batch_size, b_H_param (unified_optimization.hpp:325) */
  double step;        /* learning_rate                                                */
  double lambda;      /* L2, 1e-4 in the reference (unified_optimization.hpp:334)    */
  unsigned seed;      /* kDefaultSeed = 123 (src/seed.hpp:4; s_lbfgs.hpp:183)        */
  double fd_eps;      /* finite-difference HVP epsilon, 1e-4 (s_lbfgs.hpp:90)        */
  int hvp_exact;      /* the curvature pair's y: LBF_HVP_FD (0) the reference's central-difference HVP
                         (s_lbfgs.hpp:88-101); LBF_HVP_EXACT (1) the exact R-operator product
                         (lbf_mlp_hvp); LBF_HVP_GAUSS_NEWTON (2) the Gauss-Newton
                         product (lbf_mlp_gnvp): y.s >= lambda s.s > 0 for every pair. Any other
                         non-zero value is taken as LBF_HVP_EXACT                              */
  /* ABI 2, diagnostics (NULL / 0: off): one row of LBF_PAIR_TRACE_COLS doubles per curvature-pair
   * candidate (s_lbfgs.hpp:245-256): epoch, inner step t, y.s, s.s, y.y, accepted (|y.s| > 1e-10), live
   * pairs after it, 0. Reading each row back synchronises the stream: not for timed runs. */
  double *pair_trace;
  int pair_trace_cap;
  /* ABI 3, data parallelism (a communicator on the context): LBF_SLBFGS_DP_REPLICATED (default) runs the
   * whole minibatch chain on every rank with no collective (identical inputs, identical bits) and shards
   * only the full-batch gradient at each epoch's anchor (s_lbfgs.hpp:206, 274-284), one all-reduce per
   * epoch; LBF_SLBFGS_DP_SLICED evaluates this rank's 1/p slice of every minibatch and Hessian batch, one
   * all-reduce per inner step. Ignored without a communicator. */
  int dp_mode;
} lbf_slbfgs_params;
#define LBF_PAIR_TRACE_COLS 8
#define LBF_SLBFGS_DP_REPLICATED 0
#define LBF_SLBFGS_DP_SLICED 1
#define LBF_HVP_FD 0
#define LBF_HVP_EXACT 1
#define LBF_HVP_GAUSS_NEWTON 2

/* Gradient descent with momentum == cuda_mlp::CudaGD (src/cuda/gd.cuh:38-106; setters :22-25). */
typedef struct lbf_gd_params {
  double lr;          /* setLearningRate, 0.01                                               */
  double momentum;    /* setMomentum, 0.9 (0: plain x -= lr g)                               */
  int max_iters;      /* setMaxIterations, 200 (minimizer_base.cuh:62)                       */
  double tol;         /* setTolerance: stop when ||g|| < tol, 1e-6 (minimizer_base.cuh:63)   */
} lbf_gd_params;

/* Minibatch SGD with momentum and step decay == cuda_mlp::CudaSGD (src/cuda/sgd.cuh:50-153).
 * Contiguous, unshuffled batches as in the reference; single rank. */
typedef struct lbf_sgd_params {
  double lr, momentum; /* 0.01, 0.9                                                         */
  int batch;           /* setBatchSize                                                      */
  double decay_rate;   /* setLearningRateDecay(rate, step): lr *= rate every step epochs (1.0) */
  int decay_step;      /* 0: no decay                                                       */
  int max_epochs;      /* setMaxIterations (epochs), 200                                    */
  double tol;          /* relative epoch-loss improvement stop when > 0, 1e-6               */
} lbf_sgd_params;

/* Per-iteration history == IterationRecorder (src/iteration_recorder.hpp:13-146) plus extras.
 * Host arrays of capacity cap; any pointer may be NULL. */
typedef struct lbf_record {
  double *loss, *grad_norm, *time_ms, *alpha;
  int *ls_trials, *accepted;
  int cap, size;
} lbf_record;

typedef struct lbf_solve_info {
  int iterations;
  long long n_evals;  /* fused loss+grad evaluations executed by this solve */
  double final_loss, final_grad_norm;
  long long n_rows;   /* batch rows those evaluations covered on this rank (0 for callback objectives) */
  long long n_loss_only; /* line-search trials evaluated forward + loss only (rejected by Armijo) */
  /* ABI 2: backward passes run on the forward state of a loss-only trial (it passed Armijo). Each is
   * counted in n_evals too, so forward passes = n_evals - n_grad_after_loss + n_loss_only and
   * backward passes = n_evals. */
  long long n_grad_after_loss;
} lbf_solve_info;

void lbf_lbfgs_default_params(lbf_lbfgs_params *p, int line_search);
void lbf_slbfgs_default_params(lbf_slbfgs_params *p);

/* Full-batch L-BFGS (CudaLBFGS::solve lbfgs.cuh:39-194 / LBFGS::solve lbfgs.hpp:38-100): params are
 * updated in place. n_local rows of X/Y live on this rank; n_global = sum over ranks (the loss and
 * gradient are means over n_global, matching the single-process reference). */
int lbf_lbfgs_solve(lbf_mlp *net, const lbf_lbfgs_params *prm, float *d_params, const float *d_X,
                    const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                    lbf_solve_info *info);

/* Stateful form for benchmarking: begin evaluates the start point; iterate runs up to iters more
 * iterations (returns early on convergence); end releases the history. */
int lbf_lbfgs_begin(lbf_mlp *net, const lbf_lbfgs_params *prm, float *d_params, const float *d_X,
                    const float *d_Y, long long n_local, long long n_global, lbf_lbfgs **out);
int lbf_lbfgs_iterate(lbf_lbfgs *s, int iters, lbf_record *rec, lbf_solve_info *info);
int lbf_lbfgs_end(lbf_lbfgs *s);

/* L-BFGS on an arbitrary objective given as a callback with the reference's LossGradFun contract
 * (src/cuda/minimizer_base.cuh:15-16: loss returned, gradient written to device memory), i.e. the
 * CudaMinimizerBase::solve(n, params, ..., loss_grad) entry point (minimizer_base.cuh:54-59). The
 * history, two-loop and line-search state stay on the device; the callback is invoked once per trial. */
typedef double (*lbf_loss_grad_fn)(void *user, const float *d_params, float *d_grad);
int lbf_lbfgs_solve_fn(lbf_ctx *ctx, const lbf_lbfgs_params *prm, long long n, float *d_params,
                       lbf_loss_grad_fn fn, void *user, lbf_record *rec, lbf_solve_info *info);

/* S-LBFGS (SLBFGS::stochastic_solve s_lbfgs.hpp:165-290 via UnifiedSLBFGS_CPU,
 * unified_optimization.hpp:306-408). X/Y hold all N rows on every rank; minibatches are sampled on
 * the host with the reference's libstdc++ stream and sliced across ranks. */
/* CudaGD::solve / CudaSGD::solve (the reference's CudaMinimizerBase::solve, minimizer_base.cuh:54-59) on
 * the MLP. GD: full batch over the n_local rows of this rank (n_global = sum over ranks, as for
 * lbf_lbfgs_solve). rec: one record per iteration (GD) / the initial full-batch record then one per
 * epoch (SGD, only when rec is non-NULL, like the reference's recorder_ branch). */
void lbf_gd_default_params(lbf_gd_params *p);
void lbf_sgd_default_params(lbf_sgd_params *p);
int lbf_gd_solve(lbf_mlp *net, const lbf_gd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info);
int lbf_sgd_solve(lbf_mlp *net, const lbf_sgd_params *prm, float *d_params, const float *d_X, const float *d_Y,
                  long long N, lbf_record *rec, lbf_solve_info *info);

/* ---- Hessian-free (truncated Newton) optimisation: Gauss-Newton conjugate gradients (extension; Martens 2010).
 * New functions and structs only: LBF_ABI_VERSION stays 3.
 *
 * lbf_mlp_gn_cg solves (G + damping I) x = b by conjugate gradients from x = 0, G the Gauss-Newton matrix of
 * lbf_mlp_gnvp at d_params on the given batch (same d_idx / batch / inv_scale meaning, shards summed over a
 * communicator, batch == 0 an empty share). The forward pass runs once for the whole solve; an iteration is the
 * product on the direction plus three sweeps over the parameters, and every scalar (alpha, beta, the stopping
 * test) is formed on the device from fixed-order fp64 partial sums: no host round trip per iteration, no float
 * atomics, bitwise reproducible. The host enqueues `check` iterations, then reads the status block; launches
 * enqueued past the stopping iteration are no-ops, so the result does not depend on `check`.
 *   status 0: rr <= rtol^2 rr0 (b = 0 gives x = 0 in 0 iterations);  1: max_iters reached;
 *          2: p.Ap <= 0 or non-finite (an indefinite damping, a non-finite input): that iteration's update is not
 *             applied and x is the last good iterate.
 * rr0 = b.b, rr = r.r of the recurrence residual, xb = x.b, xr = x.r, xx = x.x (fp64). d_x and d_b: parameter
 * count floats, 4-byte aligned. LBF_ERR_INVALID: null handles, max_iters < 0, rtol < 0, check < 1. */
typedef struct lbf_cg_params {
  int max_iters;  /* 50  */
  double rtol;    /* 0.1: stop when ||r|| <= rtol ||b|| */
  double damping; /* 0   */
  int check;      /* 10: iterations enqueued between two reads of the status block */
} lbf_cg_params;
typedef struct lbf_cg_info {
  int iterations, status;
  double rr0, rr, xb, xr, xx;
} lbf_cg_info;
void lbf_cg_default_params(lbf_cg_params *p);
int lbf_mlp_gn_cg(lbf_mlp *net, const float *d_params, const float *d_b, const float *d_X, const float *d_Y,
                  const int *d_idx, long long batch, double inv_scale, const lbf_cg_params *prm, float *d_x,
                  lbf_cg_info *info);
/* Diagnostics: the recurrence residual r of the network's last lbf_mlp_gn_cg / Hessian-free step (parameter count
 * floats into a device buffer). LBF_ERR_INVALID before the first solve. */
int lbf_mlp_gn_cg_residual(lbf_mlp *net, float *d_r);

/* Hessian-free solver on the objective of lbf_gd_solve (the network's loss + its l2, a mean over n_global, n_local
 * rows on this rank). Outer iteration k, with damping lambda_k (lambda_0 = damping0):
 *   1. f, g by the fused evaluation; stop when ||g|| < tol;
 *   2. CG on (G + (l2 + lambda_k) I) p = -g, at most cg_iters iterations, relative residual cg_rtol;
 *   3. model value q = g.p + 0.5 p^T (G + l2 I) p, from the CG status block;
 *   4. backtracking: alpha = 1, rho, rho^2, .. (at most max_line_iters trials, loss-only evaluations) until
 *      f(x + alpha p) <= f + c1 alpha g.p; if every trial fails the point stays (accepted = 0, alpha = 0);
 *   5. ratio = (f(x + p) - f) / q from the first trial; lambda *= damp_up if ratio < ratio_lo, lambda *= damp_down
 *      if ratio > ratio_hi;
 *   6. lbf_record row: loss and gradient norm at the iteration's start point, alpha, ls_trials, accepted.
 * curv_rows > 0: the curvature (step 2) is taken on the contiguous window of curv_rows rows starting at
 * (k curv_rows) mod (n_local - curv_rows + 1), with inv_scale 1 / curv_rows; single rank only (LBF_ERR_INVALID
 * with a communicator, like lbf_sgd_solve). curv_rows == 0: all local rows; with a communicator every rank then
 * runs the same vector arithmetic on all-reduced inputs and takes the same decisions.
 * Traces (nullable, trace_cap entries): per outer iteration the damping after step 5, the ratio, the CG
 * iterations. info->n_evals counts the fused evaluations (one per outer iteration and the final point's),
 * n_loss_only the line-search trials. */
typedef struct lbf_hf_params {
  int max_iters;      /* outer iterations, 100 */
  double tol;         /* stop when ||g|| < tol, 1e-6 */
  int cg_iters;       /* 50  */
  double cg_rtol;     /* 0.1 */
  int cg_check;       /* 10  */
  double damping0, damp_up, damp_down, ratio_lo, ratio_hi; /* 1.0, 1.5, 2/3, 0.25, 0.75 */
  double c1, rho;     /* 1e-4, 0.5 */
  int max_line_iters; /* 20 */
  long long curv_rows; /* 0: all local rows */
  double *damping_trace, *ratio_trace;
  int *cg_trace;
  int trace_cap;
} lbf_hf_params;
void lbf_hf_default_params(lbf_hf_params *p);
int lbf_hf_solve(lbf_mlp *net, const lbf_hf_params *prm, float *d_params, const float *d_X, const float *d_Y,
                 long long n_local, long long n_global, lbf_record *rec, lbf_solve_info *info);

/* ---- Preconditioned Hessian-free (extension; Martens 2010, section 4.7). New functions and one new struct only:
 * lbf_hf_params, lbf_cg_params and lbf_cg_info are unchanged and LBF_ABI_VERSION stays 3.
 *
 * lbf_mlp_grad_sq: d_out[i] = scale * sum_b (d l_b / d w_i)^2 over the batch rows (gathered through d_idx as
 * everywhere), l_b row b's data loss at inv_scale = 1: 0.5 |a_b - y_b|^2 (LBF_LOSS_MSE) or sum_o y_bo (lse_b - z_bo)
 * (LBF_LOSS_SOFTMAX_XENT). Flat parameter layout, no l2 term, every entry >= 0: the diagonal of the empirical Fisher
 * matrix. No per-example gradient is stored: per layer one MFMA product of the squared operands over row chunks of
 * the batch, the chunks' slabs summed in a fixed order (no atomics: two calls give equal bits). With a communicator
 * every rank sums its own rows and the scaled vectors are all-reduced; batch == 0 is an empty share. It overwrites
 * the network's activation workspace like lbf_mlp_forward. LBF_ERR_INVALID: null handles, batch < 0, scale negative
 * or non-finite. Synchronises. */
int lbf_mlp_grad_sq(lbf_mlp *net, const float *d_params, const float *d_X, const float *d_Y, const int *d_idx,
                    long long batch, double scale, float *d_out);
/* lbf_mlp_gn_pcg: lbf_mlp_gn_cg preconditioned with a diagonal. d_minv: parameter count floats, the INVERSE of the
 * preconditioner's diagonal, every entry > 0 (not validated), 4-byte aligned. With z = minv .* r:
 *   alpha = r.z / p.Ap;  x += alpha p;  r -= alpha Ap;  beta = r'.z' / r.z;  p = z' + beta p   (p_0 = z_0).
 * z is never stored (the sweeps re-form it in registers): an iteration costs two more reads of the parameter count
 * and no further launch. The stopping test stays rr <= rtol^2 rr0 on the recurrence residual, and rr0, rr, xb, xr,
 * xx mean what they mean for lbf_mlp_gn_cg. Status 2 also covers a non-finite or non-positive r.z. With d_minv all
 * ones the result (x, the residual and info) is bitwise lbf_mlp_gn_cg's. */
int lbf_mlp_gn_pcg(lbf_mlp *net, const float *d_params, const float *d_b, const float *d_minv, const float *d_X,
                   const float *d_Y, const int *d_idx, long long batch, double inv_scale, const lbf_cg_params *prm,
                   float *d_x, lbf_cg_info *info);
/* lbf_hf_solve_pc: lbf_hf_solve with a preconditioned step 2. pc NULL or mode LBF_PRECOND_NONE: lbf_hf_solve, bit
 * for bit. Mode LBF_PRECOND_GRAD_SQ: step 2 becomes preconditioned CG (lbf_mlp_gn_pcg) on
 * (G + (l2 + lambda_k) I) p = -g with
 *   M_i = (cinv D_i + l2 + lambda_k)^exponent,   d_minv = 1 / M,
 * D = lbf_mlp_grad_sq on that iteration's curvature rows (the curv_rows window, or all local rows; all-reduced over
 * a communicator, so every rank holds the same M) and cinv the 1 / rows the CG uses, so M has the units of
 * G + (l2 + lambda) I. D is recomputed when k % refresh == 0; M every iteration, because lambda_k moves. l2 +
 * lambda_k must be > 0 (a parameter no row reaches has D_i = 0). Steps 1 and 3 to 6 are unchanged: they use x.b, x.r
 * and x.x only. exponent == 0 gives M = 1 and the bits of lbf_hf_solve. LBF_ERR_INVALID: as lbf_hf_solve, an unknown
 * mode, exponent outside [0, 1], refresh < 1. */
#define LBF_PRECOND_NONE 0
#define LBF_PRECOND_GRAD_SQ 1
typedef struct lbf_hf_precond {
  int mode;        /* LBF_PRECOND_NONE */
  double exponent; /* 0.75 */
  int refresh;     /* 1: outer iterations between two evaluations of D */
} lbf_hf_precond;
void lbf_hf_precond_default(lbf_hf_precond *p);
int lbf_hf_solve_pc(lbf_mlp *net, const lbf_hf_params *prm, const lbf_hf_precond *pc, float *d_params,
                    const float *d_X, const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                    lbf_solve_info *info);

/* ---- OWL-QN: L1-regularised L-BFGS (extension; Andrew & Gao 2007, libLBFGS's orthantwise_c). New functions and
 * structs only: LBF_ABI_VERSION stays 3.
 *
 * Minimises F(w) = f(w) + sum_i c_i |w_i| with f the objective of lbf_gd_solve (the network's loss, a mean over
 * n_global, + 0.5 l2 |w|^2 with the network's l2; n_local rows on this rank). c_i = l1 on every weight; on the
 * biases c_i = 0, or l1 when l1_bias != 0. Iteration k from (x, f, g):
 *   1. pseudo-gradient pg_i = g_i + c_i (x_i > 0), g_i - c_i (x_i < 0); at x_i == 0: g_i - c_i if that is > 0,
 *      else g_i + c_i if that is < 0, else +0 (each one fp32 add with c_i = (float)l1). Stop when ||pg|| < tol;
 *   2. d = -H pg by the two-loop recursion over the stored pairs (gamma = s.y / y.y of the newest, d = -pg without
 *      pairs); then d_i = 0 wherever d_i pg_i >= 0 (tested on the signs);
 *   3. orthant xi_i = sign(x_i), or sign(-pg_i) where x_i == 0 (xi_i = 0: the coordinate stays zero);
 *   4. backtracking from alpha = 1 (min(1, 1/||pg||) at k = 0), alpha *= rho after a failure, at most
 *      max_line_iters trials. Trial point: t = fmaf(alpha, d_i, x_i), x+_i = t where t != 0 has the sign xi_i, else
 *      +0. Accepted when F(x+) <= F(x) + c1 sum_i pg_i (x+_i - x_i), F(x+) from a loss-only evaluation. If every
 *      trial fails the point stays, the row records accepted = 0 and alpha = 0, and the solve ends there: a further
 *      iteration would repeat this one;
 *   5. on acceptance the gradient g+ comes from the backward pass of the accepted trial's forward state;
 *      s = x+ - x, y = g+ - g (the smooth gradients, never pg) enter the ring of m pairs when y.s > 1e-10;
 *   6. lbf_record row: F and ||pg|| at the iteration's start point, alpha, ls_trials, accepted.
 * The sign test of step 2 and the projection of steps 3 and 4 apply to the penalised coordinates: every weight,
 * whatever l1 is, and the biases when l1_bias != 0. Such a coordinate changes sign only through an iteration at
 * zero. So l1 = 0 is legal but still orthant-wise; it is not lbf_lbfgs_solve. The other coordinates (the biases
 * when l1_bias == 0) are free: pg_i = g_i, x+_i = fmaf(alpha, d_i, x_i), and no step sets them to zero.
 * info: final_loss = F and final_grad_norm = ||pg|| at the end; n_evals the gradient evaluations (the start point
 * and the accepted trials), n_loss_only the trials, n_grad_after_loss the accepted ones. stats (nullable): of the
 * final point, over the penalised coordinates. zeros_trace (nullable, trace_cap entries): the penalised coordinates
 * that are exactly zero after each iteration. With a communicator every rank evaluates its rows, and runs the same
 * vector arithmetic on the all-reduced loss and gradient: identical decisions, no further collective.
 * LBF_ERR_INVALID: null handles, l1 < 0 or non-finite, m outside 0..128, max_iters < 0, rho outside (0, 1),
 * max_line_iters < 1. */
typedef struct lbf_owlqn_params {
  int m, max_iters; double tol;            /* 10, 100, 1e-6 */
  double l1; int l1_bias;                  /* 0, 0 */
  double c1, rho; int max_line_iters;      /* 1e-4, 0.5, 20 */
  long long *zeros_trace; int trace_cap;   /* nullable: zero weights after each iteration */
} lbf_owlqn_params;
typedef struct lbf_owlqn_stats { long long zeros, penalised; double l1_term, pg_norm; } lbf_owlqn_stats;
void lbf_owlqn_default_params(lbf_owlqn_params *p);
int  lbf_owlqn_solve(lbf_mlp *net, const lbf_owlqn_params *prm, float *d_params, const float *d_X,
                     const float *d_Y, long long n_local, long long n_global, lbf_record *rec,
                     lbf_solve_info *info, lbf_owlqn_stats *stats /* nullable */);
/* The two sweeps on their own, for callers with their own objective: each is one launch over the parameters and a
 * one-workgroup finisher, every sum an fp64 sum in a fixed order (bitwise reproducible). All vectors hold the
 * network's parameter count, 4-byte aligned, and must not overlap.
 * lbf_mlp_l1_pseudo_grad: d_pg = step 1's pseudo-gradient at d_x with smooth gradient d_g; h_stats (nullable):
 *   zeros, penalised, l1_term = l1 sum |x_i| over the penalised, pg_norm.
 * lbf_mlp_l1_trial: d_xnew = step 4's trial point from the raw direction d_d (step 2's sign test is applied
 *   inside); h_l1_term, h_ww = xnew.xnew, h_dec = pg.(xnew - x), h_zeros (each nullable). */
int  lbf_mlp_l1_pseudo_grad(lbf_mlp *net, const float *d_x, const float *d_g, double l1, int l1_bias,
                            float *d_pg, lbf_owlqn_stats *h_stats);
int  lbf_mlp_l1_trial(lbf_mlp *net, const float *d_x, const float *d_d, const float *d_pg, double l1,
                      int l1_bias, float alpha, float *d_xnew, double *h_l1_term, double *h_ww,
                      double *h_dec /* pg.(xnew - x) */, long long *h_zeros);

/* ---- Adam / AdamW over shuffled minibatches (extension; Kingma & Ba 2015, Loshchilov & Hutter 2019). New
 * functions and structs only: LBF_ABI_VERSION stays 3.
 *
 * Minimises the objective of lbf_sgd_solve (the network's loss + 0.5 l2 |w|^2 with the network's l2, a mean over each
 * batch). d_X / d_Y hold all N rows on every rank, as for lbf_slbfgs_solve. Epoch e = 0, 1, ..:
 *   1. lr_e = lr, times decay_rate at every epoch e > 0 with e % decay_step == 0 (decay_step > 0), in fp64;
 *   2. the epoch's order: the identity (shuffle == 0), else lbf_adam_epoch_orders' permutation e, all epochs drawn
 *      from one mt19937(seed); batch k holds the positions [k batch, min((k + 1) batch, N)) of the order;
 *   3. per batch, step t = 1, 2, .. counted over the whole solve: one fused evaluation of the batch (inv_scale =
 *      1 / rows, the network's l2 inside the gradient), then one launch over the parameters with the nine fp32
 *      coefficients of lbf_adam_coefs(prm, lr_e, t):
 *        c   = 1, or clip_norm / ||g|| where ||g|| = sqrtf((float)(g.g)) > clip_norm   (clip_norm > 0)
 *        gi  = g_i c;   m_i = b1 m_i + a1 gi;   v_i = b2 v_i + a2 (gi gi)
 *        w_i = w_i decay - step (m_i / (sqrtf(v_i) rbc2 + eps))
 *      every operation rounded once to fp32, m = v = 0 at the start. This is Adam with bias correction; decay =
 *      1 - lr_e weight_decay is AdamW's decoupled decay, while the network's l2 is the coupled one. g.g is read on
 *      the device from the evaluation's status block: no host synchronisation inside an epoch;
 *   4. the epoch loss is sum_k (batch objective k) rows_k / N in fp64; when tol > 0 and a previous epoch exists the
 *      solve stops once |prev - loss| / max(1, |prev|) < tol (lbf_sgd_solve's test; that epoch gets no record row);
 *   5. with rec: one full-batch row (loss and gradient norm through float, like lbf_sgd_solve) for the start point
 *      and one per epoch, alpha = lr_e.
 * loss_trace (nullable, trace_cap entries): the batch objective of step t at [t - 1], evaluated before the step.
 * info: iterations = the rows recorded (epochs, + 1 with rec), as lbf_sgd_solve counts; final_loss / final_grad_norm
 * of the last full-batch row, or the last epoch loss and 0 without rec.
 * With a communicator every rank takes positions [rows r / p, rows (r + 1) / p) of every batch (the split of
 * LBF_SLBFGS_DP_SLICED; an empty slice is legal), the evaluation's all-reduce is the only collective of a step, and
 * m, v and t are replicated: all ranks hold the same bits. The full-batch rows are sharded the same way.
 * Non-finite gradients are outside the contract, as for lbf_sgd_solve.
 * LBF_ERR_INVALID: null handles, batch < 1, lr <= 0, eps <= 0, beta1 or beta2 outside [0, 1), weight_decay or
 * clip_norm negative or non-finite, decay_step < 0, max_epochs < 0, trace_cap < 0, N < 1 or N >= 2^31. */
typedef struct lbf_adam_params {
  double lr;               /* 1e-3  */
  double beta1, beta2;     /* 0.9, 0.999 */
  double eps;              /* 1e-8  */
  double weight_decay;     /* 0: Adam; > 0: AdamW */
  double clip_norm;        /* 0: off */
  int batch;               /* 128   */
  int shuffle;             /* 1     */
  unsigned seed;           /* 123   */
  double decay_rate;       /* 1.0, as lbf_sgd_params */
  int decay_step;          /* 0: no decay */
  int max_epochs;          /* 200   */
  double tol;              /* 1e-6  */
  double *loss_trace;      /* nullable */
  int trace_cap;
} lbf_adam_params;
/* The step's coefficients, fp64 expressions rounded once to float (prm's fields in capitals):
 *   b1 = BETA1, a1 = 1 - BETA1, b2 = BETA2, a2 = 1 - BETA2, step = lr_now / (1 - BETA1^t),
 *   rbc2 = 1 / sqrt(1 - BETA2^t), eps = EPS, decay = 1 - lr_now WEIGHT_DECAY, clip = CLIP_NORM,
 * with BETA^t the running product p_0 = 1, p_k = p_{k-1} BETA (t multiplications, no pow). */
typedef struct lbf_adam_coef {
  float b1, a1, b2, a2, step, rbc2, eps, decay, clip;
} lbf_adam_coef;
void lbf_adam_default_params(lbf_adam_params *p);
/* Host only. LBF_ERR_INVALID: null pointers, t < 1, lr_now <= 0 or non-finite, or parameters lbf_adam_solve rejects. */
int lbf_adam_coefs(const lbf_adam_params *prm, double lr_now, long long t, lbf_adam_coef *h_out);
/* Host only: h_out[e N + i], e < epochs, the orders of epochs 0 .. epochs - 1 as the solver draws them: each starts
 * from the identity and runs Fisher-Yates downward, for i = N - 1 .. 1: j = ((uint64)rng() (i + 1)) >> 32, swap
 * positions i and j, rng one std::mt19937(seed) for all epochs, its raw 32-bit draws (no distribution object, so
 * the orders do not depend on the standard library). j is uniform up to a bias of at most N / 2^32. */
int lbf_adam_epoch_orders(long long N, unsigned seed, int epochs, int *h_out);
/* The step of item 3 on device vectors of the caller's own (n floats each, 4-byte aligned, distinct). d_gg
 * (nullable): a device double holding g.g; null or coef->clip == 0: no clipping. Asynchronous. */
int lbf_adam_step(lbf_ctx *ctx, long long n, const lbf_adam_coef *coef, float *d_w, float *d_m, float *d_v,
                  const float *d_g, const double *d_gg);
int lbf_adam_solve(lbf_mlp *net, const lbf_adam_params *prm, float *d_params, const float *d_X, const float *d_Y,
                   long long N, lbf_record *rec, lbf_solve_info *info);
/* Stateful form: begin allocates m = v = 0 and records nothing yet; iterate runs up to `epochs` more epochs (fewer
 * when the tol test stops the solve) with d_params updated in place; end releases the solver. begin +
 * iterate(max_epochs) + end is lbf_adam_solve, and any chunking of the epochs gives the same bits. rec: pass a
 * record to every iterate call or to none. h_epochs (nullable): the epochs completed so far. */
typedef struct lbf_adam lbf_adam;
int lbf_adam_begin(lbf_mlp *net, const lbf_adam_params *prm, float *d_params, const float *d_X, const float *d_Y,
                   long long N, lbf_adam **out);
int lbf_adam_iterate(lbf_adam *s, int epochs, lbf_record *rec, lbf_solve_info *info, int *h_epochs);
int lbf_adam_end(lbf_adam *s);

int lbf_slbfgs_solve(lbf_mlp *net, const lbf_slbfgs_params *prm, float *d_params, const float *d_X,
                     const float *d_Y, long long N, lbf_record *rec, lbf_solve_info *info);
/* Stateful S-LBFGS (benchmarking, and callers that check progress between epochs): begin copies nothing
 * yet; iterate runs up to `epochs` more epochs (returns early on convergence) with d_params updated after
 * each call; end releases the solver. One begin + iterate(max_epochs) is lbf_slbfgs_solve. */
typedef struct lbf_slbfgs lbf_slbfgs;
int lbf_slbfgs_begin(lbf_mlp *net, const lbf_slbfgs_params *prm, float *d_params, const float *d_X,
                     const float *d_Y, long long N, lbf_slbfgs **out);
int lbf_slbfgs_iterate(lbf_slbfgs *s, int epochs, lbf_record *rec, lbf_solve_info *info);
int lbf_slbfgs_end(lbf_slbfgs *s);
/* Diagnostics (pair_trace on): the first traced curvature-pair candidate's iterate w_t after inner step t,
 * the iterate average u, s = u - u_prev and the y stored for it (s_lbfgs.hpp:236-256), n floats each into
 * device buffers (any may be NULL). LBF_ERR_INVALID until a candidate has been traced. */
int lbf_slbfgs_pair0(lbf_slbfgs *s, float *d_wt, float *d_u, float *d_s, float *d_y);
/* Diagnostics, teacher forcing of the curvature pairs (set before the first iterate; a new function, so no struct
 * of ABI 3 changes). A curvature event is every inner step t > 0 with t % L == 0 (s_lbfgs.hpp:236-261), the
 * first, which only pushes u, included; with ld = (n + 3) & ~3, event e (counted over epochs, e < cap):
 *   d_rec   (nullable) receives [w_{t+1} | u | g(u + eps s) | g(u - eps s)] at d_rec + 4 e ld (ld floats each;
 *           the two gradients of the batch loss + lambda w, zero at the first event; with hvp_exact the second
 *           is zero and the first is H(u) s + lambda s; in mode LBF_HVP_GAUSS_NEWTON the record holds
 *           G(u) s + lambda s (lbf_mlp_gnvp on the Hessian batch), then zeros);
 *   d_force (nullable, same layout, e.g. another run's d_rec) replaces u before s = u - u_prev and the two
 *           gradients before y = (g+ - g-) / (2 eps) is stored, so the ring receives the other run's pairs
 *           while the iterates w_t stay this run's own. Two routes forced with one run's record then compare
 *           non-chaotically: the gradients at the same points, and the iterates under the same history. */
int lbf_slbfgs_pair_io(lbf_slbfgs *s, int cap, float *d_rec, const float *d_force);

/* ---- profiling: HIP-event timing of every kernel class on the context stream (benchmark use).
 * Section id = kind*16 + layer; kinds: 0 fwd GEMM, 1 dW GEMM, 2 dX GEMM, 3 loss, 4 split-K reduce,
 * 5 finalize, 6 Gram sweep, 7 coefficients, 8 combine sweep, 9 line-search axpy, 10 all-reduce.
 * (The reference times whole iterations only: lbfgs.cuh:80-87, 176-182.) */
int lbf_prof_enable(lbf_ctx *ctx, int on);
/* Restrict timing to one section id (-1: all). Two events per launch of that section only, so the
 * timed region of a benchmark is not serialised by event packets around every kernel. */
int lbf_prof_select(lbf_ctx *ctx, int section_id);
/* Time only every `every`-th launch of the selected sections (1 = all): live timing inside a timed
 * region at 1/every of the event cost (an event record idles the GPU for ~5 us). */
int lbf_prof_sample(lbf_ctx *ctx, int every);
int lbf_prof_read(lbf_ctx *ctx, int cap, int *ids, double *ms, long long *counts, int *n_out);
/* ABI 2: the work units of the timed launches per section, same order as lbf_prof_read (GEMM sections: the
 * batch rows of every timed launch, so a sampled section's flops are 2 * In * Out * work). */
int lbf_prof_read_work(lbf_ctx *ctx, int cap, int *ids, double *work, int *n_out);

/* ---- Curvature spectrum: device-side Lanczos on the Hessian or the Gauss-Newton matrix (extension; Lanczos 1950,
 * Golub & Meurant's quadrature). New functions and structs only: LBF_ABI_VERSION stays 3.
 *
 * lbf_mlp_lanczos runs prm->steps steps of the Lanczos iteration on A = H(params) + l2 I (matrix LBF_HVP_EXACT,
 * the product of lbf_mlp_hvp) or A = G(params) + l2 I (LBF_HVP_GAUSS_NEWTON, lbf_mlp_gnvp) on the given batch (same
 * d_idx / batch / inv_scale meaning, shards summed over a communicator, batch == 0 an empty share), from
 * q_0 = d_v0 float(1 / |d_v0|). Vectors are fp32; every scalar is an fp64 sum of fixed-order partials formed on the
 * device (the rules of lbf_mlp_gn_cg: no float atomics, two calls give equal bits). Step j = 0 .. steps - 1:
 *   w = A q_j                       (Gauss-Newton: one forward pass serves the whole run)
 *   per pass: c_i = q_i.w for the rows i of R_j, then w -= sum_i float(c_i) q_i
 *             reorth 1: R_j = {0..j}, two passes;  reorth 0: R_j = {max(0, j-1)..j}, one pass
 *   alpha_j = the sum over the passes of c_j;   beta_j = |w|
 *   beta_j <= breakdown_rtol max(|alpha_0..j|, beta_0..j-1): the Krylov space is exhausted, status 1,
 *             info->steps = j + 1, no q_{j+1};
 *   alpha_j or beta_j non-finite: status 2, info->steps = j;   else q_{j+1} = w float(1 / beta_j).
 * Status 0: all steps ran. A zero or non-finite |d_v0| gives status 2 with 0 steps. The host enqueues `check` steps,
 * then reads the status block; steps enqueued past a stop are no-ops, so the result does not depend on `check`.
 * h_alpha, h_beta: prm->steps doubles each, zeros from info->steps on; T = tridiag(beta; alpha; beta) of order
 * info->steps is A restricted to the Krylov space of q_0 (h_beta[info->steps - 1] is the residual norm, not an entry
 * of T). d_basis (nullable): rows q_0 .. q_steps at stride ld >= parameter count floats; with reorth 1 the run works
 * in it, with reorth 0 it is written and never read. Without it reorth 1 keeps steps + 1 vectors in a workspace of
 * the network, reorth 0 three. All device pointers 4-byte aligned; besides the inputs the bits depend only on the
 * offsets from a 16-byte boundary of d_v0 and of the basis rows a step reads (so with a d_basis on ld % 4: a step
 * runs on float4 when its rows and the product share one offset, else scalar). With a communicator every rank passes the same d_v0 and
 * all ranks end with the same bits. LBF_ERR_INVALID: null handles, steps outside 1..128, matrix LBF_HVP_FD or
 * unknown, reorth outside {0, 1}, check < 1, a negative or non-finite l2 or breakdown_rtol, ld < parameter count
 * with a basis. Synchronises.
 *
 * lbf_tridiag_eig (host only): the eigenvalues of T = tridiag(beta[0..m-2]; alpha[0..m-1]; beta[0..m-2]) by implicit
 * QL in fp64, ascending into theta[m]; first_sq (nullable, m): the squared first components of the normalised
 * eigenvectors, the weights of the Gauss quadrature of q_0's spectral measure (they sum to 1); vecs (nullable,
 * m * m): vecs[i * m + k] is component i of theta[k]'s eigenvector. A zero beta and m == 1 are legal.
 * LBF_ERR_INVALID: m < 1, a null alpha / theta (beta with m > 1), no convergence (a non-finite entry). */
typedef struct lbf_lanczos_params {
  int steps;  /* 32 */
  int matrix; /* LBF_HVP_GAUSS_NEWTON */
  int reorth; /* 1 */
  int check;  /* 8: steps enqueued between two reads of the status block */
  double l2;  /* 0 */
  double breakdown_rtol; /* 1.1e-3: the geometric mean of the largest noise-level and the smallest healthy
                            beta_j / max(|alpha|, beta) measured on the MI355X */
} lbf_lanczos_params;
typedef struct lbf_lanczos_info {
  int steps, status;
  double v0_norm;
} lbf_lanczos_info;
void lbf_lanczos_default_params(lbf_lanczos_params *p);
int lbf_mlp_lanczos(lbf_mlp *net, const float *d_params, const float *d_v0, const float *d_X, const float *d_Y,
                    const int *d_idx, long long batch, double inv_scale, const lbf_lanczos_params *prm,
                    double *h_alpha, double *h_beta, float *d_basis, long long ld, lbf_lanczos_info *info);
int lbf_tridiag_eig(int m, const double *alpha, const double *beta, double *theta, double *first_sq, double *vecs);

/* ---- device memory, so C/C++ consumers need no HIP headers (the reference's DeviceBuffer,
 * src/cuda/device_buffer.cuh:7-96). kind: 0 host->device, 1 device->host, 2 device->device;
 * lbf_memcpy is ordered on the context stream and returns when the copy is complete. */
int lbf_device_alloc(lbf_ctx *ctx, size_t bytes, void **out);
int lbf_device_free(lbf_ctx *ctx, void *p);
int lbf_memcpy(lbf_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);

/* ---- host helpers (not on the timed path) ------------------------------------------------------
 * Synthetic MNIST-shaped data (SURVEY.md §8(d) recipe), row-major [N][In] / [N][classes]. */
int lbf_synth_mnist(long long N, int In, int classes, unsigned seed, float *h_X, float *h_Y);
/* Partial Fisher-Yates minibatch draws from one mt19937(seed) (s_lbfgs.hpp:141-160). */
int lbf_sample_indices(long long N, int b, unsigned seed, int calls, long long *h_out);
/* IDX datasets (MNIST / Fashion-MNIST files) == the reference's MNISTLoader (tests/mnist/mnist_loader.hpp:
 * 8-100): images (magic 2051) scaled by 1/255 into row-major [N][rows*cols] fp32, labels (magic 2049)
 * one-hot into [N][classes] (labels >= classes stay all-zero); max_* > 0 caps the count. Call with a
 * NULL output first to read the header (count, rows, cols), then with a buffer of that size. */
int lbf_idx_read_images(const char *path, long long max_images, float *h_out, long long *count, int *rows,
                        int *cols);
int lbf_idx_read_labels(const char *path, long long max_labels, int classes, float *h_onehot, long long *count);
/* BASELINE config 5's synthetic regression data, generated on the device (no reference counterpart:
 * the reference reads MNIST files): X ~ N(0,1) [N][In], y = tanh(v.x / 64) + 0.01 e [N][1]; stream
 * defined in lbfgs-ffnn_amd/csrc/synth.hip, restated in oracle/oracle.py. Writes rows [row0, row0+N)
 * of the stream (a data-parallel shard). Synchronises. */
int lbf_synth_regression(lbf_ctx *ctx, long long row0, long long N, int In, unsigned seed_x, unsigned seed_t,
                         float *d_X, float *d_Y);

#ifdef __cplusplus
}
#endif

#endif /* LBFGS_AMD_H */
