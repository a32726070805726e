/*
 * tdmpc_icem_learner.h -- C ABI of the MLP iCEM agent's update in libtdmpc_hip.so (TdICemSimMlp.update,
 * tdmpc_icem_similarity_mlp.py:313-428; tdmpc_amd/icem_learner.py drives it).
 *
 * The model is TOLD with the LayerNorm state encoder plus the `_predictor` similarity head (Linear, train-mode
 * BatchNorm1d, ELU, Linear: the module of tdmpc_drnn_learner.h's similarity loss). Its dynamics are a plain MLP without
 * a hidden state, so every entry point takes the planner's tdmpc_dims (tdmpc_hip.h); there is no hidden_dim to check.
 *
 * Conventions as in tdmpc_drnn_learner.h: every pointer a device pointer to contiguous float32, everything enqueued on
 * `stream`, no allocation, no sync, no float atomics, every reduction in a fixed order (two runs and a graph replay give
 * the same bits). The products are grouped tdmpc_lg_gemm launches on the exact f32 MFMA, reading the model's own
 * parameter tensors in place, as pointer tables in state_dict order:
 *   dynamics (TDMPC_ICEM_DYN_TENSORS = 6):   _dynamics.{0.weight [M,L+A], 0.bias, 2.weight [M,M], 2.bias,
 *                                                        4.weight [L,M], 4.bias}
 *   similarity loss (TDMPC_DT_LOSS_TENSORS = 8): _predictor.{0.weight [M,L], 0.bias, 1.weight, 1.bias, 1.running_mean,
 *                                                            1.running_var, 3.weight [L,M], 3.bias}
 *
 * Admitted shapes: state observations, mlp_dim M = 512, 1 <= latent_dim <= 256, action_dim >= 1,
 * 2 <= rows <= TDMPC_DT_MAX_ROWS (one row has no batch variance). Anything else, a null required pointer included,
 * returns TDMPC_E_DIMS with a tdmpc_last_error message before any HIP call and before any output is written.
 */
#ifndef TDMPC_ICEM_LEARNER_H
#define TDMPC_ICEM_LEARNER_H

#include "tdmpc_drnn_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC_ICEM_LEARNER_VERSION 1
#define TDMPC_ICEM_DYN_TENSORS 6

/* Returns TDMPC_ICEM_LEARNER_VERSION. */
int tdmpc_icem_learner_version(void);

/* Workspace floats of one tdmpc_icem_intrinsic_fwd over `segments` segments of `seg_rows` rows. */
int tdmpc_icem_intrinsic_workspace_floats(const tdmpc_dims* dims, int32_t segments, int32_t seg_rows, size_t* out);

/* intrinsic_rewards' model uncertainty (:323-335) as one launch chain: S = `segments` independent one-step rollouts of
 * seg_rows rows each, rows s * seg_rows + b. z [S B, L], a [S B, A], keys [S B, L] ->
 * loss [S B] = 2 - 2 cos(_predictor(_dynamics([z | a])), keys), forward only. `_dynamics` has no BatchNorm and runs
 * over all S B rows: three products, the first over the two K segments [z | a], ELU in the first two's epilogues.
 * `_predictor`'s BatchNorm normalises PER SEGMENT and its running statistics (loss_tensors[4] / [5]) move S times in
 * segment order. The GEMM tile is chosen as for seg_rows rows, so loss and the statistics are bitwise those of S
 * one-segment calls on the segments in order. The reward head is not run (the reference computes and drops it).
 * Admitted: the shapes above, 1 <= segments, 2 <= seg_rows, segments * seg_rows <= TDMPC_DT_MAX_ROWS. */
int tdmpc_icem_intrinsic_fwd(const tdmpc_dims* dims, float* const* dyn_tensors, int32_t n_dyn,
                             float* const* loss_tensors, int32_t n_loss, const float* z, const float* a,
                             const float* keys, int32_t segments, int32_t seg_rows, float* loss, float* workspace,
                             size_t workspace_floats, void* stream);

/* similarity_loss (:294-300): tdmpc_drnn_simloss_fwd / _bwd behind tdmpc_dims -- the same internals, tensor table,
 * saved-buffer layout and bits. Float counts for `rows` rows (monotone in rows). */
typedef struct tdmpc_icem_simloss_sizes {
    size_t loss_saved_floats, workspace_floats;
} tdmpc_icem_simloss_sizes;
int tdmpc_icem_simloss_sizes_for(const tdmpc_dims* dims, int32_t rows, tdmpc_icem_simloss_sizes* out);
int tdmpc_icem_simloss_fwd(const tdmpc_dims* dims, float* const* tensors, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, float* loss, float* saved, size_t saved_floats,
                           float* workspace, size_t workspace_floats, void* stream);
int tdmpc_icem_simloss_bwd(const tdmpc_dims* dims, float* const* tensors, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, const float* saved, size_t saved_floats,
                           const float* dloss, float* dqueries, float* const* grads, float* workspace,
                           size_t workspace_floats, void* stream);

/* TdICemSimMlp.update's loss composition (:384-411). All [H][B] float32 but w [B]; r_t = (float)(rho ** t), the power
 * taken in double as the reference's Python float `cfg.rho ** t` and rounded once, as a float32 tensor times that
 * scalar is.
 *   td [H][B]:   td[t] = rwpi[t] + discount nq[t] (one-step targets)
 *   rows [5][B]: sum_t sim, sum_t r_t (rp - rw)^2, sum_t r_t ((q1 - td)^2 + (q2 - td)^2),
 *                min(sum_t r_t (|q1 - td| + |q2 - td|), 1e4) (the priority),
 *                total = sim_coef min(sim, 1e4) + reward_coef min(rew, 1e4) + value_coef min(val, 1e4)
 *   scal [6]:    the means of sim, rew, val, total; weighted; mean(w).
 * weighted: the reference's `(total_loss * weights).mean()` multiplies total_loss [B, 1] by weights [B] (the buffer's
 * sample() returns them one-dimensional), a [B, B] broadcast whose mean is mean(total) mean(w) -- NOT the per-sample
 * importance weighting mean(total_b w_b). The recording (tests/golden/icem_update) confirms it: the float32 restatement
 * with the literal broadcast equals the reference run bit for bit. weighted = mean(total) mean(w) here. */
typedef struct tdmpc_icem_loss_args {
    const float *sim, *q1, *q2, *rp, *rw, *rwpi, *nq, *w;
    int32_t H, B;
    float sim_coef, reward_coef, value_coef, discount;
    double rho;
} tdmpc_icem_loss_args;
int tdmpc_icem_loss_forward(const tdmpc_icem_loss_args* a, float* td, float* rows, float* scal, void* stream);
/* gw [1] = dL / dweighted -> dsim, dq1, dq2, drp [H][B] (each may be null) in one elementwise pass. The reference's
 * `weighted_loss.register_hook(grad / horizon)` is part of it: every output carries the factor 1 / H. The clamps pass
 * gradient where the sum is <= 1e4 (torch.clamp). */
int tdmpc_icem_loss_backward(const tdmpc_icem_loss_args* a, const float* td, const float* rows, const float* scal,
                             const float* gw, float* dsim, float* dq1, float* dq2, float* drp, void* stream);

/* The rest of intrinsic_rewards (:336-344) is tdmpc_drnn_intrinsic_finish (tdmpc_drnn_learner.h), which takes no dims. */

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_ICEM_LEARNER_H */
