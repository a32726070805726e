/*
 * tdmpc_drnn_learner.h -- C ABI of the DSSM learner's two differentiable parts in libtdmpc_hip.so:
 *
 *   * DSSM.next in train mode (tdmpc_amd/dssm.py; the reference's tdmpc_similarity_drnn.py:57-60 under model.train()):
 *     the NormGRUCell (three row LayerNorms, eps 1e-3), prior_mlp with its BatchNorm1d on BATCH statistics (eps 1e-5,
 *     running statistics moved with momentum 0.1) and the reward MLP on the new hidden state -- forward and backward;
 *   * similarity_loss(queries, keys) of both reference DSSM agents: _predictor (Linear, train-mode BatchNorm, ELU,
 *     Linear) on the queries, F.normalize on both sides, 2 - 2 cos per row -- forward and backward (keys detached).
 *
 * Conventions as in tdmpc_learner.h: every pointer a device pointer to contiguous float32, everything enqueued on
 * `stream`, no allocation, no sync, graph-capturable; 0 or a negative TDMPC_E_* code with a tdmpc_last_error message.
 * The large products run as grouped tdmpc_lg_gemm launches on the exact f32 MFMA; every reduction runs in a fixed
 * order (no float atomics), so two runs and a graph replay give the same bits.
 *
 * The weights are the model's own fp32 parameter tensors, read in place (they change with every optimiser step), as
 * pointer tables in state_dict order:
 *   next (TDMPC_DT_NEXT_TENSORS = 22):
 *      0.. 7  _dynamics.prior_mlp.{0.weight [M,Hd], 0.bias, 1.weight, 1.bias, 1.running_mean, 1.running_var,
 *                                  3.weight [L,M], 3.bias}
 *      8..15  _dynamics.gru_cell.{weight_ih.weight [3Hd,L+A], weight_hh.weight [3Hd,Hd], ln_reset.{weight, bias},
 *                                 ln_update.{weight, bias}, ln_newval.{weight, bias}}
 *     16..21  _reward.{0.weight [M,Hd], 0.bias, 2.weight [M,M], 2.bias, 4.weight [1,M], 4.bias}
 *   similarity loss (TDMPC_DT_LOSS_TENSORS = 8):
 *      0.. 7  _predictor.{0.weight [M,L], 0.bias, 1.weight, 1.bias, 1.running_mean, 1.running_var, 3.weight [L,M],
 *                         3.bias}
 * A gradient table has the same length and order; its running_mean / running_var slots are ignored (may be null).
 *
 * Admitted shapes (the planner's, tdmpc_drnn.h): state observations, mlp_dim M = 512, hidden_dim a multiple of 32 up
 * to 256, 1 <= latent_dim <= 256, action_dim >= 1; 2 <= rows <= 4096 (one row has no batch variance; nn.BatchNorm1d
 * refuses it too). Anything else, a null required pointer included, returns TDMPC_E_DIMS with a message before any
 * HIP call and without writing an output.
 */
#ifndef TDMPC_DRNN_LEARNER_H
#define TDMPC_DRNN_LEARNER_H

#include "tdmpc_drnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC_DRNN_TRAIN_VERSION 1
#define TDMPC_DT_NEXT_TENSORS 22
#define TDMPC_DT_LOSS_TENSORS 8
#define TDMPC_DT_MAX_ROWS 4096

/* Returns TDMPC_DRNN_TRAIN_VERSION. */
int tdmpc_drnn_train_version(void);

/* Float counts for `rows` rows (monotone in rows): the saved-activation buffer of one tdmpc_drnn_next_fwd, of one
 * tdmpc_drnn_simloss_fwd, and the workspace (scratch; shared by all four passes, nothing lives in it between calls). */
typedef struct tdmpc_drnn_train_sizes {
    size_t next_saved_floats, loss_saved_floats, workspace_floats;
} tdmpc_drnn_train_sizes;
int tdmpc_drnn_train_sizes_for(const tdmpc_drnn_dims* dims, int32_t rows, tdmpc_drnn_train_sizes* out);

/* DSSM.next, train mode: z [R,L], a [R,A], h [R,Hd] -> z_out [R,L], h_out [R,Hd], r_out [R]. tensors[4] / [5]
 * (prior_mlp.1.running_mean / running_var) are updated in place: (1 - 0.1) old + 0.1 (batch mean / batch variance
 * times R / (R - 1)). `saved` (next_saved_floats) receives, in this order:
 *   gh     [R,3Hd]  weight_hh(h): the reset / update / newval pre-activations' hidden halves (newval_h = gh[:, 2Hd:])
 *   gate   [R,3Hd]  reset, update, newval (after sigmoid / sigmoid / tanh)
 *   lnx    [R,3Hd]  the three LayerNorms' xhat
 *   lnr    [R,4]    their 1/std per row (fourth column unused)
 *   hn     [R,Hd]   h'
 *   bnx    [R,M]    prior_mlp.1's xhat          bnr [M]  its columns' 1/std
 *   e      [R,M]    prior_mlp.2's ELU output
 *   q1, q2 [R,M]    _reward.1's and _reward.3's ELU outputs */
int tdmpc_drnn_next_fwd(const tdmpc_drnn_dims* dims, float* const* tensors, int32_t n_tensors, const float* z,
                        const float* a, const float* h, int32_t rows, float* z_out, float* h_out, float* r_out,
                        float* saved, size_t saved_floats, float* workspace, size_t workspace_floats, void* stream);

/* Backward of tdmpc_drnn_next_fwd over its `saved` buffer and its inputs z, a, h. dz_out [R,L], dh_out [R,Hd],
 * dr_out [R]: upstream gradients, each may be null (zero). dz [R,L], da [R,A], dh [R,Hd]: input gradients, each may be
 * null (not wanted). grads [22]: one buffer per parameter tensor, overwritten (not accumulated); all 20 required. */
int tdmpc_drnn_next_bwd(const tdmpc_drnn_dims* dims, float* const* tensors, int32_t n_tensors, const float* z,
                        const float* a, const float* h, int32_t rows, const float* saved, size_t saved_floats,
                        const float* dz_out, const float* dh_out, const float* dr_out, float* dz, float* da, float* dh,
                        float* const* grads, float* workspace, size_t workspace_floats, void* stream);

/* similarity_loss: queries [R,L], keys [R,L] -> loss [R] = 2 - 2 <normalize(predictor(queries)), normalize(keys)>,
 * normalize(x) = x / max(||x||, 1e-12). tensors[4] / [5] (_predictor.1's running statistics) are updated in place.
 * `saved` (loss_saved_floats): bnx [R,M], bnr [M], e [R,M], pred [R,L]. */
int tdmpc_drnn_simloss_fwd(const tdmpc_drnn_dims* dims, float* const* tensors, int32_t n_tensors,
                           const float* queries, const float* keys, int32_t rows, float* loss, float* saved,
                           size_t saved_floats, float* workspace, size_t workspace_floats, void* stream);

/* Backward: dloss [R] (required) -> dqueries [R,L] (may be null) and grads [8] (the six parameter gradients,
 * overwritten). The keys get no gradient (the reference detaches them). */
int tdmpc_drnn_simloss_bwd(const tdmpc_drnn_dims* dims, float* const* tensors, int32_t n_tensors,
                           const float* queries, const float* keys, int32_t rows, const float* saved,
                           size_t saved_floats, const float* dloss, float* dqueries, float* const* grads,
                           float* workspace, size_t workspace_floats, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The DSSM update's own parts (TdICemSimDssm.update, tdmpc_icem_similarity_drnn.py:421-553).
 * ------------------------------------------------------------------------------------------------------------- */

/* Workspace floats of one tdmpc_drnn_intrinsic_fwd over `segments` segments of `seg_rows` rows. */
int tdmpc_drnn_intrinsic_workspace_floats(const tdmpc_drnn_dims* dims, int32_t segments, int32_t seg_rows,
                                          size_t* out);

/* intrinsic_rewards' model uncertainty (:421-433) as one launch chain: `segments` independent one-step rollouts of
 * seg_rows rows each from a zero hidden state, rows s * seg_rows + b. z [S B, L], a [S B, A], keys [S B, L] ->
 * loss [S B] = similarity_loss(next(z, a, 0).z', keys), forward only. Both BatchNorms (prior_mlp.1, _predictor.1)
 * normalise PER SEGMENT, and their running statistics (next_tensors[4] / [5], loss_tensors[4] / [5]) move `segments`
 * times in segment order, so the result and the statistics are bitwise those of `segments` pairs of
 * tdmpc_drnn_next_fwd (h = zeros) + tdmpc_drnn_simloss_fwd calls on the segments in order. The reward head is not run.
 * Admitted: the shapes above, 1 <= segments, 2 <= seg_rows, segments * seg_rows <= TDMPC_DT_MAX_ROWS. */
int tdmpc_drnn_intrinsic_fwd(const tdmpc_drnn_dims* dims, float* const* next_tensors, int32_t n_next,
                             float* const* loss_tensors, int32_t n_loss, const float* z, const float* a,
                             const float* keys, int32_t segments, int32_t seg_rows, float* loss, float* workspace,
                             size_t workspace_floats, void* stream);

/* The rest of intrinsic_rewards (:435-443) without the host: mean and population variance of loss [n] (float64, fixed
 * order), gym's RunningMeanStd.update_from_moments(mean, var, 1) on the device state rms = double {mean, var, count}
 * (initially 0, 1, 1e-4), then intrinsic[i] = max(loss[i] / sqrt(var') - mean' / sqrt(var'), 0) and
 * reward_pi[i] = coef[0] * intrinsic[i] + reward[i]. coef: a device float (the explore schedule's value).
 * One workgroup; 1 <= n <= TDMPC_DT_MAX_ROWS. */
int tdmpc_drnn_intrinsic_finish(const float* loss, int32_t n, double* rms, const float* coef, const float* reward,
                                float* intrinsic, float* reward_pi, void* stream);

/* TdICemSimDssm.update's loss composition (:471-485, :497-499, :522-530). All [H][B] float32 but w [B]:
 *   td[t]     TD-lambda targets, backwards from last = nq[H-1]: td[t] = rwpi[t] + discount nq[t] (1 - td_lambda) +
 *             discount td_lambda td[t+1] (td[H] = nq[H-1])
 *   rows [6][B]: sum_t sim, sum_t (rp - rw)^2, sum_t (q1 - td)^2 + (q2 - td)^2, min(sum_t |q1 - td| + |q2 - td|, 1e4),
 *             model_loss = sim_coef min(sim, 1e4) + reward_coef min(rew, 1e4), td_loss = value_coef min(val, 1e4)
 *   scal [8]: the means of sim, rew, val, model_loss + td_loss; weighted = mean(model_loss) mean(w) + mean(td_loss)
 *             (the reference's mean over the [B, B] broadcast of model_loss [B, 1] * w [B]); mean(w); mean(model_loss);
 *             mean(td_loss). */
typedef struct tdmpc_drnn_loss_args {
    const float *sim, *q1, *q2, *rp, *rw, *rwpi, *nq, *w;
    int32_t H, B;
    float sim_coef, reward_coef, value_coef, discount, td_lambda;
} tdmpc_drnn_loss_args;
int tdmpc_drnn_loss_forward(const tdmpc_drnn_loss_args* a, float* td, float* rows, float* scal, void* stream);
/* gw [1] = dL / dweighted -> dsim, dq1, dq2, drp [H][B] (each may be null); the clamps pass gradient where the sum
 * is <= 1e4 (torch.clamp). */
int tdmpc_drnn_loss_backward(const tdmpc_drnn_loss_args* a, const float* td, const float* rows, const float* scal,
                             const float* gw, float* dsim, float* dq1, float* dq2, float* drp, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * TdMpcSimDssm.update's own parts (tdmpc_similarity_drnn.py:373-496).
 * ------------------------------------------------------------------------------------------------------------- */

/* Workspace floats of one tdmpc_drnn_intrinsic_chain_fwd over `segments` segments of `seg_rows` rows. */
int tdmpc_drnn_intrinsic_chain_workspace_floats(const tdmpc_drnn_dims* dims, int32_t segments, int32_t seg_rows,
                                                size_t* out);

/* TdMpcSimDssm.intrinsic_rewards' model uncertainty (:373-391, similarity_horizon 1): ONE hidden state runs through the
 * S = `segments` closed-loop steps, h_0 = 0, h_{s+1} = cell([z_s | a_s], h_s) over rows s * seg_rows + b of
 * z [S B, L], a [S B, A]. prior_mlp runs on every h_{s+1} (each segment normalises its BatchNorm over its own B rows
 * and moves next_tensors[4] / [5] once, in segment order: S times). Segments s >= warm go on through _predictor and
 * loss[s B + b] = 2 - 2 cos(pred, keys[s B + b]) (loss_tensors[4] / [5] move S - warm times); loss is zero in the
 * first `warm` segments. h_out [B, Hd] = h_S. Forward only; the reward head is not run.
 *   mode 0  the recurrence as a launch chain (per step h weight_hh^T and the gate kernel): loss, h_out and the running
 *           statistics are bitwise those of S tdmpc_drnn_next_fwd calls with the hidden state handed on (the first from
 *           zeros) and tdmpc_drnn_simloss_fwd on z' of the segments >= warm, in order;
 *   mode 1  the recurrence in one launch (a workgroup owns 16 batch rows through all S steps); the same math with the
 *           hidden product summed in another order.
 * The workspace begins with hn [S B, Hd], every segment's new hidden state. Admitted: the shapes of
 * tdmpc_drnn_intrinsic_fwd, 0 <= warm < segments. */
int tdmpc_drnn_intrinsic_chain_fwd(const tdmpc_drnn_dims* dims, float* const* next_tensors, int32_t n_next,
                                   float* const* loss_tensors, int32_t n_loss, const float* z, const float* a,
                                   const float* keys, int32_t segments, int32_t seg_rows, int32_t warm, int32_t mode,
                                   float* loss, float* h_out, float* workspace, size_t workspace_floats, void* stream);

/* TdMpcSimDssm.update's loss composition (:423, :447-471) over H steps of which the last N = H - W are shoot steps
 * (1 <= W <= H - 1). sim [H][B]; q1, q2, rp, rw, rwpi, nq [N][B] (shoot step t = W + i at row i); w [B].
 *   td [N][B]:   td = rwpi + discount nq (one step; rho ** shoot_count is 1 in the reference)
 *   rows [5][B]: sum_{t<H} sim, sum_i (rp - rw)^2, sum_i (q1 - td)^2 + (q2 - td)^2, min(sum_i |q1 - td| + |q2 - td|,
 *                1e4), total = sim_coef min(sim, 1e4) + reward_coef min(rew, 1e4) + value_coef min(val, 1e4)
 *   scal [6]:    the means of sim, rew, val, total; weighted = mean(total) mean(w) (the reference's mean over the
 *                [B, B] broadcast of total [B, 1] * w [B]); mean(w). */
typedef struct tdmpc_drnn_sim_loss_args {
    const float *sim, *q1, *q2, *rp, *rw, *rwpi, *nq, *w;
    int32_t H, W, B;
    float sim_coef, reward_coef, value_coef, discount;
} tdmpc_drnn_sim_loss_args;
int tdmpc_drnn_sim_loss_forward(const tdmpc_drnn_sim_loss_args* a, float* td, float* rows, float* scal, void* stream);
/* gw [1] = dL / dweighted -> dsim [H][B], dq1, dq2, drp [N][B] (each may be null) in one elementwise pass; the clamps
 * pass gradient where the sum is <= 1e4. */
int tdmpc_drnn_sim_loss_backward(const tdmpc_drnn_sim_loss_args* a, const float* td, const float* rows,
                                 const float* scal, const float* gw, float* dsim, float* dq1, float* dq2, float* drp,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_DRNN_LEARNER_H */
