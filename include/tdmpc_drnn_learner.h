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

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_DRNN_LEARNER_H */
