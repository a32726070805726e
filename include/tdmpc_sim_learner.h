/*
 * tdmpc_sim_learner.h -- C ABI of the similarity TD-MPC agent's update in libtdmpc_hip.so (TDMPCSIM.update,
 * tdmpc_similarity.py:298-375; tdmpc_amd/sim_engine.py drives it on the learner engine of tdmpc_learner.h; DESIGN.md
 * §7 f11).
 *
 * TDMPCSIM.update is TDMPC.update with the consistency term replaced by the similarity head: `_predictor` (Linear,
 * train-mode BatchNorm1d over all H B rollout rows, ELU, Linear) on the predicted latents, F.normalize on both sides,
 * 2 - 2 cos against the target encoder's latents. The engine runs the head's four products (two forward, two dX) and its
 * two dW products in its own grouped tdmpc_lg_gemm launches; this header exposes what lies between them -- the
 * BatchNorm and cosine passes of tdmpc_drnn_learner.h's similarity loss, the same kernels and bits -- and the update's
 * loss composition over the engine's buffers.
 *
 * Conventions as in tdmpc_icem_learner.h: every pointer a device pointer to contiguous float32, everything enqueued on
 * `stream`, no allocation, no sync, no float atomics, every reduction in a fixed order (two runs and a graph replay give
 * the same bits). An inadmissible shape or a null required pointer returns TDMPC_E_DIMS with a tdmpc_last_error message
 * before any HIP call and before any output is written.
 */
#ifndef TDMPC_SIM_LEARNER_H
#define TDMPC_SIM_LEARNER_H

#include "tdmpc_icem_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC_SIM_LEARNER_VERSION 1
#define TDMPC_SIM_BN_WIDTH 512   /* the BatchNorm's columns: `_predictor`'s hidden width, mlp_dim */

/* Returns TDMPC_SIM_LEARNER_VERSION. */
int tdmpc_sim_learner_version(void);

/* TDMPCSIM.update's loss composition (:336-352). All [H][B] float32 but w [B]; r_t = (float)(rho ** t), the power taken
 * in double as the reference's Python float `cfg.rho ** t` and rounded once. td is GIVEN (the engine's row kernel has
 * written reward + discount min(Q1', Q2')), which is all that differs from tdmpc_icem_loss_*:
 *   rows [5][B]: sum_t sim, sum_t r_t (rp - rw)^2, sum_t r_t ((q1 - td)^2 + (q2 - td)^2),
 *                min(sum_t r_t (|q1 - td| + |q2 - td|), 1e4) (the priority),
 *                total = sim_coef min(sim, 1e4) + reward_coef min(rew, 1e4) + value_coef min(val, 1e4)
 *   scal [6]:    the means of sim, rew, val, total; weighted = mean(total) mean(w) (the reference's [B, 1] * [B]
 *                broadcast, see tdmpc_icem_learner.h; tests/golden/sim_update confirms it for this agent); mean(w). */
typedef struct tdmpc_sim_loss_args {
    const float *sim, *q1, *q2, *rp, *rw, *td, *w;
    int32_t H, B;
    float sim_coef, reward_coef, value_coef;
    double rho;
} tdmpc_sim_loss_args;
int tdmpc_sim_loss_forward(const tdmpc_sim_loss_args* a, float* rows, float* scal, void* stream);
/* gw [1] = dL / dweighted -> dsim, dq1, dq2, drp [H][B] (each may be null) in one elementwise pass, the reference's
 * `weighted_loss.register_hook(grad / horizon)` included: every output carries the factor 1 / H. The clamps pass
 * gradient where the sum is <= 1e4 (torch.clamp). */
int tdmpc_sim_loss_backward(const tdmpc_sim_loss_args* a, const float* rows, const float* scal, const float* gw,
                            float* dsim, float* dq1, float* dq2, float* drp, void* stream);

/* `_predictor.1` (BatchNorm1d over TDMPC_SIM_BN_WIDTH columns on batch statistics) + ELU over 2 <= rows <=
 * TDMPC_DT_MAX_ROWS rows, in 128-row chunks combined in chunk order.
 * part: scratch of tdmpc_sim_bn_part_floats(rows) floats, shared by the forward and the backward. */
int tdmpc_sim_bn_part_floats(int32_t rows, size_t* out);
/* x [rows][512] (the first Linear's output) -> xhat [rows][512], rstd [512], e = ELU(g xhat + b) [rows][512]; moves
 * rmean / rvar [512] once (momentum 0.1, the unbiased variance), as nn.BatchNorm1d in train mode. */
int tdmpc_sim_bn_fwd(const float* x, const float* g, const float* b, float* rmean, float* rvar, float* xhat,
                     float* rstd, float* e, float* part, int32_t rows, void* stream);
/* de [rows][512] = dL / d(ELU output) -> dx [rows][512] = dL / dx (may be de itself), dg [512], db [512]. */
int tdmpc_sim_bn_bwd(const float* de, const float* g, const float* xhat, const float* rstd, const float* e,
                     float* part, float* dx, float* dg, float* db, int32_t rows, void* stream);

/* loss [rows] = 2 - 2 <normalize(pred), normalize(keys)> per row of 1 <= L <= 256 features (F.normalize's 1e-12 clamp);
 * 1 <= rows <= TDMPC_DT_MAX_ROWS. The backward: dpred [rows][L] from dloss [rows] (the keys carry no gradient). */
int tdmpc_sim_cos_fwd(const float* pred, const float* keys, float* loss, int32_t rows, int32_t L, void* stream);
int tdmpc_sim_cos_bwd(const float* pred, const float* keys, const float* dloss, float* dpred, int32_t rows, int32_t L,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_SIM_LEARNER_H */
