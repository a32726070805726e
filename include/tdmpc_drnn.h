/*
 * tdmpc_drnn.h -- C ABI of the recurrent-latent (DSSM) planner in libtdmpc_hip.so.
 *
 * The reference's DSSM agent (`TdMpcSimDssm`, src/algorithm/tdmpc_similarity_drnn.py) rolls candidates out through a
 * layer-normed GRU cell (models/rnns.py:NormGRUCell) followed by a prior MLP (models/gru_dyna.py:DGruDyna) and reads
 * the reward from the GRU hidden state. Its `plan(obs, hidden, ...)` draws its noise in the order `TDMPC.plan` does,
 * so the noise layout, tdmpc_reference_normals, the encoder (enc_norm = 1), the terminal pi / Q kernels and the CEM
 * kernel of tdmpc_hip.h are shared; the rollout step is drnn_step_kernel (csrc/drnn.inc).
 *
 * Conventions as in tdmpc_hip.h: device pointers, everything enqueued on `stream`, no allocation, no sync, capturable,
 * 0 or a negative TDMPC_E_* code. Supported shapes: state observations with the LayerNorm encoder (enc_norm = 1),
 * mlp_dim 512, hidden_dim a multiple of 32 up to 256, latent_dim <= 256 and first-layer width
 * (action and latent each padded to 8) <= 512, within what the chain pi / Q kernels accept; anything else returns
 * TDMPC_E_DIMS with a message (tdmpc_last_error).
 */
#ifndef TDMPC_DRNN_H
#define TDMPC_DRNN_H

#include "tdmpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC_DRNN_VERSION 1

/* Static shape of one DSSM planner: the planner dims plus the GRU width (cfg.hidden_dim). base.num_pi is
 * int(mixture_coef * num_samples) of the call (regularization_schedule moves it; sizes are monotone in it, so size the
 * buffers with the largest value). */
typedef struct tdmpc_drnn_dims {
    tdmpc_dims base;
    int32_t hidden_dim;    /* Hd */
} tdmpc_drnn_dims;

/* Returns TDMPC_DRNN_VERSION. */
int tdmpc_drnn_version(void);

/* Byte sizes for `dims` (packed buffer: zero-filled once when allocated, like tdmpc_pack_weights'). */
int tdmpc_drnn_sizes_for(const tdmpc_drnn_dims* dims, tdmpc_sizes* out);

/* Number of parameter tensors tdmpc_drnn_pack_weights expects: every floating-point tensor of the reference DSSM
 * state_dict in its order (num_batches_tracked left out):
 *   _dynamics.prior_mlp.{0.weight, 0.bias, 1.weight, 1.bias, 1.running_mean, 1.running_var, 3.weight, 3.bias},
 *   _dynamics.gru_cell.{weight_ih.weight, weight_hh.weight, ln_reset.*, ln_update.*, ln_newval.*},
 *   _reward.{0,2,4}.*, _pi.{0,2,4}.*, _Q1.{0,1,3,4,6}.*, _Q2.{0,1,3,4,6}.*, _encoder.{0,1,3}.*,
 *   _predictor.{0.weight, 0.bias, 1.weight, 1.bias, 1.running_mean, 1.running_var, 3.weight, 3.bias} (unused). */
int tdmpc_drnn_num_param_tensors(const tdmpc_drnn_dims* dims);

/* Pack the DSSM parameters into `packed`. One job table and one launch, with the nonce / stale protection of
 * tdmpc_pack_weights (TDMPC_STATUS_PACK_STALE, tdmpc_pack_forget). */
int tdmpc_drnn_pack_weights(const tdmpc_drnn_dims* dims, const float* const* tensors, int32_t n_tensors,
                            void* packed, size_t packed_bytes, void* stream);

/* Diagnostic, host only (no HIP call), as tdmpc_debug_pack_check: builds the job table of tdmpc_drnn_pack_weights over
 * fake tensor bases and checks that the shared heads' jobs write inside the planner layout, the DSSM jobs behind it and
 * inside the packed size, that no two DSSM jobs write the same float, and that every job reads inside its source
 * tensor of numel[i] floats. Returns the job count, or a negative TDMPC_E_* code with a message. */
int tdmpc_drnn_debug_pack_check(const tdmpc_drnn_dims* dims, const int64_t* numel, int32_t n_tensors);

/* DSSM.next (tdmpc_similarity_drnn.py:57-60) for `rows` independent rows (rows <= max_batch * (N + P) rounded up to
 * 32): z [rows, L], a [rows, A], h [rows, Hd] -> z_out [rows, L], h_out [rows, Hd] (may alias h), r_out [rows]. */
int tdmpc_drnn_next(const tdmpc_drnn_dims* dims, const void* packed, const float* z, const float* a, const float* h,
                    int32_t rows, float* z_out, float* h_out, float* r_out, void* workspace, size_t workspace_bytes,
                    void* stream);

/* TdMpcSimDssm.estimate_value (:136-144) for `batch` envs with `rows` = N + P candidates each:
 *   z0 [batch, L], h0 [batch, Hd], actions [batch, H, rows, A], eps_term [batch, rows, A]
 *   value [batch, rows] out (after nan_to_num), reward_last [batch, rows] out */
int tdmpc_drnn_estimate_value(const tdmpc_drnn_dims* dims, const tdmpc_plan_params* params, const void* packed,
                              const float* z0, const float* h0, const float* actions, const float* eps_term,
                              int32_t rows, float* value, float* reward_last, void* workspace, size_t workspace_bytes,
                              void* stream);

/* The policy pre-rollout (:203-209), hidden carried: z0 [batch, L], h0 [batch, Hd], eps_pi [batch, H, P, A]
 * -> pi_actions [batch, H, P, A]. */
int tdmpc_drnn_pi_rollout(const tdmpc_drnn_dims* dims, const tdmpc_plan_params* params, const void* packed,
                          const float* z0, const float* h0, const float* eps_pi, float* pi_actions, void* workspace,
                          size_t workspace_bytes, void* stream);

/* One TdMpcSimDssm.plan (:184-267, after the memory replay) for params->batch envs: tdmpc_plan with
 *   hidden [batch, Hd] in   the GRU state the rollouts start from
 *   z_out  [batch, L]  out  optional: the encoded observation (what the caller appends to its memory)
 * and every other argument as tdmpc_plan (state observations, fp32). The kernel path is fixed (the x6 chain kernels
 * for pi / Q, drnn_step_kernel for the step): params->path must be a valid TDMPC_PATH_* value and selects nothing. */
int tdmpc_drnn_plan(const tdmpc_drnn_dims* dims, const tdmpc_plan_params* params, const void* packed, const void* obs,
                    const float* hidden, const float* noise, const double* u, float* prev_mean, float* action,
                    float* metrics, float* z_out, float* elite_out, float* score_out, float* value_out,
                    float* mean_out, float* std_out, void* workspace, size_t workspace_bytes, void* stream);

/* Diagnostic kernel timer, as tdmpc_profile_begin / tdmpc_profile_end for drnn_step_kernel: arms a per-thread recorder
 * that brackets every later step launch over exactly `rows` rows (0 = any) by HIP events; _end returns the launch
 * count, the summed time and the algorithmic FLOPs (2 * rows * MACs per row at the real widths). Eager use only. */
int tdmpc_drnn_profile_begin(int32_t rows, int32_t max_launches);
int tdmpc_drnn_profile_end(int32_t* launches, double* total_ms, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_DRNN_H */
