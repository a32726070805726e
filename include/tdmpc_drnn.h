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

#define TDMPC_DRNN_VERSION 2

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

/* ---- iCEM on the DSSM (`TdICemSimDssm`, src/algorithm/tdmpc_icem_similarity_drnn.py), version 2 ---- */

/* Byte sizes of the iCEM DSSM planner: the workspace holds N + K + num_pi rows per env (as tdmpc_icem_sizes_for) plus
 * the two hidden ping-pong buffers; the packed size is tdmpc_drnn_sizes_for's. noise_floats_per_env is an upper bound
 * of one env's noise stream at max_horizon / max_iterations with K reused elites (the layout itself is the caller's:
 * tdmpc_icem_params offsets). */
int tdmpc_drnn_icem_sizes_for(const tdmpc_drnn_dims* dims, tdmpc_sizes* out);

/* One TdICemSimDssm.plan (:169-272, after the seed-step branch) for params->batch envs: tdmpc_plan_icem's order of
 * work with the rollout step replaced by drnn_step_kernel from each env's hidden state, then DSSM.next(z0, action,
 * hidden) with the returned (noised) action (:267).
 *   hidden     [batch, Hd] in   the GRU state the rollouts start from
 *   hidden_out [batch, Hd] out  required; may alias `hidden`
 *   z_out      [batch, L]  out  optional: the encoded observation
 * and every other argument as tdmpc_plan_icem (state observations, fp32). The policy rows' pre-rollout (their G,
 * last reward and z_H) is computed once and reused by every iteration. params->path is checked and selects nothing. */
int tdmpc_drnn_plan_icem(const tdmpc_drnn_dims* dims, const tdmpc_icem_params* params, const void* packed,
                         const void* obs, const float* hidden, const float* noise, const double* u, float* prev_mean,
                         float* elites, float* action, float* metrics, float* hidden_out, float* z_out,
                         float* value_out, float* mean_out, float* std_out, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Power-law (coloured) noise sequences written straight into the per-env noise streams (drnn_colored_noise_kernel).
 * A job is `n` sequences (r, a), r < n, a < A, of L samples each, for the block [L][rows][A] at `dst` floats into
 * the env's stream, columns c0 .. c0 + n: sample t of sequence (r, a) goes to
 *   noise[env * env_stride + dst + (t * rows + c0 + r) * A + a].
 * Sequence s = r * A + a takes 2F standard normals, F = L / 2 + 1, from
 *   normals[env * normals_env + src + k * n * A + s],  k < 2F  (k < F: real parts, then the imaginary parts)
 * multiplies them by its spectrum's factors re[k] / im[k] (colored_noise.spectrum_rows: f^(-beta/2) with the low
 * cutoff, sqrt(2) on the DC and even-L Nyquist real parts, 0 for their imaginary parts, 1/sigma folded in) and
 * applies the inverse real DFT as the [2F][L] matrix `dft` (colored_noise.irfft_matrices; rows of 16 floats). */
#define TDMPC_NOISE_MAX_JOBS 17
#define TDMPC_NOISE_MAX_SPECTRA 4
typedef struct tdmpc_noise_job {
    int32_t spectrum, n, rows, c0;
    int64_t dst, src;
} tdmpc_noise_job;
typedef struct tdmpc_colored_noise_params {
    int32_t L, A, batch, n_jobs, n_spectra, pad_;
    int64_t env_stride, normals_env;
    tdmpc_noise_job jobs[TDMPC_NOISE_MAX_JOBS];
    float re[TDMPC_NOISE_MAX_SPECTRA][9], im[TDMPC_NOISE_MAX_SPECTRA][9];
    float dft[18][16];
} tdmpc_colored_noise_params;

/* Domain: 2 <= L <= 16, A <= 64, 1 <= n_jobs <= 17, 1 <= n_spectra <= 4. Every job must lie inside its env's stream
 * (batch * env_stride <= noise_floats) and read inside normals (batch * normals_env <= normals_floats); otherwise
 * TDMPC_E_SIZE / TDMPC_E_DIMS with a message and nothing is launched. */
int tdmpc_drnn_colored_noise(const tdmpc_colored_noise_params* params, const float* normals, size_t normals_floats,
                             float* noise, size_t noise_floats, void* stream);

/* Diagnostic kernel timer, as tdmpc_profile_begin / tdmpc_profile_end for drnn_step_kernel: arms a per-thread recorder
 * that brackets every later step launch over exactly `rows` rows (0 = any) by HIP events; _end returns the launch
 * count, the summed time and the algorithmic FLOPs (2 * rows * MACs per row at the real widths). Eager use only. */
int tdmpc_drnn_profile_begin(int32_t rows, int32_t max_launches);
int tdmpc_drnn_profile_end(int32_t* launches, double* total_ms, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_DRNN_H */
