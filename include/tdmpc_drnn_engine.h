/*
 * tdmpc_drnn_engine.h -- C ABI of the DSSM recurrent step as learner-engine passes in libtdmpc_hip.so (DESIGN.md §7
 * f14; csrc/drnn_engine.inc, included by drnn_learner.hip after sim_learner.inc).
 *
 * tdmpc_drnn_next_fwd / _bwd (tdmpc_drnn_learner.h) are built for autograd: each call runs the whole step and the reward
 * head and overwrites all twenty parameter gradients. An engine that rolls the step out H times itself issues the
 * products -- [z | a] weight_ih^T, h weight_hh^T, prior_mlp.0 / .3, their dX, and every dW once over all steps' rows --
 * in its own grouped tdmpc_lg_gemm launches; this header exposes what lies between them, as tdmpc_sim_learner.h does for
 * the similarity head:
 *
 *   * tdmpc_drnn_gate_fwd / _bwd: NormGRUCell's pointwise part (models/rnns.py:19-29) over given products -- three row
 *     LayerNorms (eps 1e-3), sigmoid, sigmoid, tanh, the blend -- the kernels and bits of tdmpc_drnn_next_fwd / _bwd;
 *   * prior_mlp.1 + ELU is a train-mode BatchNorm over 512 columns: tdmpc_sim_bn_fwd / _bwd are that operation.
 *
 * Conventions as in tdmpc_sim_learner.h: every pointer a device pointer to contiguous float32, everything enqueued on
 * `stream`, no allocation, no sync, no float atomics, every reduction in a fixed order (two runs and a graph replay give
 * the same bits). An inadmissible shape or a null required pointer returns TDMPC_E_DIMS with a tdmpc_last_error message
 * before any HIP call and before any output is written.
 *
 * Admitted shapes: hidden_dim Hd a multiple of 32 up to 256, 2 <= rows <= TDMPC_DT_MAX_ROWS.
 */
#ifndef TDMPC_DRNN_ENGINE_H
#define TDMPC_DRNN_ENGINE_H

#include "tdmpc_drnn_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDMPC_DRNN_ENGINE_VERSION 1
#define TDMPC_DRNN_GATE_PART_ROWS 32   /* rows per workgroup of tdmpc_drnn_gate_bwd: one LayerNorm-affine partial each */

/* Returns TDMPC_DRNN_ENGINE_VERSION. */
int tdmpc_drnn_engine_version(void);

/* The cell over given gate products. gi [R,3Hd] = [z | a] weight_ih^T, gh [R,3Hd] = h weight_hh^T, h [R,Hd]; each
 * third of gi / gh is the reset / update / newval pre-activation's share. ln [6]: ln_reset.{weight, bias},
 * ln_update.{weight, bias}, ln_newval.{weight, bias}, [Hd] each (state_dict order).
 *   reset  = sigmoid(ln_reset(gi_r + gh_r)),  update = sigmoid(ln_update(gi_u + gh_u)),
 *   newval = tanh(ln_newval(gi_n + reset gh_n)),  hn = update newval + (1 - update) h
 * Saved for the backward: gate [R,3Hd] = reset | update | newval, lnx [R,3Hd] = the three LayerNorms' xhat,
 * lnr [R,4] = their 1/std per row (fourth column zero); hn [R,Hd] = h'.
 * gh == h == null: the hidden state is zero (step 0 of a rollout, where h weight_hh^T is never computed); neither is
 * read, and the result is bitwise that of explicit zeros. One of the two null alone is refused. */
int tdmpc_drnn_gate_fwd(const float* gi, const float* gh, const float* h, const float* const* ln, float* gate,
                        float* lnx, float* lnr, float* hn, int32_t rows, int32_t hidden_dim, void* stream);

/* Floats of tdmpc_drnn_gate_bwd's `part` for `rows` rows: ceil(rows / 32) slices of 6 Hd floats. */
int tdmpc_drnn_gate_part_floats(int32_t rows, int32_t hidden_dim, size_t* out);

/* Backward of tdmpc_drnn_gate_fwd over its saved regions: dhn [R,Hd] = dL/dh' ->
 *   dgi [R,3Hd]  dL/dgi (the dY of weight_ih's dX and dW products)
 *   dgh [R,3Hd]  dL/dgh (of weight_hh's)
 *   dhd [R,Hd]   dhn (1 - update): the direct path to h (dL/dh = dhd + dgh weight_hh)
 *   part         slice p < ceil(R / 32), at part + p * 6 Hd: the sums over rows 32 p .. 32 p + 31 of d ln_reset.weight,
 *                d ln_reset.bias, d ln_update.weight, .bias, d ln_newval.weight, .bias, [Hd] each. This is a
 *                tdmpc_lg_finalize source as it lies -- tensor k: src = part + k Hd, rows 1, cols Hd, ld Hd,
 *                nslices = ceil(R / 32), sstride = 6 Hd -- and the `part` buffers of H steps laid end to end
 *                (tdmpc_drnn_gate_part_floats(R, Hd) floats each) are one source of H ceil(R / 32) slices, summed in
 *                step and slice order.
 * ln [6] as above (the three weights are read). gh == h == null (with gi's forward run that way): neither is read,
 * dgh and dhd are not written (and may be null), dgi's reset third and the ln_reset partials are exactly zero, as with
 * explicit zeros. With a hidden state, dgh and dhd are required. */
int tdmpc_drnn_gate_bwd(const float* dhn, const float* gh, const float* h, const float* const* ln, const float* gate,
                        const float* lnx, const float* lnr, float* dgi, float* dgh, float* dhd, float* part,
                        int32_t rows, int32_t hidden_dim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TDMPC_DRNN_ENGINE_H */
