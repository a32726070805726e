// drnn_learner.hip -- the DSSM learner's two differentiable parts for MI355X (gfx950): DSSM.next in train mode and
// similarity_loss, forward and backward (include/tdmpc_drnn_learner.h).
//
// Reference: DSSM.next (tdmpc_similarity_drnn.py:57-60) = DGruDyna (models/gru_dyna.py:11-29: NormGRUCell,
// models/rnns.py:8-29, then prior_mlp = helper.mlp_norm with BatchNorm1d) + the reward MLP, under model.train();
// similarity_loss (tdmpc_similarity_drnn.py / tdmpc_icem_similarity_drnn.py: _predictor, F.normalize, 2 - 2 cos).
//
// The products are grouped tdmpc_lg_gemm launches (learner_engine.hip) on the exact f32 MFMA, reading the model's own
// fp32 parameter tensors: the two gate products ([z | a] as two K segments of one job), prior_mlp.0 / _reward.0,
// prior_mlp.3 / _reward.2, their dX, and every dW with the bias as the ones column. The kernels here cover the rest:
//   * dt_gate_fwd / dt_gate_bwd: one wave per row of Hd <= 256 features -- three LayerNorms (eps 1e-3), sigmoid,
//     sigmoid, tanh, the blend; the backward also writes the LayerNorm-affine gradients as per-workgroup partials;
//   * dt_bn_stat / dt_bn_fwd / dt_bn_bwd_stat / dt_bn_bwd: BatchNorm1d on batch statistics over 512 columns (+ ELU):
//     per 128-row chunk a (mean, M2) or (sum dY, sum dY xhat) partial per column, combined in chunk order;
//   * dt_cos_fwd / dt_cos_bwd: F.normalize on both sides and 2 - 2 cos, one wave per row;
//   * dt_finish (column sums of partials in order), dt_unpack (a [out][in + 1] weight-gradient product -> dW, db).
// For the DSSM update (TdICemSimDssm.update, tdmpc_icem_similarity_drnn.py:421-553):
//   * tdmpc_drnn_intrinsic_fwd: intrinsic_rewards' H + 1 one-step rollouts from a zero hidden state and their similarity
//     losses as one launch chain over S B rows -- dt_bn_stat / dt_bn_fwd normalise per segment of B rows and move the
//     running statistics S times in segment order, dt_gate_fwd<true> reads no hidden state;
//   * dt_intrinsic_finish: float64 moments of the losses, the RunningMeanStd update on the device, the rewards;
//   * dt_loss_rows / dt_loss_means / dt_loss_bwd: the TD-lambda targets and the loss composition, forward and backward
//     (loss_means: the batch means of every loss composition here).
// For TdMpcSimDssm.update (tdmpc_similarity_drnn.py:373-496):
//   * tdmpc_drnn_intrinsic_chain_fwd: intrinsic_rewards with ONE hidden state carried through the S = H + 1 closed-loop
//     steps. weight_ih's product does not depend on the hidden state and runs once over all S B rows; the recurrence is
//     either a launch chain (per step h weight_hh^T + dt_gate_fwd) or dt_gru_chain, one launch in which a workgroup owns
//     16 batch rows for all steps (the cell has only row LayerNorms, so rows are independent through time);
//   * sl_loss_rows / sl_loss_means / sl_loss_bwd: the one-step TD targets and the loss composition over the shoot
//     steps W..H-1 (the similarity term over all H), forward and backward; instantiated a second time, with rho ** t and
//     the 1 / horizon hook, for the MLP iCEM agent's update.
// predictor_fwd is `_predictor` and the cosine loss behind every similarity loss and intrinsic-reward pass.
// The MLP iCEM agent's update (TdICemSimMlp.update) is icem_learner.inc, included at the end; after it
// sim_learner.inc, the similarity TD-MPC agent's (TDMPCSIM.update); last drnn_engine.inc, the gate
// kernels as entry points of their own for an engine that issues the step's products itself.
// Every reduction runs in a fixed order: wave butterflies, LDS sums over waves in wave order, partials in index order.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "../../include/tdmpc_drnn_engine.h"
#include "../../include/tdmpc_drnn_learner.h"
#include "../../include/tdmpc_icem_learner.h"
#include "../../include/tdmpc_learner.h"
#include "../../include/tdmpc_sim_learner.h"

namespace tdmpc_internal {
void set_error(const char* msg);
}

namespace {

constexpr int M = 512;          // mlp_dim
constexpr int CHUNK = 128;      // rows per BatchNorm partial
constexpr int GROWS = 32;       // rows per workgroup of dt_gate_bwd (one LayerNorm-affine partial each)
constexpr float LN_EPS = 1e-3f, BN_EPS = 1e-5f, BN_MOM = 0.1f, NORM_EPS = 1e-12f;

// tensor table indices (tdmpc_drnn_learner.h)
enum { P0W = 0, P0B, P1G, P1B, P1RM, P1RV, P3W, P3B, WIH, WHH, LRG, LRB, LUG, LUB, LNG, LNB, R0W, R0B, R2W, R2B, R4W,
       R4B };

__device__ __forceinline__ float wsum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// Row LayerNorm over Hd features held 4 per lane (feature lane + 64 i, valid where ok[i]): xhat and 1 / std.
__device__ __forceinline__ float ln_row(const float (&x)[4], const bool (&ok)[4], int Hd, float (&xh)[4]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += ok[i] ? x[i] : 0.f;
    const float mean = wsum(s) / (float)Hd;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) q += ok[i] ? (x[i] - mean) * (x[i] - mean) : 0.f;
    const float rstd = 1.f / sqrtf(wsum(q) / (float)Hd + LN_EPS);
#pragma unroll
    for (int i = 0; i < 4; ++i) xh[i] = (x[i] - mean) * rstd;
    return rstd;
}

struct GateArgs {
    const float* gi; const float* gh; const float* h;      // [R,3Hd], [R,3Hd], [R,Hd]
    const float* g[3]; const float* b[3];                  // ln_reset / ln_update / ln_newval
    float* gate; float* lnx; float* lnr; float* hn; float* h_out;
    // backward
    const float* dhn; float* dgi; float* dgh; float* dhd; float* part;
    int rows, Hd;
};

// NormGRUCell.forward (models/rnns.py:19-29), one wave per row, four rows per workgroup. ZH: the hidden state is zero
// (a.gh and a.h are not read: weight_hh(0) = 0).
template <bool ZH>
__global__ void __launch_bounds__(256) dt_gate_fwd(const GateArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), Hd = a.Hd;
    if (row >= a.rows) return;
    const size_t r3 = (size_t)row * 3 * Hd, r1 = (size_t)row * Hd;
    bool ok[4];
    float sr[4], su[4], ghn[4], gin[4], hp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        ok[i] = c < Hd;
        const int cc = ok[i] ? c : 0;
        sr[i] = a.gi[r3 + cc] + (ZH ? 0.f : a.gh[r3 + cc]);
        su[i] = a.gi[r3 + Hd + cc] + (ZH ? 0.f : a.gh[r3 + Hd + cc]);
        gin[i] = a.gi[r3 + 2 * Hd + cc];
        ghn[i] = ZH ? 0.f : a.gh[r3 + 2 * Hd + cc];
        hp[i] = ZH ? 0.f : a.h[r1 + cc];
    }
    float xr[4], xu[4], xn[4], rs[4], sn[4];
    const float rstd_r = ln_row(sr, ok, Hd, xr);
    const float rstd_u = ln_row(su, ok, Hd, xu);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cc = ok[i] ? lane + 64 * i : 0;
        rs[i] = sigmoid_f(xr[i] * a.g[0][cc] + a.b[0][cc]);
        sn[i] = gin[i] + rs[i] * ghn[i];
    }
    const float rstd_n = ln_row(sn, ok, Hd, xn);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (!ok[i]) continue;
        const float u = sigmoid_f(xu[i] * a.g[1][c] + a.b[1][c]);
        const float n = tanhf(xn[i] * a.g[2][c] + a.b[2][c]);
        const float hn = u * n + (1.f - u) * hp[i];
        a.gate[r3 + c] = rs[i];
        a.gate[r3 + Hd + c] = u;
        a.gate[r3 + 2 * Hd + c] = n;
        a.lnx[r3 + c] = xr[i];
        a.lnx[r3 + Hd + c] = xu[i];
        a.lnx[r3 + 2 * Hd + c] = xn[i];
        a.hn[r1 + c] = hn;
        a.h_out[r1 + c] = hn;
    }
    if (lane < 4) a.lnr[(size_t)row * 4 + lane] = lane == 0 ? rstd_r : lane == 1 ? rstd_u : lane == 2 ? rstd_n : 0.f;
}

// LayerNorm backward of one row: dy (w.r.t. the affine output) -> dx (w.r.t. the input); dg / db accumulate the affine
// gradients of this lane's features.
__device__ __forceinline__ void ln_row_bwd(const float (&dy)[4], const float (&xh)[4], const float (&g)[4],
                                           const bool (&ok)[4], float rstd, int Hd, float (&dx)[4], float (&dg)[4],
                                           float (&db)[4]) {
    float s1 = 0.f, s2 = 0.f, d[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d[i] = ok[i] ? dy[i] * g[i] : 0.f;
        s1 += d[i];
        s2 += ok[i] ? d[i] * xh[i] : 0.f;
        dg[i] += ok[i] ? dy[i] * xh[i] : 0.f;
        db[i] += ok[i] ? dy[i] : 0.f;
    }
    const float m1 = wsum(s1) / (float)Hd, m2 = wsum(s2) / (float)Hd;
#pragma unroll
    for (int i = 0; i < 4; ++i) dx[i] = rstd * (d[i] - m1 - xh[i] * m2);
}

// Backward of the cell: dhn [R,Hd] = dL/dh' -> dgi, dgh [R,3Hd] (w.r.t. weight_ih / weight_hh's outputs), dhd [R,Hd]
// (the direct (1 - update) path to h) and part [nwg][6][Hd]: the workgroup's sums over its GROWS rows of the three
// LayerNorms' (dweight, dbias). Wave w takes rows base + w, base + w + 4, ...; the four waves add in wave order.
// ZH: the hidden state was zero (dt_gate_fwd<true>): a.gh and a.h are not read, a.dgh and a.dhd not written; newval_h = 0
// leaves the reset gate without gradient (dgi's reset third and ln_reset's partials are zero).
template <bool ZH>
__global__ void __launch_bounds__(256) dt_gate_bwd(const GateArgs a) {
    __shared__ float red[4][6][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, Hd = a.Hd;
    bool ok[4];
    float g[3][4], acc[6][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        ok[i] = c < Hd;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k][i] = a.g[k][ok[i] ? c : 0];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k][i] = 0.f;
    }
    for (int q = wave; q < GROWS; q += 4) {
        const int row = blockIdx.x * GROWS + q;
        if (row >= a.rows) break;   // (wave-uniform)
        const size_t r3 = (size_t)row * 3 * Hd, r1 = (size_t)row * Hd;
        const float rstd_r = a.lnr[(size_t)row * 4], rstd_u = a.lnr[(size_t)row * 4 + 1],
                    rstd_n = a.lnr[(size_t)row * 4 + 2];
        float r[4], u[4], n[4], xr[4], xu[4], xn[4], ghn[4], dH[4], hp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cc = ok[i] ? lane + 64 * i : 0;
            r[i] = a.gate[r3 + cc];
            u[i] = a.gate[r3 + Hd + cc];
            n[i] = a.gate[r3 + 2 * Hd + cc];
            xr[i] = a.lnx[r3 + cc];
            xu[i] = a.lnx[r3 + Hd + cc];
            xn[i] = a.lnx[r3 + 2 * Hd + cc];
            ghn[i] = ZH ? 0.f : a.gh[r3 + 2 * Hd + cc];
            dH[i] = a.dhn[r1 + cc];
            hp[i] = ZH ? 0.f : a.h[r1 + cc];
        }
        float dyn[4], dyu[4], dyr[4], dsn[4], dsu[4], dsr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dyn[i] = dH[i] * u[i] * (1.f - n[i] * n[i]);
            dyu[i] = dH[i] * (n[i] - hp[i]) * u[i] * (1.f - u[i]);
        }
        ln_row_bwd(dyn, xn, g[2], ok, rstd_n, Hd, dsn, acc[4], acc[5]);
        ln_row_bwd(dyu, xu, g[1], ok, rstd_u, Hd, dsu, acc[2], acc[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) dyr[i] = dsn[i] * ghn[i] * r[i] * (1.f - r[i]);
        if (ZH) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dsr[i] = 0.f;
        } else {
            ln_row_bwd(dyr, xr, g[0], ok, rstd_r, Hd, dsr, acc[0], acc[1]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;
            if (!ok[i]) continue;
            a.dgi[r3 + c] = dsr[i];
            a.dgi[r3 + Hd + c] = dsu[i];
            a.dgi[r3 + 2 * Hd + c] = dsn[i];
            if (ZH) continue;
            a.dgh[r3 + c] = dsr[i];
            a.dgh[r3 + Hd + c] = dsu[i];
            a.dgh[r3 + 2 * Hd + c] = dsn[i] * r[i];
            a.dhd[r1 + c] = dH[i] * (1.f - u[i]);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave][k][lane + 64 * i] = acc[k][i];
    __syncthreads();
    for (int e = threadIdx.x; e < 6 * Hd; e += 256) {
        const int k = e / Hd, c = e % Hd;
        a.part[((size_t)blockIdx.x * 6 + k) * Hd + c] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
    }
}

// out[k][c] = sum over p < nparts (in order) of part[p][k][c], k < nvec, c < C; out[k] are separate tensors.
struct FinishArgs {
    const float* part; float* out[8];
    int nparts, nvec, C;
};
__global__ void __launch_bounds__(256) dt_finish(const FinishArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nvec * a.C) return;
    float s = 0.f;
    for (int p = 0; p < a.nparts; ++p) s += a.part[(size_t)p * a.nvec * a.C + e];
    a.out[e / a.C][e % a.C] = s;
}

// ---- BatchNorm1d on batch statistics over C columns (+ ELU). Geometry of all four kernels: grid (C / 64, chunks),
// 256 threads = 64 columns x 4 row phases; thread (tx, ty) takes rows chunk * CHUNK + ty, + 4, ... of column
// 64 blockIdx.x + tx, and the four row phases add through LDS in phase order.
// The two forward kernels normalise per segment of `seg` rows (rows = nseg * seg; one segment everywhere but in
// tdmpc_drnn_intrinsic_fwd): blockIdx.y = segment * chunks(seg) + chunk, every segment's chunks start at its own row 0,
// part and rstd are indexed per segment.
struct BnArgs {
    const float* x;          // fwd: the Linear's output [R,C]; bwd: dL/d(ELU output) [R,C]
    const float* g; const float* b; float* rmean; float* rvar;
    float* xhat; float* rstd; float* e;     // saved [R,C], [C], [R,C] (bwd reads them)
    float* part;             // [chunks][2][C]
    float* dx; float* dg; float* db;        // bwd outputs: [R,C] (may be x), [C], [C]
    int rows, C;
    int seg, nseg;           // fwd: rows per segment and segments (bn_forward fills them in: rows, 1)
};

__device__ __forceinline__ float phase_sum(float (&red)[4][64], float v, int tx, int ty) {
    __syncthreads();
    red[ty][tx] = v;
    __syncthreads();
    return ((red[0][tx] + red[1][tx]) + red[2][tx]) + red[3][tx];
}

// part[chunk][0][c] = the chunk's column mean, part[chunk][1][c] = its sum of squared deviations from that mean.
__global__ void __launch_bounds__(256) dt_bn_stat(const BnArgs a) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx, C = a.C;
    const int cps = (a.seg + CHUNK - 1) / CHUNK, sg = blockIdx.y / cps, ch = blockIdx.y % cps;
    const int r0 = sg * a.seg + ch * CHUNK, r1 = min((sg + 1) * a.seg, r0 + CHUNK);
    float s = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) s += a.x[(size_t)r * C + c];
    const float mean = phase_sum(red, s, tx, ty) / (float)(r1 - r0);
    float q = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) {
        const float d = a.x[(size_t)r * C + c] - mean;
        q += d * d;
    }
    const float m2 = phase_sum(red, q, tx, ty);
    if (ty == 0) {
        a.part[((size_t)blockIdx.y * 2) * C + c] = mean;
        a.part[((size_t)blockIdx.y * 2 + 1) * C + c] = m2;
    }
}

// The chunks' (mean, M2) combined in chunk order (Chan et al.'s pairwise update): the column's mean and M2 over R rows.
__device__ __forceinline__ void bn_combine(const float* part, int rows, int C, int c, float& mean, float& m2) {
    float n = 0.f;
    mean = 0.f;
    m2 = 0.f;
    for (int p = 0; p * CHUNK < rows; ++p) {
        const float nb = (float)(min(rows, (p + 1) * CHUNK) - p * CHUNK);
        const float mb = part[((size_t)p * 2) * C + c], qb = part[((size_t)p * 2 + 1) * C + c];
        const float d = mb - mean, nt = n + nb;
        mean += d * (nb / nt);
        m2 += qb + d * d * (n * nb / nt);
        n = nt;
    }
}

// xhat = (x - mean) / sqrt(biased var + eps), e = ELU(g xhat + b); a segment's chunk 0 also writes its columns' 1 / std
// and block row 0 moves the running statistics (momentum 0.1, the unbiased variance M2 / (R - 1), as nn.BatchNorm1d).
__global__ void __launch_bounds__(256) dt_bn_fwd(const BnArgs a) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx, C = a.C;
    const int cps = (a.seg + CHUNK - 1) / CHUNK, sg = blockIdx.y / cps, ch = blockIdx.y % cps;
    const int r0 = sg * a.seg + ch * CHUNK, r1 = min((sg + 1) * a.seg, r0 + CHUNK);
    float mean, m2;
    bn_combine(a.part + (size_t)sg * cps * 2 * C, a.seg, C, c, mean, m2);
    const float rstd = 1.f / sqrtf(m2 / (float)a.seg + BN_EPS);
    const float g = a.g[c], b = a.b[c];
    for (int r = r0 + ty; r < r1; r += 4) {
        const float xh = (a.x[(size_t)r * C + c] - mean) * rstd;
        a.xhat[(size_t)r * C + c] = xh;
        a.e[(size_t)r * C + c] = elu_f(xh * g + b);
    }
    if (ch == 0 && ty == 0) a.rstd[(size_t)sg * C + c] = rstd;
    if (blockIdx.y == 0 && ty == 0) {
        // the block that owns the column moves its running statistics once per segment, in segment order
        float rm = a.rmean[c], rv = a.rvar[c];
        for (int s = 0; s < a.nseg; ++s) {
            if (s) bn_combine(a.part + (size_t)s * cps * 2 * C, a.seg, C, c, mean, m2);
            // (1 - momentum) old, rounded, then one fma with the new term: spelled out so that the bits do not hang on
            // which of the two products the compiler chooses to contract
            rm = __fmaf_rn(BN_MOM, mean, __fmul_rn(1.f - BN_MOM, rm));
            rv = __fmaf_rn(BN_MOM, m2 / (float)(a.seg - 1), __fmul_rn(1.f - BN_MOM, rv));
        }
        a.rmean[c] = rm;
        a.rvar[c] = rv;
    }
}

// dY = x ELU'(e) (the gradient at the BatchNorm's output); part[chunk][0][c] = sum dY, [1] = sum dY xhat.
__global__ void __launch_bounds__(256) dt_bn_bwd_stat(const BnArgs a) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx, C = a.C;
    const int r0 = blockIdx.y * CHUNK, r1 = min(a.rows, r0 + CHUNK);
    float s1 = 0.f, s2 = 0.f;
    for (int r = r0 + ty; r < r1; r += 4) {
        const size_t i = (size_t)r * C + c;
        const float e = a.e[i], dy = a.x[i] * (e > 0.f ? 1.f : e + 1.f);
        s1 += dy;
        s2 += dy * a.xhat[i];
    }
    s1 = phase_sum(red, s1, tx, ty);
    s2 = phase_sum(red, s2, tx, ty);
    if (ty == 0) {
        a.part[((size_t)blockIdx.y * 2) * C + c] = s1;
        a.part[((size_t)blockIdx.y * 2 + 1) * C + c] = s2;
    }
}

// dx = g rstd (dY - mean(dY) - xhat mean(dY xhat)); chunk 0 also writes dg = sum dY xhat and db = sum dY.
__global__ void __launch_bounds__(256) dt_bn_bwd(const BnArgs a) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx, C = a.C;
    const int r0 = blockIdx.y * CHUNK, r1 = min(a.rows, r0 + CHUNK);
    float s1 = 0.f, s2 = 0.f;
    for (int p = 0; p * CHUNK < a.rows; ++p) {
        s1 += a.part[((size_t)p * 2) * C + c];
        s2 += a.part[((size_t)p * 2 + 1) * C + c];
    }
    const float k = a.g[c] * a.rstd[c], m1 = s1 / (float)a.rows, m2 = s2 / (float)a.rows;
    for (int r = r0 + ty; r < r1; r += 4) {
        const size_t i = (size_t)r * C + c;
        const float e = a.e[i], dy = a.x[i] * (e > 0.f ? 1.f : e + 1.f);
        a.dx[i] = k * (dy - m1 - a.xhat[i] * m2);
    }
    if (blockIdx.y == 0 && ty == 0) {
        a.dg[c] = s2;
        a.db[c] = s1;
    }
}

// ---- 2 - 2 <normalize(p), normalize(k)> per row of L <= 256 features, one wave per row.
__device__ __forceinline__ void cos_row(const float* p, const float* k, int L, int lane, float (&pv)[4], float (&kv)[4],
                                        float& pp, float& kk, float& pk) {
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        pv[i] = j < L ? p[j] : 0.f;
        kv[i] = j < L ? k[j] : 0.f;
        a += pv[i] * pv[i];
        b += kv[i] * kv[i];
        c += pv[i] * kv[i];
    }
    pp = wsum(a);
    kk = wsum(b);
    pk = wsum(c);
}

__global__ void __launch_bounds__(256) dt_cos_fwd(const float* pred, const float* keys, float* loss, int rows, int L) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float pv[4], kv[4], pp, kk, pk;
    cos_row(pred + (size_t)row * L, keys + (size_t)row * L, L, lane, pv, kv, pp, kk, pk);
    const float np = fmaxf(sqrtf(pp), NORM_EPS), nk = fmaxf(sqrtf(kk), NORM_EPS);
    if (lane == 0) loss[row] = 2.f - 2.f * (pk / (np * nk));
}

// dpred = -2 dloss (khat - phat <phat, khat>) / ||p|| (a row with ||p|| below the clamp: -2 dloss khat / 1e-12).
__global__ void __launch_bounds__(256) dt_cos_bwd(const float* pred, const float* keys, const float* dloss,
                                                  float* dpred, int rows, int L) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float pv[4], kv[4], pp, kk, pk;
    cos_row(pred + (size_t)row * L, keys + (size_t)row * L, L, lane, pv, kv, pp, kk, pk);
    const float n0 = sqrtf(pp), np = fmaxf(n0, NORM_EPS), nk = fmaxf(sqrtf(kk), NORM_EPS);
    const float cs = n0 >= NORM_EPS ? pk / (np * nk) : 0.f, s = -2.f * dloss[row] / np;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = lane + 64 * i;
        if (j < L) dpred[(size_t)row * L + j] = s * (kv[i] / nk - (pv[i] / np) * cs);
    }
}

// A weight-gradient product with the ones column, src [out][in + 1] -> dw [out][in], db [out].
struct UnpackJob { const float* src; float* dw; float* db; int out, in; };
struct UnpackArgs { UnpackJob job[8]; };
__global__ void __launch_bounds__(256) dt_unpack(const UnpackArgs a) {
    const UnpackJob& j = a.job[blockIdx.y];
    const int n = j.out * (j.in + 1);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int r = e / (j.in + 1), c = e % (j.in + 1);
        const float v = j.src[e];
        if (c < j.in) j.dw[(size_t)r * j.in + c] = v;
        else j.db[r] = v;
    }
}

// ---- intrinsic_rewards' normalisation (tdmpc_icem_similarity_drnn.py:435-443) in one workgroup: float64 moments of
// n <= 4096 losses (thread-strided sums, then the 256 threads' sums in thread order), gym's update_from_moments with
// batch_count 1 on the device state, the normalised and thresholded rewards.
__device__ __forceinline__ double block_sum_f64(double (&red)[256], double v) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += red[i];
    return s;
}

__global__ void __launch_bounds__(256) dt_intrinsic_finish(const float* loss, int n, double* rms, const float* coef,
                                                           const float* reward, float* intrinsic, float* reward_pi) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)loss[i];
    const double bm = block_sum_f64(red, s) / (double)n;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = (double)loss[i] - bm;
        q += d * d;
    }
    const double bv = block_sum_f64(red, q) / (double)n;
    const double mean = rms[0], var = rms[1], count = rms[2];
    const double delta = bm - mean, tot = count + 1.0;
    const double mean2 = mean + delta / tot;
    const double var2 = (var * count + bv + delta * delta * count / tot) / tot;
    __syncthreads();   // every thread has read the old state
    if (threadIdx.x == 0) {
        rms[0] = mean2;
        rms[1] = var2;
        rms[2] = tot;
    }
    const double sd = sqrt(var2), thr = mean2 / sd;
    const float k = coef[0];
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = (float)fmax((double)loss[i] / sd - thr, 0.0);
        intrinsic[i] = v;
        reward_pi[i] = k * v + reward[i];
    }
}

// ---- TdICemSimDssm.update's loss composition (tdmpc_drnn_learner.h): one thread per batch column for the TD-lambda
// recursion and the per-row sums, one workgroup for the means, one elementwise pass for the backward.
constexpr float LOSS_CLAMP = 1e4f;

__global__ void __launch_bounds__(256) dt_loss_rows(const tdmpc_drnn_loss_args a, float* td, float* rows) {
    const int b = blockIdx.x * 256 + threadIdx.x, H = a.H, B = a.B;
    if (b >= B) return;
    float last = a.nq[(size_t)(H - 1) * B + b];
    for (int t = H - 1; t >= 0; --t) {
        const size_t i = (size_t)t * B + b;
        const float in = a.rwpi[i] + a.discount * a.nq[i] * (1.f - a.td_lambda);
        last = in + a.discount * last * a.td_lambda;
        td[i] = last;
    }
    float sim = 0.f, rew = 0.f, val = 0.f, pri = 0.f;
    for (int t = 0; t < H; ++t) {
        const size_t i = (size_t)t * B + b;
        const float dr = a.rp[i] - a.rw[i], d1 = a.q1[i] - td[i], d2 = a.q2[i] - td[i];
        sim += a.sim[i];
        rew += dr * dr;
        val += d1 * d1 + d2 * d2;
        pri += fabsf(d1) + fabsf(d2);
    }
    rows[b] = sim;
    rows[B + b] = rew;
    rows[2 * B + b] = val;
    rows[3 * B + b] = fminf(pri, LOSS_CLAMP);
    rows[4 * B + b] = a.sim_coef * fminf(sim, LOSS_CLAMP) + a.reward_coef * fminf(rew, LOSS_CLAMP);
    rows[5 * B + b] = a.value_coef * fminf(val, LOSS_CLAMP);
}

// The means over the batch of K - 1 rows of `rows` [*, B] (row numbers `at`) and, last, of w [B], by one workgroup of 512
// threads: thread-strided sums, wsum, the eight wave sums added in wave order by thread 0, which alone gets m.
template <int K>
__device__ __forceinline__ void loss_means(const float* rows, const int (&at)[K - 1], const float* w, int B,
                                           float (&m)[K]) {
    __shared__ float red[K][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.f;
    for (int b = tid; b < B; b += 512) {
#pragma unroll
        for (int k = 0; k < K - 1; ++k) s[k] += rows[(size_t)at[k] * B + b];
        s[K - 1] += w[b];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float v = wsum(s[k]);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 0; k < K; ++k) {
        float v = 0.f;
        for (int wv = 0; wv < 8; ++wv) v += red[k][wv];
        m[k] = v / (float)B;
    }
}

__global__ void __launch_bounds__(512) dt_loss_means(const tdmpc_drnn_loss_args a, const float* rows, float* scal) {
    float m[6];
    loss_means<6>(rows, {0, 1, 2, 4, 5}, a.w, a.B, m);
    if (threadIdx.x == 0) {
        scal[0] = m[0]; scal[1] = m[1]; scal[2] = m[2];
        scal[3] = m[3] + m[4];
        scal[4] = m[3] * m[5] + m[4];
        scal[5] = m[5]; scal[6] = m[3]; scal[7] = m[4];
    }
}

__global__ void __launch_bounds__(256) dt_loss_bwd(const tdmpc_drnn_loss_args a, const float* td, const float* rows,
                                                   const float* scal, const float* gw, float* dsim, float* dq1,
                                                   float* dq2, float* drp) {
    const int B = a.B;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.H * B) return;
    const int b = (int)(i % B);
    const float dmodel = gw[0] * scal[5] / (float)B, dtd = gw[0] / (float)B;
    const float ds = rows[b] <= LOSS_CLAMP ? a.sim_coef * dmodel : 0.f;
    const float dr = rows[B + b] <= LOSS_CLAMP ? a.reward_coef * dmodel : 0.f;
    const float dv = rows[2 * B + b] <= LOSS_CLAMP ? a.value_coef * dtd : 0.f;
    if (dsim) dsim[i] = ds;
    if (drp) drp[i] = 2.f * (a.rp[i] - a.rw[i]) * dr;
    if (dq1) dq1[i] = 2.f * (a.q1[i] - td[i]) * dv;
    if (dq2) dq2[i] = 2.f * (a.q2[i] - td[i]) * dv;
}

// ---- The GRU recurrence of tdmpc_drnn_intrinsic_chain_fwd (mode 1) in one launch. A workgroup owns CROWS batch rows
// and walks the S segments itself: the h tile [CROWS][Hd] and the step's weight_hh(h) [CROWS][3Hd] live in LDS,
// weight_hh [3Hd][Hd] streams from L2 every step, the product runs on the exact f32 MFMA (v_mfma_f32_16x16x4_f32; lane
// (r = lane % 16, q = lane / 16) loads k0 + 4q .. k0 + 4q + 3 of row r of h and of output column r of the tile as one
// float4 each, so the MFMA's four k slots of a step are k0 + i, k0 + 4 + i, k0 + 8 + i, k0 + 12 + i: a permutation of
// the sum), wave w of the 16 takes the 16-column tiles w, w + 16, ...; then wave w runs dt_gate_fwd's epilogue on row w
// and writes h' to hn[s] and back into the tile. Rows past B compute on zeros and write nothing.
constexpr int CROWS = 16;
constexpr int CWAVES = 16;   // one wave per row in the epilogue, 3 Hd / 16 column tiles over 16 waves in the product
typedef float floatx4 __attribute__((ext_vector_type(4)));

struct ChainArgs {
    const float* gi;         // [S B, 3Hd]: [z | a] weight_ih^T
    const float* whh;        // [3Hd, Hd]
    const float* g[3]; const float* b[3];
    float* hn;               // [S B, Hd]: every segment's h'
    int S, B, Hd;
};

__global__ void __launch_bounds__(64 * CWAVES) dt_gru_chain(const ChainArgs a) {
    extern __shared__ float lds[];
    const int Hd = a.Hd, B = a.B, hs = Hd + 4, ps = 3 * Hd + 4;   // row strides: 16-B aligned, off the bank grid
    float* ht = lds;                   // [CROWS][hs]
    float* pre = lds + CROWS * hs;     // [CROWS][ps]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
    const int row0 = blockIdx.x * CROWS;
    for (int e = threadIdx.x; e < CROWS * hs; e += 64 * CWAVES) ht[e] = 0.f;
    bool ok[4];
    float g[3][4], bb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        ok[i] = c < Hd;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g[k][i] = a.g[k][ok[i] ? c : 0];
            bb[k][i] = a.b[k][ok[i] ? c : 0];
        }
    }
    __syncthreads();
    for (int s = 0; s < a.S; ++s) {
        if (s) {
            for (int t = wave; t < 3 * Hd / 16; t += CWAVES) {
                const float* wrow = a.whh + (size_t)(t * 16 + r) * Hd + 4 * q;
                const float* hrow = ht + r * hs + 4 * q;
                floatx4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int k0 = 0; k0 < Hd; k0 += 32) {   // (Hd is a multiple of 32: two groups of 16 k in flight)
                    const float4 w0 = *reinterpret_cast<const float4*>(wrow + k0);
                    const float4 w1 = *reinterpret_cast<const float4*>(wrow + k0 + 16);
                    const float4 h0 = *reinterpret_cast<const float4*>(hrow + k0);
                    const float4 h1 = *reinterpret_cast<const float4*>(hrow + k0 + 16);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h0.x, w0.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h0.y, w0.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h0.z, w0.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h0.w, w0.w, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h1.x, w1.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h1.y, w1.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h1.z, w1.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h1.w, w1.w, acc, 0, 0, 0);
                }
                // D: lane (r, q) holds rows 4q .. 4q + 3 of column r
#pragma unroll
                for (int i = 0; i < 4; ++i) pre[(4 * q + i) * ps + t * 16 + r] = acc[i];
            }
            __syncthreads();
        }
        for (int lr = wave; lr < CROWS; lr += CWAVES) {
            const int b = row0 + lr;
            if (b >= B) break;   // (wave-uniform)
            const size_t r3 = ((size_t)s * B + b) * 3 * Hd, r1 = ((size_t)s * B + b) * Hd;
            const float* pr = pre + lr * ps;
            float sr[4], su[4], ghn[4], gin[4], hp[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cc = ok[i] ? lane + 64 * i : 0;
                sr[i] = a.gi[r3 + cc] + (s ? pr[cc] : 0.f);
                su[i] = a.gi[r3 + Hd + cc] + (s ? pr[Hd + cc] : 0.f);
                gin[i] = a.gi[r3 + 2 * Hd + cc];
                ghn[i] = s ? pr[2 * Hd + cc] : 0.f;
                hp[i] = ht[lr * hs + cc];
            }
            float xr[4], xu[4], xn[4], sn[4];
            ln_row(sr, ok, Hd, xr);
            ln_row(su, ok, Hd, xu);
#pragma unroll
            for (int i = 0; i < 4; ++i) sn[i] = gin[i] + sigmoid_f(xr[i] * g[0][i] + bb[0][i]) * ghn[i];
            ln_row(sn, ok, Hd, xn);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                if (!ok[i]) continue;
                const float u = sigmoid_f(xu[i] * g[1][i] + bb[1][i]);
                const float n = tanhf(xn[i] * g[2][i] + bb[2][i]);
                const float hn = u * n + (1.f - u) * hp[i];
                a.hn[r1 + c] = hn;
                ht[lr * hs + c] = hn;
            }
        }
        __syncthreads();
    }
}

// ---- The loss composition with one-step TD targets, every term under the priority weights: TdMpcSimDssm.update's
// (tdmpc_drnn_sim_loss_*: the reward / value / priority sums over the N = H - W shoot steps), TdICemSimMlp.update's
// (tdmpc_icem_loss_*: N = H, those sums weighted by rho ** t, and the 1 / horizon gradient hook in the backward) and
// TDMPCSIM.update's (tdmpc_sim_loss_*: the MLP iCEM agent's over TD targets that the caller computed). RHO and
// HOOK choose the expressions at compile time: each caller keeps its own contraction into FMAs.
struct StepLossArgs {
    const float *sim, *q1, *q2, *rp, *rw, *rwpi, *nq, *w;
    int H, N, B;
    float sim_coef, reward_coef, value_coef, discount;
    double rho;
};

// (float)(rho ** t): the power in double, rounded once (a float32 tensor times a Python float).
__device__ __forceinline__ float rho_pow(double rho, int t) { return t == 0 ? 1.f : (float)pow(rho, (double)t); }

// TDIN: td is given (tdmpc_sim_loss_*: the learner engine's row kernel wrote it) and not written; rwpi / nq are not read.
template <bool RHO, bool TDIN = false>
__global__ void __launch_bounds__(256) sl_loss_rows(const StepLossArgs a, float* td, float* rows) {
    const int b = blockIdx.x * 256 + threadIdx.x, H = a.H, N = a.N, B = a.B;
    if (b >= B) return;
    float sim = 0.f, rew = 0.f, val = 0.f, pri = 0.f;
    for (int t = 0; t < H; ++t) sim += a.sim[(size_t)t * B + b];
    for (int t = 0; t < N; ++t) {
        const size_t i = (size_t)t * B + b;
        const float tg = TDIN ? td[i] : a.rwpi[i] + a.discount * a.nq[i];
        const float dr = a.rp[i] - a.rw[i], d1 = a.q1[i] - tg, d2 = a.q2[i] - tg;
        if (!TDIN) td[i] = tg;
        if (RHO) {
            const float r = rho_pow(a.rho, t);
            rew += (dr * dr) * r;
            val += (d1 * d1 + d2 * d2) * r;
            pri += (fabsf(d1) + fabsf(d2)) * r;
        } else {
            rew += dr * dr;
            val += d1 * d1 + d2 * d2;
            pri += fabsf(d1) + fabsf(d2);
        }
    }
    rows[b] = sim;
    rows[B + b] = rew;
    rows[2 * B + b] = val;
    rows[3 * B + b] = fminf(pri, LOSS_CLAMP);
    rows[4 * B + b] = a.sim_coef * fminf(sim, LOSS_CLAMP) + a.reward_coef * fminf(rew, LOSS_CLAMP) +
                      a.value_coef * fminf(val, LOSS_CLAMP);
}

__global__ void __launch_bounds__(512) sl_loss_means(const float* rows, const float* w, int B, float* scal) {
    float m[5];
    loss_means<5>(rows, {0, 1, 2, 4}, w, B, m);
    if (threadIdx.x == 0) {
        scal[0] = m[0]; scal[1] = m[1]; scal[2] = m[2]; scal[3] = m[3];
        scal[4] = m[3] * m[4];
        scal[5] = m[4];
    }
}

template <bool RHO, bool HOOK>
__global__ void __launch_bounds__(256) sl_loss_bwd(const StepLossArgs a, const float* td, const float* rows,
                                                   const float* scal, const float* gw, float* dsim, float* dq1,
                                                   float* dq2, float* drp) {
    const int B = a.B;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.H * B) return;
    const int b = (int)(i % B), t = (int)(i / B);
    // d weighted / d total_b = mean(w) / B, after the hook's 1 / horizon
    const float dtot = HOOK ? gw[0] * (1.f / (float)a.H) * scal[5] / (float)B : gw[0] * scal[5] / (float)B;
    if (dsim) dsim[i] = rows[b] <= LOSS_CLAMP ? a.sim_coef * dtot : 0.f;
    if (i >= (long)a.N * B) return;
    float dr, dv;
    if (RHO) {
        const float r = rho_pow(a.rho, t);
        dr = rows[B + b] <= LOSS_CLAMP ? a.reward_coef * dtot * r : 0.f;
        dv = rows[2 * B + b] <= LOSS_CLAMP ? a.value_coef * dtot * r : 0.f;
    } else {
        dr = rows[B + b] <= LOSS_CLAMP ? a.reward_coef * dtot : 0.f;
        dv = rows[2 * B + b] <= LOSS_CLAMP ? a.value_coef * dtot : 0.f;
    }
    if (drp) drp[i] = 2.f * (a.rp[i] - a.rw[i]) * dr;
    if (dq1) dq1[i] = 2.f * (a.q1[i] - td[i]) * dv;
    if (dq2) dq2[i] = 2.f * (a.q2[i] - td[i]) * dv;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

int bad(const char* fmt, long a = 0, long b = 0) {
    char msg[256];
    snprintf(msg, sizeof msg, fmt, a, b);
    tdmpc_internal::set_error(msg);
    return TDMPC_E_DIMS;
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char msg[256];
    snprintf(msg, sizeof msg, "drnn_learner %s: %s", what, hipGetErrorString(e));
    tdmpc_internal::set_error(msg);
    return TDMPC_E_HIP;
}

struct Shape { int L, A, Hd, R; };

int check_shape(const tdmpc_drnn_dims* d, int rows, Shape& s) {
    if (!d) return bad("drnn_learner: dims is null");
    const tdmpc_dims& b = d->base;
    if (b.modality != 0) return bad("drnn_learner: state observations only (modality %ld)", b.modality);
    if (b.mlp_dim != M) return bad("drnn_learner: mlp_dim %ld is not supported (512 only)", b.mlp_dim);
    if (d->hidden_dim < 32 || d->hidden_dim > 256 || d->hidden_dim % 32)
        return bad("drnn_learner: hidden_dim %ld is not a multiple of 32 in [32, 256]", d->hidden_dim);
    if (b.latent_dim < 1 || b.latent_dim > 256) return bad("drnn_learner: latent_dim %ld is not in [1, 256]", b.latent_dim);
    if (b.action_dim < 1) return bad("drnn_learner: action_dim %ld", b.action_dim);
    if (rows < 2 || rows > TDMPC_DT_MAX_ROWS)
        return bad("drnn_learner: rows %ld is not in [2, %ld] (train-mode BatchNorm needs two rows)", rows,
                   TDMPC_DT_MAX_ROWS);
    s = Shape{b.latent_dim, b.action_dim, d->hidden_dim, rows};
    return 0;
}

// A bump allocator over a float buffer (every region a multiple of 4 floats: 16-B aligned operands for the GEMM).
struct Bump {
    float* base; size_t off = 0;
    explicit Bump(float* b) : base(b) {}
    float* take(size_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 3) & ~(size_t)3;
        return p;
    }
};

int chunks(int R) { return (R + CHUNK - 1) / CHUNK; }
int gate_wgs(int R) { return (R + GROWS - 1) / GROWS; }

struct NextSaved { float *gh, *gate, *lnx, *lnr, *hn, *bnx, *bnr, *e, *q1, *q2; size_t total; };
NextSaved next_saved(const Shape& s, float* base) {
    Bump b(base);
    NextSaved v;
    const size_t R = s.R;
    v.gh = b.take(R * 3 * s.Hd);
    v.gate = b.take(R * 3 * s.Hd);
    v.lnx = b.take(R * 3 * s.Hd);
    v.lnr = b.take(R * 4);
    v.hn = b.take(R * s.Hd);
    v.bnx = b.take(R * M);
    v.bnr = b.take(M);
    v.e = b.take(R * M);
    v.q1 = b.take(R * M);
    v.q2 = b.take(R * M);
    v.total = b.off;
    return v;
}

struct LossSaved { float *bnx, *bnr, *e, *pred; size_t total; };
LossSaved loss_saved(const Shape& s, float* base) {
    Bump b(base);
    LossSaved v;
    const size_t R = s.R;
    v.bnx = b.take(R * M);
    v.bnr = b.take(M);
    v.e = b.take(R * M);
    v.pred = b.take(R * s.L);
    v.total = b.off;
    return v;
}

struct NextFwdWs { float *gi, *p1, *part; size_t total; };
NextFwdWs next_fwd_ws(const Shape& s, float* base) {
    Bump b(base);
    NextFwdWs v;
    v.gi = b.take((size_t)s.R * 3 * s.Hd);
    v.p1 = b.take((size_t)s.R * M);
    v.part = b.take((size_t)chunks(s.R) * 2 * M);
    v.total = b.off;
    return v;
}

struct NextBwdWs {
    float *zz, *zr, *dq2, *de, *dq1, *dhn, *dgi, *dgh, *dhd, *lnpart, *bnpart, *wp0, *wp3, *wr0, *wr2, *wr4;
    size_t total;
};
NextBwdWs next_bwd_ws(const Shape& s, float* base) {
    Bump b(base);
    NextBwdWs v;
    const size_t R = s.R;
    v.zz = b.take(R * s.L);
    v.zr = b.take(R);
    v.dq2 = b.take(R * M);
    v.de = b.take(R * M);
    v.dq1 = b.take(R * M);
    v.dhn = b.take(R * s.Hd);
    v.dgi = b.take(R * 3 * s.Hd);
    v.dgh = b.take(R * 3 * s.Hd);
    v.dhd = b.take(R * s.Hd);
    v.lnpart = b.take((size_t)gate_wgs(s.R) * 6 * s.Hd);
    v.bnpart = b.take((size_t)chunks(s.R) * 2 * M);
    v.wp0 = b.take((size_t)M * (s.Hd + 1));
    v.wp3 = b.take((size_t)s.L * (M + 1));
    v.wr0 = b.take((size_t)M * (s.Hd + 1));
    v.wr2 = b.take((size_t)M * (M + 1));
    v.wr4 = b.take(M + 1);
    v.total = b.off;
    return v;
}

struct LossFwdWs { float *p1, *part; size_t total; };
LossFwdWs loss_fwd_ws(const Shape& s, float* base) {
    Bump b(base);
    LossFwdWs v;
    v.p1 = b.take((size_t)s.R * M);
    v.part = b.take((size_t)chunks(s.R) * 2 * M);
    v.total = b.off;
    return v;
}

struct LossBwdWs { float *dpred, *de, *part, *w3, *w0; size_t total; };
LossBwdWs loss_bwd_ws(const Shape& s, float* base) {
    Bump b(base);
    LossBwdWs v;
    v.dpred = b.take((size_t)s.R * s.L);
    v.de = b.take((size_t)s.R * M);
    v.part = b.take((size_t)chunks(s.R) * 2 * M);
    v.w3 = b.take((size_t)s.L * (M + 1));
    v.w0 = b.take((size_t)M * (s.L + 1));
    v.total = b.off;
    return v;
}

// ---- tdmpc_lg_gemm jobs
tdmpc_lg_seg seg(const float* a, int lda, const float* b, int ldb, int k, int amode, int bmode, int ones = -1) {
    tdmpc_lg_seg s;
    memset(&s, 0, sizeof s);
    s.a = a; s.b = b; s.lda = lda; s.ldb = ldb; s.k = k; s.amode = amode; s.bmode = bmode; s.ones_col = ones;
    return s;
}

tdmpc_lg_job job(int m, int n, float* c, int ldc, const tdmpc_lg_seg& s0) {
    tdmpc_lg_job j;
    memset(&j, 0, sizeof j);
    j.seg[0] = s0;
    j.nseg = 1; j.m = m; j.n = n; j.c = c; j.ldc = ldc; j.splits = 1; j.epi = TDMPC_LG_EPI_NONE;
    return j;
}

// Y [R,N] = X [R,K] W [N,K]^T (+ bias)
tdmpc_lg_job linear(int R, int N, int K, const float* x, const float* w, const float* bias, float* y) {
    tdmpc_lg_job j = job(R, N, y, N, seg(x, K, w, K, K, 0, 0));
    j.bias = bias;
    return j;
}
// dX [R,K] = dY [R,N] W [N,K], columns [c0, c0 + n) of W (row stride ldw)
tdmpc_lg_job dinput(int R, int n, int N, const float* dy, const float* w, int ldw, float* dx) {
    return job(R, n, dx, n, seg(dy, N, w, ldw, N, 0, 1));
}
// dW [N,n] (row stride ldc) = dY [R,N]^T X [R,n]; ones: the bias column n (then ldc = n + 1 columns are written)
tdmpc_lg_job dweight(int R, int N, int n, const float* dy, const float* x, float* dw, int ldc, bool ones) {
    return job(N, ones ? n + 1 : n, dw, ldc, seg(dy, N, x, n, R, 1, 1, ones ? n : -1));
}
tdmpc_lg_job with_elu_bwd(tdmpc_lg_job j, const float* y) {
    j.epi = TDMPC_LG_EPI_ELU_BWD;
    j.aux = y;
    j.ldaux = j.n;
    return j;
}

// One grouped launch on the exact f32 MFMA: 64 x 64 register tiles once the largest job fills the chip with them.
// tile_rows > 0: choose the tile as for jobs of that many rows (the two tiles sum K in different orders; the segmented
// pass keeps the bits of a one-segment call).
// tile_cols > 0 likewise: as if the widest job of the launch had that many columns (a product that shares its launch
// with a wider one in tdmpc_drnn_next_fwd).
int gemm(const tdmpc_lg_job* jobs, int n, void* stream, int tile_rows = 0, int tile_cols = 0) {
    long big = 0;
    for (int q = 0; q < n; ++q)
        big = std::max(big, (long)(((tile_rows ? tile_rows : jobs[q].m) + 63) / 64) *
                                (((tile_cols ? tile_cols : jobs[q].n) + 63) / 64));
    return tdmpc_lg_gemm(jobs, n, (big >= 256 ? 2 : 1) | TDMPC_LG_TILE_EXACT, stream);
}

int bn_forward(BnArgs a, hipStream_t st) {
    if (!a.seg) { a.seg = a.rows; a.nseg = 1; }
    const dim3 g(a.C / 64, chunks(a.seg) * a.nseg);
    hipLaunchKernelGGL(dt_bn_stat, g, dim3(256), 0, st, a);
    if (int rc = launched("bn_stat")) return rc;
    hipLaunchKernelGGL(dt_bn_fwd, g, dim3(256), 0, st, a);
    return launched("bn_fwd");
}

int bn_backward(BnArgs a, hipStream_t st) {
    const dim3 g(a.C / 64, chunks(a.rows));
    hipLaunchKernelGGL(dt_bn_bwd_stat, g, dim3(256), 0, st, a);
    if (int rc = launched("bn_bwd_stat")) return rc;
    hipLaunchKernelGGL(dt_bn_bwd, g, dim3(256), 0, st, a);
    return launched("bn_bwd");
}

int unpack(const UnpackArgs& u, int n, hipStream_t st) {
    hipLaunchKernelGGL(dt_unpack, dim3(64, n), dim3(256), 0, st, u);
    return launched("unpack");
}

int need(const void* p, const char* name) {
    if (p) return 0;
    char msg[128];
    snprintf(msg, sizeof msg, "drnn_learner: %s is null", name);
    tdmpc_internal::set_error(msg);
    return TDMPC_E_DIMS;
}

int need_table(float* const* t, int n, int want, const char* name, bool stats) {
    if (int rc = need(t, name)) return rc;
    if (n != want) return bad("drnn_learner: %ld tensors given, %ld expected", n, want);
    for (int i = 0; i < want; ++i)
        if (!t[i] && (stats || (i != P1RM && i != P1RV))) return bad("drnn_learner: tensor %ld of a table is null", i);
    return 0;
}

int size_err(const char* what, size_t have, size_t want) {
    char msg[160];
    snprintf(msg, sizeof msg, "drnn_learner: %s holds %zu floats, %zu needed", what, have, want);
    tdmpc_internal::set_error(msg);
    return TDMPC_E_SIZE;
}

// tdmpc_drnn_intrinsic_fwd's workspace: what next_fwd and simloss_fwd save or stage, all scratch here. s.R = S * B rows.
struct IntrWs { float *gi, *gate, *lnx, *lnr, *hn, *p1, *bnx, *bnr, *e, *part, *zo, *pred; size_t total; };
IntrWs intr_ws(const Shape& s, int segments, int seg_rows, float* base) {
    Bump b(base);
    IntrWs v;
    const size_t R = s.R;
    v.gi = b.take(R * 3 * s.Hd);
    v.gate = b.take(R * 3 * s.Hd);
    v.lnx = b.take(R * 3 * s.Hd);
    v.lnr = b.take(R * 4);
    v.hn = b.take(R * s.Hd);
    v.p1 = b.take(R * M);
    v.bnx = b.take(R * M);
    v.bnr = b.take((size_t)segments * M);
    v.e = b.take(R * M);
    v.part = b.take((size_t)segments * chunks(seg_rows) * 2 * M);
    v.zo = b.take(R * s.L);
    v.pred = b.take(R * s.L);
    v.total = b.off;
    return v;
}

int check_segments(const tdmpc_drnn_dims* d, int segments, int seg_rows, Shape& s) {
    if (segments < 1 || seg_rows < 2 || (long)segments * seg_rows > TDMPC_DT_MAX_ROWS)
        return bad("drnn_learner: %ld segments of %ld rows (at least 1 of at least 2 rows, 4096 rows in all)", segments,
                   seg_rows);
    return check_shape(d, segments * seg_rows, s);
}

bool loss_args_ok(const tdmpc_drnn_loss_args* a) {
    return a && a->sim && a->q1 && a->q2 && a->rp && a->rw && a->rwpi && a->nq && a->w && a->H > 0 && a->B > 0;
}

// tdmpc_drnn_intrinsic_chain_fwd's workspace. hn comes first (tdmpc_drnn_learner.h promises it). gh / gate / lnx / lnr
// hold one step of seg_rows rows (the launch chain's dt_gate_fwd writes them; nothing reads them back).
struct ChainWs { float *hn, *gi, *gh, *gate, *lnx, *lnr, *p1, *bnx, *bnr, *e, *part, *zo, *pred; size_t total; };
ChainWs chain_ws(const Shape& s, int segments, int seg_rows, float* base) {
    Bump b(base);
    ChainWs v;
    const size_t R = s.R, B = seg_rows;
    v.hn = b.take(R * s.Hd);
    v.gi = b.take(R * 3 * s.Hd);
    v.gh = b.take(B * 3 * s.Hd);
    v.gate = b.take(B * 3 * s.Hd);
    v.lnx = b.take(B * 3 * s.Hd);
    v.lnr = b.take(B * 4);
    v.p1 = b.take(R * M);
    v.bnx = b.take(R * M);
    v.bnr = b.take((size_t)segments * M);
    v.e = b.take(R * M);
    v.part = b.take((size_t)segments * chunks(seg_rows) * 2 * M);
    v.zo = b.take(R * s.L);
    v.pred = b.take(R * s.L);
    v.total = b.off;
    return v;
}

int check_chain(const tdmpc_drnn_dims* d, int segments, int seg_rows, int warm, Shape& s) {
    if (int rc = check_segments(d, segments, seg_rows, s)) return rc;
    if (warm < 0 || warm >= segments)
        return bad("drnn_learner: warm %ld is not in [0, segments = %ld)", warm, segments);
    return 0;
}

bool sim_loss_args_ok(const tdmpc_drnn_sim_loss_args* a) {
    return a && a->sim && a->q1 && a->q2 && a->rp && a->rw && a->rwpi && a->nq && a->w && a->B > 0 && a->W >= 1 &&
           a->W < a->H;
}

StepLossArgs sim_step_args(const tdmpc_drnn_sim_loss_args* a) {
    return StepLossArgs{a->sim, a->q1, a->q2, a->rp, a->rw, a->rwpi, a->nq, a->w, a->H, a->H - a->W, a->B,
                        a->sim_coef, a->reward_coef, a->value_coef, a->discount, 1.0};
}

// The one-step loss family's launches over checked args (tdmpc_drnn_sim_loss_*, tdmpc_icem_loss_* and, with TDIN,
// tdmpc_sim_loss_*).
template <bool RHO, bool TDIN = false>
int step_loss_forward(const StepLossArgs& a, float* td, float* rows, float* scal, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((sl_loss_rows<RHO, TDIN>), dim3((a.B + 255) / 256), dim3(256), 0, st, a, td, rows);
    if (int rc = launched("step loss_rows")) return rc;
    hipLaunchKernelGGL(sl_loss_means, dim3(1), dim3(512), 0, st, rows, a.w, a.B, scal);
    return launched("step loss_means");
}

template <bool RHO, bool HOOK>
int step_loss_backward(const StepLossArgs& a, const float* td, const float* rows, const float* scal, const float* gw,
                       float* dsim, float* dq1, float* dq2, float* drp, void* stream) {
    const long n = (long)a.H * a.B;
    hipLaunchKernelGGL((sl_loss_bwd<RHO, HOOK>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                       td, rows, scal, gw, dsim, dq1, dq2, drp);
    return launched("step loss_bwd");
}

// `_predictor` on x [R, L] and the cosine loss against keys -> loss [R]: Linear, BatchNorm on batch statistics (over
// `nseg` segments of `seg` rows each, or over all R rows when seg is 0) + ELU, Linear, dt_cos_fwd. P: the loss table
// (its first eight slots; the running statistics move). tile_rows: gemm's row-block argument of the caller.
struct PredictorBufs { float *p1, *bnx, *bnr, *e, *part, *pred; };   // [R, M], [R, M], [nseg, M], [R, M], partials, [R, L]
int predictor_fwd(float* const* P, const float* x, const float* keys, float* loss, int R, int L, int seg, int nseg,
                  int tile_rows, const PredictorBufs& w, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    tdmpc_lg_job j = linear(R, M, L, x, P[P0W], P[P0B], w.p1);
    if (int rc = gemm(&j, 1, stream, tile_rows)) return rc;
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = w.p1; b.g = P[P1G]; b.b = P[P1B]; b.rmean = P[P1RM]; b.rvar = P[P1RV];
    b.xhat = w.bnx; b.rstd = w.bnr; b.e = w.e; b.part = w.part; b.rows = R; b.C = M;
    b.seg = seg; b.nseg = nseg;
    if (int rc = bn_forward(b, st)) return rc;
    j = linear(R, L, M, w.e, P[P3W], P[P3B], w.pred);
    if (int rc = gemm(&j, 1, stream, tile_rows)) return rc;
    hipLaunchKernelGGL(dt_cos_fwd, dim3((R + 3) / 4), dim3(256), 0, st, w.pred, keys, loss, R, L);
    return launched("cos_fwd");
}

// similarity_loss forward and backward over a checked shape (tdmpc_drnn_simloss_* and, behind the planner's tdmpc_dims,
// tdmpc_icem_simloss_*: the hidden width plays no part in them).
int simloss_fwd(const Shape& s, float* const* T, int32_t n_tensors, const float* queries, const float* keys,
                float* loss, float* saved, size_t saved_floats, float* workspace, size_t workspace_floats,
                void* stream) {
    if (int rc = need_table(T, n_tensors, TDMPC_DT_LOSS_TENSORS, "tensors", true)) return rc;
    const void* ptrs[] = {queries, keys, loss, saved, workspace};
    const char* names[] = {"queries", "keys", "loss", "saved", "workspace"};
    for (int i = 0; i < 5; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const LossSaved S = loss_saved(s, saved);
    const LossFwdWs W = loss_fwd_ws(s, workspace);
    if (saved_floats < S.total) return size_err("saved", saved_floats, S.total);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    return predictor_fwd(T, queries, keys, loss, s.R, s.L, 0, 0, 0, PredictorBufs{W.p1, S.bnx, S.bnr, S.e, W.part, S.pred},
                         stream);
}

int simloss_bwd(const Shape& s, float* const* T, int32_t n_tensors, const float* queries, const float* keys,
                const float* saved, size_t saved_floats, const float* dloss, float* dqueries, float* const* G,
                float* workspace, size_t workspace_floats, void* stream) {
    if (int rc = need_table(T, n_tensors, TDMPC_DT_LOSS_TENSORS, "tensors", true)) return rc;
    if (int rc = need_table(G, n_tensors, TDMPC_DT_LOSS_TENSORS, "grads", false)) return rc;
    const void* ptrs[] = {queries, keys, saved, dloss, workspace};
    const char* names[] = {"queries", "keys", "saved", "dloss", "workspace"};
    for (int i = 0; i < 5; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const LossSaved S = loss_saved(s, const_cast<float*>(saved));
    const LossBwdWs W = loss_bwd_ws(s, workspace);
    if (saved_floats < S.total) return size_err("saved", saved_floats, S.total);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L;

    hipLaunchKernelGGL(dt_cos_bwd, dim3((R + 3) / 4), dim3(256), 0, st, S.pred, keys, dloss, W.dpred, R, L);
    if (int rc = launched("cos_bwd")) return rc;
    tdmpc_lg_job j[3];
    j[0] = dinput(R, M, L, W.dpred, T[P3W], M, W.de);
    if (int rc = gemm(j, 1, stream)) return rc;
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.de; b.g = T[P1G]; b.xhat = S.bnx; b.rstd = S.bnr; b.e = S.e; b.part = W.part;
    b.dx = W.de; b.dg = G[P1G]; b.db = G[P1B]; b.rows = R; b.C = M;
    if (int rc = bn_backward(b, st)) return rc;
    int n = 0;
    if (dqueries) j[n++] = dinput(R, L, M, W.de, T[P0W], L, dqueries);
    j[n++] = dweight(R, L, M, W.dpred, S.e, W.w3, M + 1, true);
    j[n++] = dweight(R, M, L, W.de, queries, W.w0, L + 1, true);
    if (int rc = gemm(j, n, stream)) return rc;
    UnpackArgs u;
    memset(&u, 0, sizeof u);
    u.job[0] = UnpackJob{W.w3, G[P3W], G[P3B], L, M};
    u.job[1] = UnpackJob{W.w0, G[P0W], G[P0B], M, L};
    return unpack(u, 2, st);
}

}  // namespace

extern "C" {

int tdmpc_drnn_intrinsic_workspace_floats(const tdmpc_drnn_dims* dims, int32_t segments, int32_t seg_rows,
                                          size_t* out) {
    Shape s;
    if (int rc = check_segments(dims, segments, seg_rows, s)) return rc;
    if (int rc = need(out, "out")) return rc;
    *out = intr_ws(s, segments, seg_rows, nullptr).total;
    return 0;
}

int tdmpc_drnn_intrinsic_fwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_next, float* const* P,
                             int32_t n_loss, const float* z, const float* a, const float* keys, int32_t segments,
                             int32_t seg_rows, float* loss, float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_segments(dims, segments, seg_rows, s)) return rc;
    if (int rc = need_table(T, n_next, TDMPC_DT_NEXT_TENSORS, "next_tensors", true)) return rc;
    if (int rc = need_table(P, n_loss, TDMPC_DT_LOSS_TENSORS, "loss_tensors", true)) return rc;
    const void* ptrs[] = {z, a, keys, loss, workspace};
    const char* names[] = {"z", "a", "keys", "loss", "workspace"};
    for (int i = 0; i < 5; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const IntrWs W = intr_ws(s, segments, seg_rows, workspace);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L, A = s.A, Hd = s.Hd;

    // next from h = 0: weight_hh(h) = 0, so only [z | a] weight_ih^T is a product
    tdmpc_lg_job j = job(R, 3 * Hd, W.gi, 3 * Hd, seg(z, L, T[WIH], L + A, L, 0, 0));
    j.seg[1] = seg(a, A, T[WIH] + L, L + A, A, 0, 0);
    j.nseg = 2;
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    GateArgs g;
    memset(&g, 0, sizeof g);
    g.gi = W.gi;
    for (int k = 0; k < 3; ++k) { g.g[k] = T[LRG + 2 * k]; g.b[k] = T[LRB + 2 * k]; }
    g.gate = W.gate; g.lnx = W.lnx; g.lnr = W.lnr; g.hn = W.hn; g.h_out = W.hn;
    g.rows = R; g.Hd = Hd;
    hipLaunchKernelGGL(dt_gate_fwd<true>, dim3((R + 3) / 4), dim3(256), 0, st, g);
    if (int rc = launched("gate_fwd")) return rc;
    j = linear(R, M, Hd, W.hn, T[P0W], T[P0B], W.p1);
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.p1; b.g = T[P1G]; b.b = T[P1B]; b.rmean = T[P1RM]; b.rvar = T[P1RV];
    b.xhat = W.bnx; b.rstd = W.bnr; b.e = W.e; b.part = W.part; b.rows = R; b.C = M;
    b.seg = seg_rows; b.nseg = segments;
    if (int rc = bn_forward(b, st)) return rc;
    j = linear(R, L, M, W.e, T[P3W], T[P3B], W.zo);
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;

    // similarity_loss(z', keys): the predictor's table has the same layout as prior_mlp's first eight slots
    return predictor_fwd(P, W.zo, keys, loss, R, L, seg_rows, segments, seg_rows,
                         PredictorBufs{W.p1, W.bnx, W.bnr, W.e, W.part, W.pred}, stream);
}

int tdmpc_drnn_intrinsic_finish(const float* loss, int32_t n, double* rms, const float* coef, const float* reward,
                                float* intrinsic, float* reward_pi, void* stream) {
    if (n < 1 || n > TDMPC_DT_MAX_ROWS) return bad("drnn_learner: intrinsic_finish over %ld values (1..4096)", n);
    const void* ptrs[] = {loss, rms, coef, reward, intrinsic, reward_pi};
    const char* names[] = {"loss", "rms", "coef", "reward", "intrinsic", "reward_pi"};
    for (int i = 0; i < 6; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    hipLaunchKernelGGL(dt_intrinsic_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, loss, n, rms, coef, reward,
                       intrinsic, reward_pi);
    return launched("intrinsic_finish");
}

int tdmpc_drnn_loss_forward(const tdmpc_drnn_loss_args* a, float* td, float* rows, float* scal, void* stream) {
    if (!loss_args_ok(a) || !td || !rows || !scal) return bad("drnn_learner: loss_forward: a null pointer or H, B < 1");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dt_loss_rows, dim3((a->B + 255) / 256), dim3(256), 0, st, *a, td, rows);
    if (int rc = launched("loss_rows")) return rc;
    hipLaunchKernelGGL(dt_loss_means, dim3(1), dim3(512), 0, st, *a, rows, scal);
    return launched("loss_means");
}

int tdmpc_drnn_loss_backward(const tdmpc_drnn_loss_args* a, const float* td, const float* rows, const float* scal,
                             const float* gw, float* dsim, float* dq1, float* dq2, float* drp, void* stream) {
    if (!loss_args_ok(a) || !td || !rows || !scal || !gw)
        return bad("drnn_learner: loss_backward: a null pointer or H, B < 1");
    const long n = (long)a->H * a->B;
    hipLaunchKernelGGL(dt_loss_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a, td, rows,
                       scal, gw, dsim, dq1, dq2, drp);
    return launched("loss_bwd");
}

int tdmpc_drnn_intrinsic_chain_workspace_floats(const tdmpc_drnn_dims* dims, int32_t segments, int32_t seg_rows,
                                                size_t* out) {
    Shape s;
    if (int rc = check_segments(dims, segments, seg_rows, s)) return rc;
    if (int rc = need(out, "out")) return rc;
    *out = chain_ws(s, segments, seg_rows, nullptr).total;
    return 0;
}

int tdmpc_drnn_intrinsic_chain_fwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_next, float* const* P,
                                   int32_t n_loss, const float* z, const float* a, const float* keys, int32_t segments,
                                   int32_t seg_rows, int32_t warm, int32_t mode, float* loss, float* h_out,
                                   float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_chain(dims, segments, seg_rows, warm, s)) return rc;
    if (mode != 0 && mode != 1) return bad("drnn_learner: intrinsic_chain_fwd mode %ld (0: launch chain, 1: one launch)", mode);
    if (int rc = need_table(T, n_next, TDMPC_DT_NEXT_TENSORS, "next_tensors", true)) return rc;
    if (int rc = need_table(P, n_loss, TDMPC_DT_LOSS_TENSORS, "loss_tensors", true)) return rc;
    const void* ptrs[] = {z, a, keys, loss, h_out, workspace};
    const char* names[] = {"z", "a", "keys", "loss", "h_out", "workspace"};
    for (int i = 0; i < 6; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const ChainWs W = chain_ws(s, segments, seg_rows, workspace);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L, A = s.A, Hd = s.Hd, S = segments, B = seg_rows;

    // 1: [z | a] weight_ih^T of all S B rows (the inputs do not depend on the hidden state)
    tdmpc_lg_job j = job(R, 3 * Hd, W.gi, 3 * Hd, seg(z, L, T[WIH], L + A, L, 0, 0));
    j.seg[1] = seg(a, A, T[WIH] + L, L + A, A, 0, 0);
    j.nseg = 2;
    if (int rc = gemm(&j, 1, stream, B)) return rc;

    // 2: the recurrence, h_0 = 0
    if (mode == 1) {
        ChainArgs c;
        memset(&c, 0, sizeof c);
        c.gi = W.gi; c.whh = T[WHH]; c.hn = W.hn; c.S = S; c.B = B; c.Hd = Hd;
        for (int k = 0; k < 3; ++k) { c.g[k] = T[LRG + 2 * k]; c.b[k] = T[LRB + 2 * k]; }
        const size_t lds = (size_t)CROWS * (Hd + 4 + 3 * Hd + 4) * sizeof(float);   // 64.5 KB at Hd = 256
        static bool attr = false;
        if (!attr) {
            if (hipFuncSetAttribute((const void*)dt_gru_chain, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
                hipSuccess)
                return launched("gru_chain (LDS attribute)");
            attr = true;
        }
        hipLaunchKernelGGL(dt_gru_chain, dim3((B + CROWS - 1) / CROWS), dim3(64 * CWAVES), lds, st, c);
        if (int rc = launched("gru_chain")) return rc;
    } else {
        GateArgs g;
        memset(&g, 0, sizeof g);
        for (int k = 0; k < 3; ++k) { g.g[k] = T[LRG + 2 * k]; g.b[k] = T[LRB + 2 * k]; }
        g.gate = W.gate; g.lnx = W.lnx; g.lnr = W.lnr; g.rows = B; g.Hd = Hd;
        for (int t = 0; t < S; ++t) {
            float* hn = W.hn + (size_t)t * B * Hd;
            g.gi = W.gi + (size_t)t * B * 3 * Hd;
            g.hn = hn; g.h_out = hn;
            if (t == 0) {
                hipLaunchKernelGGL(dt_gate_fwd<true>, dim3((B + 3) / 4), dim3(256), 0, st, g);
            } else {
                g.h = hn - (size_t)B * Hd;
                g.gh = W.gh;
                j = linear(B, 3 * Hd, Hd, g.h, T[WHH], nullptr, W.gh);
                if (int rc = gemm(&j, 1, stream)) return rc;
                hipLaunchKernelGGL(dt_gate_fwd<false>, dim3((B + 3) / 4), dim3(256), 0, st, g);
            }
            if (int rc = launched("gate_fwd")) return rc;
        }
    }
    if (hipMemcpyAsync(h_out, W.hn + (size_t)(S - 1) * B * Hd, (size_t)B * Hd * sizeof(float), hipMemcpyDeviceToDevice,
                       st) != hipSuccess)
        return launched("memcpy");

    // 3: prior_mlp over every segment (the warm-up steps move its BatchNorm's running statistics too)
    j = linear(R, M, Hd, W.hn, T[P0W], T[P0B], W.p1);
    if (int rc = gemm(&j, 1, stream, B)) return rc;
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.p1; b.g = T[P1G]; b.b = T[P1B]; b.rmean = T[P1RM]; b.rvar = T[P1RV];
    b.xhat = W.bnx; b.rstd = W.bnr; b.e = W.e; b.part = W.part; b.rows = R; b.C = M;
    b.seg = B; b.nseg = S;
    if (int rc = bn_forward(b, st)) return rc;

    // 4: prior_mlp.3, _predictor and the cosine loss over segments warm .. S - 1
    const int R2 = (S - warm) * B;
    const size_t o = (size_t)warm * B;
    if (warm && hipMemsetAsync(loss, 0, o * sizeof(float), st) != hipSuccess) return launched("memset");
    j = linear(R2, L, M, W.e + o * M, T[P3W], T[P3B], W.zo);
    if (int rc = gemm(&j, 1, stream, B, M)) return rc;   // (next_fwd launches it beside _reward.2, M columns)
    return predictor_fwd(P, W.zo, keys + o * L, loss + o, R2, L, B, S - warm, B,
                         PredictorBufs{W.p1, W.bnx, W.bnr, W.e, W.part, W.pred}, stream);
}

int tdmpc_drnn_sim_loss_forward(const tdmpc_drnn_sim_loss_args* a, float* td, float* rows, float* scal, void* stream) {
    if (!sim_loss_args_ok(a) || !td || !rows || !scal)
        return bad("drnn_learner: sim_loss_forward: a null pointer, B < 1 or W outside [1, H - 1]");
    return step_loss_forward<false>(sim_step_args(a), td, rows, scal, stream);
}

int tdmpc_drnn_sim_loss_backward(const tdmpc_drnn_sim_loss_args* a, const float* td, const float* rows,
                                 const float* scal, const float* gw, float* dsim, float* dq1, float* dq2, float* drp,
                                 void* stream) {
    if (!sim_loss_args_ok(a) || !td || !rows || !scal || !gw)
        return bad("drnn_learner: sim_loss_backward: a null pointer, B < 1 or W outside [1, H - 1]");
    return step_loss_backward<false, false>(sim_step_args(a), td, rows, scal, gw, dsim, dq1, dq2, drp, stream);
}

int tdmpc_drnn_train_version(void) { return TDMPC_DRNN_TRAIN_VERSION; }

int tdmpc_drnn_train_sizes_for(const tdmpc_drnn_dims* dims, int32_t rows, tdmpc_drnn_train_sizes* out) {
    Shape s;
    if (int rc = check_shape(dims, rows, s)) return rc;
    if (int rc = need(out, "out")) return rc;
    out->next_saved_floats = next_saved(s, nullptr).total;
    out->loss_saved_floats = loss_saved(s, nullptr).total;
    out->workspace_floats = std::max(std::max(next_fwd_ws(s, nullptr).total, next_bwd_ws(s, nullptr).total),
                                     std::max(loss_fwd_ws(s, nullptr).total, loss_bwd_ws(s, nullptr).total));
    return 0;
}

int tdmpc_drnn_next_fwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_tensors, const float* z,
                        const float* a, const float* h, int32_t rows, float* z_out, float* h_out, float* r_out,
                        float* saved, size_t saved_floats, float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_shape(dims, rows, s)) return rc;
    if (int rc = need_table(T, n_tensors, TDMPC_DT_NEXT_TENSORS, "tensors", true)) return rc;
    const void* ptrs[] = {z, a, h, z_out, h_out, r_out, saved, workspace};
    const char* names[] = {"z", "a", "h", "z_out", "h_out", "r_out", "saved", "workspace"};
    for (int i = 0; i < 8; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const NextSaved S = next_saved(s, saved);
    const NextFwdWs W = next_fwd_ws(s, workspace);
    if (saved_floats < S.total) return size_err("saved", saved_floats, S.total);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L, A = s.A, Hd = s.Hd;

    tdmpc_lg_job j[2];
    // the gate products: [z | a] weight_ih^T as two K segments, h weight_hh^T
    j[0] = job(R, 3 * Hd, W.gi, 3 * Hd, seg(z, L, T[WIH], L + A, L, 0, 0));
    j[0].seg[1] = seg(a, A, T[WIH] + L, L + A, A, 0, 0);
    j[0].nseg = 2;
    j[1] = linear(R, 3 * Hd, Hd, h, T[WHH], nullptr, S.gh);
    if (int rc = gemm(j, 2, stream)) return rc;

    GateArgs g;
    memset(&g, 0, sizeof g);
    g.gi = W.gi; g.gh = S.gh; g.h = h;
    for (int k = 0; k < 3; ++k) { g.g[k] = T[LRG + 2 * k]; g.b[k] = T[LRB + 2 * k]; }
    g.gate = S.gate; g.lnx = S.lnx; g.lnr = S.lnr; g.hn = S.hn; g.h_out = h_out;
    g.rows = R; g.Hd = Hd;
    hipLaunchKernelGGL(dt_gate_fwd<false>, dim3((R + 3) / 4), dim3(256), 0, st, g);
    if (int rc = launched("gate_fwd")) return rc;

    j[0] = linear(R, M, Hd, S.hn, T[P0W], T[P0B], W.p1);
    j[1] = linear(R, M, Hd, S.hn, T[R0W], T[R0B], S.q1);
    j[1].epi = TDMPC_LG_EPI_ELU;
    if (int rc = gemm(j, 2, stream)) return rc;

    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.p1; b.g = T[P1G]; b.b = T[P1B]; b.rmean = T[P1RM]; b.rvar = T[P1RV];
    b.xhat = S.bnx; b.rstd = S.bnr; b.e = S.e; b.part = W.part; b.rows = R; b.C = M;
    if (int rc = bn_forward(b, st)) return rc;

    j[0] = linear(R, L, M, S.e, T[P3W], T[P3B], z_out);
    j[1] = linear(R, M, M, S.q1, T[R2W], T[R2B], S.q2);
    j[1].epi = TDMPC_LG_EPI_ELU;
    if (int rc = gemm(j, 2, stream)) return rc;

    j[0] = linear(R, 1, M, S.q2, T[R4W], T[R4B], r_out);
    return gemm(j, 1, stream);
}

int tdmpc_drnn_next_bwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_tensors, const float* z,
                        const float* a, const float* h, int32_t rows, const float* saved, size_t saved_floats,
                        const float* dz_out, const float* dh_out, const float* dr_out, float* dz, float* da, float* dh,
                        float* const* G, float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_shape(dims, rows, s)) return rc;
    if (int rc = need_table(T, n_tensors, TDMPC_DT_NEXT_TENSORS, "tensors", true)) return rc;
    if (int rc = need_table(G, n_tensors, TDMPC_DT_NEXT_TENSORS, "grads", false)) return rc;
    const void* ptrs[] = {z, a, h, saved, workspace};
    const char* names[] = {"z", "a", "h", "saved", "workspace"};
    for (int i = 0; i < 5; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const NextSaved S = next_saved(s, const_cast<float*>(saved));
    const NextBwdWs W = next_bwd_ws(s, workspace);
    if (saved_floats < S.total) return size_err("saved", saved_floats, S.total);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L, A = s.A, Hd = s.Hd;

    // an absent upstream gradient is a zero one
    if (!dz_out) {
        if (hipMemsetAsync(W.zz, 0, (size_t)R * L * sizeof(float), st) != hipSuccess) return launched("memset");
        dz_out = W.zz;
    }
    if (!dr_out) {
        if (hipMemsetAsync(W.zr, 0, (size_t)R * sizeof(float), st) != hipSuccess) return launched("memset");
        dr_out = W.zr;
    }

    tdmpc_lg_job j[12];
    // dq2 = (dr w4) ELU'(q2); de = dz' W3
    j[0] = with_elu_bwd(dinput(R, M, 1, dr_out, T[R4W], M, W.dq2), S.q2);
    j[1] = dinput(R, M, L, dz_out, T[P3W], M, W.de);
    if (int rc = gemm(j, 2, stream)) return rc;

    // prior_mlp.2 / .1 backward: de becomes the gradient at prior_mlp.0's output
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.de; b.g = T[P1G]; b.xhat = S.bnx; b.rstd = S.bnr; b.e = S.e; b.part = W.bnpart;
    b.dx = W.de; b.dg = G[P1G]; b.db = G[P1B]; b.rows = R; b.C = M;
    if (int rc = bn_backward(b, st)) return rc;

    j[0] = with_elu_bwd(dinput(R, M, M, W.dq2, T[R2W], M, W.dq1), S.q1);
    if (int rc = gemm(j, 1, stream)) return rc;

    // dL/dh' = dh'(upstream) + dp1 W_p0 + dq1 W_r0
    j[0] = dinput(R, Hd, M, W.de, T[P0W], Hd, W.dhn);
    j[0].seg[1] = seg(W.dq1, M, T[R0W], Hd, M, 0, 1);
    j[0].nseg = 2;
    if (dh_out) { j[0].res = dh_out; j[0].ldres = Hd; }
    if (int rc = gemm(j, 1, stream)) return rc;

    GateArgs g;
    memset(&g, 0, sizeof g);
    g.gh = S.gh; g.h = h;
    for (int k = 0; k < 3; ++k) g.g[k] = T[LRG + 2 * k];
    g.gate = S.gate; g.lnx = S.lnx; g.lnr = S.lnr;
    g.dhn = W.dhn; g.dgi = W.dgi; g.dgh = W.dgh; g.dhd = W.dhd; g.part = W.lnpart;
    g.rows = R; g.Hd = Hd;
    hipLaunchKernelGGL(dt_gate_bwd<false>, dim3(gate_wgs(R)), dim3(256), 0, st, g);
    if (int rc = launched("gate_bwd")) return rc;
    FinishArgs f;
    memset(&f, 0, sizeof f);
    f.part = W.lnpart; f.nparts = gate_wgs(R); f.nvec = 6; f.C = Hd;
    for (int k = 0; k < 6; ++k) f.out[k] = G[LRG + k];
    hipLaunchKernelGGL(dt_finish, dim3((6 * Hd + 255) / 256), dim3(256), 0, st, f);
    if (int rc = launched("finish")) return rc;

    // the input gradients and every weight gradient, one launch
    int n = 0;
    if (dz) j[n++] = dinput(R, L, 3 * Hd, W.dgi, T[WIH], L + A, dz);
    if (da) j[n++] = dinput(R, A, 3 * Hd, W.dgi, T[WIH] + L, L + A, da);
    if (dh) {
        j[n] = dinput(R, Hd, 3 * Hd, W.dgh, T[WHH], Hd, dh);
        j[n].res = W.dhd;
        j[n++].ldres = Hd;
    }
    j[n++] = dweight(R, 3 * Hd, L, W.dgi, z, G[WIH], L + A, false);
    j[n++] = dweight(R, 3 * Hd, A, W.dgi, a, G[WIH] + L, L + A, false);
    j[n++] = dweight(R, 3 * Hd, Hd, W.dgh, h, G[WHH], Hd, false);
    j[n++] = dweight(R, M, Hd, W.de, S.hn, W.wp0, Hd + 1, true);
    j[n++] = dweight(R, L, M, dz_out, S.e, W.wp3, M + 1, true);
    j[n++] = dweight(R, M, Hd, W.dq1, S.hn, W.wr0, Hd + 1, true);
    j[n++] = dweight(R, M, M, W.dq2, S.q1, W.wr2, M + 1, true);
    j[n++] = dweight(R, 1, M, dr_out, S.q2, W.wr4, M + 1, true);
    if (int rc = gemm(j, n, stream)) return rc;

    UnpackArgs u;
    memset(&u, 0, sizeof u);
    u.job[0] = UnpackJob{W.wp0, G[P0W], G[P0B], M, Hd};
    u.job[1] = UnpackJob{W.wp3, G[P3W], G[P3B], L, M};
    u.job[2] = UnpackJob{W.wr0, G[R0W], G[R0B], M, Hd};
    u.job[3] = UnpackJob{W.wr2, G[R2W], G[R2B], M, M};
    u.job[4] = UnpackJob{W.wr4, G[R4W], G[R4B], 1, M};
    return unpack(u, 5, st);
}

int tdmpc_drnn_simloss_fwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, float* loss, float* saved, size_t saved_floats,
                           float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_shape(dims, rows, s)) return rc;
    return simloss_fwd(s, T, n_tensors, queries, keys, loss, saved, saved_floats, workspace, workspace_floats, stream);
}

int tdmpc_drnn_simloss_bwd(const tdmpc_drnn_dims* dims, float* const* T, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, const float* saved, size_t saved_floats,
                           const float* dloss, float* dqueries, float* const* G, float* workspace,
                           size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_shape(dims, rows, s)) return rc;
    return simloss_bwd(s, T, n_tensors, queries, keys, saved, saved_floats, dloss, dqueries, G, workspace,
                       workspace_floats, stream);
}

}  // extern "C"

#include "icem_learner.inc"
#include "sim_learner.inc"
#include "drnn_engine.inc"
