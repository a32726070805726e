// drnn.inc -- the recurrent-latent (DSSM) rollout step for gfx950 and its C ABI (include/tdmpc_drnn.h).
// Included twice from tdmpc_kernels.hip: once beside plan1.inc / wide_step.inc for the device code (it shares the x6
// helpers and the row-block idiom of chain_kernel), once at the end of the file (DRNN_HOST) for the host side, which
// shares Ctx, the pack table and the profiler. The planning algorithms' launch sequences are not here: the CEM plan,
// the iCEM plan, estimate_value and the policy pre-rollout are tdmpc_kernels.hip's drivers (cem_run, icem_run,
// estimate_value_run, pi_rollout_run), which this file instantiates with its own step (DrnnStep); its entry points
// keep the setup, the z_out copy and the final DSSM.next for hidden_out.
//
// Reference: DSSM.next (src/algorithm/tdmpc_similarity_drnn.py:57-60) = DGruDyna (models/gru_dyna.py:25-29: a
// NormGRUCell over [z, a], then prior_mlp = Linear - BatchNorm1d - ELU - Linear on the new hidden) and the reward MLP
// on the new hidden; NormGRUCell.forward is models/rnns.py:19-29.
//
// drnn_step_kernel: one launch per rollout step. A workgroup of 8 waves owns 32 rows and keeps their activations in
// LDS from layer to layer (fp32 [K/4][32][4] blocks, the x6 B operand of ring6_run); products are the x6 form
// (fp32 = three bf16 planes, six v_mfma_f32_32x32x16_bf16 per 16 k). Per block:
//   1. stage [a | z] (the X_t panel) and h; BatchNorm's running statistics become a per-column scale / shift
//   2. gates: wave b < Hd / 32 owns hidden features [32 b, 32 b + 32) of all three gates: W_ih [a | z] and W_hh h
//      accumulate into the same tiles for reset / update; the new-value gate keeps its two parts apart
//   3. the three row LayerNorms (eps 1e-3, two passes, per-row moments through LDS), sigmoid / tanh, blend -> h'
//   4. prior: ELU(BN(W_p0 h' + b)) -> LDS, then W_p3 . + b split over k slices -> z' (X_{t+1}'s latent columns)
//   5. reward: ELU(W_r0 h' + b) -> LDS, ELU(W_r2 . + b) . w_r4 + b -> r; G (+)= gamma^t r
// Rows never share a statistic: every reduction is over one row's features, so a non-finite row stays alone.
#ifndef DRNN_HOST

struct DrnnArgs {
    int rows, Hd, Kx, L, Lp, nb3;        // logical rows; GRU width; X panel width; latent dims; Lr / 32
    RowMap amap;                         // logical row -> X row
    const float* X; float* Xo; long x_ts; int out_q0;   // X_t in; X_{t+1} out: latent quads from out_q0
    const float* hin; int h_G;           // h_G > 0: row m starts from hin[m / h_G] (its env's hidden), else hin[X row]
    float* hout;                         // [X row][Hd]
    const unsigned short* Xih; const unsigned short* Xhh;     // x6 [3 Hd][Kx], [3 Hd][Hd]
    const unsigned short* Xp0r0;         // x6 [2 M][Hd]: prior_mlp.0 rows, then _reward.0 rows
    const unsigned short* Xp3;           // x6 [Lr][M]
    const unsigned short* Xr2;           // x6 [M][M]
    const float* ln;                     // [6][Hd]: reset gain, shift; update gain, shift; newval gain, shift
    const float* b_p0; const float* bn_w; const float* bn_b; const float* bn_m; const float* bn_v;   // [M]
    const float* b_p3;                   // [Lr]
    const float* b_r0; const float* b_r2; const float* w_r4; const float* b_r4;
    float* G; float* rlast; float disc; int first, last;   // G null: no return; rlast written when last
};

constexpr int DRNN_M = 512, DRNN_NW = 8;
// LDS floats: activation block | h block | prior last-layer partial tiles | row reductions | parameter vectors
__host__ __device__ inline int drnn_lds_floats(int Hd, int Lr) {
    return DRNN_M * 32 + Hd * 32 + 8 * 1024 + 4 * DRNN_NW * 32 + 6 * Hd + 6 * DRNN_M + Lr;
}
// k slices of the prior's last layer (Lr / 32 column blocks x slices <= 8 waves)
__host__ __device__ inline int drnn_ks(int nb3) { return nb3 >= 5 ? 1 : nb3 >= 3 ? 2 : nb3 == 2 ? 4 : 8; }

DEVI float drnn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Per-row mean and 1 / sqrt(var + 1e-3) over the Hd features of two gate tiles at once (biased variance, two
// passes): each active wave holds 32 features of every row, lanes (r, h) 16 of them.
DEVI void drnn_moments2(const floatx16& a, const floatx16& b, bool active, float* red, int wave, int r, int h, int nb,
                        float inv_n, float& ma, float& ra, float& mb, float& rb) {
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { sa += a[i]; sb += b[i]; }
    sa += __shfl_xor(sa, 32);
    sb += __shfl_xor(sb, 32);
    if (active && h == 0) { red[wave * 32 + r] = sa; red[(DRNN_NW + wave) * 32 + r] = sb; }
    lds_barrier();
    float ta = 0.f, tb = 0.f;
    for (int w = 0; w < nb; ++w) { ta += red[w * 32 + r]; tb += red[(DRNN_NW + w) * 32 + r]; }
    ma = ta * inv_n; mb = tb * inv_n;
    float qa = 0.f, qb = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float da = a[i] - ma, db = b[i] - mb;
        qa += da * da; qb += db * db;
    }
    qa += __shfl_xor(qa, 32);
    qb += __shfl_xor(qb, 32);
    if (active && h == 0) { red[(2 * DRNN_NW + wave) * 32 + r] = qa; red[(3 * DRNN_NW + wave) * 32 + r] = qb; }
    lds_barrier();
    float va = 0.f, vb = 0.f;
    for (int w = 0; w < nb; ++w) { va += red[(2 * DRNN_NW + w) * 32 + r]; vb += red[(3 * DRNN_NW + w) * 32 + r]; }
    ra = 1.0f / sqrtf(fmaxf(va * inv_n, 0.f) + 1e-3f);
    rb = 1.0f / sqrtf(fmaxf(vb * inv_n, 0.f) + 1e-3f);
}

__global__ void __launch_bounds__(64 * DRNN_NW) drnn_step_kernel(const DrnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int M = DRNN_M, NTH = 64 * DRNN_NW;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int Hd = a.Hd, nb = Hd / 32, Lr = a.nb3 * 32;
    const int m0 = blockIdx.x * 32;
    float* sX = sm;                       // [max(Kx16, M) / 4][32][4]
    float* sH = sX + M * 32;              // [Hd / 4][32][4]
    float* sR = sH + Hd * 32;             // [8][32 features][32 rows]
    float* red = sR + 8 * 1024;           // [4][NW][32]
    float* sln = red + 4 * DRNN_NW * 32;  // [6][Hd]
    float* sbp0 = sln + 6 * Hd;           // [M] each: prior.0 bias, BN scale, BN shift, reward.0 bias, reward.2 bias,
    float* sal = sbp0 + M;                //           reward.4 weight
    float* sbe = sal + M;
    float* sbr0 = sbe + M;
    float* sbr2 = sbr0 + M;
    float* swr4 = sbr2 + M;
    float* sbp3 = swr4 + M;               // [Lr]
    const int kq1 = (a.Kx + 15) / 16 * 4; // quads of the staged input (k padded to 16 with zeros)

    // ---- 1. stage
    for (int i = tid; i < kq1 * 32; i += NTH) {
        const int q = i >> 5, rr = i & 31, m = m0 + rr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < a.rows && q * 4 < a.Kx) {
            const int x = map_row(a.amap, m);
            v = *(const float4*)(a.X + (size_t)(x >> 5) * a.x_ts + (size_t)q * 128 + (x & 31) * 4);
        }
        *(float4*)(sX + (q * 32 + rr) * 4) = v;
    }
    for (int i = tid; i < (Hd / 4) * 32; i += NTH) {
        const int q = i >> 5, rr = i & 31, m = m0 + rr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < a.rows) {
            const size_t hr = a.h_G > 0 ? (size_t)(m / a.h_G) : (size_t)map_row(a.amap, m);
            v = *(const float4*)(a.hin + hr * Hd + q * 4);
        }
        *(float4*)(sH + (q * 32 + rr) * 4) = v;
    }
    for (int i = tid; i < 6 * Hd; i += NTH) sln[i] = a.ln[i];
    for (int i = tid; i < M; i += NTH) {
        // eval-mode BatchNorm1d as ATen's CPU kernel forms it: alpha = weight / sqrt(var + eps), beta = bias - mean alpha
        const float al = fmul(a.bn_w[i], 1.0f / sqrtf(a.bn_v[i] + 1e-5f));
        sbp0[i] = a.b_p0[i]; sal[i] = al; sbe[i] = fadd(a.bn_b[i], -fmul(a.bn_m[i], al));
        sbr0[i] = a.b_r0[i]; sbr2[i] = a.b_r2[i]; swr4[i] = a.w_r4[i];
    }
    for (int i = tid; i < Lr; i += NTH) sbp3[i] = a.b_p3[i];
    lds_barrier();

    // ---- 2. gates (waves b < nb)
    const bool gate = wave < nb;
    floatx16 g3[3], gni;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) g3[j][i] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) gni[i] = 0.f;
    if (gate) {
        uint4 wr[2][3][3];
        const int kg1 = kq1 / 4, kg2 = Hd / 16;
        const unsigned short* Wi = a.Xih + (size_t)wave * kg1 * 1536 + lane * 8;
        const long wbi = (long)nb * kg1 * 1536;
        ring6_fill<3, 2>(wr, Wi, wbi, 0, kg1);
        ring6_run<3, 2>(g3, wr, sX, Wi, wbi, 0, kg1, r, h);
        gni = g3[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) g3[2][i] = 0.f;
        const unsigned short* Wh = a.Xhh + (size_t)wave * kg2 * 1536 + lane * 8;
        const long wbh = (long)nb * kg2 * 1536;
        ring6_fill<3, 2>(wr, Wh, wbh, 0, kg2);
        ring6_run<3, 2>(g3, wr, sH, Wh, wbh, 0, kg2, r, h);
    }

    // ---- 3. LayerNorms, gate non-linearities, blend
    const float inv_n = 1.0f / (float)Hd;
    float mr, rr_, mu, ru;
    drnn_moments2(g3[0], g3[1], gate, red, wave, r, h, nb, inv_n, mr, rr_, mu, ru);
    floatx16 upd, npre;
    if (gate) {
        const float shr = -rr_ * mr, shu = -ru * mu;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int f = wave * 32 + 8 * (i >> 2) + 4 * h + (i & 3);
            const float rs = drnn_sigmoid(fadd(fmul(fadd(fmul(g3[0][i], rr_), shr), sln[f]), sln[Hd + f]));
            upd[i] = drnn_sigmoid(fadd(fmul(fadd(fmul(g3[1][i], ru), shu), sln[2 * Hd + f]), sln[3 * Hd + f]));
            npre[i] = fadd(gni[i], fmul(rs, g3[2][i]));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) { upd[i] = 0.f; npre[i] = 0.f; }
    }
    float mn, rn, m_unused, r_unused;
    drnn_moments2(npre, npre, gate, red, wave, r, h, nb, inv_n, mn, rn, m_unused, r_unused);
    if (gate) {
        const float shn = -rn * mn;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cq = wave * 8 + 2 * q + h;
            float* hp = sH + (cq * 32 + r) * 4;
            const float4 ho = *(const float4*)hp;
            const float hv[4] = {ho.x, ho.y, ho.z, ho.w};
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j, f = cq * 4 + j;
                const float nv = tanhf(fadd(fmul(fadd(fmul(npre[i], rn), shn), sln[4 * Hd + f]), sln[5 * Hd + f]));
                o[j] = fadd(fmul(upd[i], nv), fmul(fadd(1.0f, -upd[i]), hv[j]));
            }
            *(float4*)hp = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    lds_barrier();
    for (int i = tid; i < (Hd / 4) * 32; i += NTH) {
        const int q = i >> 5, rr = i & 31, m = m0 + rr;
        if (m < a.rows)
            *(float4*)(a.hout + (size_t)map_row(a.amap, m) * Hd + q * 4) = *(const float4*)(sH + (q * 32 + rr) * 4);
    }

    // ---- 4. prior MLP
    const int kgh = Hd / 16, cw0 = wave * 2;
    {
        floatx16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
        uint4 wr[2][2][3];
        const unsigned short* Wp = a.Xp0r0 + (size_t)cw0 * kgh * 1536 + lane * 8;
        const long wbs = (long)kgh * 1536;
        ring6_fill<2, 2>(wr, Wp, wbs, 0, kgh);
        ring6_run<2, 2>(acc, wr, sH, Wp, wbs, 0, kgh, r, h);
        // (every wave is past the gates' reads of sX: the barriers above)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (cw0 + j) * 32 + 8 * q + 4 * h;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    o[e] = elu_f(fadd(fmul(fadd(acc[j][4 * q + e], sbp0[c + e]), sal[c + e]), sbe[c + e]));
                *(float4*)(sX + (((cw0 + j) * 8 + 2 * q + h) * 32 + r) * 4) = make_float4(o[0], o[1], o[2], o[3]);
            }
    }
    lds_barrier();
    {
        const int ks = drnn_ks(a.nb3), units = a.nb3 * ks;
        if (wave < units) {
            const int b3 = wave % a.nb3, s = wave / a.nb3, gs = (M / 16) / ks;
            floatx16 acc[1];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
            uint4 wr[2][1][3];
            const unsigned short* Wp = a.Xp3 + (size_t)b3 * (M / 16) * 1536 + lane * 8;
            ring6_fill<1, 2>(wr, Wp, 0, s * gs, (s + 1) * gs);
            ring6_run<1, 2>(acc, wr, sX, Wp, 0, s * gs, (s + 1) * gs, r, h);
#pragma unroll
            for (int i = 0; i < 16; ++i) sR[wave * 1024 + (8 * (i >> 2) + 4 * h + (i & 3)) * 32 + r] = acc[0][i];
        }
        lds_barrier();
        // z' = sum over the k slices + bias -> X_{t+1}'s latent quads (columns >= L are written as 0)
        for (int i = tid; i < (a.Lp / 4) * 32; i += NTH) {
            const int fq = i >> 5, rr = i & 31, m = m0 + rr;
            if (m >= a.rows) continue;
            const int b3 = fq >> 3, fl = (fq & 7) * 4;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t = 0.f;
                for (int s = 0; s < ks; ++s) t += sR[(s * a.nb3 + b3) * 1024 + (fl + e) * 32 + rr];
                o[e] = fq * 4 + e < a.L ? t + sbp3[fq * 4 + e] : 0.f;
            }
            const int x = map_row(a.amap, m);
            *(float4*)(a.Xo + (size_t)(x >> 5) * a.x_ts + (size_t)(a.out_q0 + fq) * 128 + (x & 31) * 4) =
                make_float4(o[0], o[1], o[2], o[3]);
        }
    }

    // ---- 5. reward MLP on h'
    {
        floatx16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
        uint4 wr[2][2][3];
        const unsigned short* Wp = a.Xp0r0 + (size_t)(M / 32 + cw0) * kgh * 1536 + lane * 8;
        const long wbs = (long)kgh * 1536;
        ring6_fill<2, 2>(wr, Wp, wbs, 0, kgh);
        ring6_run<2, 2>(acc, wr, sH, Wp, wbs, 0, kgh, r, h);
        // (every wave is past the prior's reads of sX: the barrier after its partial tiles)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (cw0 + j) * 32 + 8 * q + 4 * h;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = elu_f(acc[j][4 * q + e] + sbr0[c + e]);
                *(float4*)(sX + (((cw0 + j) * 8 + 2 * q + h) * 32 + r) * 4) = make_float4(o[0], o[1], o[2], o[3]);
            }
    }
    lds_barrier();
    {
        floatx16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
        uint4 wr[2][2][3];
        const unsigned short* Wp = a.Xr2 + (size_t)cw0 * (M / 16) * 1536 + lane * 8;
        const long wbs = (long)(M / 16) * 1536;
        ring6_fill<2, 2>(wr, Wp, wbs, 0, M / 16);
        ring6_run<2, 2>(acc, wr, sX, Wp, wbs, 0, M / 16, r, h);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (cw0 + j) * 32 + 8 * q + 4 * h;
                s += (elu_f(acc[j][4 * q] + sbr2[c]) * swr4[c] + elu_f(acc[j][4 * q + 1] + sbr2[c + 1]) * swr4[c + 1]) +
                     (elu_f(acc[j][4 * q + 2] + sbr2[c + 2]) * swr4[c + 2] +
                      elu_f(acc[j][4 * q + 3] + sbr2[c + 3]) * swr4[c + 3]);
            }
        s += __shfl_xor(s, 32);
        if (h == 0) red[wave * 32 + r] = s;
        lds_barrier();
        if (tid < 32 && m0 + tid < a.rows) {
            const int x = map_row(a.amap, m0 + tid);
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < DRNN_NW; ++w) tot += red[w * 32 + tid];
            const float o = tot + a.b_r4[0];
            if (a.G) {
                // G += discount * reward (tdmpc_similarity_drnn.py:141), float32(discount) like ATen's scalar mul
                const float dr = fmul(a.disc, o);
                a.G[x] = a.first ? dr : fadd(a.G[x], dr);
            }
            if (a.last && a.rlast) a.rlast[x] = o;
        }
    }
}

// z [rows][zld], a [rows][A] -> the [a | 0 | z | 0] rows of an X panel (padding written as 0)
__global__ void drnn_scatter_kernel(const float* z, int zld, const float* act, float* X, int rows, int L, int A, int Ap,
                                    int Kx) {
    const size_t total = (size_t)rows * Kx;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / Kx;
        const int c = (int)(i % Kx);
        const float v = c < A ? act[m * A + c] : (c >= Ap && c < Ap + L ? z[m * zld + (c - Ap)] : 0.f);
        X[pidx(m, c, Kx)] = v;
    }
}

// two vectors of n floats in one launch (estimate_value's outputs)
__global__ void drnn_copy2_kernel(const float* s0, float* d0, const float* s1, float* d1, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        d0[i] = s0[i];
        d1[i] = s1[i];
    }
}

// src [rows][sld] -> dst [rows][dld], the first n columns
__global__ void drnn_copy_rows_kernel(const float* src, int sld, float* dst, int dld, int n, int rows) {
    const int total = rows * n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
        dst[(size_t)(i / n) * dld + i % n] = src[(size_t)(i / n) * sld + i % n];
}

// Power-law noise sequences straight into the planner's per-env noise streams (tdmpc_drnn_colored_noise; the
// reference's colorednoise.powerlaw_psd_gaussian per candidate, tdmpc_icem_similarity_drnn.py:135-146). One thread
// per sequence s = r * A + a of a job (blockIdx.y) of an env (blockIdx.z): its 2F normals lie n * A apart, so the
// lanes of a wave read consecutive floats for every k, and they write consecutive floats for every sample t
// (the block is [L][rows][A]). The spectrum factors and the [2F][16] inverse-DFT matrix travel in the kernel
// arguments; k is uniform, so they are scalar loads. y[] stays in registers (fixed trip count of 16, rows past L are 0).
struct ColoredJob { int spectrum, n, rows, c0; long dst, src; };
struct ColoredArgs {
    int L, A, F;
    long env_stride, normals_env;
    const float* normals; float* noise;
    ColoredJob jobs[17];
    float re[4][9], im[4][9];
    float dft[18][16];
};

__global__ void __launch_bounds__(256) drnn_colored_noise_kernel(const ColoredArgs a) {
    const ColoredJob& j = a.jobs[blockIdx.y];
    const int nA = j.n * a.A;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nA) return;
    const float* z = a.normals + (size_t)blockIdx.z * a.normals_env + j.src + s;
    float y[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) y[t] = 0.f;
    for (int k = 0; k < 2 * a.F; ++k) {
        const float f = k < a.F ? a.re[j.spectrum][k] : a.im[j.spectrum][k - a.F];
        const float x = z[(size_t)k * nA] * f;
#pragma unroll
        for (int t = 0; t < 16; ++t) y[t] = fmaf(x, a.dft[k][t], y[t]);
    }
    float* o = a.noise + (size_t)blockIdx.z * a.env_stride + j.dst + (size_t)j.c0 * a.A + s;
    const size_t ts = (size_t)j.rows * a.A;
#pragma unroll
    for (int t = 0; t < 16; ++t)
        if (t < a.L) o[t * ts] = y[t];
}

#else  // ================================================================================================ DRNN_HOST

namespace {

// The packed buffer of a DSSM planner: the TOLD layout of its base dims (encoder, pi, Q1, Q2 and the job table; the
// TOLD dynamics / reward regions stay unused), then the regions below (float offsets from the buffer's start).
struct DrnnLayout {
    int Hd;
    size_t x_ih, x_hh, ln, x_p0r0, b_p0, bn_w, bn_b, bn_m, bn_v, x_p3, b_p3, b_r0, x_r2, b_r2, w_r4, b_r4;
    size_t total;
};

bool drnn_check(const tdmpc_drnn_dims* d, Layout* w, DrnnLayout* dl) {
    if (!check_dims(&d->base)) { snprintf(g_err, sizeof g_err, "drnn: bad planner dims"); return false; }
    make_layout(&d->base, w);
    const int Hd = d->hidden_dim;
    if (d->base.modality != 0 || !d->base.enc_norm) {
        snprintf(g_err, sizeof g_err, "drnn: state observations with the LayerNorm encoder only (modality %d, enc_norm %d)",
                 d->base.modality, d->base.enc_norm);
        return false;
    }
    if (w->M != DRNN_M) { snprintf(g_err, sizeof g_err, "drnn: mlp_dim %d (512 only)", w->M); return false; }
    if (Hd < 32 || Hd > 256 || Hd % 32) {
        snprintf(g_err, sizeof g_err, "drnn: hidden_dim %d (a multiple of 32 up to 256)", Hd);
        return false;
    }
    if (w->Lr > 256 || rup(w->Kx, 16) > (size_t)DRNN_M || !chain_shape_ok(*w)) {
        snprintf(g_err, sizeof g_err, "drnn: latent_dim %d / action_dim %d outside the step and chain kernels' range",
                 w->L, w->A);
        return false;
    }
    if ((size_t)drnn_lds_floats(Hd, w->Lr) * 4 > 160 * 1024) { snprintf(g_err, sizeof g_err, "drnn: LDS"); return false; }
    size_t o = w->total;
    auto take = [&](size_t n) { size_t r = o; o += rup(n, 64); return r; };
    auto x6f = [](size_t r, size_t k) { return rup(r, 32) * rup(k, 16) * 3 / 2; };
    const size_t M = DRNN_M;
    dl->Hd = Hd;
    dl->x_ih = take(x6f(3 * Hd, w->Kx)); dl->x_hh = take(x6f(3 * Hd, Hd)); dl->ln = take(6 * Hd);
    dl->x_p0r0 = take(x6f(2 * M, Hd));
    dl->b_p0 = take(M); dl->bn_w = take(M); dl->bn_b = take(M); dl->bn_m = take(M); dl->bn_v = take(M);
    dl->x_p3 = take(x6f(w->Lr, M)); dl->b_p3 = take(w->Lr);
    dl->b_r0 = take(M); dl->x_r2 = take(x6f(M, M)); dl->b_r2 = take(M); dl->w_r4 = take(M); dl->b_r4 = take(1);
    dl->total = o;
    return true;
}

// workspace: the planner's (make_work), then two hidden-state buffers [xrows][Hd] (ping-pong over the steps)
struct DrnnWork { float* hb[2]; size_t total; };
// (extra: rows per env beyond N + P, as make_work's: the iCEM planner's reused elites)
void drnn_work(const tdmpc_drnn_dims* d, const Layout& w, char* base, DrnnWork* dw, int extra = 0) {
    Work k;
    make_work(&d->base, w, nullptr, &k, extra);
    size_t o = k.total;
    for (int i = 0; i < 2; ++i) {
        dw->hb[i] = base ? (float*)(base + o) : nullptr;
        o += rup((size_t)k.xrows * d->hidden_dim * 4, 256);
    }
    dw->total = o;
}

constexpr int DRNN_NT = 62;   // tensors of tdmpc_drnn_pack_weights (tdmpc_drnn.h)
constexpr int DRNN_PROF_CFG = 7;

struct DrnnCtx { Ctx c; DrnnLayout dl; DrnnWork dw; };

// drnn_step_kernel's dynamic LDS limit (once; the pack sets it too, so a first plan under capture makes no such call)
int drnn_attrs() {
    static int done = 0;
    if (done) return 0;
    HIPCHK(hipFuncSetAttribute((const void*)drnn_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done = 1;
    return 0;
}

int drnn_setup(DrnnCtx& x, const tdmpc_drnn_dims* d, const void* packed, void* ws, size_t ws_bytes, int batch, int H,
               int I, hipStream_t s, int extra = 0) {
    Layout w;
    if (!drnn_check(d, &w, &x.dl)) return TDMPC_E_DIMS;
    drnn_work(d, w, nullptr, &x.dw, extra);
    if (ws_bytes < x.dw.total) { snprintf(g_err, sizeof g_err, "drnn: workspace too small"); return TDMPC_E_SIZE; }
    drnn_work(d, w, (char*)ws, &x.dw, extra);
    int rc = setup_ctx(x.c, &d->base, packed, ws, ws_bytes, batch, H, I, s, extra);
    if (rc) return rc;
    // one kernel family for every launch size, so a row's arithmetic does not depend on the batch it is planned in
    x.c.path = TDMPC_PATH_CHAIN_X6;
    return drnn_attrs();
}

// One DSSM.next over `rows` logical rows of X_t (+ the return update). hin / h_G as DrnnArgs; step t reads the
// hidden buffer t & 1 unless hin is given, and writes buffer (t + 1) & 1 unless hout is given.
int drnn_step(const DrnnCtx& x, int t, int rows, RowMap map, const float* hin, int h_G, float* hout, float* G,
              float* rlast, float disc, int first, int last) {
    if (rows <= 0) return 0;
    const Ctx& c = x.c;
    const Layout& w = c.w;
    const DrnnLayout& dl = x.dl;
    DrnnArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows; a.Hd = dl.Hd; a.Kx = c.Kx; a.L = w.L; a.Lp = w.Lp; a.nb3 = w.Lr / 32; a.amap = map;
    a.X = Xt(c, t); a.Xo = Xt(c, t + 1); a.x_ts = (long)c.Kx * 32; a.out_q0 = w.Ap / 4;
    a.hin = hin ? hin : x.dw.hb[t & 1]; a.h_G = hin ? h_G : 0;
    a.hout = hout ? hout : x.dw.hb[(t + 1) & 1];
    auto us = [&](size_t off) { return (const unsigned short*)(c.pw + off); };
    a.Xih = us(dl.x_ih); a.Xhh = us(dl.x_hh); a.Xp0r0 = us(dl.x_p0r0); a.Xp3 = us(dl.x_p3); a.Xr2 = us(dl.x_r2);
    a.ln = c.pw + dl.ln; a.b_p0 = c.pw + dl.b_p0; a.bn_w = c.pw + dl.bn_w; a.bn_b = c.pw + dl.bn_b;
    a.bn_m = c.pw + dl.bn_m; a.bn_v = c.pw + dl.bn_v; a.b_p3 = c.pw + dl.b_p3; a.b_r0 = c.pw + dl.b_r0;
    a.b_r2 = c.pw + dl.b_r2; a.w_r4 = c.pw + dl.w_r4; a.b_r4 = c.pw + dl.b_r4;
    a.G = G; a.rlast = rlast; a.disc = disc; a.first = first; a.last = last;
    Profiler& pf = g_prof;
    const bool prof = prof_armed() && pf.cfg == DRNN_PROF_CFG && (pf.rows == 0 || rows == pf.rows);
    if (prof) snprintf(pf.kernel, sizeof pf.kernel, "drnn_step_kernel");
    HIPCHK(prof_begin(prof, c.s));
    const size_t lds = (size_t)drnn_lds_floats(dl.Hd, w.Lr) * 4;
    hipLaunchKernelGGL(drnn_step_kernel, dim3((rows + 31) / 32), dim3(64 * DRNN_NW), lds, c.s, a);
    HIPCHK(hipGetLastError());
    const double Hd = dl.Hd, M = DRNN_M;
    HIPCHK(prof_end(prof, c.s, 2.0 * rows * (3 * Hd * (w.L + w.A + Hd) + 2 * Hd * M + M * w.L + M * M + M)));
    return 0;
}

// The step functor of tdmpc_kernels.hip's drivers: a rollout's rows start from their env's hidden state (row m of a
// map with G rows per env from hidden[m / G]) and carry their own through the ping-pong buffers after that.
struct DrnnStep {
    const DrnnCtx& x; const float* hidden;
    int operator()(int t, int rows, RowMap map, float disc, int first, int last, int) const {
        return drnn_step(x, t, rows, map, t == 0 ? hidden : nullptr, map.G, nullptr, x.c.k.G, x.c.k.rlast, disc, first,
                         last);
    }
};

// the encoder's z0 [B][Lp] -> the caller's z_out [B][L] (optional)
int drnn_z_out(const Ctx& c, float* z_out) {
    if (!z_out) return 0;
    hipLaunchKernelGGL(drnn_copy_rows_kernel, dim3(c.B), dim3(256), 0, c.s, c.k.z0, c.w.Lp, z_out, c.w.L, c.w.L, c.B);
    HIPCHK(hipGetLastError());
    return 0;
}

// The job list of tdmpc_drnn_pack_weights from the DRNN_NT tensors t: the shared heads' jobs (pack_jobs, heads only),
// then the DSSM regions' (DrnnLayout). Returns the number of head jobs in front.
int drnn_pack_jobs(const Layout& w, const DrnnLayout& dl, const float* const* t, std::vector<PackJob>& jobs) {
    // the shared heads in the planner's own layout: encoder (48..53), pi (22..27), Q1 (28..37), Q2 (38..47)
    const float* heads[32];
    for (int i = 0; i < 6; ++i) heads[i] = t[48 + i];
    for (int i = 0; i < 26; ++i) heads[6 + i] = t[22 + i];
    pack_jobs(w, heads, jobs, true);
    const int nheads = (int)jobs.size();
    const int M = DRNN_M, Hd = dl.Hd, L = w.L, A = w.A;
    auto job = [&](int kind, size_t dst, long work) -> PackJob& {
        PackJob j;
        memset(&j, 0, sizeof j);
        j.kind = kind; j.dst = dst; j.work = work;
        jobs.push_back(j);
        return jobs.back();
    };
    auto cp = [&](size_t dst, const float* src, int cnt) {
        PackJob& j = job(PJ_COPY, dst, (long)rup(cnt, 64));
        j.src = src; j.n = cnt;
    };
    auto x6 = [&](size_t dst, const float* p0, const float* p1, int r0, int r1, int sld, int ncols, int first, int pk) {
        PackJob& j = job(PJ_X6, dst, (long)((r0 + r1 + 31) / 32) * ((pk + 15) / 16) * 512);
        memset(&j.m, 0, sizeof j.m);
        j.m.p0 = p0; j.m.p1 = p1 ? p1 : p0; j.m.r0 = r0; j.m.r1 = r1; j.m.sld = sld; j.m.ncols = ncols;
        j.m.first = first; j.m.L = L; j.m.A = A; j.m.Ap = w.Ap;
        j.prow = r0 + r1; j.pk = pk;
    };
    x6(dl.x_ih, t[8], nullptr, 3 * Hd, 0, L + A, L, 1, w.Kx);          // gru_cell.weight_ih: [z | a] -> [a | 0 | z | 0]
    x6(dl.x_hh, t[9], nullptr, 3 * Hd, 0, Hd, Hd, 0, Hd);
    // The six LayerNorm vectors lie Hd apart, so a copy's zero tail must not run to the next 64: with Hd % 64 == 32 it
    // would zero the next vector's first 32 floats, and the jobs of one launch run unordered. Only the last one pads
    // the slot out.
    for (int i = 0; i < 6; ++i) {
        const size_t work = i < 5 ? (size_t)Hd : rup(6 * (size_t)Hd, 64) - 5 * (size_t)Hd;
        PackJob& j = job(PJ_COPY, dl.ln + (size_t)i * Hd, (long)work);
        j.src = t[10 + i]; j.n = Hd;
    }
    x6(dl.x_p0r0, t[0], t[16], M, M, Hd, Hd, 0, Hd);                    // prior_mlp.0 rows, then _reward.0 rows
    cp(dl.b_p0, t[1], M); cp(dl.bn_w, t[2], M); cp(dl.bn_b, t[3], M); cp(dl.bn_m, t[4], M); cp(dl.bn_v, t[5], M);
    x6(dl.x_p3, t[6], nullptr, L, 0, M, M, 0, M);
    {   // (the bias slot holds Lr floats: zeros past L)
        PackJob& j = job(PJ_COPY, dl.b_p3, (long)rup(w.Lr, 64));
        j.src = t[7]; j.n = L;
    }
    cp(dl.b_r0, t[17], M);
    x6(dl.x_r2, t[18], nullptr, M, 0, M, M, 0, M);
    cp(dl.b_r2, t[19], M); cp(dl.w_r4, t[20], M); cp(dl.b_r4, t[21], 1);
    return nheads;
}

// The iCEM planner keeps N + K + num_pi rows per env: the CEM kernel's LDS and row limits at that width.
bool drnn_icem_dims_ok(const tdmpc_dims& b) {
    const int Tw = b.num_samples + b.num_elites + b.num_pi;
    if (b.num_pi <= 0 || Tw > 4096 || cem_lds_bytes(Tw, b.max_horizon, b.num_elites, b.action_dim) > 160 * 1024) {
        snprintf(g_err, sizeof g_err, "drnn iCEM: %d rows per env (num_pi %d) outside the CEM kernel's range", Tw, b.num_pi);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int tdmpc_drnn_version(void) { return TDMPC_DRNN_VERSION; }

int tdmpc_drnn_sizes_for(const tdmpc_drnn_dims* d, tdmpc_sizes* out) {
    if (!d || !out) return TDMPC_E_NULL;
    Layout w;
    DrnnLayout dl;
    if (!drnn_check(d, &w, &dl)) return TDMPC_E_DIMS;
    DrnnWork dw;
    drnn_work(d, w, nullptr, &dw);
    out->packed_weight_bytes = rup(dl.total * 4, 256);
    out->workspace_bytes = dw.total;
    out->noise_floats_per_env = tdmpc_noise_floats(&d->base, d->base.max_horizon, d->base.max_iterations);
    return 0;
}

int tdmpc_drnn_num_param_tensors(const tdmpc_drnn_dims* d) {
    if (!d) return TDMPC_E_NULL;
    return DRNN_NT;
}

int tdmpc_drnn_pack_weights(const tdmpc_drnn_dims* d, const float* const* t, int32_t n, void* packed, size_t bytes,
                            void* stream) {
    if (!d || !t || !packed) return TDMPC_E_NULL;
    Layout w;
    DrnnLayout dl;
    if (!drnn_check(d, &w, &dl)) return TDMPC_E_DIMS;
    if (n != DRNN_NT) { snprintf(g_err, sizeof g_err, "drnn pack: %d tensors, %d expected", n, DRNN_NT); return TDMPC_E_DIMS; }
    if (bytes < dl.total * 4) return TDMPC_E_SIZE;
    if (init_attrs() || drnn_attrs()) return TDMPC_E_HIP;
    for (int i = 0; i < n; ++i)
        if (!t[i]) return TDMPC_E_NULL;
    std::vector<PackJob> jobs;
    drnn_pack_jobs(w, dl, t, jobs);
    return launch_pack(jobs, w, (float*)packed, (hipStream_t)stream);
}

int tdmpc_drnn_debug_pack_check(const tdmpc_drnn_dims* d, const int64_t* numel, int32_t n) {
    // Host-only, as tdmpc_debug_pack_check (no HIP call; tensor i at the fake base (i + 1) << 40): the shared heads'
    // jobs write inside the base layout, the DSSM jobs behind it and inside DrnnLayout::total, no two DSSM jobs write
    // the same float (the jobs of one launch run unordered), and every job reads inside its source tensor.
    if (!d || !numel) return TDMPC_E_NULL;
    Layout w;
    DrnnLayout dl;
    if (!drnn_check(d, &w, &dl)) return TDMPC_E_DIMS;
    if (n != DRNN_NT) return TDMPC_E_DIMS;
    std::vector<const float*> t(n);
    for (int i = 0; i < n; ++i) t[i] = (const float*)((uintptr_t)(i + 1) << 40);
    std::vector<PackJob> jobs;
    const int nheads = drnn_pack_jobs(w, dl, t.data(), jobs);
    if (jobs.size() > (size_t)PACK_MAX_JOBS) {
        snprintf(g_err, sizeof g_err, "drnn pack: %zu jobs > %d", jobs.size(), PACK_MAX_JOBS);
        return TDMPC_E_SIZE;
    }
    auto end_of = [](const PackJob& J) {
        return J.kind == PJ_X6 || J.kind == PJ_X6Q ? (double)J.dst + 1.5 * J.work : (double)(J.dst + J.work);
    };
    for (int j = 0; j < (int)jobs.size(); ++j) {
        const PackJob& J = jobs[j];
        const bool head = j < nheads;
        if (!pack_job_in_bounds(J, numel, n, head ? 0 : w.total, head ? w.total : dl.total)) {
            snprintf(g_err, sizeof g_err, "drnn pack job %d (kind %d, dst %zu) out of bounds", j, J.kind, J.dst);
            return TDMPC_E_SIZE;
        }
        for (int k = nheads; k < j; ++k)
            if ((double)J.dst < end_of(jobs[k]) && (double)jobs[k].dst < end_of(J)) {
                snprintf(g_err, sizeof g_err, "drnn pack jobs %d (dst %zu) and %d (dst %zu) overlap", k, jobs[k].dst, j,
                         J.dst);
                return TDMPC_E_SIZE;
            }
    }
    return (int)jobs.size();
}

int tdmpc_drnn_next(const tdmpc_drnn_dims* d, const void* packed, const float* z, const float* act, const float* h,
                    int32_t rows, float* z_out, float* h_out, float* r_out, void* workspace, size_t ws_bytes,
                    void* stream) {
    if (!d || !packed || !z || !act || !h || !z_out || !h_out || !r_out || !workspace) return TDMPC_E_NULL;
    DrnnCtx x;
    int rc;
    if ((rc = drnn_setup(x, d, packed, workspace, ws_bytes, 1, 1, 1, (hipStream_t)stream))) return rc;
    const Ctx& c = x.c;
    if (rows <= 0 || rows > c.k.xrows) {
        snprintf(g_err, sizeof g_err, "drnn_next: %d rows (1..%d)", rows, c.k.xrows);
        return TDMPC_E_DIMS;
    }
    const long total = (long)rows * c.Kx;
    hipLaunchKernelGGL(drnn_scatter_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 1024)), dim3(256), 0, c.s,
                       z, c.w.L, act, c.k.X, rows, c.w.L, c.w.A, c.w.Ap, c.Kx);
    HIPCHK(hipGetLastError());
    if ((rc = drnn_step(x, 0, rows, RowMap{1 << 30, 0, 0}, h, 0, h_out, nullptr, r_out, 1.f, 1, 1))) return rc;
    hipLaunchKernelGGL(gather_z_kernel, dim3(256), dim3(256), 0, c.s, Xt(c, 1), c.Kx, c.w.Ap, c.w.L, rows, z_out);
    HIPCHK(hipGetLastError());
    return 0;
}

int tdmpc_drnn_estimate_value(const tdmpc_drnn_dims* d, const tdmpc_plan_params* prm, const void* packed,
                              const float* z0, const float* h0, const float* actions, const float* eps_term,
                              int32_t rows, float* value, float* reward_last, void* workspace, size_t ws_bytes,
                              void* stream) {
    if (!d || !prm || !packed || !z0 || !h0 || !actions || !eps_term || !value || !reward_last || !workspace)
        return TDMPC_E_NULL;
    DrnnCtx x;
    int rc;
    if ((rc = drnn_setup(x, d, packed, workspace, ws_bytes, prm->batch, prm->horizon, 1, (hipStream_t)stream))) return rc;
    if (resolve_path(prm->path, true) < 0) return TDMPC_E_DIMS;   // (checked as in the TOLD entry points; the path itself is fixed)
    if (rows != x.c.T) { snprintf(g_err, sizeof g_err, "rows must equal N+P"); return TDMPC_E_DIMS; }
    return estimate_value_run(x.c, DrnnStep{x, h0}, prm, z0, actions, eps_term, value, reward_last, nullptr);
}

int tdmpc_drnn_pi_rollout(const tdmpc_drnn_dims* d, const tdmpc_plan_params* prm, const void* packed, const float* z0,
                          const float* h0, const float* eps_pi, float* pi_actions, void* workspace, size_t ws_bytes,
                          void* stream) {
    if (!d || !prm || !packed || !z0 || !h0 || !eps_pi || !pi_actions || !workspace) return TDMPC_E_NULL;
    DrnnCtx x;
    int rc;
    if ((rc = drnn_setup(x, d, packed, workspace, ws_bytes, prm->batch, prm->horizon, 1, (hipStream_t)stream))) return rc;
    if (resolve_path(prm->path, true) < 0) return TDMPC_E_DIMS;   // (checked as in the TOLD entry points; the path itself is fixed)
    return pi_rollout_run(x.c, DrnnStep{x, h0}, prm, z0, eps_pi, pi_actions);
}

int tdmpc_drnn_plan(const tdmpc_drnn_dims* d, const tdmpc_plan_params* prm, const void* packed, const void* obs,
                    const float* hidden, const float* noise, const double* u, float* prev_mean, float* action,
                    float* metrics, float* z_out, float* elite_out, float* score_out, float* value_out,
                    float* mean_out, float* std_out, void* workspace, size_t ws_bytes, void* stream) {
    if (!d || !prm || !packed || !obs || !hidden || !noise || !u || !prev_mean || !action || !metrics || !workspace)
        return TDMPC_E_NULL;
    DrnnCtx x;
    int rc;
    if ((rc = drnn_setup(x, d, packed, workspace, ws_bytes, prm->batch, prm->horizon, prm->iterations,
                         (hipStream_t)stream)))
        return rc;
    if (resolve_path(prm->path, true) < 0) return TDMPC_E_DIMS;   // (checked as in the TOLD entry points; the path itself is fixed)
    Ctx& c = x.c;
    // z0 = h(obs) and mean = 0 (warm: prev_mean shifted), std = 2
    if ((rc = encode(c, obs, 0, c.B, prev_mean, prm->warm_start, 0, 2.f, prm->warm_flags))) return rc;
    if ((rc = drnn_z_out(c, z_out))) return rc;
    // tdmpc_similarity_drnn.py:203-262 is tdmpc_plan's sequence with DSSM.next for the step, every row starting from
    // its env's hidden. None of the TOLD fast forms: they are other launch sequences with other rounding.
    return cem_run(c, DrnnStep{x, hidden}, PlanFast{}, prm, noise, u, prev_mean, action, metrics, elite_out, score_out,
                   value_out, mean_out, std_out);
}

int tdmpc_drnn_icem_sizes_for(const tdmpc_drnn_dims* d, tdmpc_sizes* out) {
    if (!d || !out) return TDMPC_E_NULL;
    Layout w;
    DrnnLayout dl;
    if (!drnn_check(d, &w, &dl)) return TDMPC_E_DIMS;
    const tdmpc_dims& b = d->base;
    if (!drnn_icem_dims_ok(b)) return TDMPC_E_DIMS;
    DrnnWork dw, dw0;
    drnn_work(d, w, nullptr, &dw, b.num_elites);
    // (never below tdmpc_drnn_sizes_for's, whose layout may carry a region this one leaves out: one workspace then
    // serves tdmpc_drnn_next and the other entry points on the same dims too)
    drnn_work(d, w, nullptr, &dw0);
    out->packed_weight_bytes = rup(dl.total * 4, 256);
    out->workspace_bytes = std::max(dw.total, dw0.total);
    const size_t A = w.A, H = b.max_horizon, N = b.num_samples, P = b.num_pi, K = b.num_elites;
    out->noise_floats_per_env = H * P * A + b.max_iterations * (H * N * A + (N + K + P) * A) + H * K * A + A;
    return 0;
}

int tdmpc_drnn_plan_icem(const tdmpc_drnn_dims* d, const tdmpc_icem_params* prm, const void* packed, const void* obs,
                         const float* hidden, const float* noise, const double* u, float* prev_mean, float* elites,
                         float* action, float* metrics, float* hidden_out, float* z_out, float* value_out,
                         float* mean_out, float* std_out, void* workspace, size_t ws_bytes, void* stream) {
    if (!d || !prm || !packed || !obs || !hidden || !noise || !u || !prev_mean || !elites || !action || !metrics ||
        !hidden_out || !workspace)
        return TDMPC_E_NULL;
    DrnnCtx x;
    int rc;
    if (!icem_counts_ok(prm, &d->base, "drnn iCEM") || !drnn_icem_dims_ok(d->base)) return TDMPC_E_DIMS;
    if ((rc = drnn_setup(x, d, packed, workspace, ws_bytes, prm->batch, prm->horizon, prm->iterations,
                         (hipStream_t)stream, d->base.num_elites)))
        return rc;
    if (resolve_path(prm->path, true) < 0) return TDMPC_E_DIMS;   // (checked as in the TOLD entry points; the path itself is fixed)
    Ctx& c = x.c;
    // z0 = h(obs); mean = 0 (warm: mean[:-1] = prev[1:], mean[-1] = prev[-1]), std = init_std (0.5)
    if ((rc = encode(c, obs, 0, c.B, prev_mean, prm->warm_start, 1, prm->init_std))) return rc;
    if ((rc = drnn_z_out(c, z_out))) return rc;
    if ((rc = icem_run(c, DrnnStep{x, hidden}, prm, noise, u, prev_mean, elites, action, metrics, value_out, mean_out,
                       std_out)))
        return rc;
    // :267: the GRU state after DSSM.next(z0, action, hidden) with the returned action: [action | z0] into rows
    // 0..B-1 of X_0 (the plan is past its last read of it), one step launch over B rows
    const long total = (long)c.B * c.Kx;
    hipLaunchKernelGGL(drnn_scatter_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 1024)), dim3(256), 0, c.s,
                       c.k.z0, c.w.Lp, action, c.k.X, c.B, c.w.L, c.w.A, c.w.Ap, c.Kx);
    HIPCHK(hipGetLastError());
    return drnn_step(x, 0, c.B, RowMap{1 << 30, 0, 0}, hidden, 0, hidden_out, nullptr, nullptr, 1.f, 1, 0);
}

int tdmpc_drnn_colored_noise(const tdmpc_colored_noise_params* p, const float* normals, size_t normals_floats,
                             float* noise, size_t noise_floats, void* stream) {
    if (!p || !normals || !noise) return TDMPC_E_NULL;
    if (p->L < 2 || p->L > 16 || p->A <= 0 || p->A > 64 || p->batch <= 0 || p->batch > 65535 || p->n_jobs <= 0 ||
        p->n_jobs > TDMPC_NOISE_MAX_JOBS || p->n_spectra <= 0 || p->n_spectra > TDMPC_NOISE_MAX_SPECTRA) {
        snprintf(g_err, sizeof g_err, "coloured noise: L %d (2..16), A %d (1..64), batch %d, %d jobs (1..%d), %d spectra (1..%d)",
                 p->L, p->A, p->batch, p->n_jobs, TDMPC_NOISE_MAX_JOBS, p->n_spectra, TDMPC_NOISE_MAX_SPECTRA);
        return TDMPC_E_DIMS;
    }
    const long L = p->L, A = p->A, F = L / 2 + 1;
    if (p->env_stride < 0 || p->normals_env < 0 || (size_t)p->batch * (size_t)p->env_stride > noise_floats ||
        (size_t)p->batch * (size_t)p->normals_env > normals_floats) {
        snprintf(g_err, sizeof g_err, "coloured noise: %d env streams of %ld / %ld floats exceed the buffers", p->batch,
                 (long)p->env_stride, (long)p->normals_env);
        return TDMPC_E_SIZE;
    }
    ColoredArgs a;
    memset(&a, 0, sizeof a);
    long max_seq = 0;
    for (int j = 0; j < p->n_jobs; ++j) {
        const tdmpc_noise_job& J = p->jobs[j];
        if (J.spectrum < 0 || J.spectrum >= p->n_spectra || J.n < 0 || J.n > (1 << 20) || J.rows < 0 ||
            J.rows > (1 << 20) || J.c0 < 0 || (long)J.c0 + J.n > J.rows || J.dst < 0 || J.src < 0) {
            snprintf(g_err, sizeof g_err, "coloured noise: bad job %d", j);
            return TDMPC_E_DIMS;
        }
        // last float written: dst + ((L - 1) rows + c0 + n) A - 1; last read: src + 2F n A - 1
        if (J.dst + L * J.rows * A > p->env_stride || J.src + 2 * F * J.n * A > p->normals_env) {
            snprintf(g_err, sizeof g_err, "coloured noise: job %d leaves its env's stream", j);
            return TDMPC_E_SIZE;
        }
        a.jobs[j] = ColoredJob{J.spectrum, J.n, J.rows, J.c0, (long)J.dst, (long)J.src};
        max_seq = std::max(max_seq, (long)J.n * A);
    }
    if (!max_seq) return 0;
    a.L = (int)L; a.A = (int)A; a.F = (int)F; a.env_stride = p->env_stride; a.normals_env = p->normals_env;
    a.normals = normals; a.noise = noise;
    memcpy(a.re, p->re, sizeof a.re);
    memcpy(a.im, p->im, sizeof a.im);
    for (int k = 0; k < 2 * F; ++k)
        for (int t = 0; t < L; ++t) a.dft[k][t] = p->dft[k][t];   // (rows past 2F and columns past L stay 0)
    hipLaunchKernelGGL(drnn_colored_noise_kernel, dim3((unsigned)((max_seq + 255) / 256), p->n_jobs, p->batch), dim3(256),
                       0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

int tdmpc_drnn_profile_begin(int32_t rows, int32_t max_launches) {
    return tdmpc_profile_begin(DRNN_PROF_CFG, -1, 0, rows, max_launches);
}

int tdmpc_drnn_profile_end(int32_t* launches, double* total_ms, double* flops) {
    return tdmpc_profile_end(launches, total_ms, flops);
}

}  // extern "C"

#endif  // DRNN_HOST
