// wide_heads.inc -- included by tdmpc_kernels.hip after wide_ring.inc (the design: the ring with its read-ahead, the
// fragment stream, the x tile, the shape of the two-layer super-chunk and of the last layer) and wide_step.inc
// (uses also RowMap, tanh_f / elu_f and the reference-rounding helpers).
//
// The terminal heads of estimate_value (/root/reference/src/algorithm/tdmpc.py:91-92) on the wide kernels' design,
// one workgroup per CU and head-block of 128 rows:
//  * WH_PI: TOLD.pi + TruncatedNormal.sample (tdmpc.py:39-45, helper.py:86-96): Linear(L -> M), ELU, Linear(M -> M),
//    ELU, Linear(M -> A), tanh, (eps * std).clamp(+-0.3), clamp(mu + eps, +-(1 - 1e-6)) -> the X_H action columns;
//  * WH_Q: helper.q (helper.py:197-201): Linear(L + A -> M), LayerNorm, Tanh, Linear(M -> M), LayerNorm, ELU,
//    Linear(M -> 1) -> q of the row (the value combination happens in cem_kernel).
// One launch runs up to three jobs (role x head x row set), each on its own XCD groups (blockIdx.x % 8): the
// terminal pi of the sampled rows beside the policy rows' two Q heads, then the sampled rows' two Q heads -- two
// whole rounds of 256 workgroups where the chain kernels took 66 + 187 us (plan_cem).
//
// The first LayerNorm needs a row's 512 layer-1 outputs before any of them can feed layer 2, and they do not fit
// beside layer 2's accumulators. Its moments come instead from a STATISTICS BLOCK of extra layer-1 output rows that
// the pack derives from the weights (qstat_gram_kernel / qstat_chol_kernel below): with c = [x_real; 1] and
// C = [W1 | b1] column-centred over the M outputs,
//    mean = wbar . x + bbar                      (row 0: wbar = the mean of W1's rows, bbar = mean(b1))
//    var  = |C c|^2 / M = |R c|^2 / M            (rows 1..n: R upper-triangular with R^T R = C^T C, fp64 Cholesky)
// so the layer-1 weights stream once (the former two-pass kernel streamed W1 twice: 31 of its 157 us) and the
// variance is a sum of squares (no E[y^2] - mean^2 cancellation). Its conditioning is the reference's: R c has the
// absolute error eps |R| |c| = eps |C| |c|, as the reference's y - mean has eps |W1| |x|. The mean and LayerNorm-1's
// gain are folded into the first layer the kernel streams (diag(g1) (W1 - 1 wbar^T), bias g1 (b1 - bbar), fp64 in
// the pack), so its output is g1 (y - mean) and the chunk epilogue is one multiply-add before the tanh.

enum { WH_PI = 0, WH_Q = 1 };

// Timing diagnostics (results WRONG; named variant builds only, as wide_step.inc's WS_DIAG_*): WH_DIAG_ELU = the Q
// chunk epilogue as the step kernel's ELU (no LayerNorm / tanh), WH_DIAG_NOSTATS = no statistics pass, WH_DIAG_NOLN2 =
// no LayerNorm-2 epilogue
#if (defined(WH_DIAG_ELU) || defined(WH_DIAG_NOSTATS) || defined(WH_DIAG_NOLN2)) && !defined(TDMPC_VARIANT)
#error "WH_DIAG_* diagnostics produce wrong results: build them only as a named variant (tdmpc_amd.build --variant)"
#endif
#ifdef WH_DIAG_NOSTATS
constexpr int WH_STATS_ON = 0;
#else
constexpr int WH_STATS_ON = 1;
#endif

struct WHJob {
    int role, head;            // WH_PI / WH_Q; Q head 0 / 1
    int x0, nx;                // the job's XCD groups: blockIdx.x % 8 in [x0, x0 + nx)
    int rows, nrb;             // logical rows (multiple of 16), 128-row blocks
    RowMap map;                // logical row -> X_H row
    long eps_env, eps_off;     // PI: noise of logical row m at eps + (m / eps_G) eps_env + eps_off + (m % eps_G) A
    int eps_G;
};

struct WHQHead {
    const unsigned short* S;   // statistics block, x6q [nsr rows][g1s groups]
    const unsigned short* X1;  // layer 1 FOLDED: diag(g1) (W1 - 1 wbar^T), x6q [M rows][g1s groups]; b1 = g1 (b1 - bbar)
    const unsigned short* X2;  // layer 2, x6q [M rows][M / 32 groups]
    const float* bs;           // statistics bias [nsr]
    const float *b1, *g1, *be1, *b2, *g2, *be2, *w3, *b3;
};

struct WHArgs {
    WHJob job[3]; int njob;
    float* X; long x_ts;                       // X_H panel [rows/32][Kx/4][32][4]
    // PI
    const unsigned short *P1, *P2, *P3;        // x6q: [M][Lp], [M][M], [Ar][M]
    const float *pb1, *pb2, *pb3;
    int A, Ap, pq1, pkq, pg1s;                 // action dims; input quads [pq1, pq1 + pkq); x6q groups of P1
    const float* eps; float min_std, lo, hi;
    // Q
    WHQHead q[2];
    int qkq, qg1s;                             // input quads [0, qkq); x6q groups of S / X1
    float* qv; long q_ld;                      // q of head h, X_H row r -> qv[h * q_ld + r]
};

template <int G> constexpr size_t wh_lds() { return ws_lds<G>(); }

// a wave-uniform pointer as a scalar constant-space pointer: its loads become s_loads (lgkmcnt-counted, speculable --
// no exec-masked branches around the per-lane selects of vec4 -- and invisible to the ring's counted vmcnt waits)
DEVI float wh_u(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
DEVI const w2cf* wh_cp(const float* p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return (const w2cf*)(((unsigned long long)hi << 32) | lo);
}

// ---------------------------------------------------------------------------------------------------- WH_PI
template <int G1, int NB3, int GX>
DEVI void wh_pi(const WHArgs& a, const WHJob& J, int rb, char* wsm) {
    constexpr int NS = ws_ns<GX>();
    static_assert(NS >= 3 && NS - 1 < G1 + 16, "ring depth");
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    p1f4* sx = (p1f4*)(wsm + NS * WS_SLOT) + wave * (G1 * 2 * 64) + lane;
    const float* sb2 = (const float*)(wsm + NS * WS_SLOT);   // [512] (after the last first layer)
    const float* sb3 = sb2 + 512;                             // [256]
    const int m0 = rb * 128 + wave * 16;
    const bool live = m0 < J.rows;
    const int xr0 = live ? map_row(J.map, m0) : 0;
    WRing<NS, WS_SLOT, 3 * (NS - 3), w2_glds> R(wsm, lane, wave);
    auto src_main2 = [&](int sc, int j) __attribute__((always_inline)) { return wr_src<G1>(a.P1, a.pg1s, a.P2, wave, sc, j); };
    auto src_tail = [&](int l) __attribute__((always_inline)) {   // layer 3, then dummy refills
        return l < 2 * NB3 ? wr_l3_src<NB3>(a.P3, l, wave) : a.P2;
    };
#pragma unroll
    for (int k = 0; k < NS - 1; ++k) R.issue(k, src_main2(0, k));
    // x: the latent quads [pq1, pq1 + pkq) of X_H
    const bool xfin = wr_xtile<G1>(sx, a.X, a.x_ts, xr0, n, q, a.pq1, a.pkq, live);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    R.prime();

    floatx4 acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int sc = 0; sc < 4; ++sc) {
        auto sync = [&](int j, bool tail_bias) __attribute__((always_inline)) {
            return R.sync(wr_next<G1, NS>(src_main2, src_tail, sc, j), [&](int) __attribute__((always_inline)) {
                if (tail_bias && wave < 3)   // b2 [512] | b3 [256] into the dead x tile (see wide_step_kernel)
                    w2_glds(wave < 2 ? a.pb2 + 256 * wave : a.pb3, R.voff, R.lds + (unsigned)(NS * WS_SLOT) + wave * 1024);
            });
        };
        floatx4 a1[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) a1[b] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < G1; ++g) {
            const char* sl = sync(g, false);
            const p1f4 x0 = sx[(2 * g) * 64], x1 = sx[(2 * g + 1) * 64];
            const WSX xb = ws_opnd(make_float4(x0[0], x0[1], x0[2], x0[3]), make_float4(x1[0], x1[1], x1[2], x1[3]), xfin);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                uint4 w0, w1, w2;
                R.frag(sl, b, w0, w1, w2);
                ws_prod(a1[b], w0, w1, w2, xb);
            }
        }
#pragma unroll
        for (int co = 0; co < 2; ++co) {
            const int c = 2 * sc + co;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const w2cf* bv = wh_cp(a.pb1) + 64 * c + 16 * b;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float c0 = wh_u(bv[i]), c1 = wh_u(bv[4 + i]), c2 = wh_u(bv[8 + i]), c3 = wh_u(bv[12 + i]);
                    const float lo = (q & 1) ? c1 : c0, hi = (q & 1) ? c3 : c2;
                    a1[4 * co + b][i] = elu_f(a1[4 * co + b][i] + ((q & 2) ? hi : lo));
                }
            }
            const floatx4* t = a1 + 4 * co;
            const bool hfin = ws_wave_finite(ws_sum8(make_float4(t[0][0], t[0][1], t[0][2], t[0][3]),
                                                     make_float4(t[1][0], t[1][1], t[1][2], t[1][3])) +
                                             ws_sum8(make_float4(t[2][0], t[2][1], t[2][2], t[2][3]),
                                                     make_float4(t[3][0], t[3][1], t[3][2], t[3][3])));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const floatx4& t0 = t[2 * s2];
                const floatx4& t1 = t[2 * s2 + 1];
                const WSX xb = ws_opnd(make_float4(t0[0], t0[1], t0[2], t0[3]), make_float4(t1[0], t1[1], t1[2], t1[3]), hfin);
#pragma unroll
                for (int jq = 0; jq < 4; ++jq) {
                    const char* sl = sync(G1 + 8 * co + 4 * s2 + jq, sc == 3 && co == 0 && s2 == 0 && jq == 0);
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) {
                        uint4 w0, w1, w2;
                        R.frag(sl, jj, w0, w1, w2);
                        ws_prod(acc[8 * jq + jj], w0, w1, w2, xb);
                    }
                }
            }
        }
    }
    int n_ep, q_ep;
    wr_lane_ep(R.voff, n_ep, q_ep);
    // ---- layer 3: mu = W3 h2 + b3 (NB3 16-column tiles), group-major fragments, 8 per step
    floatx4 a3[NB3];
#pragma unroll
    for (int j = 0; j < NB3; ++j) a3[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const char* sl = nullptr;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const float4 ha = wr_h2t(acc, sb2, 2 * g, q), hb = wr_h2t(acc, sb2, 2 * g + 1, q);
        const WSX xb = ws_opnd(ha, hb, ws_wave_finite(ws_sum8(ha, hb)));
#pragma unroll
        for (int jj = 0; jj < NB3; ++jj) {
            const int f = g * NB3 + jj;
            if (f % WS_NW == 0) sl = R.sync(src_tail(f / WS_NW + NS - 1));
            uint4 w0, w1, w2;
            R.frag(sl, f % WS_NW, w0, w1, w2);
            ws_prod(a3[jj], w0, w1, w2, xb);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (live) {
        // TOLD.pi + TruncatedNormal.sample(clip = 0.3) with the reference's roundings (the chain CH_PI epilogue's)
        const int m = m0 + n_ep, xr = xr0 + n_ep;
        const float* ep = a.eps + (size_t)(m / J.eps_G) * J.eps_env + J.eps_off + (size_t)(m % J.eps_G) * a.A;
        float* xo = a.X + (size_t)(xr >> 5) * a.x_ts + (xr & 31) * 4;
#pragma unroll
        for (int jj = 0; jj < NB3; ++jj) {
            const int cq = 4 * jj + q_ep, col = 4 * cq;
            if (col < a.Ap) {   // (the pad columns [A, Ap) written as 0, as the chain CH_PI epilogue does)
                const float4 bv = *(const float4*)(sb3 + col);
                const float o4[4] = {a3[jj][0] + bv.x, a3[jj][1] + bv.y, a3[jj][2] + bv.z, a3[jj][3] + bv.w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = 0.f;
                    if (col + e < a.A) {
                        const float muv = tanhf(o4[e]);
                        x = muv;
                        if (a.min_std > 0.f) {
                            const float ee = tclamp(fmul(ep[col + e], a.min_std), -0.3f, 0.3f);
                            x = tclamp(fadd(muv, ee), a.lo, a.hi);
                        }
                    }
                    o[e] = x;
                }
                *(float4*)(xo + (size_t)cq * 128) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------- WH_Q
template <int G1, int NST, int GX>
DEVI void wh_q(const WHArgs& a, const WHJob& J, int rb, char* wsm) {
    constexpr int NS = ws_ns<GX>();
    constexpr int SPC2 = G1 + 16;
    constexpr int NSS = WH_STATS_ON * (NST / 8) * G1;   // statistics steps: 8 blocks x one k group each
    static_assert(NST % 8 == 0 && NS >= 3 && NS - 1 < SPC2 && NS - 1 <= NSS + SPC2, "ring depth");
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const WHQHead Hd = J.head ? a.q[1] : a.q[0];   // (selects: no dynamic index into the kernel arguments)
    p1f4* sx = (p1f4*)(wsm + NS * WS_SLOT) + wave * (G1 * 2 * 64) + lane;
    const float* sv = (const float*)(wsm + NS * WS_SLOT);   // b2 | g2 | be2 | w3 [512] each (after the last first layer)
    const int m0 = rb * 128 + wave * 16;
    const bool live = m0 < J.rows;
    const int xr0 = live ? map_row(J.map, m0) : 0;
    WRing<NS, WS_SLOT, 3 * (NS - 3), w2_glds> R(wsm, lane, wave);
    // the static fragment stream: NSS statistics steps, then 4 super-chunks of G1 + 16 steps, then dummies
    auto src_main2 = [&](int sc, int j) __attribute__((always_inline)) { return wr_src<G1>(Hd.X1, a.qg1s, Hd.X2, wave, sc, j); };
    auto src_tail = [&](int) __attribute__((always_inline)) { return Hd.X2; };
    auto src_abs = [&](int j) __attribute__((always_inline)) -> const unsigned short* {   // step j of the stream
        if (j < NSS) return Hd.S + ((size_t)(8 * (j / G1) + wave) * a.qg1s + j % G1) * 1536;
        return src_main2((j - NSS) / SPC2, (j - NSS) % SPC2);
    };
#pragma unroll
    for (int k = 0; k < NS - 1; ++k) R.issue(k, src_abs(k));
    const bool xfin = wr_xtile<G1>(sx, a.X, a.x_ts, xr0, n, q, 0, a.qkq, live);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    R.prime();
    // the lane's 4 features of tile t (16t + 4q + i) of a per-feature vector, by scalar loads
    const bool qb0 = (q & 1) != 0, qb1 = (q & 2) != 0;
    const w2cf* vb1 = wh_cp(Hd.b1);
    const w2cf* vbe1 = wh_cp(Hd.be1);
    const w2cf* vbs = wh_cp(Hd.bs);
    // (each candidate made uniform first: otherwise hipcc turns the select of four loads into one per-lane load from a
    // selected address -- a vector load with exec-masked branches around it)
    auto vec4 = [&](const w2cf* v, int t, int i) __attribute__((always_inline)) -> float {
        const w2cf* p = v + 16 * t;
        const float c0 = wh_u(p[i]), c1 = wh_u(p[4 + i]), c2 = wh_u(p[8 + i]), c3 = wh_u(p[12 + i]);
        const float lo = qb0 ? c1 : c0, hi = qb0 ? c3 : c2;   // (two-level select on the lane's q bits)
        return qb1 ? hi : lo;
    };

    // ---- statistics block: s_1.. = R [x; 1], var = sum_{i >= 1} s_i^2 / M (s_0, the mean of layer 1's M outputs, is
    // streamed with the block but unused: the folded first layer below yields y - mean directly)
    float mean_l = 0.f, ssq = 0.f;
#pragma unroll
    for (int ss = 0; ss < WH_STATS_ON * NST / 8; ++ss) {
        floatx4 as[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) as[b] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < G1; ++g) {
            const char* sl = R.sync(src_abs(ss * G1 + g + NS - 1));
            const p1f4 x0 = sx[(2 * g) * 64], x1 = sx[(2 * g + 1) * 64];
            const WSX xb = ws_opnd(make_float4(x0[0], x0[1], x0[2], x0[3]), make_float4(x1[0], x1[1], x1[2], x1[3]), xfin);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                uint4 w0, w1, w2;
                R.frag(sl, b, w0, w1, w2);
                ws_prod(as[b], w0, w1, w2, xb);
            }
        }
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = as[b][i] + vec4(vbs, 8 * ss + b, i);
                if (ss == 0 && b == 0 && i == 0) mean_l = s;   // (feature 0 sits in lanes q = 0)
                else ssq += s * s;
            }
    }
    // (lanes q = 1..3 hold feature 4q of tile 0, a variance row, in mean_l's place: add it back)
    if (q != 0) ssq += mean_l * mean_l;
    ssq += __shfl_xor(ssq, 16);
    ssq += __shfl_xor(ssq, 32);
    const float rs1 = 1.0f / sqrtf(ssq / 512.f + 1e-5f);
    (void)mean_l;   // (row 0 of the block, the mean, is folded into the first layer: see the chunk epilogue)

    floatx4 acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int sc = 0; sc < 4; ++sc) {
        auto sync = [&](int j, bool tail_bias) __attribute__((always_inline)) {
            return R.sync(wr_next<G1, NS>(src_main2, src_tail, sc, j), [&](int) __attribute__((always_inline)) {
                if (tail_bias) {   // b2 | g2 | be2 | w3 into the dead x tile: one 1 KiB LDS-DMA per wave
                    const float* vs[4] = {Hd.b2, Hd.g2, Hd.be2, Hd.w3};
                    w2_glds(vs[wave >> 1] + 256 * (wave & 1), R.voff, R.lds + (unsigned)(NS * WS_SLOT) + wave * 1024);
                }
            });
        };
        floatx4 a1[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) a1[b] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < G1; ++g) {
            const char* sl = sync(g, false);
            const p1f4 x0 = sx[(2 * g) * 64], x1 = sx[(2 * g + 1) * 64];
            const WSX xb = ws_opnd(make_float4(x0[0], x0[1], x0[2], x0[3]), make_float4(x1[0], x1[1], x1[2], x1[3]), xfin);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                uint4 w0, w1, w2;
                R.frag(sl, b, w0, w1, w2);
                ws_prod(a1[b], w0, w1, w2, xb);
            }
        }
#pragma unroll
        for (int co = 0; co < 2; ++co) {
            const int c = 2 * sc + co;
            // h1 chunk c = tanh(LN(y)) = tanh(g1 (y - mean) rstd + be1): the folded layer gives u = g1 (y - mean)
            // directly (u = diag(g1) (W1 - 1 wbar^T) x + g1 (b1 - bbar)), so the epilogue is u rstd + be1
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = a1[4 * co + b][i] + vec4(vb1, 4 * c + b, i);
#ifndef WH_DIAG_ELU
                    a1[4 * co + b][i] = tanh_f(fadd(fmul(v, rs1), vec4(vbe1, 4 * c + b, i)));
#else
                    a1[4 * co + b][i] = elu_f(v);
#endif
                }
            const floatx4* t = a1 + 4 * co;
            const bool hfin = ws_wave_finite(ws_sum8(make_float4(t[0][0], t[0][1], t[0][2], t[0][3]),
                                                     make_float4(t[1][0], t[1][1], t[1][2], t[1][3])) +
                                             ws_sum8(make_float4(t[2][0], t[2][1], t[2][2], t[2][3]),
                                                     make_float4(t[3][0], t[3][1], t[3][2], t[3][3])));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const floatx4& t0 = t[2 * s2];
                const floatx4& t1 = t[2 * s2 + 1];
                const WSX xb = ws_opnd(make_float4(t0[0], t0[1], t0[2], t0[3]), make_float4(t1[0], t1[1], t1[2], t1[3]), hfin);
#pragma unroll
                for (int jq = 0; jq < 4; ++jq) {
                    const char* sl = sync(G1 + 8 * co + 4 * s2 + jq, sc == 3 && co == 0 && s2 == 0 && jq == 0);
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) {
                        uint4 w0, w1, w2;
                        R.frag(sl, jj, w0, w1, w2);
                        ws_prod(acc[8 * jq + jj], w0, w1, w2, xb);
                    }
                }
            }
        }
    }
    // the ring's dummy refills and the vectors' DMA landed; every wave's DMA visible
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    int n_ep, q_ep;
    wr_lane_ep(R.voff, n_ep, q_ep);
    auto lv = [&](int vsel, int t) __attribute__((always_inline)) -> float4 {
        return *(const float4*)(sv + vsel * 512 + 16 * t + 4 * q_ep);
    };
#ifdef WH_DIAG_NOLN2
    if (live && q_ep == 0) a.qv[(size_t)J.head * a.q_ld + xr0 + n_ep] = acc[0][0] + acc[31][3] + rs1;
    return;
#endif
    // ---- LN2 (two-pass moments over the row's 512 values: 128 per lane x the 4 q-lanes), ELU, Linear(M -> 1)
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const float4 bv = lv(0, t);
        acc[t][0] += bv.x; acc[t][1] += bv.y; acc[t][2] += bv.z; acc[t][3] += bv.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += acc[t][i];
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    const float mean2 = s / 512.f;
    float v2 = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = acc[t][i] - mean2;
            v2 += d * d;
        }
    v2 += __shfl_xor(v2, 16);
    v2 += __shfl_xor(v2, 32);
    const float rs2 = 1.0f / sqrtf(v2 / 512.f + 1e-5f);
    const float sh2 = -rs2 * mean2;
    float o = 0.f;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const float4 gv = lv(1, t), bv = lv(2, t), wv = lv(3, t);
        const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
        float y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = elu_f(fadd(fmul(fadd(fmul(acc[t][i], rs2), sh2), gg[i]), bb[i]));
        o += (y[0] * wv.x + y[1] * wv.y) + (y[2] * wv.z + y[3] * wv.w);
    }
    o += __shfl_xor(o, 16);
    o += __shfl_xor(o, 32);
    if (live && q_ep == 0) a.qv[(size_t)J.head * a.q_ld + xr0 + n_ep] = o + Hd.b3[0];
}

// The launch: block b runs the job whose XCD groups hold b % 8, on its 128-row block (b >> 3) nx + (b % 8 - x0).
template <int G1P, int NB3P, int G1Q, int NSTQ>
__global__ void __launch_bounds__(64 * WS_NW) __attribute__((amdgpu_waves_per_eu(2, 2)))
wide_heads_kernel(const WHArgs a) {
    constexpr int GX = G1P > G1Q ? G1P : G1Q;
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int bid = blockIdx.x, xg = bid & 7, slot = bid >> 3;
    int j = -1;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (i < a.njob && xg >= a.job[i].x0 && xg < a.job[i].x0 + a.job[i].nx) j = i;
    if (j < 0) return;
    const WHJob J = j == 0 ? a.job[0] : j == 1 ? a.job[1] : a.job[2];   // (selects, as above)
    const int rb = slot * J.nx + (xg - J.x0);
    if (rb >= J.nrb) return;   // (uniform per workgroup)
    if (J.role == WH_PI) wh_pi<G1P, NB3P, GX>(a, J, rb, wsm);
    else wh_q<G1Q, NSTQ, GX>(a, J, rb, wsm);
}

// instantiated (pi first-layer 32-k groups, pi last-layer 16-row tiles, Q first-layer groups, statistics tiles):
// humanoid L100 A21, dog L100 A38, cheetah L50 A6, quadruped L50 A12
#define WIDE_HEADS_FOR_EACH(X) X(4, 2, 4, 8) X(4, 3, 5, 16) X(2, 1, 2, 8) X(2, 1, 3, 8)

// ------------------------------------------------------------------------------ statistics block (the pack)
// Real first-layer columns of helper.q (the panel's [a | 0 | z | 0] without the padding) and the bias column.
__host__ __device__ inline int qs_col(int i, int A, int L, int Ap) { return i < A ? i : i < A + L ? Ap + (i - A) : -1; }
// panel element (r, k) of a [rows][pk] fp32 panel ([r/32][k/4][r%32][k%4])
__host__ __device__ inline size_t qs_pidx(int r, int k, int pk) {
    return ((size_t)(r >> 5) * (pk / 4) + (k >> 2)) * 128 + (r & 31) * 4 + (k & 3);
}

struct QStatArgs {
    const float* W1;    // packed Q first-layer panel [2M][Kx]
    const float* b1;    // [2M]
    double* gram;       // [2][n][n] (upper triangle)
    int M, Kx, A, L, Ap, n;
    unsigned short* S;  // x6q statistics blocks [2][nsr][g1s groups]
    float* bs;          // [2][nsr]
    int nsr, g1s;
    unsigned short* F;  // x6q folded first layers diag(g1) (W1 - 1 wbar^T) [2][M][g1s groups]
    float* bf;          // g1 (b1 - bbar) [2][M]
    const float* g1;    // LayerNorm-1 gamma [2][M]
};

// value of column i (< n) of head h's [W1 | b1] at output m
DEVI float qs_val(const QStatArgs& a, int h, int m, int i) {
    const int k = qs_col(i, a.A, a.L, a.Ap);
    return k >= 0 ? a.W1[qs_pidx(h * a.M + m, k, a.Kx)] : a.b1[h * a.M + m];
}

// the column means of head h's columns [c0, c0 + 32) over the M outputs, fp64, fixed order (8 partial sums per column
// over rows m = p (mod 8), summed in order) -> mu[32]
DEVI void qs_means(const QStatArgs& a, int h, int c0, double* mu, double* part) {
    const int tid = threadIdx.x, col = tid & 31, p = tid >> 5;   // 256 threads: 32 columns x 8 row phases
    double s = 0.0;
    if (c0 + col < a.n)
        for (int m = p; m < a.M; m += 8) s += (double)qs_val(a, h, m, c0 + col);
    part[p * 32 + col] = s;
    __syncthreads();
    if (tid < 32) {
        double t = 0.0;
        for (int q = 0; q < 8; ++q) t += part[q * 32 + tid];
        mu[tid] = t / a.M;
    }
    __syncthreads();
}

// G = C^T C of head blockIdx.z, 16 x 16 tiles (blockIdx.x <= blockIdx.y), fp64; C = [W1 | b1] minus its column means
__global__ void __launch_bounds__(256) qstat_gram_kernel(const QStatArgs a) {
    const int h = blockIdx.z, bi = blockIdx.x, bj = blockIdx.y;
    if (bi > bj) return;
    __shared__ double mu[2][32], part[256], ci[32][17], cj[32][17];
    qs_means(a, h, 16 * bi, mu[0], part);   // mu[0][0..15]: the tile's i columns
    qs_means(a, h, 16 * bj, mu[1], part);
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
    double g = 0.0;
    for (int m0 = 0; m0 < a.M; m0 += 32) {
        for (int e = tid; e < 32 * 32; e += 256) {   // rows m0.. m0 + 31 of the 16 i and 16 j columns, centred
            const int r = e >> 5, c = e & 31;
            const int col = c < 16 ? 16 * bi + c : 16 * bj + c - 16;
            const double v = col < a.n ? (double)qs_val(a, h, m0 + r, col) - (c < 16 ? mu[0][c] : mu[1][c - 16]) : 0.0;
            if (c < 16) ci[r][c] = v;
            else cj[r][c - 16] = v;
        }
        __syncthreads();
        for (int r = 0; r < 32; ++r) g += ci[r][ti] * cj[r][tj];
        __syncthreads();
    }
    const int i = 16 * bi + ti, j = 16 * bj + tj;
    if (i < a.n && j < a.n && i <= j) a.gram[((size_t)h * a.n + i) * a.n + j] = g;
}

// Cholesky G = R^T R (upper, in LDS, packed by rows; a pivot <= 1e-13 of the largest diagonal -> a zero row: C^T C is
// positive semi-definite, so its remaining column is zero too), then the statistics block of head blockIdx.x:
// row 0 = the column means (mean of layer 1 = wbar . x + bbar; kept in the block, the kernel's folded first layer no
// longer reads it), rows 1 + i = R's row i, in the x6q layout; then the folded first layer diag(g1) (W1 - 1 wbar^T).
__global__ void __launch_bounds__(1024) qstat_chol_kernel(const QStatArgs a) {
    extern __shared__ double U[];   // n (n + 1) / 2 upper-packed, then the n column means
    const int h = blockIdx.x, n = a.n, tid = threadIdx.x;
    auto ix = [n](int i, int j) { return (size_t)i * n - (size_t)i * (i - 1) / 2 + (j - i); };
    double* mu = U + (size_t)n * (n + 1) / 2;
    for (int i = 0; i < n; ++i)
        for (int j = i + tid; j < n; j += 1024) U[ix(i, j)] = a.gram[((size_t)h * n + i) * n + j];
    // column means (the gram kernel's order: 8 row phases summed in order)
    for (int c = tid; c < n; c += 1024) {
        double t = 0.0;
        for (int p = 0; p < 8; ++p) {
            double s = 0.0;
            for (int m = p; m < a.M; m += 8) s += (double)qs_val(a, h, m, c);
            t += s;
        }
        mu[c] = t / a.M;
    }
    __syncthreads();
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = fmax(dmax, U[ix(i, i)]);
    for (int k = 0; k < n; ++k) {
        const double d = U[ix(k, k)];
        const double r = d > 1e-13 * dmax ? sqrt(d) : 0.0;
        const double inv = r > 0.0 ? 1.0 / r : 0.0;
        __syncthreads();   // (every thread has read d)
        for (int j = k + 1 + tid; j < n; j += 1024) U[ix(k, j)] *= inv;
        if (tid == 0) U[ix(k, k)] = r;
        __syncthreads();
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += 1024) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (i <= j) U[ix(i, j)] -= U[ix(k, i)] * U[ix(k, j)];
        }
        __syncthreads();
    }
    // the block: element (r, kk) of the [nsr][32 g1s] panel into the x6q layout
    const int G = a.g1s, K = 32 * G;
    unsigned short* d = a.S + (size_t)h * (a.nsr / 16) * G * 1536;
    for (int e = tid; e < a.nsr * K; e += 1024) {
        const int r = e / K, kk = e % K;
        double v = 0.0;
        // the real column at panel column kk (qs_col's inverse)
        const int src = kk < a.A ? kk : kk >= a.Ap && kk < a.Ap + a.L ? a.A + kk - a.Ap : -1;
        if (src >= 0) {
            if (r == 0) v = mu[src];
            else if (r - 1 < n && src >= r - 1) v = U[ix(r - 1, src)];
        }
        x6q_put(d, G, r, kk, (float)v);
    }
    for (int r = tid; r < a.nsr; r += 1024)
        a.bs[h * a.nsr + r] = r == 0 ? (float)mu[n - 1] : r - 1 < n ? (float)U[ix(r - 1, n - 1)] : 0.f;
    // the folded first layer: row m = g1[m] (W1[m] - wbar) over the real columns, bias g1[m] (b1[m] - bbar)
    unsigned short* f = a.F + (size_t)h * (a.M / 16) * G * 1536;
    for (int e = tid; e < a.M * K; e += 1024) {
        const int r = e / K, kk = e % K;
        const int src = kk < a.A ? kk : kk >= a.Ap && kk < a.Ap + a.L ? a.A + kk - a.Ap : -1;
        const double g = (double)a.g1[h * a.M + r];
        const double v = src >= 0 ? g * ((double)a.W1[qs_pidx(h * a.M + r, kk, a.Kx)] - mu[src]) : 0.0;
        x6q_put(f, G, r, kk, (float)v);
    }
    for (int r = tid; r < a.M; r += 1024)
        a.bf[h * a.M + r] = (float)((double)a.g1[h * a.M + r] * ((double)a.b1[h * a.M + r] - mu[n - 1]));
}
