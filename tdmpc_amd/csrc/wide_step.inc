// wide_step.inc -- included by tdmpc_kernels.hip inside its anonymous namespace after wide_ring.inc (the design: the
// LDS weight ring with its read-ahead, the static fragment stream, the x tile and the shape of the two-layer
// super-chunk and of the group-major last layer; uses also RowMap, elu_f and the reference-rounding helpers).
//
// TOLD.next (/root/reference/src/algorithm/tdmpc.py:34-37: _dynamics and _reward, helper.mlp helper.py:169-176) plus
// the return update of estimate_value (tdmpc.py:88-90) for the wide step launches (>= one 128-row block per CU and
// head: B >= 32 envs at N = 512), on 128-row workgroups.
//
// This kernel's own:
//  * Two heads per launch. Layer 3 of the dynamics head (M -> L, L rounded up to 16-row tiles) is the design's last
//    layer; the reward head's Linear(M -> 1) is a per-lane dot + two cross-lane shuffles (each wave holds whole rows:
//    no cross-wave sums).
//  * b1 comes by scalar loads; b2 / w3 / b3 are DMA'd into the x tile's place once the last super-chunk's first layer
//    is done.
//  * XCD-aware placement: dispatch groups 0-3 (blocks b with b % 8 < 4) run the dynamics head, 4-7 the reward head,
//    so each XCD's 4 MB L2 holds one head's x6 weights (2.3 / 1.9 MB) rather than both (4.2 MB). Speed only.
// Measured (profiles/r04/, DESIGN.md §4): 104 us per humanoid B = 32 launch (16,384 rows x 2 heads), MFMA busy 0.55;
// the losing variants of rounds 3-4 (paired fragments, pipelined splits, register-staged or spread fills,
// non-temporal fills, rotated chunk order, one-chunk first layer) live in git history and DESIGN.md §4's table.
// Shape limits (use_wide): M = 512, N and T multiples of 16 (a wave's 16 rows lie in one X panel block), first-layer
// 32-k groups <= 5, L in (48, 64] or (96, 112]; with the per-env first-layer bias (z0c, t = 0) env groups of whole
// workgroups.

// wide_step_kernel modes (template MODE bits):
//  WS_XS   the x operand streamed through the ring (latent 512: 17 first-layer 32-k groups, a 272 KB x tile, do not
//          fit LDS): every slot carries, beside its 8 weight fragments, each wave's x group of that step (2 x 1 KiB
//          LDS-DMA per wave, its own 16 rows); the x is re-streamed per super-chunk from L2.
//  WS_OUTH the dynamics head stops at h2 = ELU(W2 h1 + b2) and stores it where z' would go (X_{t+1}'s latent columns):
//          the next step's first layer is the folded [W1a | W1z W3] with bias b1 + W1z b3 (pack_fold), so z' is never
//          formed between steps (latent_dim = mlp_dim: the folded first layer costs what the plain one does, and layer 3
//          -- a third of the dynamics head -- runs only at the last step). DESIGN.md §4.
enum { WS_XS = 1, WS_OUTH = 2 };
constexpr int WS_XAREA = WS_NW * 2048;   // WS_XS: a slot's x area, [8 waves][2 halves][64 lanes] float4
template <int G1, int MODE> constexpr int wsm_slot() { return (MODE & WS_XS) ? WS_SLOT + WS_XAREA : WS_SLOT; }
template <int G1, int MODE> constexpr int wsm_ns() {
    return (MODE & WS_XS) ? (160 * 1024 / wsm_slot<G1, MODE>() < 6 ? 160 * 1024 / wsm_slot<G1, MODE>() : 6) : ws_ns<G1>();
}
template <int G1, int MODE> constexpr size_t wsm_lds() {
    return (MODE & WS_XS) ? (size_t)wsm_ns<G1, MODE>() * wsm_slot<G1, MODE>() : ws_lds<G1>();
}
// the epilogue's biases b2 [512] | w3 [512] (reward) or b3 [<= 512] (dynamics): in the x tile's place, or (WS_XS) in
// the last slot's x area -- both dead once the last super-chunk's first layer is done
template <int G1, int MODE> constexpr int wsm_bias() {
    return (MODE & WS_XS) ? (wsm_ns<G1, MODE>() - 1) * wsm_slot<G1, MODE>() + WS_SLOT : ws_ns<G1>() * WS_SLOT;
}

// Timing diagnostics (results WRONG; python -m tdmpc_amd.build --variant NAME -DWS_DIAG_NODMA / -DWS_DIAG_NOSPLIT, which
// also defines TDMPC_VARIANT): no weight stream (stale fragments) / activation operands without the three-way split
#if (defined(WS_DIAG_NODMA) || defined(WS_DIAG_NOSPLIT)) && !defined(TDMPC_VARIANT)
#error "WS_DIAG_* diagnostics produce wrong results: build them only as a named variant (tdmpc_amd.build --variant)"
#endif

struct WideHead {
    const unsigned short* X1;   // first layer, this head's 32 blocks x g1s groups (x6q)
    const unsigned short* X2;   // hidden layer, 32 blocks x 16 groups (x6q)
    const float* b1; const float* b2;
    const float* w3v; const float* b3v;   // reward head: Linear(M -> 1)
};

struct WideArgs {
    WideHead p[2];
    const unsigned short* X3; const float* b3; int nvalid, nstore;   // dynamics last layer (Lr/16 blocks x 16 groups)
    int rows, nrb;               // logical rows; 128-row blocks per head
    RowMap amap;
    const float* X; long x_ts;   // X_t panel [rows/32][Kx/4][32][4]
    int kq;                      // first-layer input quads read (Kx/4; k1c/4 with z0c)
    int g1s;                     // x6q groups per first-layer block in memory
    float* Xo; int out_q0;       // X_{t+1} (same panel layout), latent columns from quad out_q0
    float* G; float* rlast; float disc; int first, last;
    const float* z0c; int z0_G;  // t = 0: the first layer's per-env bias (z0c_kernel), env = logical row / z0_G
    unsigned long long* stamps;  // diagnostic build (-DWS_STAMPS): per-step shader clocks of workgroups 0 and 4
};

// the step kernel's LDS-DMA: ws_glds where every step position is compile-time (SGPR operands), w2_glds elsewhere
template <bool SGPR>
DEVI void ws_dma(const void* gsrc, unsigned voff, unsigned lds) {
#ifndef WS_DIAG_NODMA
    if constexpr (SGPR) ws_glds(gsrc, voff, lds);
    else w2_glds(gsrc, voff, lds);
#else
    (void)gsrc; (void)voff; (void)lds;
#endif
}

template <int G1, int NB3, int MODE>
__global__ void __launch_bounds__(64 * WS_NW) __attribute__((amdgpu_waves_per_eu(2, 2)))
wide_step_kernel(const WideArgs a) {
    constexpr bool XS = (MODE & WS_XS) != 0, OUTH = (MODE & WS_OUTH) != 0;
    constexpr int WS_NS = wsm_ns<G1, MODE>();
    constexpr int SLOT = wsm_slot<G1, MODE>();
    // DMA instructions a wave leaves in flight at a step's wait: steps k and k + 1 landed at step k's barrier (step
    // k + 1's first fragment is read during step k). WS_XS: at most step k + 2's refill (3 weight DMAs, + 2 x DMAs on a
    // first-layer step, of which vmcnt(3) lets the x pair or the first two weight DMAs land early -- stricter, still exact)
    constexpr int VM = XS ? 3 : 3 * (WS_NS - 3);
    constexpr int SPC2 = G1 + 16;   // steps per super-chunk
    // the dynamics head's layer 3 after the last super-chunk: NB3 <= 8 tiles in one group-major pass (2 NB3 steps of 8
    // fragments), or (latent 512) NB3 / 8 passes of 8 tiles over the 16 k groups (16 steps each, h2's operand split
    // again per pass: a3 stays at 8 tiles beside the 32 of h2); none with WS_OUTH
    constexpr int NP3 = NB3 > 8 ? NB3 / 8 : 1;
    constexpr int TAIL = OUTH ? 0 : (NB3 > 8 ? 16 * NP3 : 2 * NB3);
    static_assert(NB3 <= 8 || NB3 % 8 == 0, "layer-3 passes of 8 tiles");
    static_assert(WS_NS >= 3 && WS_NS - 1 < SPC2, "ring depth");
    static_assert(wsm_lds<G1, MODE>() <= 160 * 1024, "wide step LDS");
    static_assert(XS ? WS_XAREA >= 6 * 1024 : ws_xbytes<G1>() >= 6 * 1024, "bias area");
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform: every address below derived from it is scalar)
    const int bid = blockIdx.x;
    const int head = (bid & 7) >> 2;                  // dispatch groups 0-3: dynamics, 4-7: reward (XCD-aware)
    const int rb = (bid >> 3) * 4 + (bid & 3);
    if (rb >= a.nrb) return;                          // (grid padded to whole dispatch groups; uniform per workgroup)
    const WideHead& P = a.p[head];
    // this lane's x (not WS_XS): group g at [2g], [2g + 1]
    p1f4* sx = (p1f4*)(wsm + WS_NS * WS_SLOT) + wave * (G1 * 2 * 64) + lane;
    const float* sb2 = (const float*)(wsm + wsm_bias<G1, MODE>());   // [512] (after the chunk loop)
    const float* sw3 = sb2 + 512;                     // [512] reward head weights
    const float* sb3 = sw3 + 512;                     // [16 NB3] dynamics last-layer bias (cols >= L: don't care)
    const int m0 = rb * 128 + wave * 16;
    const bool live = m0 < a.rows;                    // (rows are a multiple of 16: a wave is all live or all idle)
    const int xr0 = live ? map_row(a.amap, m0) : 0;   // its 16 rows lie in one X panel block

    // ---- the first steps' weights in flight first (LDS-DMA), then the wave's input rows, biases and G
    WRing<WS_NS, SLOT, VM, ws_dma<MODE == 0 && NB3 <= 8>> R(wsm, lane, wave);
    auto src_main2 = [&](int sc, int j) __attribute__((always_inline)) { return wr_src<G1>(P.X1, a.g1s, P.X2, wave, sc, j); };
    // the stream's tail: the dynamics head's layer 3 after the last super-chunk, then dummy refills
    auto src_tail = [&](int l) __attribute__((always_inline)) -> const unsigned short* {
        if (!OUTH && head == 0 && l < TAIL) {
            if constexpr (NB3 > 8) {   // pass p = l / 16 over group g = l % 16: tile 8p + wave
                return a.X3 + ((size_t)(8 * (l >> 4) + wave) * 16 + (l & 15)) * 1536;
            } else {
                return wr_l3_src<NB3>(a.X3, l, wave);
            }
        }
        return P.X2;
    };
    auto src_next2 = [&](int sc, int j) __attribute__((always_inline)) { return wr_next<G1, WS_NS>(src_main2, src_tail, sc, j); };
    // WS_XS: first-layer steps stream their x beside the weights -- the wave's x rows of group xg (row block base by
    // SGPR, row and quad by lane offset; quads past the input clamped to a valid address and zeroed after the read) into
    // the x area of step kk's slot
    const float* xrow = a.X + (size_t)(xr0 >> 5) * a.x_ts;
    const unsigned xlo = (unsigned)(((xr0 & 31) + n) * 16);
    auto issue_x = [&](int kk, int xg) __attribute__((always_inline)) {
        if constexpr (XS) {
            if (xg >= 0) {
                const unsigned xdst = R.lds + (unsigned)((kk % WS_NS) * SLOT + WS_SLOT + wave * 2048);
                const int qa = min(8 * xg + q, a.kq - 1), qb = min(8 * xg + 4 + q, a.kq - 1);
                ws_dma<false>(xrow, xlo + (unsigned)qa * 512u, xdst);
                ws_dma<false>(xrow, xlo + (unsigned)qb * 512u, xdst + 1024);
            }
        }
    };
    // the x group of step j's refill target (step j + WS_NS - 1 of super-chunk sc, or of the next one), or -1
    auto xg_next2 = [&](int sc, int j) __attribute__((always_inline)) -> int {
        const int jt = j + WS_NS - 1;
        if (jt < SPC2) return jt < G1 ? jt : -1;
        return sc < 3 && jt - SPC2 < G1 ? jt - SPC2 : -1;
    };
#pragma unroll
    for (int k = 0; k < WS_NS - 1; ++k) {
        R.issue(k, src_main2(0, k));
        issue_x(k, k < G1 ? k : -1);
    }
    bool xfin = true;
    if constexpr (!XS) xfin = wr_xtile<G1>(sx, a.X, a.x_ts, xr0, n, q, 0, a.kq, live);
    // b1: the head's bias, or per env with z0c (t = 0)
    const float* b1src = a.z0c ? a.z0c + ((size_t)(rb * 128 < a.rows ? rb * 128 / a.z0_G : 0) * 2 + head) * 512
                               : P.b1;
    float g_old = 0.f;
    if (head == 1 && q == 0 && live && !a.first) g_old = a.G[xr0 + n];
    // (the asm use makes hipcc wait for g_old here, not at its first use among the counted DMA waits)
    asm volatile("" :: "v"(g_old));
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // prologue DMA + x visible
#ifdef WS_STAMPS
    // diagnostic: lane 0 of every wave of workgroups 0 (dynamics) and 4 (reward)
    if (a.stamps && (bid == 0 || bid == 4) && lane == 0) R.st = a.stamps + (bid ? 4096 : 0) + wave * 512;
#endif
    R.prime();

    floatx4 acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int sc = 0; sc < 4; ++sc) {
        auto sync = [&](int j, bool tail_bias) __attribute__((always_inline)) {
            return R.sync(src_next2(sc, j), [&](int kk) __attribute__((always_inline)) {
                issue_x(kk, xg_next2(sc, j));
                if (tail_bias && wave < 4) {
                    // the epilogue's biases into the (now dead) x tile / x area, one 1 KiB LDS-DMA by each of waves 0-3
                    // (landed and visible after the sync VM / 3 steps later, still inside this chunk): b2 (waves 0, 1),
                    // then w3 (reward) or b3 (dynamics: 256 floats per wave, as many as its 16 NB3 columns need; none
                    // with WS_OUTH)
                    const float* bsrc = wave < 2 ? P.b2 + 256 * wave : head == 1 ? P.w3v + 256 * (wave - 2) : a.b3 + 256 * (wave - 2);
                    const unsigned bdst = R.lds + (unsigned)wsm_bias<G1, MODE>() + (unsigned)(wave < 2 || head == 1 ? wave : wave + 2) * 1024;
                    if (wave < 2 || head == 1 || (!OUTH && (wave - 2) * 256 < 16 * NB3))
                        ws_dma<MODE == 0 && NB3 <= 8>(bsrc, R.voff, bdst);
                }
            });
        };
        floatx4 a1[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) a1[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        // (WS_XS: a runtime loop over the 17 groups -- the code of one step, not 17 -- x read from the step's slot)
        // (unrolled: XS x2 / x17 174 vs 156.5 us, profiles/r06/l512_xs_unroll_ab.txt; rolled at L100 101.8 vs 99.5 us)
        constexpr int UG1 = XS ? 1 : G1;
#pragma unroll UG1
        for (int g = 0; g < G1; ++g) {
            const char* sl = sync(g, false);
            p1f4 x0, x1;
            bool fin = xfin;
            if constexpr (XS) {
                const p1f4 zero4 = {0.f, 0.f, 0.f, 0.f};
                const p1f4* xs = (const p1f4*)(sl + WS_SLOT + wave * 2048);   // (sl: slot + lane * 16)
                x0 = xs[0];
                x1 = xs[64];
                if (!live || 8 * g + q >= a.kq) x0 = zero4;
                if (!live || 8 * g + 4 + q >= a.kq) x1 = zero4;
                fin = ws_wave_finite(((x0[0] + x0[1]) + (x0[2] + x0[3])) + ((x1[0] + x1[1]) + (x1[2] + x1[3])));
            } else {
                x0 = sx[(2 * g) * 64];
                x1 = sx[(2 * g + 1) * 64];
            }
            const WSX xb = ws_opnd(make_float4(x0[0], x0[1], x0[2], x0[3]), make_float4(x1[0], x1[1], x1[2], x1[3]), fin);
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
            // h1 chunk c = ELU(. + b1): tile b of the chunk holds features 64c + 16b + 4q + i
            // (b1 by scalar loads through the constant address space)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const w2cf* bv = (const w2cf*)b1src + 64 * c + 16 * b;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a1[4 * co + b][i] = elu_f(a1[4 * co + b][i] + (q == 0 ? bv[i] : q == 1 ? bv[4 + i] : q == 2 ? bv[8 + i] : bv[12 + i]));
            }
            const floatx4* t = a1 + 4 * co;
            const bool hfin = ws_wave_finite(ws_sum8(make_float4(t[0][0], t[0][1], t[0][2], t[0][3]),
                                                     make_float4(t[1][0], t[1][1], t[1][2], t[1][3])) +
                                             ws_sum8(make_float4(t[2][0], t[2][1], t[2][2], t[2][3]),
                                                     make_float4(t[3][0], t[3][1], t[3][2], t[3][3])));
            // layer 2 over k groups 2c + s2 (tiles 2 s2, 2 s2 + 1 of the chunk); 32 output tiles, 8 per step
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const floatx4& t0 = t[2 * s2];
                const floatx4& t1 = t[2 * s2 + 1];
                const WSX xb = ws_opnd(make_float4(t0[0], t0[1], t0[2], t0[3]), make_float4(t1[0], t1[1], t1[2], t1[3]), hfin);
#pragma unroll
                for (int jq = 0; jq < 4; ++jq) {
                    const int j2 = G1 + 8 * co + 4 * s2 + jq;
                    const char* sl = sync(j2, sc == 3 && co == 0 && s2 == 0 && jq == 0);
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

    if (head == 0 && OUTH) {
        // ---- WS_OUTH: h2 where z' would go (X_{t+1}'s latent columns Ap .. Ap + 511), for the folded first layer next
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the ring's dummy refills) before the workgroup ends
        if (live) {
            const int xr = xr0 + n_ep;
            float* xo = a.Xo + (size_t)(xr >> 5) * a.x_ts + (xr & 31) * 4;
#pragma unroll
            for (int t = 0; t < 32; ++t) *(float4*)(xo + (size_t)(a.out_q0 + 4 * t + q_ep) * 128) = wr_h2t(acc, sb2, t, q);
        }
    } else if (head == 0 && NB3 > 8) {
        // ---- dynamics layer 3 in NP3 passes of 8 output tiles: pass p's tiles 8p .. 8p + 7 over the 16 k groups, one
        // step (8 fragments, one per tile) per group, the group's h2 operand split again in every pass
        floatx4 a3[8];
        const char* sl = nullptr;
#pragma unroll 1
        for (int p = 0; p < NP3; ++p) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a3[j] = floatx4{0.f, 0.f, 0.f, 0.f};
            auto l3group = [&](int g) __attribute__((always_inline)) {
                const float4 ha = wr_h2t(acc, sb2, 2 * g, q), hb = wr_h2t(acc, sb2, 2 * g + 1, q);
                const WSX xb = ws_opnd(ha, hb, ws_wave_finite(ws_sum8(ha, hb)));
                sl = R.sync(src_tail(16 * p + g + WS_NS - 1));
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    uint4 w0, w1, w2;
                    R.frag(sl, jj, w0, w1, w2);
                    ws_prod(a3[jj], w0, w1, w2, xb);
                }
            };
#pragma unroll
            for (int g = 0; g < 8; ++g) l3group(g);
#pragma unroll
            for (int g = 8; g < 16; ++g) l3group(g);
            if (live) {
                const int xr = xr0 + n_ep;
                float* xo = a.Xo + (size_t)(xr >> 5) * a.x_ts + (xr & 31) * 4;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int cq = 4 * (8 * p + jj) + q_ep, col = 4 * cq;
                    if (col < a.nstore) {
                        const float4 bv = *(const float4*)(sb3 + col);   // (cols >= nvalid zeroed below)
                        float o[4] = {a3[jj][0] + bv.x, a3[jj][1] + bv.y, a3[jj][2] + bv.z, a3[jj][3] + bv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e >= a.nvalid) o[e] = 0.f;
                        *(float4*)(xo + (size_t)(a.out_q0 + cq) * 128) = make_float4(o[0], o[1], o[2], o[3]);
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the ring's dummy refills) before the workgroup ends
    } else if (head == 0) {
        // ---- dynamics layer 3: z' = W3 h2 + b3 (NB3 16-column tiles), group-major fragments f = 32-k group g x NB3
        // + tile, 8 per step; group g + 1's operand split over group g's fragments
        floatx4 a3[NB3 > 8 ? 1 : NB3];
        constexpr int NB = NB3 > 8 ? 1 : NB3;
#pragma unroll
        for (int j = 0; j < NB; ++j) a3[j] = floatx4{0.f, 0.f, 0.f, 0.f};
        WSX xb;
        const char* sl = nullptr;
        auto l3group = [&](int g) __attribute__((always_inline)) {
            const float4 ha = wr_h2t(acc, sb2, 2 * g, q), hb = wr_h2t(acc, sb2, 2 * g + 1, q);
            xb = ws_opnd(ha, hb, ws_wave_finite(ws_sum8(ha, hb)));
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int f = g * NB + jj;
                if (f % WS_NW == 0) sl = R.sync(src_tail(f / WS_NW + WS_NS - 1));
                uint4 w0, w1, w2;
                R.frag(sl, f % WS_NW, w0, w1, w2);
                ws_prod(a3[jj], w0, w1, w2, xb);
            }
        };
        // (two loops of 8 groups: each stays under the full-unroll size limit, which one loop of 16 x 7 tiles
        // exceeds -- a partly unrolled loop indexes the accumulators dynamically, i.e. through scratch)
#pragma unroll
        for (int g = 0; g < 8; ++g) l3group(g);
#pragma unroll
        for (int g = 8; g < 16; ++g) l3group(g);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the ring's dummy refills) before the workgroup ends
        if (live) {
            const int xr = xr0 + n_ep;
            float* xo = a.Xo + (size_t)(xr >> 5) * a.x_ts + (xr & 31) * 4;
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int cq = 4 * jj + q_ep, col = 4 * cq;
                if (col < a.nstore) {
                    const float4 bv = *(const float4*)(sb3 + col);   // (cols >= nvalid zeroed below)
                    float o[4] = {a3[jj][0] + bv.x, a3[jj][1] + bv.y, a3[jj][2] + bv.z, a3[jj][3] + bv.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e >= a.nvalid) o[e] = 0.f;
                    *(float4*)(xo + (size_t)(a.out_q0 + cq) * 128) = make_float4(o[0], o[1], o[2], o[3]);
                }
            }
        }
    } else {
        // ---- reward head: Linear(M -> 1) on the row (a lane holds a quarter of its row's 512 features)
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const float4 v = wr_h2t(acc, sb2, t, q);
            const float4 wv = *(const float4*)(sw3 + 16 * t + 4 * q_ep);
            s += (v.x * wv.x + v.y * wv.y) + (v.z * wv.z + v.w * wv.w);
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (live && q_ep == 0) {
            const int xr = xr0 + n_ep;
            const float o = s + P.b3v[0];
            const float dr = fmul(a.disc, o);   // G += discount * reward (tdmpc.py:89), float32(discount)
            a.G[xr] = a.first ? dr : fadd(g_old, dr);
            if (a.last) a.rlast[xr] = o;
        }
    }
}

// instantiated (first-layer 32-k groups, last-layer 16-row tiles, mode): humanoid / dog L100 (Kx 128 / 144 -> 4 / 5
// groups; t = 0 with z0c 1 / 2; 7 tiles), cheetah / quadruped L50 (Kx 64 / 72 -> 2 / 3; z0c 1; 4 tiles); humanoid
// latent 512 (Kx 536 -> 17 groups, x streamed; t = 0 with z0c 1; 32 tiles; h2 out between steps)
#define WIDE_FOR_EACH(X) X(1, 7, 0) X(2, 7, 0) X(4, 7, 0) X(5, 7, 0) X(1, 4, 0) X(2, 4, 0) X(3, 4, 0) \
    X(1, 32, 0) X(1, 32, WS_OUTH) X(17, 32, WS_XS) X(17, 32, WS_XS | WS_OUTH)
