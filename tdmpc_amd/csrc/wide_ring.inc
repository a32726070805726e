// wide_ring.inc -- included by tdmpc_kernels.hip inside its anonymous namespace, before wide_step.inc and
// wide_heads.inc (uses its X6B split, elu_f, the x6q weight layout and the wave-finite helpers).
//
// The design the wide kernels share (wide_step_kernel and the two roles of wide_heads_kernel), and its parts that are
// written once: the LDS weight ring with its read-ahead, the static fragment stream, the x tile and the epilogue's
// helpers. The two-layer super-chunk loop and the last layer stay written out in each kernel, on the ring's calls: as
// shared functions they compiled to different code (these kernels sit at the register limit; DESIGN.md §4).
//
// Why. chain_kernel carries a 32-row block through a head with the hidden activations in LDS; every workgroup streams
// the head's whole x6 weight set (2.3 MB for the dynamics head) from L2 into registers, so a CU needs 64 B/clk of
// weight fragments to keep its MFMA pipes busy and its vector-memory path delivers ~35 B/clk
// (profiles/r02/x6_stream_probe.txt): MFMA busy ~0.5, 0.42 of the x6 roof. Rows per weight fragment are what buy that
// back, and LDS (2 KB per fp32 hidden row) capped chain_kernel at 32.
//
// Design (one workgroup per CU, 8 waves = two per SIMD, 256 registers per lane):
//  * Each wave owns 16 ROWS and ALL 512 hidden columns: the hidden layer's accumulators (16 x 512 fp32 = 128
//    registers per lane, 32 tiles of v_mfma_f32_16x16x32_bf16) never leave registers, so the activations need no LDS.
//    Two waves per SIMD: one wave's activation splits, ELUs, LDS reads and barrier waits run under the other's MFMAs.
//  * Layer 1 streams into layer 2 by 64-column chunks: chunk c of h1 = act(W1[64c:64c+64] x + b1) is produced in
//    registers (4 accumulator tiles) and consumed at once as the 64-deep k slice [64c, 64c+64) of layer 2 -- the
//    accumulator-as-operand map: a lane of tile t holds features 16t + 4q + i (q = lane >> 4) of its row, so tiles 2s
//    and 2s + 1 together are the B operand of k group s in the x6q k order with no data movement.
//  * Paired chunks: super-chunk sc = chunks 2sc, 2sc + 1; its G1 first-layer steps take one k group each over the
//    pair's 8 W1 blocks (each group's operand split feeds 48 MFMAs, once per pair of chunks; 101.2 vs 102.8 us against
//    one chunk at a time), then the two chunks' 8 layer-2 steps each. Steps per super-chunk: G1 + 16.
//  * The last layer (M -> 16 NB columns, NB <= 8 tiles) reads h2 = ELU(acc + b2) from the same registers, its
//    fragments group-major.
//  * Weights: the head's x6q fragments (16 output features x 32 k x 3 bf16 planes = 3 KiB) are streamed from L2 into
//    an LDS ring ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave instruction, no VGPR) and read
//    by all 8 waves: 128 rows per fragment, 16 B/clk of L2 -> LDS traffic per CU at the full MFMA rate. Pipeline
//    step = 8 fragments (one loaded by each wave, 3 DMA instructions); per step: counted vmcnt (this wave's DMA of
//    the step and the next has landed) + one barrier (every wave's has; every wave is done with the slot about to be
//    refilled), then the refill of the step NS - 1 ahead, then 48 MFMAs per wave. The fragment stream is static
//    (super-chunk-major: W1 blocks 8sc..8sc+7 over the first-layer groups, then W2's 32 blocks over k groups
//    4sc..4sc+3; then the tail), its addresses resolved per step position at compile time, and every wave issues
//    exactly 3 DMA instructions per step, so the vmcnt count is a constant.
//  * Each wave reads the fragments two ahead of its products (the LDS latency runs under twelve MFMAs); a
//    sched_barrier pins the reads above the products they precede.
//  * The x tile (the wave's 16 input rows, fp32) sits in LDS beside the ring and is split into bf16 parts again by
//    super-chunk; the epilogue's per-feature vectors are DMA'd into its place once the last super-chunk's first layer
//    is done (each kernel's own tail-bias DMA).
//  * Products: the x6 form (six v_mfma_f32_16x16x32_bf16 per fp32 product, fp32 accumulation), non-finite-safe split
//    (split8) for every activation. The MFMAs are builtins (the compiler schedules them and their hazards); only the
//    LDS-DMA and the per-step wait are inline asm.

constexpr int WS_NW = 8;                         // waves, two per SIMD
constexpr int WS_AHEAD = 2;                      // weight fragments read ahead of their products (3: 1.3 % slower, spills)
constexpr int WS_FRAG = 3072;                    // bytes of one x6q fragment (3 planes x 1 KiB)
constexpr int WS_SLOT = WS_NW * WS_FRAG;         // one pipeline step: 8 fragments
// LDS: ring of ws_ns() steps | x tile [WS_NW waves][G1 groups][2 halves][64 lanes] float4 (re-read by every chunk's
// first layer; after the last one the epilogue's vectors land in its place)
template <int G1> constexpr int ws_xbytes() { return WS_NW * G1 * 2048; }
template <int G1> constexpr int ws_ns() {   // ring steps beside the x tile, at most 6: 6 / 5 / 4 / 4 / 3 for G1 = 1..5
    return (160 * 1024 - ws_xbytes<G1>()) / WS_SLOT < 6 ? (160 * 1024 - ws_xbytes<G1>()) / WS_SLOT : 6;
}
template <int G1> constexpr size_t ws_lds() { return (size_t)ws_ns<G1>() * WS_SLOT + ws_xbytes<G1>(); }

// One 1 KiB LDS-DMA (global_load_lds_dwordx4: lane l's 16 bytes at gsrc + voff land at lds + 16 l) in inline asm, so
// hipcc neither counts it nor inserts its conservative vmcnt(0) before every later ds_read of the ring (it cannot see
// which LDS bytes the DMA writes); the kernel waits with counted vmcnt itself. M0 is saved and restored. The SGPR
// operands are SALU results (the wave index is read into an SGPR once at kernel start), so no VALU-write -> VMEM-read
// wait is needed (a v_readfirstlane-produced base would need s_nop 4 first).
DEVI void ws_glds(const void* gsrc, unsigned voff, unsigned lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(lds), "s"(gsrc)
                 : "memory");
}
// ws_glds with its scalar operands made scalar explicitly: under SGPR pressure the compiler may keep a uniform value in
// a VGPR, which the inline asm's "s" constraint does not convert; v_readfirstlane does, and the s_nop 4 covers the
// VALU-writes-SGPR -> VMEM-reads-it hazard the compiler cannot see through the asm
DEVI void w2_glds(const void* gsrc, unsigned voff, unsigned lds) {
    const unsigned long long g = (unsigned long long)gsrc;
    const unsigned glo = __builtin_amdgcn_readfirstlane((unsigned)g), ghi = __builtin_amdgcn_readfirstlane((unsigned)(g >> 32));
    const unsigned long long gs = ((unsigned long long)ghi << 32) | glo;
    const unsigned ls = __builtin_amdgcn_readfirstlane(lds);
    unsigned keep;
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(ls), "s"(gs)
                 : "memory");
}

// six x6 products into one accumulator, small terms first: (w_mid, x_mid), (w_lo, x_hi*), (w_hi, x_lo), (w_mid, x_hi*),
// (w_hi, x_mid), (w_hi, x_hi); x_hi* = 0 where x is not finite (the general split)
DEVI void w2_x6(floatx4& acc, const uint4& u0, const uint4& u1, const uint4& u2, const X6U& b) {
    const bf16x8_t w0 = as_bf16x8(u0), w1 = as_bf16x8(u1), w2 = as_bf16x8(u2);
    const bf16x8_t bh = as_bf16x8(b.h), bm = as_bf16x8(b.m), bl = as_bf16x8(b.l);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, bh, acc, 0, 0, 0);
}

// The activation operand in the three-plane form: the finite-only split when the wave's values are all finite (a
// wave-uniform branch; 100.5 vs 103.3 us per humanoid B = 32 launch against split8's four planes), the general one
// (non-finite x -> h = m = 0, l = x, so only w_hi x carries it) otherwise; products bitwise split8's for finite operands
typedef X6U WSX;
DEVI WSX ws_opnd(const float4& a0, const float4& a1, bool fin) {
#ifdef WS_DIAG_NOSPLIT
    (void)fin;
    X6U b;
    b.h = b.m = b.l = *(const uint4*)&a0;
    return b;
#else
    X6U b;
    if (fin) b = w2_split8_fin(a0, a1);
    else b = w2_split8(a0, a1);
    return b;
#endif
}
DEVI void ws_prod(floatx4& acc, const uint4& u0, const uint4& u1, const uint4& u2, const WSX& b) { w2_x6(acc, u0, u1, u2, b); }

// per-feature vectors read through the constant address space: wave-uniform loads there become scalar loads
// (s_load, counted by lgkmcnt, scheduled by the compiler), which leave the ring's counted vmcnt waits alone
typedef const __attribute__((address_space(4))) float w2cf;

// ------------------------------------------------------------------------------------------------ 1. the ring
// NS slots of SLOT bytes (a step's 8 fragments first; the step kernel's WS_XS slots carry an x area behind them); VM =
// the DMA instructions a wave leaves in flight at a step's wait; DMA = the kernel's LDS-DMA flavour (ws_glds where
// every step position is compile-time, w2_glds under runtime loops over steps).
template <int NS, int SLOT, int VM, void (*DMA)(const void*, unsigned, unsigned)>
struct WRing {
    char* ring;            // LDS base
    unsigned lds, voff;    // its LDS address; the DMA's lane offset (lane * 16)
    int lane, wave, k;     // k: pipeline steps consumed
    uint4 fc[WS_AHEAD][3]; // the read-ahead: fc[0] is the fragment about to be consumed, fc[1] the one after
#ifdef WS_STAMPS
    // diagnostic: the shader clock before each step's wait and after its barrier (global stores: they only make the
    // counted vmcnt waits stricter)
    unsigned long long* st = nullptr;
#endif
    DEVI WRing(char* base, int lane_, int wave_)
        : ring(base), lds((unsigned)(size_t)(__attribute__((address_space(3))) char*)base), voff(lane_ * 16),
          lane(lane_), wave(wave_), k(0) {}

    // this wave's fragment of step kk: three 1 KiB planes
    DEVI void issue(int kk, const unsigned short* src) const {
        const unsigned dst = lds + (unsigned)((kk % NS) * SLOT + wave * WS_FRAG);
#pragma unroll
        for (int p = 0; p < 3; ++p) DMA(src + p * 512, voff, dst + p * 1024);
    }
    // step k: this wave's DMA of steps k and k + 1 has landed (vmcnt), every wave's has and every wave is done reading
    // step k - 1's slot (barrier); then refill that slot with step k + NS - 1 from nsrc, and after(k + NS - 1) for the
    // caller's own DMAs of the step (extra vector-memory ops only make the following counted waits stricter). (No
    // lgkmcnt(0): the only LDS reads in flight here are this wave's read-ahead of step k's first fragments, which the
    // refill of step k - 1's slot does not touch; their consumers wait with the compiler's own counts.)
    template <class After>
    DEVI const char* sync(const unsigned short* nsrc, After after) {
#ifdef WS_STAMPS
        if (st && k < 256) st[2 * k] = __builtin_amdgcn_s_memtime();
#endif
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(VM) : "memory");
#ifdef WS_STAMPS
        if (st && k < 256) st[2 * k + 1] = __builtin_amdgcn_s_memtime();
#endif
        const char* sl = ring + (k % NS) * SLOT + lane * 16;
        issue(k + NS - 1, nsrc);
        after(k + NS - 1);
        ++k;
        return sl;
    }
    DEVI const char* sync(const unsigned short* nsrc) { return sync(nsrc, [](int) {}); }

    static DEVI void rd(uint4 (&f)[3], const char* p) {
        f[0] = *(const uint4*)p;
        f[1] = *(const uint4*)(p + 1024);
        f[2] = *(const uint4*)(p + 2048);
    }
    // after the prologue's barrier: the first fragments of step 0 (it has >= 4)
    DEVI void prime() {
#pragma unroll
        for (int d = 0; d < WS_AHEAD; ++d) rd(fc[d], ring + d * WS_FRAG + lane * 16);
    }
    // The fragment stream is read two fragments ahead of the products (software-pipelined: the LDS latency of a
    // fragment runs under the previous two fragments' twelve MFMAs, so a wave keeps its SIMD busy even while its
    // partner waits at the barrier): frag(sl, i) hands out fc[0] and reads fragment i + 2 of the step at sl, or
    // fragment i + 2 - WS_NW (0 or 1) of the next step (landed: see VM).
    DEVI void frag(const char* sl, int i, uint4& w0, uint4& w1, uint4& w2) {
        w0 = fc[0][0];
        w1 = fc[0][1];
        w2 = fc[0][2];
#pragma unroll
        for (int d = 0; d + 1 < WS_AHEAD; ++d)
#pragma unroll
            for (int p = 0; p < 3; ++p) fc[d][p] = fc[d + 1][p];
        rd(fc[WS_AHEAD - 1], i + WS_AHEAD <= WS_NW - 1 ? sl + (i + WS_AHEAD) * WS_FRAG
                                                       : ring + (k % NS) * SLOT + (i + WS_AHEAD - WS_NW) * WS_FRAG + lane * 16);
        // (keeps the reads above this fragment's products: hipcc's scheduler otherwise sinks them to just before
        // their first use to save registers)
        __builtin_amdgcn_sched_barrier(0);
    }
};

// --------------------------------------------------------------------------------- 2. the static fragment stream
// this wave's fragment of step j of super-chunk sc: first-layer group j of W1 block 8sc + wave (g1s groups per block in
// memory), then W2's 32 blocks over k groups 4sc..4sc+3
template <int G1>
DEVI const unsigned short* wr_src(const unsigned short* const& X1, const int& g1s, const unsigned short* const& X2, int wave,
                                  int sc, int j) {
    if (j < G1) return X1 + ((size_t)(8 * sc + wave) * g1s + j) * 1536;
    const int s2 = j - G1, co = s2 >> 3, st = s2 & 7;
    return X2 + ((size_t)(8 * (st & 3) + wave) * 16 + 2 * (2 * sc + co) + (st >> 2)) * 1536;
}
// refill target of step j of super-chunk sc: step j + NS - 1 of it (src), or of the next one, or step l of the tail
// after the last (tail(l): the last layer, then dummy refills of any valid address past the end, never consumed)
template <int G1, int NS, class Src, class Tail>
DEVI const unsigned short* wr_next(Src src, Tail tail, int sc, int j) {
    const int jt = j + NS - 1;
    if (jt < G1 + 16) return src(sc, jt);
    return sc < 3 ? src(sc + 1, jt - (G1 + 16)) : tail(jt - (G1 + 16));
}
// the last layer group-major, step l: fragment f3 = 8l + wave = group x NB + tile
template <int NB>
DEVI const unsigned short* wr_l3_src(const unsigned short* const& X3, int l, int wave) {
    const int f3 = 8 * l + wave;
    return X3 + ((size_t)(f3 % NB) * 16 + f3 / NB) * 1536;
}

// ------------------------------------------------------------------------------------------------ 3. the x tile
// the wave's 16 rows (X panel rows xr0 + n) into LDS at sx (this lane's slot: group g at [2g], [2g + 1]): k group g =
// quads q0 + 8g + q and q0 + 8g + 4 + q of row n (the x6q k order), quads past the kq valid ones zero; returns whether
// every value of the wave is finite (the x tile's operand splits then take the finite-only form)
template <int G1>
DEVI bool wr_xtile(p1f4* sx, const float* const& X, const long& x_ts, int xr0, int n, int q, const int& q0, const int& kq,
                   bool live) {
    const float* xp = X + (size_t)(xr0 >> 5) * x_ts + (size_t)q0 * 128 + ((xr0 & 31) + n) * 4;
    const p1f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    float xsum = 0.f;
#pragma unroll
    for (int g = 0; g < G1; ++g) {
        const int qa = 8 * g + q, qb = qa + 4;
        const p1f4 va = live && qa < kq ? *(const p1f4*)(xp + (size_t)qa * 128) : zero4;
        const p1f4 vb = live && qb < kq ? *(const p1f4*)(xp + (size_t)qb * 128) : zero4;
        sx[(2 * g) * 64] = va;
        sx[(2 * g + 1) * 64] = vb;
        xsum += ((va[0] + va[1]) + (va[2] + va[3])) + ((vb[0] + vb[1]) + (vb[2] + vb[3]));
    }
    return ws_wave_finite(xsum);
}

// --------------------------------------------------------------------------------------------- 4. the epilogue
// Epilogue lane indices re-derived from an opaque copy of the DMA's lane offset (live through the loop): otherwise
// hipcc shares 4 jj + q with the prologue's x-tile quad indices 8 g + q (+ 4) and keeps them live -- spilled -- across
// the main loop
DEVI void wr_lane_ep(unsigned voff, int& n_ep, int& q_ep) {
    int l16 = (int)voff;
    asm volatile("" : "+v"(l16));
    n_ep = (l16 >> 4) & 15;
    q_ep = (l16 >> 8) & 3;
}
// tile t of h2 = ELU(acc + b2) (features 16t + 4q + i), formed where it is read: the accumulators stay in place
DEVI float4 wr_h2t(const floatx4 (&acc)[32], const float* sb2, int t, int q) {
    const float4 bv = *(const float4*)(sb2 + 16 * t + 4 * q);
    return make_float4(elu_f(acc[t][0] + bv.x), elu_f(acc[t][1] + bv.y), elu_f(acc[t][2] + bv.z), elu_f(acc[t][3] + bv.w));
}

// ------------------------------------------------------------------------------------------- the x6q layout (packs)
// x's three bf16 planes at (block, lane, element) of the planes at d; x6q_put: element (row r, column kk) of a
// [rows][32 G] matrix -> block (r / 16, kk / 32) of G per block row, lane (r % 16) + 16 ((kk % 16) / 4), element
// 4 ((kk % 32) / 16) + kk % 4
DEVI void x6_put(unsigned short* d, size_t blk, int lane, int j, __bf16 hi, __bf16 md, __bf16 lo) {
    d[(blk * 3 + 0) * 512 + lane * 8 + j] = __builtin_bit_cast(unsigned short, hi);
    d[(blk * 3 + 1) * 512 + lane * 8 + j] = __builtin_bit_cast(unsigned short, md);
    d[(blk * 3 + 2) * 512 + lane * 8 + j] = __builtin_bit_cast(unsigned short, lo);
}
DEVI void x6q_put(unsigned short* d, int G, int r, int kk, float x) {
    __bf16 hi, md, lo;
    split3(x, hi, md, lo);
    const int nb = r / 16, g = kk / 32, k2 = kk % 32;
    const int lane = (r % 16) + 16 * ((k2 % 16) / 4), j = 4 * (k2 / 16) + (k2 % 4);
    x6_put(d, (size_t)nb * G + g, lane, j, hi, md, lo);
}
