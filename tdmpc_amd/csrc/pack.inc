// The fused weight pack of tdmpc_kernels.hip (included there, inside its anonymous namespace): the job table, the pack
// and fold kernels, the per-buffer table cache and its nonce.
// ---- the fused weight pack (tdmpc_pack_weights): ONE launch writes every region of the packed buffer -- fp32
// copies, transposes, weight panels, their x6 and x6q bf16 planes -- straight from the reference's tensors (the
// learner passes views of its flat parameter buffer, so a post-update repack is one kernel, capturable into the
// update's HIP graph). Each job's padded region is written whole (zeros where the layout pads), so no memset.
// The x6 / x6q planes are split from the source tensors directly (the same values as from the fp32 panel).
struct PackSrc {                 // a weight panel's source: rows [0, r0) of p0, then [r0, r0 + r1) of p1
    const float* p0; const float* p1;
    int r0, r1, sld, ncols;      // source row length; plain map: panel column k < ncols <- source column k
    int first;                   // first-layer map: panel [a | 0 | z | 0] <- source [z | a] (L = ncols, A below)
    int L, A, Ap;
};
__host__ __device__ inline float pack_val(const PackSrc& m, int r, int k) {
    const float* row;
    if (r < m.r0) row = m.p0 + (size_t)r * m.sld;
    else if (r < m.r0 + m.r1) row = m.p1 + (size_t)(r - m.r0) * m.sld;
    else return 0.f;
    int col;
    if (m.first) col = k < m.A ? m.L + k : (k >= m.Ap && k < m.Ap + m.L ? k - m.Ap : -1);
    else col = k < m.ncols ? k : -1;
    return col < 0 ? 0.f : row[col];
}
enum { PJ_COPY, PJ_TRANS, PJ_PANEL, PJ_X6, PJ_X6Q };
struct PackJob {
    int kind;
    int blk0;                    // first workgroup of this job in the launch
    size_t dst;                  // float offset into the packed buffer
    long work;                   // work items
    const float* src; int n, rows, cols;   // COPY: n values then zeros to `work`; TRANS: [rows][cols] -> [cols][rows]
    PackSrc m; int prow, pk;     // PANEL: [prow][pk] panel; X6 / X6Q: prow rows x pk k of the source map
};
static_assert(sizeof(PackJob) <= PACK_JOB_BYTES, "job-table slot");
constexpr int PACK_WG = 256, PACK_PER = 8;   // threads per workgroup, items per thread
// elements per item: an x6 / x6q lane's 8 values (16-B stores per plane), a panel's k quad, else one; items per
// thread: one for those (the split and the gathered reads of 4 - 8 values already give each thread its work), else
// PACK_PER
__host__ __device__ constexpr int pack_per_item(int kind) { return kind == PJ_X6 || kind == PJ_X6Q ? 8 : kind == PJ_PANEL ? 4 : 1; }
__host__ __device__ constexpr int pack_items(int kind) { return pack_per_item(kind) > 1 ? 1 : PACK_PER; }

__global__ void __launch_bounds__(PACK_WG) pack_fused_kernel(PackHdr* hdr, const PackJob* jobs, int nj, float* pw,
                                                              unsigned long long nonce, long nweights) {
    if (hdr->nonce != nonce) {
        // not the table this launch was issued for (the buffer was re-allocated, re-zeroed or re-keyed since): pack
        // nothing from it, poison every weight region and raise the buffer's sticky status (plans pass it on)
        for (long i = (long)blockIdx.x * PACK_WG + threadIdx.x; i < nweights; i += (long)gridDim.x * PACK_WG)
            pw[i] = __builtin_nanf("");
        if (blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_fetch_or(&hdr->status, TDMPC_STATUS_PACK_STALE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    // the workgroup's job: last job whose blk0 <= blockIdx.x (binary search over the job table)
    int lo = 0, hi = nj - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PackJob& J = jobs[lo];
    const int epi = pack_per_item(J.kind), ipt = pack_items(J.kind);
    const long base = (long)(blockIdx.x - J.blk0) * PACK_WG * ipt;
    for (int u = 0; u < ipt; ++u) {
        const long i = (base + (long)u * PACK_WG + threadIdx.x) * epi;   // first element of the thread's item
        if (i >= J.work) break;
        switch (J.kind) {
            case PJ_COPY: pw[J.dst + i] = i < J.n ? J.src[i] : 0.f; break;
            case PJ_TRANS: {
                const long r = i % J.rows, c = i / J.rows;   // dst[c * rows + r] = src[r * cols + c]
                pw[J.dst + i] = J.src[r * J.cols + c];
                break;
            }
            case PJ_PANEL: {   // dst index i = pidx(r, k, pk): [r / 32][k / 4][r % 32][k % 4]; the item: one k quad
                const int rr = (i >> 2) & 31;
                const long q = i >> 7;
                const int kq = (int)(q % (J.pk / 4));
                const int r = (int)(q / (J.pk / 4)) * 32 + rr, k = kq * 4;
                *(float4*)(pw + J.dst + i) = make_float4(pack_val(J.m, r, k), pack_val(J.m, r, k + 1),
                                                         pack_val(J.m, r, k + 2), pack_val(J.m, r, k + 3));
                break;
            }
            case PJ_X6: case PJ_X6Q: {   // the item: one lane's 8 values of a block, 16 B per plane
                const int lane = (i >> 3) & 63;
                const long blk = i >> 9;
                int r, k0, k1;   // values j = 0..3 at k0 + j, j = 4..7 at k1 + j - 4
                if (J.kind == PJ_X6) {   // the x6 layout (Layout::x6): 32-row x 16-k blocks
                    const int G = (J.pk + 15) / 16;
                    const int g = (int)(blk % G), nb = (int)(blk / G);
                    r = 32 * nb + (lane & 31);
                    k0 = 16 * g + 4 * (lane >> 5);
                    k1 = k0 + 8;
                } else {                 // the x6q layout (Layout::x6q): 16-row x 32-k blocks
                    const int G = (J.pk + 31) / 32;
                    const int g = (int)(blk % G), nb = (int)(blk / G);
                    r = 16 * nb + (lane & 15);
                    k0 = 32 * g + 4 * (lane >> 4);
                    k1 = k0 + 16;
                }
                unsigned short hv[8], mv[8], lv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = (j < 4 ? k0 : k1) + (j & 3);
                    const float x = k < J.pk && r < J.prow ? pack_val(J.m, r, k) : 0.f;
                    __bf16 h, m, l;
                    split3(x, h, m, l);
                    hv[j] = __builtin_bit_cast(unsigned short, h);
                    mv[j] = __builtin_bit_cast(unsigned short, m);
                    lv[j] = __builtin_bit_cast(unsigned short, l);
                }
                auto pk8 = [](const unsigned short (&v)[8]) {
                    return make_uint4(v[0] | (unsigned)v[1] << 16, v[2] | (unsigned)v[3] << 16, v[4] | (unsigned)v[5] << 16,
                                      v[6] | (unsigned)v[7] << 16);
                };
                uint4* d = (uint4*)(pw + J.dst);   // 1 KiB per plane and block, 16 B per lane
                d[(blk * 3 + 0) * 64 + lane] = pk8(hv);
                d[(blk * 3 + 1) * 64 + lane] = pk8(mv);
                d[(blk * 3 + 2) * 64 + lane] = pk8(lv);
                break;
            }
        }
    }
}

// ---- the folded first layer (latent_dim == mlp_dim; Layout::fold): W1z W3 and b1 + W1z b3 for both TOLD.next heads,
// from the packed fp32 panels (w1x's z columns [2M][Ap .. Ap + L), w3d [Lr][M], b3d, b1x), fp64 sums rounded once to
// fp32, then split into the x6q planes with the a columns of w1x in front. A step whose input latent columns hold the
// previous step's h2 = ELU(W2 h1 + b2) computes W1 [a; W3 h2 + b3] + b1 as [W1a | W1z W3] [a; h2] + (b1 + W1z b3).
struct FoldArgs {
    const float* W; int Kp, zoff;          // source first layer: fp32 panel [R][Kp], z in columns [zoff, zoff + L)
    const float* w3d; const float* b3; const float* b;   // W3 panel [Lr][M], b3 [L], the source bias [R]
    float* fw; float* bf;                  // W_z W3 [R][M] fp32 and b + W_z b3 [R]
    unsigned short* x6; int kind, pk;      // planes of [W_a | W_z W3] (k < zoff from W, then fw): kind 0 x6q, 1 x6
    int M, L;
};
__global__ void __launch_bounds__(256) fold_gemm_kernel(const FoldArgs a) {
    // 16 x 16 output tile per workgroup: rows i [0, R), columns j of W3 [0, M) -- tile column M / 16 is the bias
    // column (j = M: b3)
    __shared__ double sA[16][17], sB[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const int i = i0 + ty, j = j0 + tx;
    double acc = 0.0;
    for (int l0 = 0; l0 < a.L; l0 += 16) {
        const int la = l0 + tx, lb = l0 + ty;
        sA[ty][tx] = la < a.L ? (double)a.W[pidx(i0 + ty, a.zoff + la, a.Kp)] : 0.0;
        double b = 0.0;
        if (lb < a.L) b = j < a.M ? (double)a.w3d[pidx(lb, j, a.M)] : (j == a.M ? (double)a.b3[lb] : 0.0);
        sB[ty][tx] = b;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = fma(sA[ty][k], sB[k][tx], acc);
        __syncthreads();
    }
    if (j < a.M) a.fw[(size_t)i * a.M + j] = (float)acc;
    else if (j == a.M) a.bf[i] = (float)((double)a.b[i] + acc);
}
__global__ void __launch_bounds__(256) fold_split_kernel(const FoldArgs a, long work) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= work) return;
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const long blk = i >> 9;
    int r, k;
    if (a.kind == 0) {   // x6q: 16-row x 32-k blocks (the wide kernels)
        const int G = (a.pk + 31) / 32;
        const int g = (int)(blk % G), nb = (int)(blk / G);
        r = 16 * nb + (lane & 15);
        k = 32 * g + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
    } else {             // x6: 32-row x 16-k blocks (the chain kernels)
        const int G = (a.pk + 15) / 16;
        const int g = (int)(blk % G), nb = (int)(blk / G);
        r = 32 * nb + (lane & 31);
        k = 16 * g + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
    }
    float x = 0.f;
    if (k < a.zoff) x = a.W[pidx(r, k, a.Kp)];
    else if (k < a.zoff + a.M && k < a.pk) x = a.fw[(size_t)r * a.M + (k - a.zoff)];
    __bf16 h, m, l;
    split3(x, h, m, l);
    x6_put(a.x6, (size_t)blk, lane, j, h, m, l);
}
int fold_one(const Layout& w, float* pw, hipStream_t s, size_t W, int R, int Kp, int zoff, size_t b, size_t fw,
             size_t bf, size_t x6, int kind, int pk, bool gemm = true) {
    FoldArgs f;
    memset(&f, 0, sizeof f);
    f.W = pw + W; f.Kp = Kp; f.zoff = zoff; f.w3d = pw + w.w3d; f.b3 = pw + w.b3d; f.b = pw + b;
    f.fw = pw + fw; f.bf = pw + bf; f.x6 = (unsigned short*)(pw + x6); f.kind = kind; f.pk = pk;
    f.M = w.M; f.L = w.L;
    if (gemm) {
        hipLaunchKernelGGL(fold_gemm_kernel, dim3(w.M / 16 + 1, R / 16), dim3(256), 0, s, f);
        HIPCHK(hipGetLastError());
    }
    const long work = kind == 0 ? (long)(R / 16) * ((pk + 31) / 32) * 512 : (long)((R + 31) / 32) * ((pk + 15) / 16) * 512;
    hipLaunchKernelGGL(fold_split_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, f, work);
    HIPCHK(hipGetLastError());
    return 0;
}
int pack_fold(const Layout& w, float* pw, hipStream_t s) {
    int rc, r, k;
    // TOLD.next (both heads, the wide kernel's x6q): [W1a | W1z W3], b1 + W1z b3
    if ((rc = fold_one(w, pw, s, w.w1x, 2 * w.M, w.Kx, w.Ap, w.b1x, w.fold_w, w.bfw, w.x6qw, 0, w.Kx))) return rc;
    // (the same product split again into the chain kernels' x6 layout)
    x6_shape(w, X6_W1X, &r, &k);
    if ((rc = fold_one(w, pw, s, w.w1x, 2 * w.M, w.Kx, w.Ap, w.b1x, w.fold_w, w.bfw, w.fw1_x6, 1, k, false))) return rc;
    // pi (chain x6): [Wp1 W3], bp1 + Wp1 b3
    x6_shape(w, X6_WP1, &r, &k);
    if ((rc = fold_one(w, pw, s, w.wp1, w.M, w.Lp, 0, w.bp1, w.fold_p, w.fpi_b, w.fpi_x6, 1, k))) return rc;
    // Q1 | Q2 (chain x6): [Wq1a | Wq1z W3], bq1 + Wq1z b3
    x6_shape(w, X6_WQ1X, &r, &k);
    return fold_one(w, pw, s, w.wq1x, 2 * w.M, w.Kx, w.Ap, w.bq1x, w.fold_q, w.fq_b, w.fq_x6, 1, k);
}

// The job list of a layout and the reference tensors t (state_dict order, tdmpc_num_param_tensors of them).
// heads_only (the DSSM planner, drnn.inc): t holds the encoder, pi, Q1 and Q2 tensors only, and the TOLD dynamics /
// reward regions get no job.
void pack_jobs(const Layout& w, const float* const* t, std::vector<PackJob>& jobs, bool heads_only = false) {
    const int M = w.M, L = w.L, A = w.A;
    auto job = [&](int kind, size_t dst, long work) -> PackJob& {
        PackJob j;
        memset(&j, 0, sizeof j);
        j.kind = kind; j.dst = dst; j.work = work;
        jobs.push_back(j);
        return jobs.back();
    };
    auto cp = [&](size_t dst, const float* src, int n) {   // zero tail to the 64-float slot take() reserved
        PackJob& j = job(PJ_COPY, dst, (long)rup(n, 64));
        j.src = src; j.n = n;
    };
    auto tr = [&](size_t dst, const float* src, int rows, int cols) {
        PackJob& j = job(PJ_TRANS, dst, (long)rows * cols);
        j.src = src; j.rows = rows; j.cols = cols;
    };
    auto msrc = [&](const float* p0, const float* p1, int r0, int r1, int sld, int ncols, int first) {
        PackSrc m;
        memset(&m, 0, sizeof m);
        m.p0 = p0; m.p1 = p1 ? p1 : p0; m.r0 = r0; m.r1 = r1; m.sld = sld; m.ncols = ncols; m.first = first;
        m.L = L; m.A = A; m.Ap = w.Ap;
        return m;
    };
    auto panel = [&](size_t dst, const PackSrc& m, int prow, int pk) {
        PackJob& j = job(PJ_PANEL, dst, (long)rup(prow, 32) * pk);
        j.m = m; j.prow = prow; j.pk = pk;
    };
    int i = 0;
    if (w.modality == 0) {
        tr(w.enc_w1t, t[i++], w.E, w.obs_dim);
        cp(w.enc_b1, t[i++], w.E);
        if (w.enc_norm) { cp(w.enc_lng, t[i++], w.E); cp(w.enc_lnb, t[i++], w.E); }
        tr(w.enc_w2t, t[i++], L, w.E);
        cp(w.enc_b2, t[i++], L);
    } else {
        static const int ks[4] = {7, 5, 3, 3};
        int cin = w.img_c;
        for (int c = 0; c < 4; ++c) {
            const float* cw = t[i++];
            cp(w.cw[c], cw, w.nch * cin * ks[c] * ks[c]);
            tr(w.cwt[c], cw, w.nch, cin * ks[c] * ks[c]);
            cp(w.cb[c], t[i++], w.nch);
            cin = w.nch;
        }
        tr(w.pl_wt, t[i++], L, w.flat);
        cp(w.pl_b, t[i++], L);
    }
    const int KI = L + A;
    const float* const* dyn = t + i;        // 0.w 0.b 2.w 2.b 4.w 4.b
    const float* const* rew = dyn + 6;
    const float* const* pi = heads_only ? dyn : rew + 6;
    const float* const* q1 = pi + 6;        // 0.w 0.b 1.w 1.b 3.w 3.b 4.w 4.b 6.w 6.b
    const float* const* q2 = q1 + 10;
    const PackSrc sW1X = msrc(dyn[0], rew[0], M, M, KI, L, 1), sW2D = msrc(dyn[2], nullptr, M, 0, M, M, 0),
                  sW2R = msrc(rew[2], nullptr, M, 0, M, M, 0), sW3D = msrc(dyn[4], nullptr, L, 0, M, M, 0),
                  sWP1 = msrc(pi[0], nullptr, M, 0, L, L, 0), sWP2 = msrc(pi[2], nullptr, M, 0, M, M, 0),
                  sWP3 = msrc(pi[4], nullptr, A, 0, M, M, 0), sWQ1X = msrc(q1[0], q2[0], M, M, KI, L, 1),
                  sWQ2 = msrc(q1[4], q2[4], M, M, M, M, 0);
    if (!heads_only) {
        panel(w.w1x, sW1X, 2 * M, w.Kx);
        cp(w.b1x, dyn[1], M); cp(w.b1x + M, rew[1], M);
        panel(w.w2d, sW2D, M, M); cp(w.b2d, dyn[3], M);
        panel(w.w3d, sW3D, w.Lr, M); cp(w.b3d, dyn[5], L);
        panel(w.w2r, sW2R, M, M); cp(w.b2r, rew[3], M);
        cp(w.w3r, rew[4], M); cp(w.b3r, rew[5], 1);
    }
    panel(w.wp1, sWP1, M, w.Lp); cp(w.bp1, pi[1], M);
    panel(w.wp2, sWP2, M, M); cp(w.bp2, pi[3], M);
    panel(w.wp3, sWP3, w.Ar, M); cp(w.bp3, pi[5], A);
    panel(w.wq1x, sWQ1X, 2 * M, w.Kx);
    panel(w.wq2, sWQ2, 2 * M, M);
    const float* const* qs[2] = {q1, q2};
    for (int q = 0; q < 2; ++q) {
        const float* const* Q = qs[q];
        // (the 2M-float LN / bias slots hold both heads: each copy's zero tail stops at the next head's start)
        PackJob* jb;
        cp(w.bq1x + q * M, Q[1], M); cp(w.g1 + q * M, Q[2], M); cp(w.be1 + q * M, Q[3], M);
        cp(w.bq2 + q * M, Q[5], M); cp(w.g2 + q * M, Q[6], M); cp(w.be2 + q * M, Q[7], M);
        cp(w.wq3 + q * M, Q[8], M);
        jb = &job(PJ_COPY, w.bq3 + q, 1);
        jb->src = Q[9]; jb->n = 1;
    }
    const PackSrc* xs[X6_N] = {&sW1X, &sW2D, &sW2R, &sW3D, &sWP1, &sWP2, &sWP3, &sWQ1X, &sWQ2};
    for (int x = heads_only ? X6_WP1 : 0; x < X6_N; ++x) {
        int rows, k;
        x6_shape(w, x, &rows, &k);
        PackJob& j = job(PJ_X6, w.x6[x], (long)((rows + 31) / 32) * ((k + 15) / 16) * 512);
        j.m = *xs[x]; j.prow = rows; j.pk = k;
    }
    for (int x = heads_only ? X6_WP1 : 0; x < X6_N; ++x) {
        int rows, k;
        x6_shape(w, x, &rows, &k);
        PackJob& j = job(PJ_X6Q, w.x6q[x], (long)((rows + 15) / 16) * ((k + 31) / 32) * 512);
        j.m = *xs[x]; j.prow = rows; j.pk = k;
    }
}

// The job table lives in the caller's packed buffer (Layout::jobtab), so it lives and dies with that buffer and the
// HIP graphs the caller captured over it -- nothing device-side is global or leaks. Every pack outside a stream
// capture uploads header + table (an async copy from a pinned staging buffer kept per packed buffer, whose previous
// copy's event is waited for before it is rewritten -- long done by then); a pack inside a capture uploads nothing and
// requires the table last uploaded into that buffer to be this one (pack once before capturing, as the learner does).
// Staleness is checked on the device, not trusted from the host record: every launch carries the nonce of the table
// the record says is in the buffer and pack_fused_kernel compares it with the header's (a buffer re-allocated at a
// recorded address or zeroed again fails loudly: NaN weights + TDMPC_STATUS_PACK_STALE). An uncaptured pack keeps the
// record's nonce when its table is unchanged (graphs captured over the buffer stay valid) and draws a new one
// otherwise; once a capture has packed from a buffer, an uncaptured pack with OTHER tensors is refused (it would
// silently re-point the captured graph) until tdmpc_pack_forget drops the record -- after which such a graph's pack
// sees a nonce mismatch and fails loudly. Records live until tdmpc_pack_forget; only their pinned staging buffers are
// recycled (PACK_PINNED of them, least recently used first). One mutex guards it.
struct PackTable {
    std::vector<PackJob> host; const float* pw; int device;
    unsigned long long nonce; bool captured;
    char* pinned; hipEvent_t done; bool recorded;
};
std::vector<PackTable> g_pack_tables;   // most recently used last
std::mutex g_pack_mu;
constexpr size_t PACK_PINNED = 64;
constexpr size_t PACK_UPLOAD_BYTES = (size_t)PACK_HDR_BYTES + (size_t)PACK_MAX_JOBS * sizeof(PackJob);

void pack_table_unpin(PackTable& t) {
    if (t.recorded) (void)hipEventSynchronize(t.done);
    if (t.done) (void)hipEventDestroy(t.done);
    if (t.pinned) (void)hipHostFree(t.pinned);
    t.pinned = nullptr;
    t.done = nullptr;
    t.recorded = false;
}

// table nonces: never 0 (a zeroed buffer's header) and distinct across processes and buffers with high probability
unsigned long long pack_next_nonce() {
    static std::atomic<unsigned long long> ctr{0};
    static const unsigned long long base =
        ((unsigned long long)std::chrono::high_resolution_clock::now().time_since_epoch().count() * 0x9E3779B97F4A7C15ull) ^
        ((unsigned long long)getpid() << 32);
    for (;;) {
        unsigned long long z = base + 0x9E3779B97F4A7C15ull * (ctr.fetch_add(1) + 1);   // splitmix64 finaliser
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        if (z) return z;
    }
}

int launch_pack(std::vector<PackJob>& jobs, const Layout& w, float* pw, hipStream_t s) {
    if (jobs.size() > (size_t)PACK_MAX_JOBS) {
        snprintf(g_err, sizeof g_err, "tdmpc_pack_weights: %zu jobs > %d", jobs.size(), PACK_MAX_JOBS);
        return TDMPC_E_SIZE;
    }
    int blk = 0;
    for (PackJob& j : jobs) {
        j.blk0 = blk;
        const long per_blk = (long)PACK_WG * pack_items(j.kind) * pack_per_item(j.kind);
        blk += (int)((j.work + per_blk - 1) / per_blk);
    }
    const size_t nb = jobs.size() * sizeof(PackJob);
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    PackHdr* hdr = (PackHdr*)(pw + w.jobtab);
    PackJob* dev = (PackJob*)((char*)hdr + PACK_HDR_BYTES);
    unsigned long long nonce = 0;
    {
        std::lock_guard<std::mutex> lock(g_pack_mu);
        size_t hit = g_pack_tables.size();
        for (size_t i = 0; i < g_pack_tables.size(); ++i)
            if (g_pack_tables[i].pw == pw && g_pack_tables[i].device == device) { hit = i; break; }
        const bool same = hit < g_pack_tables.size() && g_pack_tables[hit].host.size() == jobs.size() &&
                          !memcmp(g_pack_tables[hit].host.data(), jobs.data(), nb);
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIPCHK(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) {
            if (!same) {
                snprintf(g_err, sizeof g_err, hit == g_pack_tables.size()
                         ? "tdmpc_pack_weights: no table uploaded into this buffer while capturing (pack once before capture)"
                         : "tdmpc_pack_weights: new tensors while capturing (pack once before capture)");
                return TDMPC_E_DIMS;
            }
            g_pack_tables[hit].captured = true;
        } else {
            if (hit < g_pack_tables.size() && g_pack_tables[hit].captured && !same) {
                snprintf(g_err, sizeof g_err, "tdmpc_pack_weights: a captured graph packs into this buffer from other "
                         "tensors; call tdmpc_pack_forget(packed) first (that graph's pack then fails loudly)");
                return TDMPC_E_DIMS;
            }
            if (hit == g_pack_tables.size()) {
                g_pack_tables.push_back(PackTable{{}, pw, device, 0, false, nullptr, nullptr, false});
                hit = g_pack_tables.size() - 1;
            }
            PackTable& t = g_pack_tables[hit];
            if (!same || !t.nonce) t.nonce = pack_next_nonce();
            if (!t.pinned) {
                size_t npin = 0;
                for (const PackTable& o : g_pack_tables) npin += o.pinned != nullptr;
                for (size_t i = 0; npin >= PACK_PINNED && i < g_pack_tables.size(); ++i)
                    if (g_pack_tables[i].pinned) { pack_table_unpin(g_pack_tables[i]); --npin; }
                HIPCHK(hipHostMalloc((void**)&t.pinned, PACK_UPLOAD_BYTES, hipHostMallocDefault));
                HIPCHK(hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
            }
            if (t.recorded) HIPCHK(hipEventSynchronize(t.done));
            PackHdr h;
            memset(&h, 0, sizeof h);
            h.nonce = t.nonce; h.status = 0; h.njobs = (int)jobs.size();
            memset(t.pinned, 0, PACK_HDR_BYTES);
            memcpy(t.pinned, &h, sizeof h);
            memcpy(t.pinned + PACK_HDR_BYTES, jobs.data(), nb);
            HIPCHK(hipMemcpyAsync(hdr, t.pinned, PACK_HDR_BYTES + nb, hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(t.done, s));
            t.recorded = true;
            t.host = jobs;
        }
        nonce = g_pack_tables[hit].nonce;
        PackTable t = std::move(g_pack_tables[hit]);   // most recently used last
        g_pack_tables.erase(g_pack_tables.begin() + hit);
        g_pack_tables.push_back(std::move(t));
    }
    hipLaunchKernelGGL(pack_fused_kernel, dim3((unsigned)blk), dim3(PACK_WG), 0, s, hdr, (const PackJob*)dev,
                       (int)jobs.size(), pw, nonce, (long)w.jobtab);
    HIPCHK(hipGetLastError());
    return 0;
}

// Host-only bounds check of one pack job (no HIP call), shared by tdmpc_debug_pack_check and
// tdmpc_drnn_debug_pack_check: its writes inside the float offsets [lo, hi) of the packed buffer, its reads inside its
// source tensor, where tensor i of n has the fake base address (i + 1) << 40 and numel[i] floats.
bool pack_job_in_bounds(const PackJob& J, const int64_t* numel, int n, size_t lo, size_t hi) {
    auto in_tensor = [&](const float* p, long last) -> bool {   // reads p[0 .. last]
        const uintptr_t u = (uintptr_t)p;
        const long i = (long)(u >> 40) - 1;
        if (i < 0 || i >= n) return false;
        const long off = (long)((u & (((uintptr_t)1 << 40) - 1)) / 4);
        return off + last < numel[i];
    };
    auto src_ok = [&](const PackSrc& m, int maxk) -> bool {
        const int maxcol = m.first ? m.L + m.A - 1 : std::min(maxk, m.ncols - 1);
        if (m.r0 > 0 && !in_tensor(m.p0, (long)(m.r0 - 1) * m.sld + maxcol)) return false;
        if (m.r1 > 0 && !in_tensor(m.p1, (long)(m.r1 - 1) * m.sld + maxcol)) return false;
        return true;
    };
    const double end = J.kind == PJ_X6 || J.kind == PJ_X6Q ? (double)J.dst + 1.5 * J.work : (double)(J.dst + J.work);
    if (J.dst < lo || end > (double)hi) return false;
    if (J.kind == PJ_COPY) return J.n <= J.work && in_tensor(J.src, J.n - 1);
    if (J.kind == PJ_TRANS) return in_tensor(J.src, (long)J.rows * J.cols - 1);
    return src_ok(J.m, J.pk - 1);
}
