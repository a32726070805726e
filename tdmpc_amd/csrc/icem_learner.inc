// icem_learner.inc -- the MLP iCEM agent's update (TdICemSimMlp.update, tdmpc_icem_similarity_mlp.py:313-428;
// include/tdmpc_icem_learner.h; DESIGN.md §7 f10). Included at the end of drnn_learner.hip, whose BatchNorm, cosine and
// similarity-loss code it shares:
//   * tdmpc_icem_intrinsic_fwd: intrinsic_rewards' H + 1 one-step rollouts through the MLP dynamics and their
//     similarity losses as one launch chain over S B rows -- three products for `_dynamics` (no BatchNorm: rows are
//     independent), then `_predictor` with dt_bn_stat / dt_bn_fwd normalising per segment of B rows, then dt_cos_fwd;
//   * tdmpc_icem_simloss_*: simloss_fwd / simloss_bwd behind the planner's tdmpc_dims;
//   * it_loss_rows / it_loss_means / it_loss_bwd: the one-step TD targets and the loss composition with rho ** t and
//     the 1 / horizon gradient hook, forward and backward.

namespace {

enum { D0W = 0, D0B, D2W, D2B, D4W, D4B };   // the dynamics table (tdmpc_icem_learner.h)

// (float)(rho ** t): the power in double, rounded once (a float32 tensor times a Python float).
__device__ __forceinline__ float rho_pow(double rho, int t) { return t == 0 ? 1.f : (float)pow(rho, (double)t); }

__global__ void __launch_bounds__(256) it_loss_rows(const tdmpc_icem_loss_args a, float* td, float* rows) {
    const int b = blockIdx.x * 256 + threadIdx.x, H = a.H, B = a.B;
    if (b >= B) return;
    float sim = 0.f, rew = 0.f, val = 0.f, pri = 0.f;
    for (int t = 0; t < H; ++t) {
        const size_t i = (size_t)t * B + b;
        const float r = rho_pow(a.rho, t);
        const float tg = a.rwpi[i] + a.discount * a.nq[i];
        const float dr = a.rp[i] - a.rw[i], d1 = a.q1[i] - tg, d2 = a.q2[i] - tg;
        td[i] = tg;
        sim += a.sim[i];
        rew += (dr * dr) * r;
        val += (d1 * d1 + d2 * d2) * r;
        pri += (fabsf(d1) + fabsf(d2)) * r;
    }
    rows[b] = sim;
    rows[B + b] = rew;
    rows[2 * B + b] = val;
    rows[3 * B + b] = fminf(pri, LOSS_CLAMP);
    rows[4 * B + b] = a.sim_coef * fminf(sim, LOSS_CLAMP) + a.reward_coef * fminf(rew, LOSS_CLAMP) +
                      a.value_coef * fminf(val, LOSS_CLAMP);
}

__global__ void __launch_bounds__(512) it_loss_means(const tdmpc_icem_loss_args a, const float* rows, float* scal) {
    __shared__ float red[5][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = a.B;
    float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = tid; b < B; b += 512) {
        s[0] += rows[b];
        s[1] += rows[B + b];
        s[2] += rows[2 * B + b];
        s[3] += rows[4 * B + b];
        s[4] += a.w[b];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float v = wsum(s[k]);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    if (tid == 0) {
        float m[5];
        for (int k = 0; k < 5; ++k) {
            float v = 0.f;
            for (int w = 0; w < 8; ++w) v += red[k][w];
            m[k] = v / (float)B;
        }
        scal[0] = m[0]; scal[1] = m[1]; scal[2] = m[2]; scal[3] = m[3];
        scal[4] = m[3] * m[4];
        scal[5] = m[4];
    }
}

__global__ void __launch_bounds__(256) it_loss_bwd(const tdmpc_icem_loss_args a, const float* td, const float* rows,
                                                   const float* scal, const float* gw, float* dsim, float* dq1,
                                                   float* dq2, float* drp) {
    const int B = a.B;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.H * B) return;
    const int b = (int)(i % B), t = (int)(i / B);
    // the hook's 1 / horizon, then d weighted / d total_b = mean(w) / B
    const float dtot = gw[0] * (1.f / (float)a.H) * scal[5] / (float)B;
    const float r = rho_pow(a.rho, t);
    const float dr = rows[B + b] <= LOSS_CLAMP ? a.reward_coef * dtot * r : 0.f;
    const float dv = rows[2 * B + b] <= LOSS_CLAMP ? a.value_coef * dtot * r : 0.f;
    if (dsim) dsim[i] = rows[b] <= LOSS_CLAMP ? a.sim_coef * dtot : 0.f;
    if (drp) drp[i] = 2.f * (a.rp[i] - a.rw[i]) * dr;
    if (dq1) dq1[i] = 2.f * (a.q1[i] - td[i]) * dv;
    if (dq2) dq2[i] = 2.f * (a.q2[i] - td[i]) * dv;
}

int check_icem_shape(const tdmpc_dims* d, int rows, Shape& s) {
    if (!d) return bad("icem_learner: dims is null");
    if (d->modality != 0) return bad("icem_learner: state observations only (modality %ld)", d->modality);
    if (d->mlp_dim != M) return bad("icem_learner: mlp_dim %ld is not supported (512 only)", d->mlp_dim);
    if (d->latent_dim < 1 || d->latent_dim > 256)
        return bad("icem_learner: latent_dim %ld is not in [1, 256]", d->latent_dim);
    if (d->action_dim < 1) return bad("icem_learner: action_dim %ld", d->action_dim);
    if (rows < 2 || rows > TDMPC_DT_MAX_ROWS)
        return bad("icem_learner: rows %ld is not in [2, %ld] (train-mode BatchNorm needs two rows)", rows,
                   TDMPC_DT_MAX_ROWS);
    s = Shape{d->latent_dim, d->action_dim, 0, rows};
    return 0;
}

int check_icem_segments(const tdmpc_dims* d, int segments, int seg_rows, Shape& s) {
    if (segments < 1 || seg_rows < 2 || (long)segments * seg_rows > TDMPC_DT_MAX_ROWS)
        return bad("icem_learner: %ld segments of %ld rows (at least 1 of at least 2 rows, 4096 rows in all)", segments,
                   seg_rows);
    return check_icem_shape(d, segments * seg_rows, s);
}

// tdmpc_icem_intrinsic_fwd's workspace, all scratch. s.R = S * B rows. y1 holds _dynamics.1's output and then
// _predictor.0's (the BatchNorm's input); y2 _dynamics.3's output and then the BatchNorm's ELU output.
struct IcemIntrWs { float *y1, *y2, *zo, *bnx, *bnr, *part, *pred; size_t total; };
IcemIntrWs icem_intr_ws(const Shape& s, int segments, int seg_rows, float* base) {
    Bump b(base);
    IcemIntrWs v;
    const size_t R = s.R;
    v.y1 = b.take(R * M);
    v.y2 = b.take(R * M);
    v.zo = b.take(R * s.L);
    v.bnx = b.take(R * M);
    v.bnr = b.take((size_t)segments * M);
    v.part = b.take((size_t)segments * chunks(seg_rows) * 2 * M);
    v.pred = b.take(R * s.L);
    v.total = b.off;
    return v;
}

int need_dyn_table(float* const* t, int n) {
    if (int rc = need(t, "dyn_tensors")) return rc;
    if (n != TDMPC_ICEM_DYN_TENSORS) return bad("icem_learner: %ld dynamics tensors given, %ld expected", n,
                                                TDMPC_ICEM_DYN_TENSORS);
    for (int i = 0; i < n; ++i)
        if (!t[i]) return bad("icem_learner: tensor %ld of the dynamics table is null", i);
    return 0;
}

bool icem_loss_args_ok(const tdmpc_icem_loss_args* a) {
    return a && a->sim && a->q1 && a->q2 && a->rp && a->rw && a->rwpi && a->nq && a->w && a->H > 0 && a->B > 0;
}

}  // namespace

extern "C" {

int tdmpc_icem_learner_version(void) { return TDMPC_ICEM_LEARNER_VERSION; }

int tdmpc_icem_intrinsic_workspace_floats(const tdmpc_dims* dims, int32_t segments, int32_t seg_rows, size_t* out) {
    Shape s;
    if (int rc = check_icem_segments(dims, segments, seg_rows, s)) return rc;
    if (int rc = need(out, "out")) return rc;
    *out = icem_intr_ws(s, segments, seg_rows, nullptr).total;
    return 0;
}

int tdmpc_icem_intrinsic_fwd(const tdmpc_dims* dims, float* const* D, int32_t n_dyn, float* const* P, int32_t n_loss,
                             const float* z, const float* a, const float* keys, int32_t segments, int32_t seg_rows,
                             float* loss, float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_icem_segments(dims, segments, seg_rows, s)) return rc;
    if (int rc = need_dyn_table(D, n_dyn)) return rc;
    if (int rc = need_table(P, n_loss, TDMPC_DT_LOSS_TENSORS, "loss_tensors", true)) return rc;
    const void* ptrs[] = {z, a, keys, loss, workspace};
    const char* names[] = {"z", "a", "keys", "loss", "workspace"};
    for (int i = 0; i < 5; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    const IcemIntrWs W = icem_intr_ws(s, segments, seg_rows, workspace);
    if (workspace_floats < W.total) return size_err("workspace", workspace_floats, W.total);
    const hipStream_t st = (hipStream_t)stream;
    const int R = s.R, L = s.L, A = s.A;

    // _dynamics([z | a]): Linear + ELU over the two K segments, Linear + ELU, Linear
    tdmpc_lg_job j = job(R, M, W.y1, M, seg(z, L, D[D0W], L + A, L, 0, 0));
    j.seg[1] = seg(a, A, D[D0W] + L, L + A, A, 0, 0);
    j.nseg = 2;
    j.bias = D[D0B];
    j.epi = TDMPC_LG_EPI_ELU;
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    j = linear(R, M, M, W.y1, D[D2W], D[D2B], W.y2);
    j.epi = TDMPC_LG_EPI_ELU;
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    j = linear(R, L, M, W.y2, D[D4W], D[D4B], W.zo);
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;

    // similarity_loss(z', keys) with the BatchNorm per segment
    j = linear(R, M, L, W.zo, P[P0W], P[P0B], W.y1);
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    BnArgs b;
    memset(&b, 0, sizeof b);
    b.x = W.y1; b.g = P[P1G]; b.b = P[P1B]; b.rmean = P[P1RM]; b.rvar = P[P1RV];
    b.xhat = W.bnx; b.rstd = W.bnr; b.e = W.y2; b.part = W.part; b.rows = R; b.C = M;
    b.seg = seg_rows; b.nseg = segments;
    if (int rc = bn_forward(b, st)) return rc;
    j = linear(R, L, M, W.y2, P[P3W], P[P3B], W.pred);
    if (int rc = gemm(&j, 1, stream, seg_rows)) return rc;
    hipLaunchKernelGGL(dt_cos_fwd, dim3((R + 3) / 4), dim3(256), 0, st, W.pred, keys, loss, R, L);
    return launched("cos_fwd");
}

int tdmpc_icem_simloss_sizes_for(const tdmpc_dims* dims, int32_t rows, tdmpc_icem_simloss_sizes* out) {
    Shape s;
    if (int rc = check_icem_shape(dims, rows, s)) return rc;
    if (int rc = need(out, "out")) return rc;
    out->loss_saved_floats = loss_saved(s, nullptr).total;
    out->workspace_floats = std::max(loss_fwd_ws(s, nullptr).total, loss_bwd_ws(s, nullptr).total);
    return 0;
}

int tdmpc_icem_simloss_fwd(const tdmpc_dims* dims, float* const* T, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, float* loss, float* saved, size_t saved_floats,
                           float* workspace, size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_icem_shape(dims, rows, s)) return rc;
    return simloss_fwd(s, T, n_tensors, queries, keys, loss, saved, saved_floats, workspace, workspace_floats, stream);
}

int tdmpc_icem_simloss_bwd(const tdmpc_dims* dims, float* const* T, int32_t n_tensors, const float* queries,
                           const float* keys, int32_t rows, const float* saved, size_t saved_floats,
                           const float* dloss, float* dqueries, float* const* G, float* workspace,
                           size_t workspace_floats, void* stream) {
    Shape s;
    if (int rc = check_icem_shape(dims, rows, s)) return rc;
    return simloss_bwd(s, T, n_tensors, queries, keys, saved, saved_floats, dloss, dqueries, G, workspace,
                       workspace_floats, stream);
}

int tdmpc_icem_loss_forward(const tdmpc_icem_loss_args* a, float* td, float* rows, float* scal, void* stream) {
    if (!icem_loss_args_ok(a) || !td || !rows || !scal)
        return bad("icem_learner: loss_forward: a null pointer or H, B < 1");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(it_loss_rows, dim3((a->B + 255) / 256), dim3(256), 0, st, *a, td, rows);
    if (int rc = launched("icem loss_rows")) return rc;
    hipLaunchKernelGGL(it_loss_means, dim3(1), dim3(512), 0, st, *a, rows, scal);
    return launched("icem loss_means");
}

int tdmpc_icem_loss_backward(const tdmpc_icem_loss_args* a, const float* td, const float* rows, const float* scal,
                             const float* gw, float* dsim, float* dq1, float* dq2, float* drp, void* stream) {
    if (!icem_loss_args_ok(a) || !td || !rows || !scal || !gw)
        return bad("icem_learner: loss_backward: a null pointer or H, B < 1");
    const long n = (long)a->H * a->B;
    hipLaunchKernelGGL(it_loss_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a, td, rows,
                       scal, gw, dsim, dq1, dq2, drp);
    return launched("icem loss_bwd");
}

}  // extern "C"
