// icem_learner.inc -- the MLP iCEM agent's update (TdICemSimMlp.update, tdmpc_icem_similarity_mlp.py:313-428;
// include/tdmpc_icem_learner.h; DESIGN.md §7 f10). Included at the end of drnn_learner.hip, whose BatchNorm, cosine and
// similarity-loss code it shares:
//   * tdmpc_icem_intrinsic_fwd: intrinsic_rewards' H + 1 one-step rollouts through the MLP dynamics and their
//     similarity losses as one launch chain over S B rows -- three products for `_dynamics` (no BatchNorm: rows are
//     independent), then predictor_fwd normalising per segment of B rows;
//   * tdmpc_icem_simloss_*: simloss_fwd / simloss_bwd behind the planner's tdmpc_dims;
//   * tdmpc_icem_loss_*: the one-step loss family (sl_loss_*) over all H steps with rho ** t and the 1 / horizon
//     gradient hook, forward and backward.

namespace {

enum { D0W = 0, D0B, D2W, D2B, D4W, D4B };   // the dynamics table (tdmpc_icem_learner.h)

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

StepLossArgs icem_step_args(const tdmpc_icem_loss_args* a) {
    return StepLossArgs{a->sim, a->q1, a->q2, a->rp, a->rw, a->rwpi, a->nq, a->w, a->H, a->H, a->B,
                        a->sim_coef, a->reward_coef, a->value_coef, a->discount, a->rho};
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
    return predictor_fwd(P, W.zo, keys, loss, R, L, seg_rows, segments, seg_rows,
                         PredictorBufs{W.y1, W.bnx, W.bnr, W.y2, W.part, W.pred}, stream);
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
    return step_loss_forward<true>(icem_step_args(a), td, rows, scal, stream);
}

int tdmpc_icem_loss_backward(const tdmpc_icem_loss_args* a, const float* td, const float* rows, const float* scal,
                             const float* gw, float* dsim, float* dq1, float* dq2, float* drp, void* stream) {
    if (!icem_loss_args_ok(a) || !td || !rows || !scal || !gw)
        return bad("icem_learner: loss_backward: a null pointer or H, B < 1");
    return step_loss_backward<true, true>(icem_step_args(a), td, rows, scal, gw, dsim, dq1, dq2, drp, stream);
}

}  // extern "C"
