// sim_learner.inc -- the similarity TD-MPC agent's update (TDMPCSIM.update, tdmpc_similarity.py:298-375;
// include/tdmpc_sim_learner.h; DESIGN.md §7 f11). Included at the end of drnn_learner.hip, after icem_learner.inc, whose
// BatchNorm, cosine and one-step loss code it exposes to the learner engine (tdmpc_amd/sim_engine.py):
//   * tdmpc_sim_loss_*: the one-step loss family (sl_loss_*) over all H steps with rho ** t and the 1 / horizon gradient
//     hook, over TD targets that the engine's row kernel has written (TDIN);
//   * tdmpc_sim_bn_* / tdmpc_sim_cos_*: bn_forward / bn_backward and dt_cos_fwd / dt_cos_bwd as entry points of their
//     own, so that `_predictor`'s products run in the engine's grouped launches and its weight gradients reach
//     tdmpc_lg_finalize as split-K slices.

namespace {

bool sim_loss_args_in(const tdmpc_sim_loss_args* a) {
    return a && a->sim && a->q1 && a->q2 && a->rp && a->rw && a->td && a->w && a->H > 0 && a->B > 0;
}

StepLossArgs sim_td_step_args(const tdmpc_sim_loss_args* a) {
    return StepLossArgs{a->sim, a->q1, a->q2, a->rp, a->rw, nullptr, nullptr, a->w, a->H, a->H, a->B,
                        a->sim_coef, a->reward_coef, a->value_coef, 0.f, a->rho};
}

int check_bn_rows(int rows) {
    if (rows < 2 || rows > TDMPC_DT_MAX_ROWS)
        return bad("sim_learner: rows %ld is not in [2, %ld] (train-mode BatchNorm needs two rows)", rows,
                   TDMPC_DT_MAX_ROWS);
    return 0;
}

int check_cos_shape(int rows, int L) {
    if (rows < 1 || rows > TDMPC_DT_MAX_ROWS) return bad("sim_learner: rows %ld is not in [1, %ld]", rows, TDMPC_DT_MAX_ROWS);
    if (L < 1 || L > 256) return bad("sim_learner: latent_dim %ld is not in [1, 256]", L);
    return 0;
}

int need_all(const void* const* ptrs, const char* const* names, int n) {
    for (int i = 0; i < n; ++i)
        if (int rc = need(ptrs[i], names[i])) return rc;
    return 0;
}

}  // namespace

extern "C" {

int tdmpc_sim_learner_version(void) { return TDMPC_SIM_LEARNER_VERSION; }

int tdmpc_sim_loss_forward(const tdmpc_sim_loss_args* a, float* rows, float* scal, void* stream) {
    if (!sim_loss_args_in(a) || !rows || !scal) return bad("sim_learner: loss_forward: a null pointer or H, B < 1");
    return step_loss_forward<true, true>(sim_td_step_args(a), const_cast<float*>(a->td), rows, scal, stream);
}

int tdmpc_sim_loss_backward(const tdmpc_sim_loss_args* a, const float* rows, const float* scal, const float* gw,
                            float* dsim, float* dq1, float* dq2, float* drp, void* stream) {
    if (!sim_loss_args_in(a) || !rows || !scal || !gw)
        return bad("sim_learner: loss_backward: a null pointer or H, B < 1");
    return step_loss_backward<true, true>(sim_td_step_args(a), a->td, rows, scal, gw, dsim, dq1, dq2, drp, stream);
}

int tdmpc_sim_bn_part_floats(int32_t rows, size_t* out) {
    if (int rc = check_bn_rows(rows)) return rc;
    if (int rc = need(out, "out")) return rc;
    *out = (size_t)chunks(rows) * 2 * M;
    return 0;
}

int tdmpc_sim_bn_fwd(const float* x, const float* g, const float* b, float* rmean, float* rvar, float* xhat,
                     float* rstd, float* e, float* part, int32_t rows, void* stream) {
    if (int rc = check_bn_rows(rows)) return rc;
    const void* ptrs[] = {x, g, b, rmean, rvar, xhat, rstd, e, part};
    const char* names[] = {"x", "g", "b", "rmean", "rvar", "xhat", "rstd", "e", "part"};
    if (int rc = need_all(ptrs, names, 9)) return rc;
    BnArgs a;
    memset(&a, 0, sizeof a);
    a.x = x; a.g = g; a.b = b; a.rmean = rmean; a.rvar = rvar;
    a.xhat = xhat; a.rstd = rstd; a.e = e; a.part = part; a.rows = rows; a.C = M;
    return bn_forward(a, (hipStream_t)stream);
}

int tdmpc_sim_bn_bwd(const float* de, const float* g, const float* xhat, const float* rstd, const float* e,
                     float* part, float* dx, float* dg, float* db, int32_t rows, void* stream) {
    if (int rc = check_bn_rows(rows)) return rc;
    const void* ptrs[] = {de, g, xhat, rstd, e, part, dx, dg, db};
    const char* names[] = {"de", "g", "xhat", "rstd", "e", "part", "dx", "dg", "db"};
    if (int rc = need_all(ptrs, names, 9)) return rc;
    BnArgs a;
    memset(&a, 0, sizeof a);
    a.x = de; a.g = g; a.xhat = const_cast<float*>(xhat); a.rstd = const_cast<float*>(rstd);
    a.e = const_cast<float*>(e); a.part = part; a.dx = dx; a.dg = dg; a.db = db; a.rows = rows; a.C = M;
    return bn_backward(a, (hipStream_t)stream);
}

int tdmpc_sim_cos_fwd(const float* pred, const float* keys, float* loss, int32_t rows, int32_t L, void* stream) {
    if (int rc = check_cos_shape(rows, L)) return rc;
    const void* ptrs[] = {pred, keys, loss};
    const char* names[] = {"pred", "keys", "loss"};
    if (int rc = need_all(ptrs, names, 3)) return rc;
    hipLaunchKernelGGL(dt_cos_fwd, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, pred, keys, loss, rows, L);
    return launched("cos_fwd");
}

int tdmpc_sim_cos_bwd(const float* pred, const float* keys, const float* dloss, float* dpred, int32_t rows, int32_t L,
                      void* stream) {
    if (int rc = check_cos_shape(rows, L)) return rc;
    const void* ptrs[] = {pred, keys, dloss, dpred};
    const char* names[] = {"pred", "keys", "dloss", "dpred"};
    if (int rc = need_all(ptrs, names, 4)) return rc;
    hipLaunchKernelGGL(dt_cos_bwd, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, pred, keys, dloss, dpred,
                       rows, L);
    return launched("cos_bwd");
}

}  // extern "C"
