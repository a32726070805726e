// drnn_engine.inc -- the DSSM recurrent step as learner-engine passes (include/tdmpc_drnn_engine.h; DESIGN.md §7 f14).
// Included at the end of drnn_learner.hip, after sim_learner.inc: dt_gate_fwd / dt_gate_bwd, NormGRUCell's pointwise
// part, as entry points of their own over given gate products, so that an engine issues [z | a] weight_ih^T,
// h weight_hh^T and every dX / dW in its own grouped launches and the LayerNorm-affine partials of all H steps reach
// tdmpc_lg_finalize as slices of one source (no dt_finish, no dt_unpack). A null hidden state takes the <true>
// instances, which read neither gh nor h. prior_mlp.1 + ELU is tdmpc_sim_bn_fwd / _bwd (sim_learner.inc) as they stand.

namespace {

int check_gate_shape(int rows, int Hd) {
    if (Hd < 32 || Hd > 256 || Hd % 32)
        return bad("drnn_engine: hidden_dim %ld is not a multiple of 32 in [32, 256]", Hd);
    if (rows < 2 || rows > TDMPC_DT_MAX_ROWS)
        return bad("drnn_engine: rows %ld is not in [2, %ld]", rows, TDMPC_DT_MAX_ROWS);
    return 0;
}

// gh and h come together: both given, or both null (a zero hidden state).
int check_hidden(const float* gh, const float* h) {
    if ((gh == nullptr) != (h == nullptr))
        return bad(gh ? "drnn_engine: h is null but gh is not (a zero hidden state has neither)"
                      : "drnn_engine: gh is null but h is not (a zero hidden state has neither)");
    return 0;
}

int check_ln(const float* const* ln) {
    if (int rc = need(ln, "ln")) return rc;
    for (int i = 0; i < 6; ++i)
        if (!ln[i]) return bad("drnn_engine: ln[%ld] is null", i);
    return 0;
}

}  // namespace

extern "C" {

int tdmpc_drnn_engine_version(void) { return TDMPC_DRNN_ENGINE_VERSION; }

int tdmpc_drnn_gate_part_floats(int32_t rows, int32_t hidden_dim, size_t* out) {
    if (int rc = check_gate_shape(rows, hidden_dim)) return rc;
    if (int rc = need(out, "out")) return rc;
    static_assert(GROWS == TDMPC_DRNN_GATE_PART_ROWS, "the header promises dt_gate_bwd's rows per workgroup");
    *out = (size_t)gate_wgs(rows) * 6 * hidden_dim;
    return 0;
}

int tdmpc_drnn_gate_fwd(const float* gi, const float* gh, const float* h, const float* const* ln, float* gate,
                        float* lnx, float* lnr, float* hn, int32_t rows, int32_t hidden_dim, void* stream) {
    if (int rc = check_gate_shape(rows, hidden_dim)) return rc;
    if (int rc = check_hidden(gh, h)) return rc;
    if (int rc = check_ln(ln)) return rc;
    const void* ptrs[] = {gi, gate, lnx, lnr, hn};
    const char* names[] = {"gi", "gate", "lnx", "lnr", "hn"};
    if (int rc = need_all(ptrs, names, 5)) return rc;
    GateArgs g;
    memset(&g, 0, sizeof g);
    g.gi = gi; g.gh = gh; g.h = h;
    for (int k = 0; k < 3; ++k) { g.g[k] = ln[2 * k]; g.b[k] = ln[2 * k + 1]; }
    g.gate = gate; g.lnx = lnx; g.lnr = lnr; g.hn = hn; g.h_out = hn;
    g.rows = rows; g.Hd = hidden_dim;
    const dim3 grid((rows + 3) / 4);
    if (h) hipLaunchKernelGGL(dt_gate_fwd<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(dt_gate_fwd<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
    return launched("gate_fwd");
}

int tdmpc_drnn_gate_bwd(const float* dhn, const float* gh, const float* h, const float* const* ln, const float* gate,
                        const float* lnx, const float* lnr, float* dgi, float* dgh, float* dhd, float* part,
                        int32_t rows, int32_t hidden_dim, void* stream) {
    if (int rc = check_gate_shape(rows, hidden_dim)) return rc;
    if (int rc = check_hidden(gh, h)) return rc;
    if (int rc = check_ln(ln)) return rc;
    const void* ptrs[] = {dhn, gate, lnx, lnr, dgi, part, dgh, dhd};
    const char* names[] = {"dhn", "gate", "lnx", "lnr", "dgi", "part", "dgh", "dhd"};
    if (int rc = need_all(ptrs, names, h ? 8 : 6)) return rc;
    GateArgs g;
    memset(&g, 0, sizeof g);
    g.gh = gh; g.h = h;
    for (int k = 0; k < 3; ++k) g.g[k] = ln[2 * k];
    g.gate = const_cast<float*>(gate); g.lnx = const_cast<float*>(lnx); g.lnr = const_cast<float*>(lnr);
    g.dhn = dhn; g.dgi = dgi; g.dgh = dgh; g.dhd = dhd; g.part = part;
    g.rows = rows; g.Hd = hidden_dim;
    const dim3 grid(gate_wgs(rows));
    if (h) hipLaunchKernelGGL(dt_gate_bwd<false>, grid, dim3(256), 0, (hipStream_t)stream, g);
    else hipLaunchKernelGGL(dt_gate_bwd<true>, grid, dim3(256), 0, (hipStream_t)stream, g);
    return launched("gate_bwd");
}

}  // extern "C"
