// extern "C" entry points of the Gumbel root search (include/m0_gumbel.h): the switch of a self-play engine, the result of a
// split-step search, and the host exports of the arithmetic (gumbel_core.h), which need no GPU.
#include <math.h>
#include "selfplay_engine.h"

using namespace m0;

extern "C" {

int m0_selfplay_set_gumbel(m0_selfplay* sp, const m0_gumbel_cfg* cfg) {
    if (!sp || !cfg) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_set_gumbel", KIND_SELFPLAY, true);
    if (const int rc = mode_settable(sp, MODE_GUMBEL, "the Gumbel root search")) return rc;
    if (cfg->max_considered < 1 || cfg->max_considered > M0_MAX_CHILDREN) {
        m0_set_error("max_considered must be in 1 .. 256");
        return M0_ERR_INVALID;
    }
    if (const char* bad = gumbel_bad_constants(cfg)) { m0_set_error(bad); return M0_ERR_INVALID; }
    if (!sp->d.gumbel_gl) {
        double* gl = dalloc<double>(sp, (size_t)sp->G * M0_MAX_CHILDREN);
        GumbelResult* res = dalloc<GumbelResult>(sp, sp->G);
        M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
        if (!hip_ok(sp, "hipMalloc failed for the Gumbel root search")) return M0_ERR_HIP;
        sp->d.gumbel_gl = gl;
        sp->d.gumbel_results = res;
        sp->hgres.resize(sp->G);
    }
    sp->tc.mode = MODE_GUMBEL;
    sp->tc.gumbel_cfg = *cfg;
    return M0_OK;
}

int m0_search_gumbel_result(m0_selfplay* sp, int g, int* pick, double* v_mix, double* pi, double* gl, int* miss) {
    M0_ENGINE_CALL(sp, "m0_search_gumbel_result", KIND_SELFPLAY, true);
    bool finished;
    if (const int rc = mode_result_fetch(sp, g, MODE_GUMBEL, "m0_search_gumbel_result", &finished)) return rc;
    if (miss) *miss = sp->hg[g].gumbel_miss;
    if (pick) *pick = -1;
    if (!finished) return M0_OK;
    const GumbelResult& R = sp->hgres[g];
    const int k = sp->hres[g].nchild;
    if (pick) *pick = R.pick;
    if (v_mix) *v_mix = R.v_mix;
    for (int i = 0; i < k; ++i) {
        if (pi) pi[i] = R.pi[i];
        if (gl) gl[i] = R.gl[i];
    }
    return M0_OK;
}

int m0_gumbel_schedule(int m_eff, int n, int32_t* seq, int32_t* phase_end) {
    if (m_eff < 0 || n < 0) { m0_set_error("m_eff and n must not be negative"); return M0_ERR_INVALID; }
    for (int s = 0; s < n; ++s) {
        const GumbelSlot at = gumbel_slot(m_eff, n, s);
        if (seq) seq[s] = at.considered;
        if (phase_end) phase_end[s] = at.phase_end;
    }
    return M0_OK;
}

int m0_gumbel_improve(int k, const double* prior, const double* q, const int32_t* n, const double* gl, double root_v,
                      const m0_gumbel_cfg* cfg, double* pi, double* v_mix, int* pick) {
    if (!prior || !q || !n || !gl || k < 1 || k > M0_MAX_CHILDREN) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    if (const char* bad = gumbel_bad_constants(cfg)) { m0_set_error(bad); return M0_ERR_INVALID; }
    gumbel_improve(k, prior, q, n, gl, root_v, *cfg, pi, v_mix, pick);
    return M0_OK;
}

}  // extern "C"
