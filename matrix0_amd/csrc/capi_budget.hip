// extern "C" entry points of the self-play budget mix (include/m0_budget.h): the switch of a self-play engine, the result of a
// split-step search, a record's per-ply budget, the counters, and the host exports of the arithmetic (budget_core.h), which
// need no GPU.
#include <math.h>
#include "selfplay_engine.h"

using namespace m0;

extern "C" {

int m0_selfplay_set_budget(m0_selfplay* sp, const m0_budget_cfg* cfg) {
    if (!sp || !cfg) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_set_budget", KIND_SELFPLAY, false);
    if (const int rc = mode_settable(sp, MODE_BUDGET, "the self-play budget mix")) return rc;
    if (const char* bad = budget_bad_cfg(cfg)) { m0_set_error(bad); return M0_ERR_INVALID; }
    sp->tc.mode = MODE_BUDGET;
    sp->tc.forced_k = cfg->forced_k;
    sp->budget = *cfg;
    return M0_OK;
}

int m0_search_budget_result(m0_selfplay* sp, int g, int32_t* pruned_n, double* pi, int* forced_descents) {
    M0_ENGINE_CALL(sp, "m0_search_budget_result", KIND_SELFPLAY, true);
    bool finished;
    if (const int rc = mode_result_fetch(sp, g, MODE_BUDGET, "m0_search_budget_result", &finished)) return rc;
    if (forced_descents) *forced_descents = -1;
    if (!finished) return M0_OK;
    const RootResult& R = sp->hres[g];
    const bool prune = sp->budget.prune_targets && sp->budget.forced_k > 0.0;
    budget_prune(R.nchild, R.child_prior, R.child_q, R.child_n, R.root_n, cpuct_at_root(sp->tc), prune ? sp->budget.forced_k : 0.0,
                 pruned_n, pi, nullptr);
    if (forced_descents) *forced_descents = (int)sp->hg[g].forced_descents;
    return M0_OK;
}

int m0_game_record_budget(const m0_game_record* rec, const uint8_t** full, const int32_t** sims) {
    if (!rec) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    const GameRecordOwner* o = (const GameRecordOwner*)rec->owner;
    const bool have = o && o->budget && (int)o->full.size() == rec->moves && (int)o->sims.size() == rec->moves;
    if (full) *full = have ? o->full.data() : nullptr;
    if (sims) *sims = have ? o->sims.data() : nullptr;
    return M0_OK;
}

int m0_selfplay_budget_stats(m0_selfplay* sp, uint64_t* out) {
    if (!sp || !out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_budget_stats", KIND_SELFPLAY, false);
    if (!is_budget(sp->tc)) { m0_set_error("m0_selfplay_budget_stats: the self-play budget mix is not set on this engine"); return M0_ERR_STATE; }
    uint64_t forced = 0;
    for (const GameDev& g : sp->hg) forced += g.forced_descents;      // the mirror the last step copied
    out[0] = sp->budget_full; out[1] = sp->budget_fast; out[2] = forced; out[3] = sp->budget_pruned;
    return M0_OK;
}

int m0_budget_is_full(uint64_t seed, int game_index, int ply, double full_prob, int* full) {
    if (!full || ply < 0 || !(full_prob > 0.0 && full_prob <= 1.0)) {
        m0_set_error("m0_budget_is_full: a null output, a negative ply or full_prob outside (0, 1]");
        return M0_ERR_INVALID;
    }
    *full = budget_is_full(seed, game_index, ply, full_prob) ? 1 : 0;
    return M0_OK;
}

int m0_budget_forced(double forced_k, double prior, int64_t n_sum, double* n_forced) {
    if (!n_forced || !(forced_k >= 0.0) || isinf(forced_k) || !(prior >= 0.0) || isinf(prior) || n_sum < 0) {
        m0_set_error("m0_budget_forced: a null output, forced_k or prior negative or not finite, or a negative n_sum");
        return M0_ERR_INVALID;
    }
    *n_forced = budget_forced(forced_k, prior, n_sum);
    return M0_OK;
}

int m0_budget_prune(int k, const double* prior, const double* q, const int32_t* n, int root_n, double cpuct, double forced_k,
                    int32_t* pruned_n, double* pi, int* best) {
    if (!prior || !q || !n || k < 1 || k > M0_MAX_CHILDREN || !(forced_k >= 0.0) || isinf(forced_k)) {
        m0_set_error("m0_budget_prune: a null input, k outside 1 .. 256, or forced_k negative or not finite");
        return M0_ERR_INVALID;
    }
    for (int i = 0; i < k; ++i)
        if (n[i] < 0) { m0_set_error("m0_budget_prune: a negative visit count"); return M0_ERR_INVALID; }
    budget_prune(k, prior, q, n, root_n, cpuct, forced_k, pruned_n, pi, best);
    return M0_OK;
}

}  // extern "C"
