// extern "C" entry points of the proof search (include/m0_proof.h): the switch of an engine, the result of a split-step search,
// and the host export of the rule (proof_core.h), which needs no GPU.
#include "selfplay_engine.h"

using namespace m0;

static_assert(M0_AN_MAX_LINES == 8, "m0_proof_lines (include/m0_proof.h) holds one entry per analysis line");

extern "C" {

int m0_selfplay_set_proof(m0_selfplay* sp, int on) {
    M0_ENGINE_CALL(sp, "m0_selfplay_set_proof", KIND_ANY, true);
    if (sp->kind == EngineKind::SelfPlay && sp->net) {
        m0_set_error("m0_selfplay_set_proof: not on a self-play engine that plays games with its own network "
                     "(searches that end early would change the policy targets)");
        return M0_ERR_STATE;
    }
    // turning it off asks the same: an engine in another mode answers that the proof search does not go with it
    if (const int rc = mode_settable(sp, MODE_PROOF, "the proof search")) return rc;
    if (on && !sp->d.t.proof) {
        int16_t* proof = dalloc<int16_t>(sp, (size_t)sp->G * 2 * sp->cap);       // zeroed: nothing is proven
        ProofResult* res = dalloc<ProofResult>(sp, sp->G);
        M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
        if (!hip_ok(sp, "hipMalloc failed for the proof search")) return M0_ERR_HIP;
        sp->d.t.proof = proof;
        sp->d.proof_results = res;
        sp->hpres.resize(sp->G);
        if (sp->an) {                           // an analysis engine: the result kernel's proof output, one entry per slot
            sp->an->proof_dev = dalloc<m0_proof_lines>(sp, sp->G);
            M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
            if (!hip_ok(sp, "hipMalloc failed for the proof search")) return M0_ERR_HIP;
            sp->an->hproof.resize(sp->G);
        }
    }
    sp->tc.mode = on ? MODE_PROOF : MODE_PUCT;
    return M0_OK;
}

int m0_search_proof_result(m0_selfplay* sp, int g, int* state, int* plies, int32_t* child_state, int32_t* child_plies, int* pick) {
    M0_ENGINE_CALL(sp, "m0_search_proof_result", KIND_GAMES, true);
    bool finished;
    if (const int rc = mode_result_fetch(sp, g, MODE_PROOF, "m0_search_proof_result", &finished)) return rc;
    if (pick) *pick = -1;
    if (state) *state = M0_PROOF_NONE;
    if (plies) *plies = 0;
    if (!finished) return M0_OK;
    const ProofResult& R = sp->hpres[g];
    const int k = sp->hres[g].nchild;
    if (pick) *pick = R.pick;
    if (state) *state = R.state;
    if (plies) *plies = R.plies;
    for (int i = 0; i < k; ++i) {
        if (child_state) child_state[i] = proof_state(R.child[i]);
        if (child_plies) child_plies[i] = proof_plies(R.child[i]);
    }
    return M0_OK;
}

int m0_proof_combine(int k, const int32_t* states, const int32_t* plies, int complete, int* state, int* plies_out) {
    if (k < 1 || k > M0_MAX_CHILDREN || !states || !plies) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    ProofFold f = proof_fold_empty();
    for (int i = 0; i < k; ++i) {
        if (states[i] < M0_PROOF_NONE || states[i] > M0_PROOF_DRAW || plies[i] < 0 || plies[i] > PROOF_MAX_PLIES) {
            m0_set_error("m0_proof_combine: a state outside 0 .. 3 or plies outside 0 .. 8191");
            return M0_ERR_INVALID;
        }
        f = proof_fold_child(f, proof_pack(states[i], plies[i]));
    }
    const int16_t r = proof_fold_result(f, complete != 0);
    if (state) *state = proof_state(r);
    if (plies_out) *plies_out = proof_plies(r);
    return M0_OK;
}

}  // extern "C"
