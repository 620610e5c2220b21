/* Self-play budget mix (Wu, "Accelerating Self-Play Learning in Go", 2019, sections 3.1 and 3.2): playout-cap randomisation,
 * forced playouts and policy-target pruning for self-play engines and the split-step search, opt-in (m0_engine.h includes this
 * file: the calls here are part of the same C ABI and the same library).  With the switch never set an engine searches and
 * plays exactly as before.
 *
 * Per searched ply of a self-play game:
 *   draw       full = u < full_prob, u the ply's draw of the game's budget stream (keyed by seed, game index and purpose 7; one
 *              draw per searched ply, also at full_prob = 1).  The game stream is consumed as without the mode.
 *   budget     num_simulations for a full search, fast_simulations for a fast one, then playout_random_frac as ever.
 *   fast       no Dirichlet noise (whatever dirichlet_plies says), no forced playouts, visit shares as the recorded target.
 *   full       noise by the existing rule; forced playouts when forced_k > 0; the pruned target when prune_targets is set.
 * Forced playouts, at depth 0 of a descent of a full search: with N the sum of the root children's completed visits n_i, P_i the
 * root priors as select scores them (after noise) and f_i the in-flight counts select tracks (0 with virtual_loss_active off),
 * child i is in deficit when n_i > 0 and n_i + f_i < sqrt(forced_k * P_i * N), compared in double.  The descent takes the
 * deficit child with the lowest index; with none the PUCT scan decides.  The jitter stream advances by the number of children
 * either way.  Below the root nothing changes.
 * Target pruning, at the end of a full search, from the root children's p_i, q_i, n_i, the root's own visits root_n and
 * c = cpuct at depth 0:  PUCT(i; m) = q_i + c * p_i * sqrt(max(1, root_n)) / (1 + m);  b = the most visited child (lowest index
 * among equals), S = PUCT(b; n_b), m_b = n_b;  for every other child with n_i > 0: F_i = min(n_i, ceil(sqrt(forced_k * p_i *
 * sum n))), m_i = the smallest integer in [n_i - F_i, n_i] with PUCT(i; m_i) < S, n_i when there is none, and 0 where that
 * leaves exactly 1 of more.  The target is m_i / sum m; the move is sampled from the m_i with the same function and draw; the
 * policy entropy is the target's. */
#ifndef M0_BUDGET_H
#define M0_BUDGET_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct m0_budget_cfg {
    double full_prob;        /* (0, 1]: probability that a move's search is a full one */
    int    fast_simulations; /* >= 1: the budget of a fast search */
    double forced_k;         /* >= 0, finite; 0 = no forced playouts (KataGo: 2) */
    int    prune_targets;    /* 0 / 1 */
} m0_budget_cfg;

/* Turns the mode on: self-play engines (with their own network, an external evaluator or the split-step m0_search_* calls),
 * before the first step or search.  M0_ERR_STATE afterwards and on match and analysis engines; M0_ERR_INVALID for a null
 * argument, a value out of the ranges above, an engine with compat tt_merge, and an engine in the Gumbel root search or the
 * proof search (whose setters in turn refuse an engine in this mode). */
int m0_selfplay_set_budget(m0_selfplay* sp, const m0_budget_cfg* cfg);
/* Split-step search, where every search begun on an engine in the mode is a full one: what the finished search of slot g gives
 * beside m0_search_result -- the pruned visit counts and the target (one entry per root child, at most 256; the plain counts
 * and shares with forced_k = 0 or prune_targets = 0) -- and `forced_descents`: the descents the forcing rule has decided in
 * this slot since the engine was made.  While the search is not finished the arrays are left alone and forced_descents is -1.
 * Each output may be NULL.  M0_ERR_STATE on an engine without the mode. */
int m0_search_budget_result(m0_selfplay* sp, int g, int32_t* pruned_n, double* pi, int* forced_descents);
/* A polled game record of an engine in the mode: per recorded ply (rec->moves entries each) whether its search was a full one
 * and the simulations it was given.  The arrays belong to the record and live until m0_game_record_free.  Both are NULL, with
 * M0_OK, for a record of an engine without the mode.  Either output may be NULL. */
int m0_game_record_budget(const m0_game_record* rec, const uint8_t** full, const int32_t** sims);
/* out[4]: full searches, fast searches, descents decided by the forcing rule (as of the last step), visits pruned from targets.
 * M0_ERR_STATE on an engine without the mode. */
int m0_selfplay_budget_stats(m0_selfplay* sp, uint64_t* out);

/* The arithmetic alone, on the host (no GPU needed); the kernels use the same definitions.
 * m0_budget_is_full: the draw of searched ply `ply` (>= 0) of game `game_index`.  M0_ERR_INVALID for a null output, a
 * negative ply or a full_prob outside (0, 1]. */
int m0_budget_is_full(uint64_t seed, int game_index, int ply, double full_prob, int* full);
/* m0_budget_forced: sqrt(forced_k * prior * n_sum), the visits a visited root child is brought up to.  M0_ERR_INVALID for a
 * null output, a forced_k or prior that is negative or not finite, or a negative n_sum. */
int m0_budget_forced(double forced_k, double prior, int64_t n_sum, double* n_forced);
/* m0_budget_prune: pruned_n[k], pi[k] and the most visited child of k children.  M0_ERR_INVALID for a null input, k outside
 * 1 .. 256, a negative visit count or a forced_k that is negative or not finite; outputs may be NULL.  Without a visit pi is
 * all zero and best is -1. */
int m0_budget_prune(int k, const double* prior, const double* q, const int32_t* n, int root_n, double cpuct,
                    double forced_k, int32_t* pruned_n, double* pi, int* best);

#ifdef __cplusplus
}
#endif
#endif /* M0_BUDGET_H */
