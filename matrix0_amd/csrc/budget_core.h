// Arithmetic of the self-play budget mix (include/m0_budget.h): the full-or-fast draw of a ply, the forced-playout threshold and
// deficit test, and the pruning of a root's visit counts into a policy target.  Plain functions without tree types, for the
// host (m0_budget_is_full, m0_budget_forced, m0_budget_prune, the game loop) and for the kernels (tree_forced.h) alike.  All in
// double.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"      // M0_HD, mix64

namespace m0 {

constexpr int PURPOSE_BUDGET = 7;                     // the game's budget stream, beside the purposes of host_rules.h
constexpr int M0_BUDGET_MAX_K = 256;                  // = M0_MAX_CHILDREN (tree.h asserts it)

// draw `ply` of the stream of (seed, game, PURPOSE_BUDGET): derive_seed and HStream of host_rules.h, position by position
M0_HD double budget_draw(uint64_t seed, int game, int ply) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t s = mix64(mix64(seed + G * (uint64_t)(game + 1)) ^ ((uint64_t)PURPOSE_BUDGET * 0xD6E8FEB86659FD93ull));
    return (double)(mix64(s + ((uint64_t)ply + 1) * G) >> 11) * (1.0 / 9007199254740992.0);
}
M0_HD bool budget_is_full(uint64_t seed, int game, int ply, double full_prob) { return budget_draw(seed, game, ply) < full_prob; }

// the visits a visited root child is brought up to
M0_HD double budget_forced(double forced_k, double prior, int64_t n_sum) { return sqrt(forced_k * prior * (double)n_sum); }
// n: completed visits, inflight: descents of this pass that are under way through the child
M0_HD bool budget_in_deficit(double forced_k, double prior, int n, int inflight, int64_t n_sum) {
    return n > 0 && (double)(n + inflight) < budget_forced(forced_k, prior, n_sum);
}
// The score a deficit child takes in select's arg-max, which prefers the larger score and the lower index among equals: above
// every PUCT score (|q| <= 1, u <= cpuct * sqrt(N)) and falling with the index, so the deficit child with the lowest index wins.
constexpr double M0_FORCED_SCORE = 1e9;
M0_HD double budget_forced_score(int i) { return M0_FORCED_SCORE - (double)i; }
M0_HD bool budget_score_is_forced(double score) { return score > 0.5 * M0_FORCED_SCORE; }

// select's scan value of a child with m visits, without jitter, virtual loss or the backtrack penalty; sq = sqrt(max(1, root_n))
M0_HD double budget_puct(double q, double cpuct, double prior, double sq, int m) { return q + cpuct * prior * sq / (1.0 + (double)m); }

// The whole pruning for k children.  Returns the number of visits taken out; `best` -1 (and pi all zero) without a visit.
inline int64_t budget_prune(int k, const double* prior, const double* q, const int32_t* n, int root_n, double cpuct, double forced_k,
                            int32_t* pruned_n, double* pi, int* best_out) {
    int b = -1;
    int64_t sum_n = 0;
    for (int i = 0; i < k; ++i) { sum_n += n[i]; if (n[i] > 0 && (b < 0 || n[i] > n[b])) b = i; }
    int32_t m[M0_BUDGET_MAX_K];
    for (int i = 0; i < k; ++i) m[i] = n[i];
    if (b >= 0 && forced_k > 0.0) {
        const double sq = sqrt((double)(root_n > 1 ? root_n : 1));
        const double S = budget_puct(q[b], cpuct, prior[b], sq, n[b]);
        for (int i = 0; i < k; ++i) {
            if (i == b || n[i] <= 0) continue;
            const double fc = ceil(budget_forced(forced_k, prior[i], sum_n));
            const int F = fc < (double)n[i] ? (int)fc : n[i];
            int mi = n[i];
            for (int c = n[i] - F; c <= n[i]; ++c)
                if (budget_puct(q[i], cpuct, prior[i], sq, c) < S) { mi = c; break; }
            if (mi == 1 && n[i] > 1) mi = 0;
            m[i] = mi;
        }
    }
    int64_t sum_m = 0;
    for (int i = 0; i < k; ++i) sum_m += m[i];
    for (int i = 0; i < k; ++i) {
        if (pruned_n) pruned_n[i] = m[i];
        if (pi) pi[i] = sum_m > 0 ? (double)m[i] / (double)sum_m : 0.0;
    }
    if (best_out) *best_out = b;
    return sum_n - sum_m;
}

// nullptr when the options are fine (m0_selfplay_set_budget)
inline const char* budget_bad_cfg(const m0_budget_cfg* c) {
    if (!c) return "cfg is null";
    if (!(c->full_prob > 0.0 && c->full_prob <= 1.0)) return "full_prob must be in (0, 1]";
    if (c->fast_simulations < 1) return "fast_simulations must be at least 1";
    if (!(c->forced_k >= 0.0) || isinf(c->forced_k)) return "forced_k must be finite and not negative";
    if (c->prune_targets != 0 && c->prune_targets != 1) return "prune_targets must be 0 or 1";
    return nullptr;
}

}  // namespace m0
