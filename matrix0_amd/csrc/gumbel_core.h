// Arithmetic of the Gumbel root search (include/m0_gumbel.h): the considered-visits schedule of sequential halving, the scores
// and the improved policy.  Plain functions without tree types, for the host (m0_gumbel_schedule, m0_gumbel_improve) and for
// the kernels (tree_gumbel.h) alike.  All in double.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"      // M0_HD

namespace m0 {

constexpr int PURPOSE_GUMBEL = 6;                     // the game's Gumbel stream, beside the purposes of host_rules.h
constexpr int M0_GUMBEL_MAX_K = 256;                  // = M0_MAX_CHILDREN (tree.h asserts it)

M0_HD int gumbel_m_eff(int max_considered, int k) { return max_considered < k ? max_considered : k; }

// Where simulation s of n stands in mctx's get_sequence_of_considered_visits(m_eff, n): the visit count of the root children it
// considers, and the first simulation after its phase.  The sequence is built in rounds: `num` children, all visited `base`
// times, get `extra` = max(1, n / (ceil(log2 m_eff) * num)) visits each, one each in turn; then num = max(2, num / 2).  The
// children still considered after a halving are a prefix of those before, so they all carry the same count, and the rounds
// at num == 2, which repeat until n is reached, are one phase.  At most 8 turns of the loop (m_eff <= 256), no table.
struct GumbelSlot { int considered, phase_end; };
M0_HD GumbelSlot gumbel_slot(int m_eff, int n, int s) {
    if (m_eff <= 1) return GumbelSlot{s, n};
    int log2max = 0;
    while ((1 << log2max) < m_eff) ++log2max;
    int num = m_eff, start = 0, base = 0;
    while (num > 2) {
        int extra = n / (log2max * num);
        if (extra < 1) extra = 1;
        const int len = extra * num;
        if (s < start + len) return GumbelSlot{base + (s - start) / num, start + len < n ? start + len : n};
        start += len; base += extra;
        num = num / 2 > 2 ? num / 2 : 2;
    }
    return GumbelSlot{base + (s - start) / 2, n};
}
M0_HD int gumbel_considered(int m_eff, int n, int s) { return gumbel_slot(m_eff, n, s).considered; }
M0_HD int gumbel_phase_end(int m_eff, int n, int s) { return gumbel_slot(m_eff, n, s).phase_end; }

M0_HD double gumbel_q01(double q) { return (q + 1.0) * 0.5; }
M0_HD double gumbel_sigma(const m0_gumbel_cfg& c, int max_n, double q) {
    return (c.c_visit + (double)max_n) * c.c_scale * gumbel_q01(q);
}
// sum_n, sum_p, sum_pq: visits, priors and prior * q summed over the visited children
M0_HD double gumbel_v_mix(double root_v, long sum_n, double sum_p, double sum_pq) {
    if (sum_n <= 0 || !(sum_p > 0.0)) return root_v;
    return (root_v + ((double)sum_n / sum_p) * sum_pq) / (1.0 + (double)sum_n);
}
// u: a uniform draw in [0, 1)
M0_HD double gumbel_from_uniform(double u) { return -log(-log(u < 1e-300 ? 1e-300 : u)); }
// what a child adds to its log-prior (the improved policy's logit) or to gl (its score)
M0_HD double gumbel_bonus(const m0_gumbel_cfg& c, int max_n, int n, double q, double v_mix) {
    return gumbel_sigma(c, max_n, n > 0 ? q : v_mix);
}
// the final move's order: more visits, then the larger score, then the lower index
M0_HD bool gumbel_pick_better(int n, double score, int i, int bn, double bscore, int bi) {
    if (bi < 0) return true;
    if (n != bn) return n > bn;
    if (score != bscore) return score > bscore;
    return i < bi;
}

// The whole result for k children, one after the other (the kernel does the same with one child per lane: tree_gumbel.h).
inline void gumbel_improve(int k, const double* prior, const double* q, const int32_t* n, const double* gl, double root_v,
                           const m0_gumbel_cfg& c, double* pi, double* v_mix_out, int* pick_out) {
    int max_n = 0;
    long sum_n = 0;
    double sum_p = 0.0, sum_pq = 0.0;
    for (int i = 0; i < k; ++i)
        if (n[i] > 0) { if (n[i] > max_n) max_n = n[i]; sum_n += n[i]; sum_p += prior[i]; sum_pq += prior[i] * q[i]; }
    const double v_mix = gumbel_v_mix(root_v, sum_n, sum_p, sum_pq);
    double mx = -INFINITY, sum = 0.0;
    int bi = -1, bn = 0;
    double bscore = 0.0;
    for (int i = 0; i < k; ++i) {
        const double b = gumbel_bonus(c, max_n, n[i], q[i], v_mix);
        const double l = log(prior[i]) + b;
        if (l > mx) mx = l;
        if (gumbel_pick_better(n[i], gl[i] + b, i, bn, bscore, bi)) { bi = i; bn = n[i]; bscore = gl[i] + b; }
    }
    if (pi) {
        for (int i = 0; i < k; ++i) { pi[i] = exp(log(prior[i]) + gumbel_bonus(c, max_n, n[i], q[i], v_mix) - mx); sum += pi[i]; }
        for (int i = 0; i < k; ++i) pi[i] /= sum;
    }
    if (v_mix_out) *v_mix_out = v_mix;
    if (pick_out) *pick_out = bi;
}

// nullptr when the constants are fine (m0_selfplay_set_gumbel, m0_gumbel_improve)
inline const char* gumbel_bad_constants(const m0_gumbel_cfg* c) {
    if (!c) return "cfg is null";
    if (!(c->c_visit >= 0.0) || !(c->c_scale >= 0.0) || isinf(c->c_visit) || isinf(c->c_scale))
        return "c_visit and c_scale must be finite and not negative";
    return nullptr;
}

}  // namespace m0
