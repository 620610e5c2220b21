/* Gumbel root search (Danihelka et al., "Policy improvement by planning with Gumbel", ICLR 2022; the algorithm of mctx's
 * gumbel_muzero_policy) for self-play engines and the split-step search, opt-in (m0_engine.h includes this file: the calls here
 * are part of the same C ABI and the same library).  With the switch never set an engine searches exactly as before.
 *
 * With k root children, n simulations and m = min(max_considered, k):
 *   schedule   seq[0..n) = mctx's get_sequence_of_considered_visits(m, n): simulation s goes to a root child that has been
 *              visited seq[s] times.  A PHASE is a maximal run of simulations under one number of considered children; a pass of
 *              the search never crosses a phase boundary, where the halving needs the values the phase brought.
 *   scores     sigma(q) = (c_visit + max_b N_b) * c_scale * (q + 1) / 2;  completedQ_i = q_i where N_i > 0, else
 *              v_mix = (root_v + (sum N / sum_{N_b>0} p_b) * sum_{N_b>0} p_b q_b) / (1 + sum N)  (root_v when nothing is visited);
 *              gl_i = g_i + log p_i with g_i = -log(-log u_i), u_i the i-th draw of the game's Gumbel stream, k draws per
 *              search;  score_i = gl_i + sigma(completedQ_i).  p: the stored root priors, q: the children's values as the
 *              search scores them, root_v: the network's value of the root.  Everything in double.
 *   descent    simulation s takes, among the root children visited seq[s] times, the one with the largest score (lowest index
 *              among equals); below the root the search is the PUCT search.  No Dirichlet noise, no jitter at the root.
 *   result     pi = softmax_i(log p_i + sigma(completedQ_i)) over all k children; the move is, among the children with the most
 *              visits, the one with the largest score (lowest index among equals).
 * Every search in this mode starts from a fresh tree.  A self-play engine records pi as the policy target and plays the move
 * (no temperature sampling: the Gumbel draw is the sampling). */
#ifndef M0_GUMBEL_H
#define M0_GUMBEL_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct m0_gumbel_cfg {
    int max_considered; /* 1 .. 256: root children that take part in the halving (the paper: 16) */
    double c_visit;     /* >= 0 (the paper: 50) */
    double c_scale;     /* >= 0 (the paper: 1) */
} m0_gumbel_cfg;

/* Turns the mode on: self-play engines (with their own network, an external evaluator or the split-step m0_search_* calls),
 * before the first step or search.  M0_ERR_STATE afterwards and on match and analysis engines; M0_ERR_INVALID for a null
 * argument, max_considered outside 1 .. 256, a constant that is negative or not finite, or an engine with compat tt_merge. */
int m0_selfplay_set_gumbel(m0_selfplay* sp, const m0_gumbel_cfg* cfg);
/* Split-step search: what the finished search of slot g found beside m0_search_result -- the move (`pick`, an index into that
 * result's children; -1 while the search is not finished), v_mix, pi and gl (one entry per root child, at most 256) and `miss`:
 * how often, since the slot was taken, no root child had the scheduled visit count (0 unless the schedule is broken).  Each
 * output may be NULL.  M0_ERR_STATE on an engine without the mode. */
int m0_search_gumbel_result(m0_selfplay* sp, int g, int* pick, double* v_mix, double* pi, double* gl, int* miss);

/* The arithmetic alone, on the host (no GPU needed); the kernels use the same definitions.
 * m0_gumbel_schedule: seq[s] and phase_end[s] (the first simulation after the phase that holds s) for s in [0, n); either may
 * be NULL.  M0_ERR_INVALID for m_eff < 0 or n < 0. */
int m0_gumbel_schedule(int m_eff, int n, int32_t* seq, int32_t* phase_end);
/* m0_gumbel_improve: pi[k], v_mix and the move from k children's prior, q, visits n and gl.  M0_ERR_INVALID for a null input,
 * k outside 1 .. 256 or constants as m0_selfplay_set_gumbel refuses them (max_considered is not read); outputs may be NULL. */
int m0_gumbel_improve(int k, const double* prior, const double* q, const int32_t* n, const double* gl, double root_v,
                      const m0_gumbel_cfg* cfg, double* pi, double* v_mix, int* pick);

#ifdef __cplusplus
}
#endif
#endif /* M0_GUMBEL_H */
