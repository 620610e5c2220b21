/* Live searches on an analysis engine: a search that can be read while it runs, ended early, and whose tree is kept for the
 * next position of a game -- what a UCI front end (matrix0_amd/uci.py) needs from the engine of m0_analysis_* (m0_engine.h,
 * which includes this file: the calls here are part of the same C ABI and the same library).
 *
 * Every call returns M0_ERR_STATE on an engine that is no analysis engine, and between an m0_analysis_ext_select and its
 * m0_analysis_ext_expand (in-flight marks are in the trees then).  m0_analysis_result keeps its layout.  An engine on which none
 * of these calls is made computes bit for bit what it computed without them.
 *
 * HELD slots.  A search submitted with keep leaves its tree in its slot when it is answered, finished or stopped: the slot is
 * then held under the search's id.  A held slot is in use but searches nothing: m0_analysis_pending does not count it, queued
 * searches do not get it, and it stays until m0_analysis_continue takes it over or m0_analysis_release frees it.  A submission
 * that is answered on the host (mate, stalemate, a root inside attached tables) holds nothing. */
#ifndef M0_ANALYSIS_LIVE_H
#define M0_ANALYSIS_LIVE_H
#ifdef __cplusplus
extern "C" {
#endif

/* m0_analysis_submit with sims > 0 (M0_ERR_INVALID otherwise) whose slot is held once the search is answered. */
int m0_analysis_submit_keep(m0_selfplay* sp, const char* fen, const char* const* ucis, int n_moves, int sims, int64_t id);
/* The current result of the search `id` while it runs.  1: `out` is written: the lines by visits and their PVs exactly as the
 * harvest of a finished search writes them, root_n, root_q, value, evals, overflow, and `sims` = the simulations done so far;
 * a root that is not expanded yet has nlines = 0.  0: the id still waits in the queue, `out` untouched.  M0_ERR_INVALID: an
 * unknown id (held ones included: their result was polled) or a policy-mode submission.  A peek only reads: the final result of
 * a search is the same bytes whether or not, and however often, it was peeked. */
int m0_analysis_peek(m0_selfplay* sp, int64_t id, m0_analysis_result* out);
/* Answer the search `id` now, without a further simulation: its result joins the answered ones (m0_analysis_poll) and equals,
 * field by field, a peek taken immediately before; `sims` holds the simulations done.  The slot is freed, or held if the search
 * was submitted with keep.  An id that still waits in the queue is removed and answered with status 0 and
 * sims = root_n = nlines = evals = 0.  With m0_analysis_keep_visits on, a stopped search reports nchild = 0: the root's
 * children are gathered from the block that only a finished search writes.  M0_ERR_INVALID: an unknown or policy-mode id. */
int m0_analysis_stop(m0_selfplay* sp, int64_t id);
/* Search the held position plus n_moves further legal moves (0 <= n_moves <= 8; 0: the same root, further) in the held slot,
 * under the new id.  The moves are played on the slot's line, so the repetition window sees them; an illegal move, n_moves out
 * of range, sims < 1 or an id that is not held: M0_ERR_INVALID, nothing changed.
 * The walk happens on the device (csrc/tree_reroot.hip) and the call waits for it.  When it reaches an expanded node through
 * expanded children, that node's subtree becomes the tree of the new search, compacted into the slot's other arena half, and
 * *reused_n (nullable) is its visit count.  Otherwise (a move that is not among a node's children with max_children /
 * min_child_prior pruning, an unexpanded node) the slot starts a fresh tree and *reused_n = 0; the result is then bit for bit
 * that of m0_analysis_submit(base fen, all moves so far, sims, id).
 * Budget: `sims` NEW simulations are run on top of the visits the kept root carries, as a self-play search on a reused
 * subtree counts them (MCTS.run on a root found again): root_n of the result = *reused_n + sims, and `sims` of the result
 * counts the new ones.  As there, a kept root is evaluated once more for `value` (one evaluation, no simulation), and
 * opts->dirichlet noise is applied again to its priors.  The random streams are reseeded from (cfg->seed, id), counters zero.
 * A final position without legal moves or, with tables attached, inside them is answered at once as m0_analysis_submit answers
 * it (*reused_n = 0) and the slot is released.  held_id stops being held either way; `id` is held afterwards if keep. */
int m0_analysis_continue(m0_selfplay* sp, int64_t held_id, const char* const* ucis, int n_moves, int sims, int64_t id, int keep,
                         int32_t* reused_n);
int m0_analysis_release(m0_selfplay* sp, int64_t held_id);   /* frees a held slot; M0_ERR_INVALID if the id is not held */
int m0_analysis_held(m0_selfplay* sp);                       /* the number of held slots */
/* m0_analysis_step / m0_analysis_ext_select with searches queued, none in a slot and every slot held: M0_ERR_STATE (release
 * one), not a pass that does nothing. */

#ifdef __cplusplus
}
#endif
#endif /* M0_ANALYSIS_LIVE_H */
