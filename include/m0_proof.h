/* Proof search: exact wins, losses and draws backed up the search tree, opt-in (m0_engine.h includes this file: the calls here
 * are part of the same C ABI and the same library).  With the switch never set an engine searches exactly as before, and while
 * nothing in a tree is proven a search with the switch set is, bit for bit, the search without it.
 *
 * A node holds a state and a distance `plies`, both from the view of the side to move at that node: WIN and LOSS mean that the
 * game is decided in `plies` plies with best play, DRAW has plies 0, NONE is not proven.
 *   sources    a leaf that the search finds terminal is proven at its first visit: checkmate LOSS 0; stalemate, insufficient
 *              material and halfmove >= 150 DRAW; a hit in attached endgame tables (m0_selfplay_set_search_tablebase) the
 *              table's verdict with its distance to mate.  Fivefold repetition depends on the path and proves nothing.
 *   combine    when a child's state changes its parent P is re-examined, then P's parent, while a state changes:
 *                1. a LOSS child: P is WIN in 1 + the smallest plies among the LOSS children;
 *                2. else, if P's children are all of its legal moves and every child is proven: DRAW with a DRAW child, else
 *                   LOSS in 1 + the largest plies;
 *                3. else P stays NONE.
 *              With max_children or min_child_prior pruning step 2 never fires: only wins are proven there.  A proven state
 *              never changes afterwards (the distance of a WIN is that of the first refutation found, an upper bound).
 *   search     a descent that arrives at a proven node stops there: a terminal sample that backs up +1, -1 or draw_penalty as
 *              a table hit of that outcome does, and counts as a simulation.  In the children scan a child that is WIN for its
 *              own mover cannot be the arg-max unless every child is one; skipping consumes no random draw.  A search whose
 *              root is proven ends: no further sample, finished whatever is left of its budget.
 *   result     `pick`, an index into the root children (ties to the lowest index): root WIN the LOSS child with the fewest
 *              plies; LOSS the child with the most plies; DRAW the DRAW child with the most visits; NONE the most visited child
 *              that is not WIN for its mover, the most visited child where there is none. */
#ifndef M0_PROOF_H
#define M0_PROOF_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_PROOF_NONE 0
#define M0_PROOF_WIN  1
#define M0_PROOF_LOSS 2
#define M0_PROOF_DRAW 3

/* What an analysis engine in this mode knows beside a m0_analysis_result (m0_analysis_last_proof): the root's state and
 * plies, and for line l of the result the state and plies of the root's side to move after that line's move (a line whose
 * move mates in 3 plies is WIN 3).  All zero for a result without a search behind it and with the mode off. */
typedef struct m0_proof_lines {
    int32_t proof;               /* M0_PROOF_* of the root */
    int32_t proof_plies;
    int32_t line_proof[8];       /* one per line: M0_AN_MAX_LINES */
    int32_t line_proof_plies[8];
} m0_proof_lines;

/* Turns the mode on (on != 0) or off, before the first step or search: engines driven by the split-step m0_search_* calls or an
 * external evaluator, match engines and analysis engines.  M0_ERR_STATE afterwards and on a self-play engine that plays games
 * with its own network (searches that end early would change the policy targets); M0_ERR_INVALID on an engine with compat
 * tt_merge (the search graph is no tree there) or with the Gumbel root search. */
int m0_selfplay_set_proof(m0_selfplay* sp, int on);
/* Split-step search: what the finished search of slot g proved, beside m0_search_result -- the root's state and plies, every
 * root child's (one entry per child of that result, at most 256; a child's are from the view of ITS side to move) and `pick`
 * (-1 while the search is not finished, and for a root without children: a kept subtree whose root is a proven leaf ends
 * with no child; such a root is not evaluated again either, the value of the root stays the previous search's).  Each output
 * may be NULL.  M0_ERR_STATE on an engine without the mode. */
int m0_search_proof_result(m0_selfplay* sp, int g, int* state, int* plies, int32_t* child_state, int32_t* child_plies, int* pick);

/* Analysis engines in this mode: the lines of a result are ranked as m0_tb_root_lines ranks table roots -- winning moves,
 * shortest first; unproven and drawn moves by visits; losing moves, longest first -- and the variation behind a line follows
 * `pick` at every proven node.  A search whose root is proven is answered at once, with fewer simulations than it asked for.
 * m0_analysis_last_proof: the proofs that go with the result which the last m0_analysis_poll, m0_analysis_poll_visits or
 * m0_analysis_peek on this engine returned (m0_analysis_result itself is as it was).  M0_ERR_STATE on an engine that is no
 * analysis engine or runs without the mode, M0_ERR_INVALID for a null argument. */
int m0_analysis_last_proof(m0_selfplay* sp, m0_proof_lines* out);

/* The rule alone, on the host (no GPU needed); the kernels use the same definitions.  The parent's state and plies from its k
 * children's; `complete`: the children are all of the parent's legal moves.  M0_ERR_INVALID for a null input, k outside
 * 1 .. 256, a state outside the four above or plies outside 0 .. 8191; outputs may be NULL. */
int m0_proof_combine(int k, const int32_t* states, const int32_t* plies, int complete, int* state, int* plies_out);

#ifdef __cplusplus
}
#endif
#endif /* M0_PROOF_H */
