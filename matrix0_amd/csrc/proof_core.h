// Arithmetic of the proof search (include/m0_proof.h): a node's proven state and distance packed into 16 bits, the rule that
// combines the children's proofs into their parent's, the value a proven node backs up and the move a proven root plays.  Plain
// functions without tree types, for the host (m0_proof_combine) and for the kernels (tree_proof.h) alike.
#pragma once
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"      // M0_HD

namespace m0 {

// state and plies are from the view of the side to move at the node; the values are those of include/m0_proof.h
constexpr int PROOF_NONE = M0_PROOF_NONE, PROOF_WIN = M0_PROOF_WIN, PROOF_LOSS = M0_PROOF_LOSS, PROOF_DRAW = M0_PROOF_DRAW;
constexpr int PROOF_MAX_PLIES = 8191;                 // 13 bits beside the 2 of the state: the sign bit of the int16 stays clear

M0_HD int16_t proof_pack(int state, int plies) {
    if (state == PROOF_NONE) return 0;
    if (state == PROOF_DRAW || plies < 0) plies = 0;
    if (plies > PROOF_MAX_PLIES) plies = PROOF_MAX_PLIES;
    return (int16_t)(state | (plies << 2));
}
M0_HD int proof_state(int16_t p) { return p & 3; }
M0_HD int proof_plies(int16_t p) { return (p >> 2) & PROOF_MAX_PLIES; }

// What a proven node backs up: the value a table hit of that outcome backs up (leaf_terminal, tree_select.hip).
M0_HD double proof_value(int state, double draw_penalty) {
    return state == PROOF_WIN ? 1.0 : (state == PROOF_LOSS ? -1.0 : draw_penalty);
}

// A table's verdict for the side to move (tb_probe: wdl, distance to mate in plies) as a proof.
M0_HD int16_t proof_from_table(int wdl, int dtm) {
    return wdl > 0 ? proof_pack(PROOF_WIN, dtm) : (wdl < 0 ? proof_pack(PROOF_LOSS, dtm) : proof_pack(PROOF_DRAW, 0));
}

// The children of one parent, folded: any order, any grouping (the kernel folds one child per lane and merges across the wave).
struct ProofFold {
    int min_loss;        // smallest plies among the LOSS children, PROOF_MAX_PLIES + 1 without one
    int max_plies;       // largest plies among the proven children
    int any_draw;
    int all_proven;
};
M0_HD ProofFold proof_fold_empty() { return ProofFold{PROOF_MAX_PLIES + 1, 0, 0, 1}; }
M0_HD ProofFold proof_fold_child(ProofFold f, int16_t child) {
    const int s = proof_state(child), p = proof_plies(child);
    if (s == PROOF_NONE) { f.all_proven = 0; return f; }
    if (s == PROOF_LOSS && p < f.min_loss) f.min_loss = p;
    if (s == PROOF_DRAW) f.any_draw = 1;
    if (p > f.max_plies) f.max_plies = p;
    return f;
}
M0_HD ProofFold proof_fold_merge(ProofFold a, const ProofFold& b) {
    if (b.min_loss < a.min_loss) a.min_loss = b.min_loss;
    if (b.max_plies > a.max_plies) a.max_plies = b.max_plies;
    a.any_draw |= b.any_draw;
    a.all_proven &= b.all_proven;
    return a;
}
// The parent of the folded children.  `complete`: the children are all of the parent's legal moves.
//   1. a LOSS child: WIN in 1 + the smallest such child's plies;
//   2. else, complete and every child proven: DRAW with a DRAW child, else LOSS in 1 + the largest plies;
//   3. else not proven.
M0_HD int16_t proof_fold_result(const ProofFold& f, bool complete) {
    if (f.min_loss <= PROOF_MAX_PLIES) return proof_pack(PROOF_WIN, f.min_loss + 1);
    if (!complete || !f.all_proven) return 0;
    return f.any_draw ? proof_pack(PROOF_DRAW, 0) : proof_pack(PROOF_LOSS, f.max_plies + 1);
}

// Is child (state, plies, visits n, index i) a better move for a root of state `root` than the best so far (index bi < 0: none)?
//   WIN: the LOSS child with the fewest plies; LOSS: the child with the most plies; DRAW: the DRAW child with the most visits;
//   NONE: the most visited child that is not WIN for its own mover (`any_not_win`: there is one), else the most visited child.
// Ties go to the lowest index.
M0_HD bool proof_pick_eligible(int root, int16_t child, bool any_not_win) {
    const int s = proof_state(child);
    if (root == PROOF_WIN) return s == PROOF_LOSS;
    if (root == PROOF_DRAW) return s == PROOF_DRAW;
    if (root == PROOF_NONE) return !any_not_win || s != PROOF_WIN;
    return true;
}
// the key by which eligible children are ranked, larger is better
M0_HD int proof_pick_key(int root, int16_t child, int n) {
    if (root == PROOF_WIN) return -proof_plies(child);
    if (root == PROOF_LOSS) return proof_plies(child);
    return n;
}
M0_HD bool proof_pick_better(int key, int i, int bkey, int bi) { return bi < 0 || key > bkey || (key == bkey && i < bi); }

// The pick over k children, one after the other (the kernel: one child per lane, tree_proof.h); -1 for k <= 0.
inline int proof_pick(int root, int k, const int16_t* child, const int32_t* n) {
    bool any_not_win = false;
    for (int i = 0; i < k; ++i) any_not_win = any_not_win || proof_state(child[i]) != PROOF_WIN;
    int bi = -1, bkey = 0;
    for (int i = 0; i < k; ++i) {
        if (!proof_pick_eligible(root, child[i], any_not_win)) continue;
        const int key = proof_pick_key(root, child[i], n[i]);
        if (proof_pick_better(key, i, bkey, bi)) { bi = i; bkey = key; }
    }
    if (bi < 0)                       // (a proven root without the child that proves it: cannot happen) the most visited
        for (int i = 0; i < k; ++i) if (proof_pick_better(n[i], i, bkey, bi)) { bi = i; bkey = n[i]; }
    return bi;
}

}  // namespace m0
