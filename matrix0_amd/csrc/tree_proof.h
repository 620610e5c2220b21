// Proof search on the device (include/m0_proof.h; the arithmetic is proof_core.h): what select_kernel's proof instantiation
// does beside the PUCT search -- the proof of a terminal leaf, the combine up its path -- and the ProofResult that expand_kernel
// writes when a search finishes.  Whole-wave functions, one wavefront per game tree.
#pragma once
#include "tree_device.h"
#include "tb_core.h"

// The proof a terminal leaf carries, in the order of leaf_terminal's tests (tree_select.hip), which found `pos` terminal:
// checkmate LOSS 0; stalemate, insufficient material and the 75-move rule DRAW; a table hit the table's verdict and distance.
// What is left is fivefold repetition, which depends on the path: no proof.
__device__ __forceinline__ int16_t leaf_proof(const TreeDev& d, const Pos& pos, int nlegal, bool tb_hit) {
    if (nlegal == 0) return in_check(pos) ? proof_pack(PROOF_LOSS, 0) : proof_pack(PROOF_DRAW, 0);
    if (is_insufficient(pos) || pos.halfmove >= 150) return proof_pack(PROOF_DRAW, 0);
    if (tb_hit) {
        int wdl, dtm;
        if (tb_probe(*d.tb_set, pos, d.tb_max_pieces, wdl, dtm)) return proof_from_table(wdl, dtm);
    }
    return 0;
}

__device__ __forceinline__ ProofFold proof_fold_wave(ProofFold f) {
    for (int o = 32; o > 0; o >>= 1) {
        ProofFold g;
        g.min_loss = __shfl_xor(f.min_loss, o); g.max_plies = __shfl_xor(f.max_plies, o);
        g.any_draw = __shfl_xor(f.any_draw, o); g.all_proven = __shfl_xor(f.all_proven, o);
        f = proof_fold_merge(f, g);
    }
    return f;
}

// Node path[depth] has just been given the proof `pv`: its parent is re-examined, then the parent's parent, while a state
// changes.  A parent's children are one block: one child per lane, 64 at a time (up to M0_MAX_CHILDREN), a wave reduction of
// the fold.  `read(i)`: the proof of node i as the caller holds it; `write(i, p)`: node i is proven (called by every lane; the
// caller stores it once).  The child that has just changed is taken from the register, not read back.  The nodes of the path
// above the leaf are unproven (a descent stops at a proven node), so a result other than NONE is a change.
template <typename Read, typename Write>
__device__ __forceinline__ void proof_combine_up(const Arena& A, const int* path, int depth, int16_t pv, bool complete, int lane,
                                                 const Read& read, const Write& write) {
    int changed = path[depth];
    for (int dd = depth - 1; dd >= 0 && pv != 0; --dd) {
        const int P = path[dd];
        const int nc = A.nch[P], cb = A.cbase[P];
        ProofFold f = proof_fold_empty();
        for (int i0 = 0; i0 < nc; i0 += 64) {
            const int ci = cb + i0 + lane;
            if (i0 + lane < nc) f = proof_fold_child(f, ci == changed ? pv : read(ci));
        }
        pv = proof_fold_result(proof_fold_wave(f), complete);
        if (pv != 0) write(P, pv);
        changed = P;
    }
}

// The finished search's ProofResult: the root's state, every root child's, and the move (proof_core.h, proof_pick).
__device__ __forceinline__ void write_proof_result(const TreeDev& d, const Arena& A, int g, int root, int lane) {
    ProofResult* R = d.proof_results + g;
    const int k = A.nch[root] > 0 ? A.nch[root] : 0;
    const int cb = A.cbase[root];
    const int16_t rp = A.proof[root];
    const int rs = proof_state(rp);
    bool notwin = false;
    for (int i = lane; i < k; i += 64) {
        const int16_t cp = A.proof[cb + i];
        R->child[i] = cp;
        notwin = notwin || proof_state(cp) != PROOF_WIN;
    }
    const bool any_not_win = __any(notwin);
    int bi = -1, bkey = 0;
    for (int pass = 0; pass < 2 && bi < 0; ++pass) {      // pass 1: no eligible child (cannot happen) -- the most visited
        for (int i = lane; i < k; i += 64) {
            const int16_t cp = A.proof[cb + i];
            const int n = A.n[cb + i];
            if (pass == 0 && !proof_pick_eligible(rs, cp, any_not_win)) continue;
            const int key = pass == 0 ? proof_pick_key(rs, cp, n) : n;
            if (proof_pick_better(key, i, bkey, bi)) { bi = i; bkey = key; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int oi = __shfl_xor(bi, o), okey = __shfl_xor(bkey, o);
            if (oi >= 0 && proof_pick_better(okey, oi, bkey, bi)) { bi = oi; bkey = okey; }
        }
    }
    if (lane == 0) { R->state = rs; R->plies = proof_plies(rp); R->pick = bi; }
}
