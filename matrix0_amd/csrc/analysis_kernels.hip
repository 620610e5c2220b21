// Result kernels of the analysis engine (capi_analysis.hip), one wavefront each:
//   analysis_lines_kernel  (finished slot, line l): the root child of rank l by visits and the principal variation behind it.
//   policy_lines_kernel    (batch row): legal-softmax priors of a position that is not searched, the best of them by prior.
//   root_children_kernel   (finished slot): every root child's policy index and visits, for policy targets (keep_visits).
// A node's children are one contiguous block, child i = lane + 64 k (CPL per lane): ranks are counted per lane from values
// passed round the wave, the arg-max of a level is a wave reduction.  No atomics, no LDS.
#include "tree_device.h"

// Rank of each of this lane's values among the n values v (CPL per lane) under "larger first, ties by index": the number of
// values that come before it.  Whole-wave.
template <typename T>
__device__ __forceinline__ void rank_descending(const T (&v)[CPL], int n, int lane, int (&rank)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) rank[k] = 0;
#pragma unroll
    for (int k2 = 0; k2 < CPL; ++k2) {
        const int lim = n - 64 * k2 < 64 ? n - 64 * k2 : 64;          // source lanes that hold a value of this round
        for (int s = 0; s < lim; ++s) {
            const T o = __shfl(v[k2], s);
            const int oi = s + 64 * k2;
#pragma unroll
            for (int k = 0; k < CPL; ++k) rank[k] += (o > v[k] || (o == v[k] && oi < lane + 64 * k)) ? 1 : 0;
        }
    }
}

// The line's writer fills what the line does not use, so that a result is the same bytes whatever the buffer held before.
__device__ __forceinline__ void pad_pv(m0_analysis_line* L, int from) {
    for (int i = from; i < M0_AN_MAX_PV; ++i) L->pv[i] = 0;
}

// A root child's rank key in the proof search's ranking, larger first: a child that is LOSS for its own mover is a winning move
// (fewest plies first), one that is WIN a losing move (most plies first), the others go by visits in between.
__device__ __forceinline__ int proof_rank_key(int16_t child, int n) {
    const int s = proof_state(child);
    if (s == PROOF_LOSS) return (2 << 24) + (PROOF_MAX_PLIES - proof_plies(child));
    if (s == PROOF_WIN) return proof_plies(child);
    return (1 << 24) + (n < (1 << 24) - 1 ? n : (1 << 24) - 1);
}

// PROOF: the instantiation for engines that run the proof search (launch_analysis_lines with proof_dev); the other one is the
// kernel it was.
template <bool PROOF>
__global__ __launch_bounds__(64) void analysis_lines_kernel(TreeDev d, const int* slots, int multipv, int pv_len,
                                                            m0_analysis_line* lines, int* nlines, m0_proof_lines* proofs) {
    const int j = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
    const int g = slots[j];
    const GameDev* gd = &d.games[g];
    const Arena A = arena_of(d.t, g, gd->arena);
    const int root = gd->root;
    const int nc = A.nch[root] > 0 ? A.nch[root] : 0;
    const int cb = A.cbase[root];
    const int nl = multipv < nc ? multipv : nc;
    if (l == 0 && lane == 0) nlines[j] = nl;
    if constexpr (PROOF) {                                             // the root's proof, and NONE for the lines nobody writes
        m0_proof_lines* PL = proofs + j;
        if (l == 0 && lane == 0) { PL->proof = proof_state(A.proof[root]); PL->proof_plies = proof_plies(A.proof[root]); }
        if (l == 0 && lane >= multipv && lane < M0_AN_MAX_LINES) { PL->line_proof[lane] = 0; PL->line_proof_plies[lane] = 0; }
        if (l >= nl && lane == 0) { PL->line_proof[l] = 0; PL->line_proof_plies[l] = 0; }
    }
    if (l >= nl) return;                                               // lines beyond the root's children are not written
    int cn[CPL], rank[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        cn[k] = i < nc ? A.n[cb + i] : -1;
        if constexpr (PROOF) { if (i < nc) cn[k] = proof_rank_key(A.proof[cb + i], cn[k]); }
    }
    rank_descending(cn, nc, lane, rank);
    int mine = -1;                                                     // exactly one (lane, k) holds rank l
#pragma unroll
    for (int k = 0; k < CPL; ++k) if (lane + 64 * k < nc && rank[k] == l) mine = lane + 64 * k;
    const unsigned long long owner = __ballot(mine >= 0);
    const int ci = __shfl(mine, __builtin_ctzll(owner));
    int node = cb + ci;
    m0_analysis_line* L = lines + (size_t)j * M0_AN_MAX_LINES + l;
    if (lane == 0) {
        L->move = A.mv[node]; L->policy_index = A.midx[node]; L->visits = A.n[node];
        L->prior = (float)A.prior[node]; L->q = A.q[node];
        L->pv[0] = A.mv[node];
        if constexpr (PROOF) {                                         // the line's proof from the root mover's view
            const int16_t cp = A.proof[node];
            const int cs = proof_state(cp);
            proofs[j].line_proof[l] = cs == PROOF_LOSS ? PROOF_WIN : (cs == PROOF_WIN ? PROOF_LOSS : cs);
            proofs[j].line_proof_plies[l] = cs == PROOF_LOSS || cs == PROOF_WIN ? proof_plies(cp) + 1 : 0;
        }
    }
    // the most visited line from there: one round of dependent loads per level (the scan of a node's children also fetches
    // each child's own child block, the winner's is passed round)
    int len = 1;
    int nch = A.nch[node], cbn = A.cbase[node];
    int ns = PROOF_NONE;                                               // proof search: the state of the node the line stands at
    if constexpr (PROOF) ns = proof_state(A.proof[node]);
    while (len < pv_len && nch > 0) {
        int bn = -1, bi = -1, b_nch = -1, b_cb = -1;
        Move b_mv = 0;
        for (int i = lane; i < nch; i += 64) {
            const int c = cbn + i;
            int n = A.n[c];
            const int c_nch = A.nch[c], c_cb = A.cbase[c];
            const Move m = A.mv[c];
            if constexpr (PROOF) {                                     // at a proven node: the move the proof search picks there
                if (ns != PROOF_NONE) {
                    const int16_t cp = A.proof[c];
                    if (!proof_pick_eligible(ns, cp, true)) continue;
                    n = (1 << 20) + proof_pick_key(ns, cp, n < (1 << 19) ? n : (1 << 19));     // above 0: `wn <= 0` is for visits
                }
            }
            if (n > bn) { bn = n; bi = i; b_nch = c_nch; b_cb = c_cb; b_mv = m; }
        }
        int wn = bn, wi = bi;
        for (int off = 32; off > 0; off >>= 1) {
            const int on = __shfl_xor(wn, off), oi = __shfl_xor(wi, off);
            if (oi >= 0 && (wi < 0 || on > wn || (on == wn && oi < wi))) { wn = on; wi = oi; }
        }
        if (wn <= 0) break;                                            // no child was visited
        const int wl = wi & 63;                                        // the lane that scanned child wi holds it as its best
        const Move m = (Move)__shfl((int)b_mv, wl);
        if constexpr (PROOF) ns = proof_state(A.proof[cbn + wi]);
        nch = __shfl(b_nch, wl); cbn = __shfl(b_cb, wl);
        if (lane == 0) L->pv[len] = m;
        ++len;
    }
    if (lane == 0) { L->pv_len = len; pad_pv(L, len); }
}

hipError_t launch_analysis_lines(const TreeDev& d, const int* slots_dev, int count, int multipv, int pv_len,
                                 m0_analysis_line* lines_dev, int* nlines_dev, hipStream_t st, m0_proof_lines* proof_dev) {
    if (count <= 0) return hipSuccess;
    if (proof_dev && !d.t.proof) return hipErrorInvalidValue;
    if (proof_dev) hipLaunchKernelGGL(analysis_lines_kernel<true>, dim3(count, multipv), dim3(64), 0, st, d, slots_dev, multipv, pv_len,
                                      lines_dev, nlines_dev, proof_dev);
    else hipLaunchKernelGGL(analysis_lines_kernel<false>, dim3(count, multipv), dim3(64), 0, st, d, slots_dev, multipv, pv_len, lines_dev,
                            nlines_dev, proof_dev);
    return hipGetLastError();
}

// A finished search already holds its root children on the device in the slot's RootResult (expand_kernel writes it with
// the `finished` flag): the two columns a policy target needs, compact, one entry per finished slot.
__global__ __launch_bounds__(64) void root_children_kernel(TreeDev d, const int* slots, int32_t* policy_idx, int32_t* visits,
                                                           int32_t* nchild) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const RootResult* R = d.results + slots[j];
    int k = R->nchild;
    k = k < 0 ? 0 : (k > M0_MAX_CHILDREN ? M0_MAX_CHILDREN : k);
    for (int i = lane; i < M0_MAX_CHILDREN; i += 64) {
        policy_idx[(size_t)j * M0_MAX_CHILDREN + i] = i < k ? (int32_t)R->child_idx[i] : 0;
        visits[(size_t)j * M0_MAX_CHILDREN + i] = i < k ? R->child_n[i] : 0;
    }
    if (lane == 0) nchild[j] = k;
}

hipError_t launch_root_children(const TreeDev& d, const int* slots_dev, int count, int32_t* policy_idx_dev, int32_t* visits_dev,
                                int32_t* nchild_dev, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(root_children_kernel, dim3(count), dim3(64), 0, st, d, slots_dev, policy_idx_dev, visits_dev, nchild_dev);
    return hipGetLastError();
}

// logits [rows][M0_POLICY_SIZE] and values [rows] of the network; nlegal / moves / idx as launch_encode_positions wrote them.
// Priors as the expansion's legal softmax computes them (wave_softmax; uniform when the row holds a non-finite logit,
// mcts.py:147-149), before its entropy noise and renormalisation: what the network says, not what a search would start from.
__global__ __launch_bounds__(64) void policy_lines_kernel(const float* logits, const float* values, const int32_t* nlegal,
                                                          const uint16_t* moves, const int32_t* idx, int rows, int multipv,
                                                          m0_analysis_line* lines, int* nlines, float* value_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= rows) return;
    int n = nlegal[r];
    n = n < 0 ? 0 : (n > M0_MAX_CHILDREN ? M0_MAX_CHILDREN : n);
    const int nl = multipv < n ? multipv : n;
    if (lane == 0) { nlines[r] = nl; value_out[r] = values[r]; }
    if (n == 0) return;
    const float* lg = logits + (size_t)r * M0_POLICY_SIZE;
    const bool bad = __any(row_nonfinite(lg, lane));
    float l[CPL], pr[CPL];
    int id[CPL];
    Move mv[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        id[k] = 0; mv[k] = 0; l[k] = -3.0e38f;
        if (i < n) {
            mv[k] = moves[(size_t)r * M0_MAX_MOVES + i];
            id[k] = idx[(size_t)r * M0_MAX_MOVES + i];
            if ((unsigned)id[k] < (unsigned)M0_POLICY_SIZE) l[k] = lg[id[k]];
        }
    }
    if (bad) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) pr[k] = 1.0f / (float)n;
    } else wave_softmax(l, n, lane, pr);
#pragma unroll
    for (int k = 0; k < CPL; ++k) if (lane + 64 * k >= n) pr[k] = -1.f;
    int rank[CPL];
    rank_descending(pr, n, lane, rank);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        if (lane + 64 * k < n && rank[k] < nl) {                       // the lanes that hold the best write their own lines
            m0_analysis_line* L = lines + (size_t)r * M0_AN_MAX_LINES + rank[k];
            L->move = mv[k]; L->policy_index = id[k]; L->visits = 0; L->prior = pr[k]; L->q = 0.0;
            L->pv_len = 1; L->pv[0] = mv[k];
            pad_pv(L, 1);
        }
    }
}

hipError_t launch_policy_lines(const float* logits_dev, const float* values_dev, const int32_t* nlegal_dev, const uint16_t* moves_dev,
                               const int32_t* idx_dev, int rows, int multipv, m0_analysis_line* lines_dev, int* nlines_dev,
                               float* value_out_dev, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(policy_lines_kernel, dim3(rows), dim3(64), 0, st, logits_dev, values_dev, nlegal_dev, moves_dev, idx_dev, rows,
                       multipv, lines_dev, nlines_dev, value_out_dev);
    return hipGetLastError();
}
