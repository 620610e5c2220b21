// expand_kernel: after the network, one wavefront per game: policy indices, legal-only softmax, entropy noise, renormalise
// (mcts.py:135-225), pruning, child block allocation, backup (mcts.py:946-953), evaluation-cache fill, virtual-loss
// release, root result extraction.  The legal moves of every leaf come from select_kernel (TreeDev::leaf_moves).
#include "tree_device.h"
#include "tree_gumbel.h"
#include "tree_proof.h"
#include "eval_cache.h"

struct ExpandScratch {          // workgroup-shared staging of one expansion (raw priors / pruning only)
    float pr[M0_MAX_CHILDREN];
    uint8_t keep[M0_MAX_CHILDREN];
    float total;
    int bad;                    // the logits of the last expansion held a non-finite value (not cached)
};

// What every expansion of one game shares, built once per kernel.
struct ExpandEnv {
    Arena A;
    int cap;                    // nodes per arena half
    GameDev* gd;
    uint64_t* TK; int* TN; int tt_cap;   // tt_merge: the game's position table, else TK == nullptr
    ExpandScratch* X;
    int lane;
};
// Where the logits of one leaf come from and whether they are kept.
struct LeafLogits {
    const float* row;           // the network's M0_POLICY_SIZE logits of the leaf's batch row, or null:
    const float* legal;         // the legal moves' logits from the evaluation cache, in move order
    float* store;               // evaluation-cache payload to fill with the legal moves' logits, or null
};
__device__ __forceinline__ LeafLogits logits_of_row(const float* row, float* store) { return LeafLogits{row, nullptr, store}; }
// (row is null: the cache is only used with legal_softmax on and raw_legal_priors off, the two paths that never read it)
__device__ __forceinline__ LeafLogits logits_of_cache(const float* payload) { return LeafLogits{nullptr, payload + EC_LOGITS, nullptr}; }

// numpy float32 add.reduce over a[0..n): pairwise with an 8-way unrolled base case (blocks of <= 128), n <= 256
static __device__ float np_sum_f32_dev(const float* a, int n) {
    auto block = [&](const float* b, int m) -> float {
        if (m < 8) { float r = 0.f; for (int i = 0; i < m; ++i) r += b[i]; return r; }
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = b[j];
        int i;
        for (i = 8; i < m - (m % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += b[i + j];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < m; ++i) res += b[i];
        return res;
    };
    if (n <= 128) return block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return block(a, n2) + block(a + n2, n - n2);
}

// Node._expand_with_legal_priors (mcts.py:227-256), the reference's in-process-model branch (mcts.py:697-703):
// priors = legal logits / their float32 sum (numpy pairwise order), uniform when the sum is <= 0 or not finite;
// no softmax, no entropy noise, and only the LEGAL logits are looked at
__device__ __forceinline__ void priors_raw(const float* lg, const int (&idx)[CPL], int n, int lane, ExpandScratch* X, float (&pr)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const int i = lane + 64 * k; if (i < n) X->pr[i] = lg[idx[k]]; }
    __syncthreads();
    if (lane == 0) X->total = np_sum_f32_dev(X->pr, n);
    __syncthreads();
    const float total = X->total;
    const bool ok = isfinite(total) && total > 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const int i = lane + 64 * k; pr[k] = i < n ? (ok ? X->pr[i] / total : 1.0f / (float)n) : 0.f; }
    __syncthreads();
}

__device__ __forceinline__ void priors_uniform(int n, float (&pr)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) pr[k] = 1.0f / (float)n;
}

// Softmax numerics: wave_softmax (tree_device.h); entropy in float64.
// Softmax over the legal moves only, entropy noise when the distribution is flat; the logits also go to src.store.
__device__ __forceinline__ void priors_legal_softmax(const LeafLogits& src, const int (&idx)[CPL], int n, int lane, GameDev* gd,
                                                     const TreeCfg& c, float (&pr)[CPL]) {
    double ent = 0.0;
    float l[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        l[k] = i < n ? (src.legal ? src.legal[i] : src.row[idx[k]]) : -3.0e38f;
        if (src.store && i < n && i < M0_EC_MAXLEGAL) src.store[EC_LOGITS + i] = l[k];
    }
    wave_softmax(l, n, lane, pr);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        if (i < n) ent -= (double)pr[k] * log((double)pr[k] + 1e-8);
    }
    ent = wave_sum_d(ent);
    const double ratio = ent / fmax(1e-9, log((double)(n > 1 ? n : 1)));
    if (c.enable_entropy_noise && ratio > 0.9) {
        const uint64_t ctr = gd->ctr_noise;
        const uint64_t seed = gd->seed_noise;
        double dd[CPL], ds = 0.0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int i = lane + 64 * k;
            dd[k] = 0.0;
            if (i < n) { dd[k] = fmax((double)pr[k] + 0.1 * normal_at(seed, ctr + 2ull * (uint64_t)i), 1e-8); ds += dd[k]; }
        }
        ds = wave_sum_d(ds);
#pragma unroll
        for (int k = 0; k < CPL; ++k) pr[k] = (float)(dd[k] / ds);
        if (lane == 0) gd->ctr_noise = ctr + 2ull * (uint64_t)n;
    }
}

// Softmax over all M0_POLICY_SIZE logits (legal_softmax == 0), the legal moves' share kept; entropy and noise over the full row.
__device__ __forceinline__ void priors_full_softmax(const float* lg, const int (&idx)[CPL], int n, int lane, GameDev* gd,
                                                    const TreeCfg& c, float (&pr)[CPL]) {
    float mx = -3.0e38f;
    double ent = 0.0;
    for (int j = lane; j < M0_POLICY_SIZE; j += 64) mx = fmaxf(mx, lg[j]);
    mx = wave_max_f(mx);
    double sum = 0.0;
    for (int j = lane; j < M0_POLICY_SIZE; j += 64) sum += exp((double)(lg[j] - mx));
    sum = wave_sum_d(sum);
    const double fsum = sum;
    for (int j = lane; j < M0_POLICY_SIZE; j += 64) {
        const double pj = (double)(float)(exp((double)(lg[j] - mx)) / sum);
        ent -= pj * log(pj + 1e-8);
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const int i = lane + 64 * k; pr[k] = i < n ? (float)(exp((double)(lg[idx[k]] - mx)) / sum) : 0.f; }
    ent = wave_sum_d(ent);
    const double ratio = ent / fmax(1e-9, log((double)(n > 1 ? n : 1)));
    if (c.enable_entropy_noise && ratio > 0.9) {
        const uint64_t ctr = gd->ctr_noise;
        const uint64_t seed = gd->seed_noise;
        double ds = 0.0;
        for (int j = lane; j < M0_POLICY_SIZE; j += 64)
            ds += fmax((double)(float)(exp((double)(lg[j] - mx)) / fsum) + 0.1 * normal_at(seed, ctr + 2ull * (uint64_t)j), 1e-8);
        ds = wave_sum_d(ds);
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int i = lane + 64 * k;
            if (i < n) {
                const int j = idx[k];
                pr[k] = (float)(fmax((double)pr[k] + 0.1 * normal_at(seed, ctr + 2ull * (uint64_t)j), 1e-8) / ds);
            }
        }
        if (lane == 0) gd->ctr_noise = ctr + 2ull * (uint64_t)M0_POLICY_SIZE;
    }
}

// renormalise over the legal moves (mcts.py:205-212): float32 values, float64 sum rounded to float32
__device__ __forceinline__ void priors_renormalise(int n, int lane, float (&pr)[CPL]) {
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const int i = lane + 64 * k; if (i < n) { if (!(pr[k] >= 0.f) || !isfinite(pr[k])) pr[k] = 0.f; tot += (double)pr[k]; } }
    tot = wave_sum_d(tot);
    const float totf = (float)tot;
    if (totf > 0.f && isfinite(totf)) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) pr[k] = pr[k] / totf;
    } else priors_uniform(n, pr);
}

// MCTS._prune_children (mcts.py:806-826): drop children below min_child_prior, then keep the max_children largest
// priors (Python's stable sort: ties stay in move order; the kept children are then IN sorted order); priors are
// not renormalised.  slot[k] = slot of this lane's k-th child in the node's child block, -1 = dropped; returns the block size.
__device__ __forceinline__ int prune_children(const TreeCfg& c, const float (&pr)[CPL], int n, int lane, ExpandScratch* X, int (&slot)[CPL]) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) slot[k] = lane + 64 * k;
    if (!(c.max_children > 0 || c.min_child_prior > 0.0)) return n;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        if (i < n) { X->pr[i] = pr[k]; X->keep[i] = (c.min_child_prior > 0.0 && !((double)pr[k] >= c.min_child_prior)) ? 0 : 1; }
    }
    __syncthreads();
    int kept = 0;
    for (int j = 0; j < n; ++j) kept += X->keep[j];
    const bool topk = c.max_children > 0 && kept > c.max_children;
    const int nkeep = topk ? c.max_children : kept;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        slot[k] = -1;
        if (i < n && X->keep[i]) {
            int r = 0;
            if (topk) { for (int j = 0; j < n; ++j) r += (X->keep[j] && (X->pr[j] > pr[k] || (X->pr[j] == pr[k] && j < i))) ? 1 : 0; }
            else { for (int j = 0; j < i; ++j) r += X->keep[j]; }
            if (r < nkeep) slot[k] = r;
        }
    }
    __syncthreads();
    return nkeep;
}

// The child block of `leaf`; false (and GameDev::overflow) if the arena half cannot take it.  q0: the q a new child starts
// with (child_seed_q).
// _register_children_in_tt (mcts.py:1330-1346): every child of an expanded NON-root node goes into the table
// under the key of the position it leads to (run() registers only the fresh root itself, mcts.py:344-358)
// A root that run() FOUND in the table and had to expand registers its children like any other node
// (mcts.py:398-413): reg_children is false only for the brand-new root, which is registered itself instead.
__device__ __forceinline__ bool write_children(const ExpandEnv& E, int leaf, const Pos& pos, const Move (&mvv)[CPL], const int (&idx)[CPL],
                                               const float (&pr)[CPL], const int (&slot)[CPL], int n, int nkeep, bool reg_children,
                                               double q0) {
    const Arena& A = E.A;
    GameDev* gd = E.gd;
    const int lane = E.lane;
    const int cb = gd->next;
    if (cb + nkeep > E.cap) { if (lane == 0) gd->overflow = 1; return false; }
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        if (i < n && slot[k] >= 0) {
            const int ci = cb + slot[k];
            node_reset(A, ci, (double)pr[k], mvv[k], (uint16_t)idx[k]);
            if (q0 != 0.0) A.q[ci] = q0;
            if (E.TK && reg_children) {
                Pos q = pos;
                make_move(q, mvv[k]);
                tt_insert(E.TK, E.TN, E.tt_cap, tt_key_of(q), ci);
            }
        }
    }
    if (E.TK && !reg_children && lane == 0) tt_insert(E.TK, E.TN, E.tt_cap, tt_key_of(pos), leaf);
    if (lane == 0) { A.cbase[leaf] = cb; A.nch[leaf] = (int16_t)nkeep; gd->next = cb + nkeep; }
    __syncthreads();
    return true;
}

// Node._expand gives a new child q = -parent.q, the q of the PARENT OF THE EXPANDED NODE as it stands then, unless that is 0 or
// the node has no parent (mcts.py:221-222).  No search reads it -- a child without visits is scored with the FPU value, the first
// backup overwrites it -- but it is the q such a child reports (a line without visits, a root child of a kept subtree).  The
// parent is the node before the leaf on the sample's path; the root has none.  The table modes keep 0: there the node's
// creation parent need not be on the path.
__device__ __forceinline__ double child_seed_q(const TreeCfg& c, const Arena& A, const int* path, int depth) {
    if (c.tt_merge || depth < 1) return 0.0;
    const double pq = A.q[path[depth - 1]];
    return pq != 0.0 ? -pq : 0.0;
}

// Node._expand (mcts.py:135-225) for one leaf: priors -> prune -> child block; returns false if the arena is exhausted.
// The legal moves of the leaf come from select (same position, same order): no second move generation.
__device__ __forceinline__ bool expand_node(const ExpandEnv& E, const TreeCfg& c, int leaf, const Pos& pos, const uint16_t* smoves, int n,
                                   const LeafLogits& src, bool is_root, bool reg_children, double q0) {
    const int lane = E.lane;
    if (n <= 0) return true;
    // non-finite logits anywhere -> uniform priors (mcts.py:147-149)
    bool bad = false;
    if (!src.legal) bad = row_nonfinite(src.row, lane);
    bad = __any(bad);
    if (lane == 0) E.X->bad = bad ? 1 : 0;
    float pr[CPL];
    int idx[CPL];
    Move mvv[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int i = lane + 64 * k;
        pr[k] = 0.f; idx[k] = 0; mvv[k] = 0;
        if (i < n) { mvv[k] = smoves[i]; idx[k] = move_to_index(pos, mvv[k]); }
    }
    if (c.raw_legal_priors && c.legal_softmax && !is_root) priors_raw(src.row, idx, n, lane, E.X, pr);
    else if (bad) priors_uniform(n, pr);
    else {
        if (c.legal_softmax) priors_legal_softmax(src, idx, n, lane, E.gd, c, pr);
        else priors_full_softmax(src.row, idx, n, lane, E.gd, c, pr);
        priors_renormalise(n, lane, pr);
    }
    int slot[CPL];
    const int nkeep = prune_children(c, pr, n, lane, E.X, slot);
    return write_children(E, leaf, pos, mvv, idx, pr, slot, n, nkeep, reg_children, q0);
}

// A leaf with a batch row of its own (SK_EVAL, or the unexpanded root SK_ROOT_INIT): expand it from the row's logits; a cacheable
// leaf (SK_EVAL with a key set by select) also puts its evaluation into the cache.  False: the node arena refused the child block.
__device__ __forceinline__ bool expand_evaluated(const TreeDev& d, const TreeCfg& c, const ExpandEnv& E, int g, const Sample& smp,
                                                 const uint16_t* moves, const float* lg, float v, double q0) {
    const Arena& A = E.A;
    GameDev* gd = E.gd;
    const int lane = E.lane, kind = smp.kind, leaf = smp.leaf;
    const Pos pos = smp.pos;
    float* cw = nullptr;
    size_t ce = 0;
    const uint64_t ckey = kind == SK_EVAL ? smp.ckey : 0ull;
    if (ckey != 0 && isfinite(v)) {
        ce = ec_choose_victim(d.ec, gd, g, ckey, lane);
        cw = ec_payload(d.ec, ce);
        ec_invalidate(d.ec, ce, lane);                  // invalid while it is being rewritten
    }
    const bool ok = expand_node(E, c, leaf, pos, moves, smp.nlegal, logits_of_row(lg, cw), kind == SK_ROOT_INIT,
                                !(kind == SK_ROOT_INIT && gd->root_fresh), q0);
    // an expansion that did not happen (node arena exhausted) must not leave the pending-row mark behind
    if (c.eval_cache && kind == SK_EVAL && lane == 0 && A.nch[leaf] < 0) A.cbase[leaf] = -1;
    const int sig = cw ? legal_sig(moves, smp.nlegal, lane) : 0;
    if (cw && lane == 0) {
        if (ok && !E.X->bad) ec_publish(d.ec, gd, ce, ckey, v, sig);
    }
    return ok;
}

// An SK_SHARED sample whose leaf is still unexpanded: the expansion from its row was refused earlier in this pass (node arena
// full).  Without the evaluation cache this sample would have been an SK_EVAL of its own and would have tried again, drawing
// entropy noise again; the games are the same with the cache on and off only if it tries again here, from the same row.  Its
// legal moves are those of the sample that owns the row (select stores them once).
__device__ __forceinline__ bool retry_refused_shared(const TreeCfg& c, const ExpandEnv& E, const Sample* S, int s, const uint16_t* LM,
                                                     const float* logits, const int* path) {
    const int leaf = S[s].leaf, row = S[s].row;
    int s0 = 0;
    while (s0 < s && !(S[s0].kind == SK_EVAL && S[s0].row == row)) ++s0;
    if (s0 >= s) return true;                       // (cannot happen: a pending row has an owner before every sharer)
    const Pos pos = S[s].pos;
    return expand_node(E, c, leaf, pos, LM + (size_t)s0 * M0_MAX_CHILDREN, S[s].nlegal,
                       logits_of_row(logits + (size_t)row * M0_POLICY_SIZE, nullptr), false, true,
                       child_seed_q(c, E.A, path, S[s].depth));
}

// release virtual losses of the whole batch (the reference's inflight dict dies with the batch)
// (integer atomics: one lane per sample, any order gives the same counts)
__device__ __forceinline__ void release_inflight(const TreeDev& d, const TreeCfg& c, const Arena& A, int g, const Sample* S, const int* P,
                                                 int ns, int lane) {
    for (int s = lane; s < ns; s += 64) {
        if (sample_holds_inflight(S[s].kind)) {
            // the in-flight counts sit on the EDGE children (tt_merge: the walk itself may have continued elsewhere)
            const int* path = (c.tt_merge ? d.epaths + (size_t)g * (d.L + 1) * M0_MAX_DEPTH : P) + (size_t)s * M0_MAX_DEPTH;
            for (int dd = 1; dd <= S[s].depth; ++dd) atomicSub(&A.vl[path[dd]], 1);
        }
    }
}

__device__ __forceinline__ void write_root_result(RootResult* R, const Arena& A, int root, int lane) {
    const int k = A.nch[root] > 0 ? A.nch[root] : 0;
    const int cb = A.cbase[root];
    for (int i = lane; i < k; i += 64) {
        R->child_node[i] = cb + i; R->child_n[i] = A.n[cb + i];
        R->child_mv[i] = A.mv[cb + i]; R->child_idx[i] = A.midx[cb + i];
        R->child_prior[i] = A.prior[cb + i]; R->child_q[i] = A.q[cb + i];
    }
    if (lane == 0) { R->nchild = k; R->root_n = A.n[root]; R->root_q = A.q[root]; }
}

__global__ __launch_bounds__(64) void expand_kernel(TreeDev d, TreeCfg c) {
    __shared__ ExpandScratch X;
    const int g = blockIdx.x, lane = threadIdx.x;
    GameDev* gd = &d.games[g];
    if (!gd->active) return;
    uint64_t* TK = c.tt_merge ? d.tt_keys + tt_table_of(d, g, gd) : nullptr;
    int* TN = c.tt_merge ? d.tt_nodes + tt_table_of(d, g, gd) : nullptr;
    const uint16_t* LM = d.leaf_moves + (size_t)g * (d.L + 1) * M0_MAX_CHILDREN;
    const int ns = gd->nsamples;
    const Arena A = arena_of(d.t, g, gd->arena);
    // proof search: a search whose root is proven has finished, whatever is left of its budget -- also one that select_kernel
    // gave no sample because its root was proven when it started (the subtree it took over)
    const bool proven = is_proof(c) && A.proof[gd->root] != 0;
    if (ns <= 0 && !(proven && !gd->finished)) return;
    const ExpandEnv E{A, d.t.cap, gd, TK, TN, d.tt_cap, &X, lane};
    const Sample* S = d.samples + (size_t)g * (d.L + 1);
    const int* P = d.paths + (size_t)g * (d.L + 1) * M0_MAX_DEPTH;
    const bool may_repeat = c.tt_merge != 0;
    int sims = 0;
    uint64_t evals = 0, hits = 0;
    bool refused = false;                        // the arena refused an expansion of this pass (wave-uniform)
    for (int s = 0; s < ns; ++s) {
        const int kind = S[s].kind;
        const int* path = P + (size_t)s * M0_MAX_DEPTH;
        const uint16_t* moves = LM + (size_t)s * M0_MAX_CHILDREN;
        if (kind == SK_SHARED) {                 // its row's value, no second expansion ...
            const float v = d.values[S[s].row];
            if (refused) {                       // ... unless the first was refused: see retry_refused_shared
                // lane 0's stores of this launch (nch of a leaf that did get its block) before the wave reads them back
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
                if (A.nch[S[s].leaf] < 0) retry_refused_shared(c, E, S, s, LM, d.logits, path);
            }
            backprop(A, path, S[s].depth, (double)v, lane, may_repeat, NoMirror{});
            ++sims; ++hits;
            __syncthreads();
        } else if (kind == SK_CACHED) {          // expand from the staged payload
            const int leaf = S[s].leaf, depth = S[s].depth;
            const float* pay = ec_hit_stage(d, g, s);
            const float v = pay[EC_VALUE];
            if (A.nch[leaf] < 0) {
                const Pos pos = S[s].pos;
                refused |= !expand_node(E, c, leaf, pos, moves, S[s].nlegal, logits_of_cache(pay), false, true,
                                        child_seed_q(c, A, path, depth));
            }
            backprop(A, path, depth, (double)v, lane, may_repeat, NoMirror{});
            ++sims; ++hits;
            __syncthreads();
        } else if (kind == SK_EVAL || kind == SK_ROOT_INIT) {
            const int leaf = S[s].leaf, depth = S[s].depth, row = S[s].row;
            const float* lg = d.logits + (size_t)row * M0_POLICY_SIZE;
            const float v = d.values[row];
            if (A.nch[leaf] < 0) refused |= !expand_evaluated(d, c, E, g, S[s], moves, lg, v, child_seed_q(c, A, path, depth));
            ++evals;
            if (kind == SK_EVAL) {
                backprop(A, path, depth, (double)v, lane, may_repeat, NoMirror{});
                ++sims;
            } else {
                const double rv = root_value(gd, v);
                if (lane == 0) {
                    gd->root_v = rv;
                    if (gd->root_q_from_v) { A.q[leaf] = rv; gd->root_q_from_v = 0; }
                }
            }
            __syncthreads();
        } else if (kind == SK_TERMINAL) {
            ++sims;
        } else if (kind == SK_ROOT_VALUE) {       // value of a reused root (mcts.py:359-371); v is read only if root.n == 0
            const double rv = root_value(gd, d.values[S[s].row]);
            if (lane == 0) gd->root_v = rv;
            ++evals;
        }
    }
    if (c.virtual_loss_active) release_inflight(d, c, A, g, S, P, ns, lane);
    __syncthreads();
    const int done = gd->sims_done + sims;
    const int root = gd->root;
    const bool fin = ((A.nch[root] >= 0 || gd->overflow) && done >= gd->sims_target) || proven;
    if (lane == 0) {
        gd->sims_done = done;
        gd->evals += evals;
        gd->cache_hits += hits;
        gd->finished = fin ? 1 : 0;
        gd->root_n = A.n[root];
        gd->root_q = A.q[root];
    }
    if (fin) write_root_result(d.results + g, A, root, lane);
    if (fin && is_gumbel(c)) write_gumbel_result(d, c, A, gd, g, root, lane);   // beside it: the move and the improved policy
    if (fin && is_proof(c)) write_proof_result(d, A, g, root, lane);            // ... or what the search proved, and the move
}

hipError_t launch_expand(const TreeDev& d, const TreeCfg& c, hipStream_t st) {
    hipLaunchKernelGGL(expand_kernel, dim3(d.G), dim3(64), 0, st, d, c);
    return hipGetLastError();
}
