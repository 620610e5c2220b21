// Device code shared by the tree kernels (tree_select.hip, tree_expand.hip, tree_advance.hip, tree_reroot.hip): the counter
// RNG, the arena view of one game's node arrays, node reset / copy, wave reductions, the backup, the position table of the
// tt_merge mode, batch-row reservation, the root value and the two ways a slot gets a new root (fresh, kept subtree).  For the tree .hip units only (it opens namespace m0).  One wavefront per game
// tree: "whole-wave" functions are called by all 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "tree.h"

using namespace m0;

#define GOLDEN64 0x9E3779B97F4A7C15ull

__device__ __forceinline__ double u01(uint64_t seed, uint64_t k) {
    return (double)(mix64(seed + (k + 1) * GOLDEN64) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double normal_at(uint64_t seed, uint64_t k) {   // consumes uniforms k, k+1
    double u1 = u01(seed, k), u2 = u01(seed, k + 1);
    if (u1 < 1e-300) u1 = 1e-300;
    return sqrt(-2.0 * log(u1)) * cos(2.0 * 3.141592653589793 * u2);
}
static __device__ double gamma_draw(uint64_t seed, uint64_t& ctr, double a) {     // Marsaglia-Tsang
    double boost = 1.0;
    if (a < 1.0) {
        double u = u01(seed, ctr++);
        boost = pow(u, 1.0 / a);
        a += 1.0;
    }
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int it = 0; it < 1000; ++it) {
        double x = normal_at(seed, ctr); ctr += 2;
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        double u = u01(seed, ctr++);
        if (u < 1e-300) u = 1e-300;
        if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) return d * v * boost;
    }
    return d * boost;
}

struct Arena {
    double* prior; double* w; double* q; int* n; int* vl; int* cbase; int16_t* nch; uint16_t* mv; uint16_t* midx;
    int16_t* proof;           // null unless the engine runs the proof search (TreeArrays::proof)
};
__device__ __forceinline__ Arena arena_of(const TreeArrays& t, int g, int half) {
    size_t b = ((size_t)g * 2 + half) * (size_t)t.cap;
    Arena a;
    a.prior = t.prior + b; a.w = t.w + b; a.q = t.q + b; a.n = t.n + b; a.vl = t.vl + b;
    a.cbase = t.cbase + b; a.nch = t.nch + b; a.mv = t.mv + b; a.midx = t.midx + b;
    a.proof = t.proof ? t.proof + b : nullptr;
    return a;
}
// a new, unexpanded, unvisited node
__device__ __forceinline__ void node_reset(const Arena& A, int i, double prior, Move mv, uint16_t midx) {
    A.prior[i] = prior; A.w[i] = 0.0; A.q[i] = 0.0; A.n[i] = 0; A.vl[i] = 0;
    A.cbase[i] = -1; A.nch[i] = -1; A.mv[i] = mv; A.midx[i] = midx;
    if (A.proof) A.proof[i] = 0;
}
// node so of S -> node dn of D, without its in-flight count; the child base is still the one in S
__device__ __forceinline__ void node_copy(const Arena& D, int dn, const Arena& S, int so) {
    D.prior[dn] = S.prior[so]; D.w[dn] = S.w[so]; D.q[dn] = S.q[so]; D.n[dn] = S.n[so]; D.vl[dn] = 0;
    D.cbase[dn] = S.cbase[so]; D.nch[dn] = S.nch[so]; D.mv[dn] = S.mv[so]; D.midx[dn] = S.midx[so];
    if (D.proof) D.proof[dn] = S.proof[so];      // a kept subtree keeps its proofs
}

__device__ __forceinline__ float wave_max_f(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// A lane's share of a leaf's children: child i = lane + 64 k, k < 4 (M0_MAX_CHILDREN = 256).
constexpr int CPL = M0_MAX_CHILDREN / 64;
static_assert(M0_POLICY_SIZE % 4 == 0, "logit rows are read as 16-byte pieces");

// This lane's part of "the row holds a non-finite logit" (mcts.py:147-149).
// (16-byte loads, all of a lane's 19 in flight together: one memory latency instead of 73 dependent-looking ones)
__device__ __forceinline__ bool row_nonfinite(const float* lg, int lane) {
    constexpr int N4 = M0_POLICY_SIZE / 4, PER_LANE = (N4 + 63) / 64;
    const uint4* lg4 = reinterpret_cast<const uint4*>(lg);         // rows are 16-byte aligned
    uint4 v[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) { const int j = lane + 64 * k; v[k] = lg4[j < N4 ? j : N4 - 1]; }   // unconditional loads
    uint32_t acc = 0;                                               // all-ones exponent = inf or nan; no short-circuit
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        acc |= (uint32_t)((v[k].x & 0x7f800000u) == 0x7f800000u) | (uint32_t)((v[k].y & 0x7f800000u) == 0x7f800000u) |
               (uint32_t)((v[k].z & 0x7f800000u) == 0x7f800000u) | (uint32_t)((v[k].w & 0x7f800000u) == 0x7f800000u);
    }
    return acc != 0;
}

// Softmax over the n <= M0_MAX_CHILDREN values l (CPL per lane, entries >= n hold -3.0e38f), whole-wave.
// Numerics: (logit - max) in float32 as torch does, exp/sum/divide in float64, result rounded to float32.  Within one
// float32 ulp of the reference's torch.softmax (mcts.py:158-168) and reproducible bit-for-bit on the host (oracle mode
// "engine").  Shared by the expansion (expand_kernel) and the policy mode of the analysis engine (policy_lines_kernel).
__device__ __forceinline__ void wave_softmax(const float (&l)[CPL], int n, int lane, float (&pr)[CPL]) {
    float mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) mx = fmaxf(mx, l[k]);
    mx = wave_max_f(mx);
    double e[CPL], sum = 0.0;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const int i = lane + 64 * k; e[k] = i < n ? exp((double)(l[k] - mx)) : 0.0; sum += e[k]; }
    sum = wave_sum_d(sum);
#pragma unroll
    for (int k = 0; k < CPL; ++k) pr[k] = (float)(e[k] / sum);
}

// The next batch row of the game's network, reserved by lane 0 and known to the whole wave.
__device__ __forceinline__ int reserve_row(const TreeDev& d, const GameDev* gd, int lane) {
    int row = 0;
    if (lane == 0) row = atomicAdd(d.row_counter + gd->net_id, 1) + gd->net_id * d.net_row_base;
    return __shfl(row, 0);
}
// A network value as the root sees it: clipped, and negated where the game asks (GameDev::flip_root_v).
__device__ __forceinline__ double root_value(const GameDev* gd, float v) {
    double rv = fmax(-1.0, fmin(1.0, (double)v));
    if (gd->flip_root_v) rv = -rv;
    return rv;
}

// ---- position table of the tt_merge mode (MCTS._tt_get / _tt_put / _register_children_in_tt, mcts.py:1231-1346):
// open addressing with linear probing over a per-game region; key 0 = empty; an entry holds the node registered LAST
// under its key (the reference's dict assignment overwrites).  Cleared when a search starts from a fresh root.
__device__ __forceinline__ uint64_t tt_key_of(const Pos& p) { const uint64_t k = tkey(p); return k ? k : 1ull; }
__device__ __forceinline__ int tt_home(uint64_t key, int cap) { return (int)((key ^ (key >> 29)) & (uint64_t)(cap - 1)); }
// table of game g (of its side gd->arena in a match engine with per-side tables)
__device__ __forceinline__ size_t tt_table_of(const TreeDev& d, int g, const GameDev* gd) {
    return ((size_t)g * d.tt_sides + (d.tt_sides == 2 ? gd->arena : 0)) * (size_t)d.tt_cap;
}
// whole-wave: empty `nkeys` keys (a multiple of 2) starting at the 16-byte aligned `keys`
__device__ __forceinline__ void tt_clear(uint64_t* keys, int nkeys, int lane) {
    uint4* tk = reinterpret_cast<uint4*>(keys);
    for (int i = lane; i < nkeys / 2; i += 64) tk[i] = make_uint4(0, 0, 0, 0);
}
// whole-wave lookup of a wave-uniform key: 64 slots per probe round; -1 = not registered
static __device__ int tt_lookup(const uint64_t* keys, const int* nodes, int cap, uint64_t key, int lane) {
    const int mask = cap - 1, home = tt_home(key, cap);
    for (int it = 0; it < cap; it += 64) {
        const uint64_t k = keys[(home + it + lane) & mask];
        const unsigned long long hit = __ballot(k == key), emp = __ballot(k == 0ull);
        const int fh = hit ? __builtin_ctzll(hit) : 64, fe = emp ? __builtin_ctzll(emp) : 64;
        if (fh < fe) return nodes[(home + it + fh) & mask];
        if (fe < 64) return -1;
    }
    return -1;
}
// per-lane insert-or-overwrite (the active lanes of one call hold distinct keys)
static __device__ void tt_insert(uint64_t* keys, int* nodes, int cap, uint64_t key, int node) {
    const int mask = cap - 1;
    int s = tt_home(key, cap);
    for (int it = 0; it < cap; ++it) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long*>(keys + s), 0ull, (unsigned long long)key);
        if (prev == 0ull || prev == (unsigned long long)key) { nodes[s] = node; return; }
        s = (s + 1) & mask;
    }
}

// MCTS._backpropagate (mcts.py:946-953): the leaf gets +v, its parent -v, ...  The nodes of a path are distinct, so
// every level is independent: lane d updates level d (all levels' loads in flight at once instead of a chain of
// dependent read-modify-writes by one lane); the arithmetic per node is that of the sequential loop (negation is exact).
// `mirror(node, n, q)` is told every node's new statistics as they go to the arena (select_kernel's LDS copy of the tree top
// follows through it; expand_kernel passes NoMirror).
struct NoMirror { __device__ __forceinline__ void operator()(int, int, double) const {} };
template <typename Mirror>
static __device__ void backprop(const Arena& A, const int* path, int depth, double value, int lane, bool may_repeat,
                                const Mirror& mirror) {   // whole-wave caller
    const double v = fmax(-1.0, fmin(1.0, value));
    if (may_repeat) {
        // tt_merge: a path can pass through the same node twice (a position repeated along the line); the reference's
        // sequential loop then updates it twice, in path order from the leaf up -- do exactly that when it happens
        bool dup = false;
        for (int d = lane; d <= depth; d += 64) {
            const int nd = path[d];
            for (int e = 0; e < d; ++e) dup = dup || path[e] == nd;
        }
        if (__any(dup)) {
            if (lane == 0) {
                double vv = v;
                for (int d = depth; d >= 0; --d) {
                    const int nd = path[d];
                    const int nn = A.n[nd] + 1;
                    const double ww = A.w[nd] + vv;
                    A.n[nd] = nn; A.w[nd] = ww; A.q[nd] = ww / (double)nn;
                    vv = -vv;
                }
            }
            return;
        }
    }
    for (int d = lane; d <= depth; d += 64) {
        const int nd = path[d];
        const int nn = A.n[nd] + 1;
        const double ww = A.w[nd] + (((depth - d) & 1) ? -v : v);
        const double qq = ww / (double)nn;
        A.n[nd] = nn; A.w[nd] = ww; A.q[nd] = qq;
        mirror(nd, nn, qq);
    }
}

// ---- a new root for a slot (advance_kernel, reroot_moves_kernel); whole-wave, one wave per block
__device__ __forceinline__ void reroot_fresh(const TreeDev& d, GameDev* gd, int g, int lane) {
    const Arena D = arena_of(d.t, g, 0);
    // a fresh root starts with an empty position table
    if (d.tt_keys) tt_clear(d.tt_keys + (size_t)g * d.tt_sides * d.tt_cap, d.tt_sides * d.tt_cap, lane);
    if (lane == 0) {
        node_reset(D, 0, 0.0, 0, 0);
        gd->arena = 0; gd->root = 0; gd->next = 1; gd->overflow = 0;
    }
}

// The subtree of node `r` of the slot's current half -> the other arena half, breadth-first: node 0 is the new root, then its
// children, their children ... (select_kernel's LDS copy of the tree top relies on this order).
__device__ __forceinline__ void reroot_keep_subtree(const TreeDev& d, GameDev* gd, int g, int r, int lane) {
    const int a = gd->arena;
    const Arena Sx = arena_of(d.t, g, a), D = arena_of(d.t, g, a ^ 1);
    if (lane == 0) node_copy(D, 0, Sx, r);
    __syncthreads();
    int head = 0, tail = 1;
    while (head < tail) {
        const int lim = tail < head + 64 ? tail : head + 64;
        const int i = head + lane;
        const int nc_i = i < lim ? (int)D.nch[i] : -1;
        const int cb_i = i < lim ? D.cbase[i] : -1;     // still the OLD child base
        unsigned long long mask = __ballot(nc_i > 0);
        while (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int nc = __shfl(nc_i, b), ocb = __shfl(cb_i, b);
            const int ncb = tail;
            for (int k = lane; k < nc; k += 64) node_copy(D, ncb + k, Sx, ocb + k);
            if (lane == 0) D.cbase[head + b] = ncb;
            tail += nc;
        }
        __syncthreads();
        head = lim;
    }
    if (lane == 0) { gd->arena = a ^ 1; gd->root = 0; gd->next = tail; gd->overflow = 0; }
}
