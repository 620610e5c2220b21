// Gumbel root search on the device (include/m0_gumbel.h; the arithmetic is gumbel_core.h): what select_kernel's Gumbel
// instantiation does at the root level -- the pass prologue (draws, scores, visit counts) and the pick of one descent -- and
// what expand_kernel writes when such a search finishes.  Whole-wave functions, one wavefront per game tree; a root may have
// more than 64 children, so every loop over them strides by 64.
#pragma once
#include "tree_device.h"

// Arg-max over the wave of (score, index) pairs with the lowest index among equal scores; index -1 = this lane has none.
// The butterfly of select_kernel's children scan.
__device__ __forceinline__ int wave_argmax_first(double best, int bi) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    return bi;
}
__device__ __forceinline__ int wave_max_i(int v) {
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// max N and v_mix over the root's k children (child block at cb) from the completed statistics in the arena
struct GumbelRootStats { int max_n; double v_mix; };
__device__ __forceinline__ GumbelRootStats gumbel_root_stats(const Arena& A, int cb, int k, double root_v, int lane) {
    int mx = 0, sn = 0;
    double sp = 0.0, spq = 0.0;
    for (int i = lane; i < k; i += 64) {
        const int n = A.n[cb + i];
        if (n > 0) { const double p = A.prior[cb + i]; mx = n > mx ? n : mx; sn += n; sp += p; spq += p * A.q[cb + i]; }
    }
    mx = wave_max_i(mx);
    for (int o = 32; o > 0; o >>= 1) sn += __shfl_xor(sn, o);
    sp = wave_sum_d(sp); spq = wave_sum_d(spq);
    return GumbelRootStats{mx, gumbel_v_mix(root_v, (long)sn, sp, spq)};
}

// Pass prologue.  On the first pass of a search the k Gumbel draws are made and gl = g + log(prior) is kept for the game.
// Then, from the completed statistics: score[i] = gl[i] + sigma(completedQ_i) and cnt[i] = N_i, both in LDS for the pass.
// cnt, not n + vl, is the visit count the descents of the pass go by: a root child that is a terminal leaf is backed up
// inside select AND keeps its in-flight count until the release, so n + vl would count it twice.
__device__ __forceinline__ void gumbel_pass_prologue(const TreeDev& d, const TreeCfg& c, const Arena& A, GameDev* gd, int g, int root,
                                                     double* score, int* cnt, int lane) {
    const int k = A.nch[root] > 0 ? A.nch[root] : 0, cb = A.cbase[root];
    double* gl = d.gumbel_gl + (size_t)g * M0_MAX_CHILDREN;
    const bool first_pass = !gd->gumbel_drawn;
    const uint64_t seed = gd->seed_gumbel, ctr = gd->ctr_gumbel;
    if (first_pass) {
        for (int i = lane; i < k; i += 64) gl[i] = gumbel_from_uniform(u01(seed, ctr + (uint64_t)i)) + log(A.prior[cb + i]);
        if (lane == 0) { gd->ctr_gumbel = ctr + (uint64_t)k; gd->gumbel_drawn = 1; }
    }
    const GumbelRootStats st = gumbel_root_stats(A, cb, k, gd->root_v, lane);
    for (int i = lane; i < k; i += 64) {                    // a lane reads back only the gl it wrote itself
        const int n = A.n[cb + i];
        score[i] = gl[i] + gumbel_bonus(c.gumbel_cfg, st.max_n, n, A.q[cb + i], st.v_mix);
        cnt[i] = n;
    }
    __syncthreads();
}

// One descent's root child: among the children visited `want` times so far (cnt), the best score, the first among equals.
// No child with that count -- which a correct schedule never produces -- : the best of all, counted in GameDev::gumbel_miss.
__device__ __forceinline__ int gumbel_pick_child(GameDev* gd, const double* score, int* cnt, int k, int want, int lane) {
    double best = -INFINITY;
    int bi = -1;
    for (int i = lane; i < k; i += 64)
        if (cnt[i] == want && (bi < 0 || score[i] > best)) { best = score[i]; bi = i; }
    bi = wave_argmax_first(best, bi);
    if (bi < 0) {
        for (int i = lane; i < k; i += 64)
            if (bi < 0 || score[i] > best) { best = score[i]; bi = i; }
        bi = wave_argmax_first(best, bi);
        if (bi < 0) bi = 0;
        if (lane == 0) gd->gumbel_miss++;
    }
    __syncthreads();                                         // every lane has read cnt before lane 0 changes it
    if (lane == 0) cnt[bi] += 1;
    __syncthreads();
    return bi;
}

// The finished search's GumbelResult: v_mix, pi = softmax(log prior + sigma(completedQ)) over all k children, gl, and the
// move (most visits, then the best score, then the lowest index).
__device__ __forceinline__ void write_gumbel_result(const TreeDev& d, const TreeCfg& c, const Arena& A, const GameDev* gd, int g, int root,
                                                    int lane) {
    GumbelResult* R = d.gumbel_results + g;
    const double* gl = d.gumbel_gl + (size_t)g * M0_MAX_CHILDREN;
    const int k = A.nch[root] > 0 ? A.nch[root] : 0, cb = A.cbase[root];
    const GumbelRootStats st = gumbel_root_stats(A, cb, k, gd->root_v, lane);
    double mx = -INFINITY, bscore = 0.0;
    int bi = -1, bn = 0;
    for (int i = lane; i < k; i += 64) {
        const int n = A.n[cb + i];
        const double b = gumbel_bonus(c.gumbel_cfg, st.max_n, n, A.q[cb + i], st.v_mix);
        mx = fmax(mx, log(A.prior[cb + i]) + b);
        if (gumbel_pick_better(n, gl[i] + b, i, bn, bscore, bi)) { bi = i; bn = n; bscore = gl[i] + b; }
        R->gl[i] = gl[i];
    }
    mx = wave_max_d(mx);
    for (int off = 32; off > 0; off >>= 1) {
        const int on = __shfl_xor(bn, off), oi = __shfl_xor(bi, off);
        const double os = __shfl_xor(bscore, off);
        if (oi >= 0 && gumbel_pick_better(on, os, oi, bn, bscore, bi)) { bi = oi; bn = on; bscore = os; }
    }
    double sum = 0.0;
    for (int i = lane; i < k; i += 64)
        sum += exp(log(A.prior[cb + i]) + gumbel_bonus(c.gumbel_cfg, st.max_n, A.n[cb + i], A.q[cb + i], st.v_mix) - mx);
    sum = wave_sum_d(sum);
    for (int i = lane; i < k; i += 64)
        R->pi[i] = exp(log(A.prior[cb + i]) + gumbel_bonus(c.gumbel_cfg, st.max_n, A.n[cb + i], A.q[cb + i], st.v_mix) - mx) / sum;
    if (lane == 0) { R->pick = bi; R->v_mix = st.v_mix; }
}
