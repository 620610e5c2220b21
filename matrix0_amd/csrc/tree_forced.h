// Forced playouts on the device (include/m0_budget.h; the arithmetic is budget_core.h): what select_kernel's forced
// instantiation adds at depth 0 of a descent of a search with GameDev::forced.  A pre-pass sums the root children's completed
// visits -- at most four of the at most 218 children per lane, then one integer butterfly over the wave: wave-uniform work, no
// LDS, no atomics -- and the children scan gives a child in deficit a score above every PUCT score that falls with its index,
// so that the scan's own arg-max (larger score, lower index among equals) returns the deficit child with the lowest index and
// broadcasts its fields as it does the PUCT winner's.  The jitter draws are indexed by counter: a child whose score the rule
// replaces has consumed its draw all the same.
#pragma once
#include "tree_device.h"

// All 64 lanes take part: call it outside lane-dependent control flow.
__device__ __forceinline__ int wave_sum_i(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the scan's score of root child i: the forcing rule's where the child is in deficit, else `puct` (the score select computed)
__device__ __forceinline__ double forced_root_score(double forced_k, double prior, int n, int inflight, int n_sum, int i, double puct) {
    return m0::budget_in_deficit(forced_k, prior, n, inflight, (int64_t)n_sum) ? m0::budget_forced_score(i) : puct;
}
