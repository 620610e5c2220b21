// reroot_moves_kernel: re-root a slot's tree on a list of MOVES (advance_kernel follows a child slot, one ply), one wavefront
// per slot.  From the slot's root it follows up to M0_REROOT_MAX_MOVES moves: at each node the contiguous child block is
// scanned, one child per lane plus stride, for the child that carries the move and is itself expanded; the winner is taken by
// ballot.  When every move is found the subtree of the node reached is compacted breadth-first into the other arena half
// (reroot_keep_subtree); when a move is not among a node's children (pruned roots), a child on the way is unexpanded or the
// list is empty and the root itself is unexpanded, the slot gets a fresh root (reroot_fresh, which also empties a position
// table).  Per entry it reports whether the subtree was kept and the statistics the kept root carries.  No atomics, no LDS.
// Runs on the engine's stream between steps, on slots that no search is using (a held analysis slot, capi_analysis.hip).
#include "tree_device.h"

__global__ __launch_bounds__(64) void reroot_moves_kernel(TreeDev d, const int* slots, const int* nmoves, const int* moves, int count,
                                                          RerootOut* out) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= count) return;
    const int g = slots[j];
    if (g < 0 || g >= d.G) return;
    GameDev* gd = &d.games[g];
    const Arena A = arena_of(d.t, g, gd->arena);
    int nm = nmoves[j];
    nm = nm < 0 ? 0 : (nm > M0_REROOT_MAX_MOVES ? M0_REROOT_MAX_MOVES : nm);
    int node = gd->root;
    // wave-uniform: the node's child block lies inside the arena half
    auto block_ok = [&](int nd) {
        const int nc = A.nch[nd], cb = A.cbase[nd];
        return nc > 0 && nc <= M0_MAX_CHILDREN && cb >= 0 && cb + nc <= d.t.cap;
    };
    bool found = node >= 0 && node < d.t.cap && block_ok(node);
    for (int m = 0; m < nm && found; ++m) {
        const int nc = A.nch[node], cb = A.cbase[node];
        const Move want = (Move)moves[(size_t)j * M0_REROOT_MAX_MOVES + m];
        int mine = -1;
        for (int i = lane; i < nc; i += 64)
            if (A.mv[cb + i] == want && A.nch[cb + i] > 0) mine = i;
        const unsigned long long hit = __ballot(mine >= 0);
        if (!hit) { found = false; break; }
        node = cb + __shfl(mine, __builtin_ctzll(hit));
        found = block_ok(node);
    }
    if (found) {
        const int n = A.n[node];
        const double q = A.q[node];
        reroot_keep_subtree(d, gd, g, node, lane);
        if (lane == 0) { out[j].kept = 1; out[j].n = n; out[j].q = q; }
    } else {
        reroot_fresh(d, gd, g, lane);
        if (lane == 0) { out[j].kept = 0; out[j].n = 0; out[j].q = 0.0; }
    }
}

hipError_t launch_reroot_moves(const TreeDev& d, const int* slots_dev, const int* nmoves_dev, const int* moves_dev, int count,
                               RerootOut* out_dev, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(reroot_moves_kernel, dim3(count), dim3(64), 0, st, d, slots_dev, nmoves_dev, moves_dev, count, out_dev);
    return hipGetLastError();
}
