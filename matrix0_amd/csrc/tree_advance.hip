// advance_kernel: re-root a game's tree on the played move, one wavefront per game.
//   child_slot >= 0       keep that child's subtree, compacted breadth-first into the other arena half (tree_device.h)
//   ROOT_FRESH            fresh tree (and an empty position table; tree_device.h)
//   ROOT_FROM_SIDE_TABLE  and below (RootMode, tree.h): match engine with per-side tables (tt_sides == 2), the root is looked
//                         up in the side's table
// and, before any of these, the slot's evaluation caches are emptied when the host flagged a new game (GameDev::ec_clear).
#include "tree_device.h"
#include "eval_cache.h"

// Per-side tables: side = the network that searches now.  Nothing is compacted or cleared between the searches of a game; the
// root is whatever node the side's table holds for the position (MCTS.run: root = self._tt_get(key), mcts.py:343), else a new
// node.  ROOT_FIRST_OF_GAME: both tables are cleared first.
__device__ __forceinline__ void reroot_from_table(const TreeDev& d, GameDev* gd, int g, int slot, int lane) {
    const int s = gd->net_id & 1;
    const int prev_side = gd->arena & 1, prev_next = gd->next;
    if (slot == ROOT_FIRST_OF_GAME) tt_clear(d.tt_keys + (size_t)g * 2 * d.tt_cap, 2 * d.tt_cap, lane);
    __syncthreads();
    int nxt = slot == ROOT_FIRST_OF_GAME ? 0 : (s == prev_side ? prev_next : gd->side_next[s]);
    const Arena A = arena_of(d.t, g, s);
    uint64_t* TK = d.tt_keys + ((size_t)g * 2 + s) * d.tt_cap;
    const int* TN = d.tt_nodes + ((size_t)g * 2 + s) * d.tt_cap;
    int node = slot == ROOT_FIRST_OF_GAME ? -1 : tt_lookup(TK, TN, d.tt_cap, tt_key_of(gd->root_pos), lane);
    // a half that cannot take another search's worth of nodes starts over: its table is dropped and the search begins from a
    // fresh root (what the reference's _cleanup_memory does to an over-full table); engine.arena_nodes sizes it for a game
    if (nxt + (d.search_nodes > 4 * M0_MAX_CHILDREN ? d.search_nodes : 4 * M0_MAX_CHILDREN) >= d.t.cap) {
        tt_clear(TK, d.tt_cap, lane);
        nxt = 0; node = -1;
        __syncthreads();
    }
    const bool found = node >= 0;
    if (lane == 0) {
        if (slot != ROOT_FIRST_OF_GAME) gd->side_next[prev_side] = prev_next;
        else { gd->side_next[0] = 0; gd->side_next[1] = 0; }
        if (!found) {
            node = nxt;
            node_reset(A, node, 0.0, 0, 0);
            nxt = node + 1;
        }
        gd->arena = s; gd->root = node; gd->next = nxt; gd->overflow = 0;
        gd->root_fresh = found ? 0 : 1; gd->root_found = found ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void advance_kernel(TreeDev d, const int* game_ids, const int* child_slots, int count) {
    const int j = blockIdx.x, lane = threadIdx.x;
    if (j >= count) return;
    const int g = game_ids[j], slot = child_slots[j];
    GameDev* gd = &d.games[g];
    // a match engine's slot starts a new game: what its two networks said about the last game's positions goes.  (Nothing of
    // this launch reads the keys again: select_kernel's probes are a later launch.)
    const bool new_game = gd->ec_clear != 0;
    if (new_game) {
        if (d.ec.sets > 0) ec_clear_game(d.ec, gd, g, lane);
        if (lane == 0) gd->ec_clear = 0;
    }
    if (slot <= ROOT_FROM_SIDE_TABLE) reroot_from_table(d, gd, g, slot, lane);
    else if (slot < 0) reroot_fresh(d, gd, g, lane);
    else reroot_keep_subtree(d, gd, g, arena_of(d.t, g, gd->arena).cbase[gd->root] + slot, lane);
}

hipError_t launch_advance(const TreeDev& d, const int* game_ids_dev, const int* child_slots_dev, int count, hipStream_t st) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(advance_kernel, dim3(count), dim3(64), 0, st, d, game_ids_dev, child_slots_dev, count);
    return hipGetLastError();
}
