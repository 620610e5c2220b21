// select_kernel: L descents per game and step, one wavefront per game tree: children scored one per lane from coalesced SoA
// loads (PUCT + FPU + virtual loss + jitter in fp64, mcts.py:851-925), wave arg-max with first-max tie-break, leaf board by
// make_move, terminal test, immediate terminal backup, evaluation-cache probe, M0_PLANES-plane encode written straight into
// the network input (lane = square).
// With endgame tablebases attached (TreeDev::tb_set) a leaf that survives the game-over tests is looked up there: a hit is a
// terminal leaf with the table's value.  A position with a castling right left is no hit; the half-move clock is ignored,
// as in adjudication (tb_core.h, tb_probe).
#include "tree_device.h"
#include "tree_gumbel.h"
#include "tree_proof.h"
#include "tree_forced.h"
#include "tb_core.h"
#include "eval_cache.h"
#include "movegen_wave.h"
#include "kernel_common.h"   // DeviceOnce

__device__ __forceinline__ double cpuct_at(const TreeCfg& c, int ply) {    // mcts.py:927-944
    if (c.use_c_base) {
        double N = fmax(1.0, (double)(ply + 1));
        return c.cpuct_c_init + log((N + c.cpuct_c_base) / c.cpuct_c_base);
    }
    if (c.cpuct_plies <= 0) return c.cpuct;
    int p = ply < 0 ? 0 : (ply > c.cpuct_plies ? c.cpuct_plies : ply);
    double t = (double)p / (double)c.cpuct_plies;
    return c.cpuct_start + (c.cpuct_end - c.cpuct_start) * t;
}
static __device__ void apply_dirichlet(const Arena& A, int root, GameDev* gd, const TreeCfg& c, double* sg, int lane) {
    const int k = A.nch[root];
    if (k <= 0 || c.dirichlet_frac <= 0.0) return;
    const int cb = A.cbase[root];
    uint64_t ctr = gd->ctr_dir;
    double sum = 0.0;
    for (int i = 0; i < k; ++i) {                 // sequential draws, uniform across lanes
        double gmm = gamma_draw(gd->seed_dir, ctr, c.dirichlet_alpha);
        if (lane == 0) sg[i] = gmm;
        sum += gmm;
    }
    __syncthreads();
    for (int i = lane; i < k; i += 64) {
        double nv = A.prior[cb + i] * (1.0 - c.dirichlet_frac) + (sg[i] / sum) * c.dirichlet_frac;
        A.prior[cb + i] = fmax(1e-8, fmin(1.0 - 1e-8, nv));
    }
    if (lane == 0) gd->ctr_dir = ctr;
    __syncthreads();
}

__device__ __forceinline__ Sample make_sample(const Pos& pos, SampleKind kind, int leaf, int depth, int row, int nlegal, uint64_t ckey) {
    Sample s; s.pos = pos; s.kind = kind; s.leaf = leaf; s.depth = depth; s.row = row; s.nlegal = nlegal; s.ckey = ckey;
    return s;
}

// is_game_over() (checkmate, stalemate, insufficient, 75-move, fivefold) -> _terminal_value in `tv`; then, with tables
// attached, the table's verdict for the side to move (`tb_hit`).  pos is wave-uniform: the probe is scalar work and one
// byte load, the same in every lane.
__device__ __forceinline__ bool leaf_terminal(const TreeDev& d, const TreeCfg& c, const Pos& pos, int nlegal, int depth,
                                              const uint64_t* pkey, const uint8_t* pirr, const uint64_t* H, int hist_len, int lane,
                                              double& tv, bool& tb_hit) {
    const bool chk = in_check(pos);
    bool term = false;
    tv = 0.0;
    if (nlegal == 0) { term = true; tv = chk ? -1.0 : c.draw_penalty; }
    else if (is_insufficient(pos)) { term = true; tv = c.draw_penalty; }
    else if (pos.halfmove >= 150) { term = true; tv = c.draw_penalty; }
    else {
        const uint64_t lk = tkey(pos);
        int cnt = 1;
        bool broke = false;
        for (int dd = depth - 1; dd >= 0; --dd) {
            if (pirr[dd]) { broke = true; break; }
            if (pkey[dd] == lk) ++cnt;
        }
        if (!broke)                                   // the game's reversible-move window: one entry per lane
            for (int i0 = 0; i0 < hist_len; i0 += 64) {
                const int i = i0 + lane;
                cnt += __popcll(__ballot(i < hist_len && H[i] == lk));
            }
        if (cnt >= 5) { term = true; tv = c.draw_penalty; }
    }
    tb_hit = false;
    if (!term && d.tb_set) {
        int wdl, dtm;
        if (tb_probe(*d.tb_set, pos, d.tb_max_pieces, wdl, dtm)) {
            term = tb_hit = true;
            tv = wdl > 0 ? 1.0 : (wdl < 0 ? -1.0 : c.draw_penalty);
        }
    }
    return term;
}

// The same unexpanded node reached again in this pass (a batch of 96 descents over a young tree lands on the same leaf
// many times; the virtual loss only spreads them): it shares the batch row of its first occurrence instead of being
// evaluated twice in one forward.  The pending row sits in the node's child-base field, which means nothing until the
// node is expanded: cbase <= -2  <=>  row -(cbase + 2) of this pass (expand_kernel resets it).
__device__ __forceinline__ bool pending_row(const Arena& A, int node, int& row) {
    const int pend = A.cbase[node];
    if (A.nch[node] < 0 && pend <= -2) { row = -(pend + 2); return true; }
    return false;
}
__device__ __forceinline__ void mark_pending_row(const Arena& A, int node, int row) { A.cbase[node] = -(row + 2); }

// mcts.py:359-371: a root taken over from the previous search is evaluated once more (value only)
__device__ __forceinline__ void emit_root_value(const TreeDev& d, GameDev* gd, Sample* S, int at, int root, int lane) {
    const int row = reserve_row(d, gd, lane);
    if (lane == 0) {
        S[at] = make_sample(gd->root_pos, SK_ROOT_VALUE, root, 0, row, 0, 0); gd->reinfer = 0;
    }
    encode_nhwc(gd->root_pos, nhwc_row(d.x0, row), lane);
}

// root not expanded: one network evaluation, no simulation
__device__ __forceinline__ void emit_root_init(const TreeDev& d, GameDev* gd, Sample* S, int* P, uint16_t* LM, int root, bool reinfer,
                                               Move* smoves, Move* spseudo, int lane) {
    if (lane == 0 && !gd->root_fresh) {
        // reused but never expanded child: run() applies Dirichlet BEFORE expanding it (a no-op on a
        // childless node, mcts.py:374-376 vs 398-413) and then sets root.q = v
        gd->need_dirichlet = 0;
        gd->root_q_from_v = 1;
    }
    const int row = reserve_row(d, gd, lane);
    const Pos rp = gd->root_pos;
    const int nl = gen_legal_wave(rp, smoves, spseudo, lane);
    for (int i = lane; i < nl; i += 64) LM[i] = smoves[i];
    if (lane == 0) {
        S[0] = make_sample(rp, SK_ROOT_INIT, root, 0, row, nl, 0); P[0] = root; gd->nsamples = reinfer ? 2 : 1;
    }
    encode_nhwc(rp, nhwc_row(d.x0, row), lane);
    if (reinfer) emit_root_value(d, gd, S, 1, root, lane);
}

// The sample of a leaf: a terminal or cache-served leaf needs no batch row; one that an earlier sample of this pass already
// sent to the network shares that row (pending_row); any other reserves a row and writes its planes there.
__device__ __forceinline__ void emit_leaf(const TreeDev& d, const TreeCfg& c, const Arena& A, GameDev* gd, Sample* smp, uint16_t* lm,
                                          const Pos& pos, int node, int depth, const Move* smoves, int nlegal, bool term, bool cached,
                                          uint64_t ckey, int lane) {
    int row = -1;
    bool shared = false;
    if (!term && !cached && c.eval_cache) shared = pending_row(A, node, row);
    if (!term && !cached && !shared) {
        row = reserve_row(d, gd, lane);
        encode_nhwc(pos, nhwc_row(d.x0, row), lane);
        if (c.eval_cache && lane == 0 && A.nch[node] < 0) mark_pending_row(A, node, row);
    }
    if (!term && !shared) for (int i = lane; i < nlegal; i += 64) lm[i] = smoves[i];
    if (lane == 0) {
        *smp = make_sample(pos, term ? SK_TERMINAL : (cached ? SK_CACHED : (shared ? SK_SHARED : SK_EVAL)), node, depth, row, nlegal,
                           cached ? 0ull : ckey);
    }
}

// The top of a game's tree lives in LDS for the duration of a select launch (north star: "tree walk over LDS-resident node
// arrays"): after every played move the kept subtree is compacted BREADTH-FIRST (advance_kernel), so the nodes with the lowest
// indices are the root, its children, their children ... -- the levels every one of the pass's 96 descents walks through.  The
// first M0_SEL_CACHE nodes' select fields are copied once per launch; the children scan reads them from LDS instead of paying a
// global round trip per level, and the two things a select launch writes to such nodes (in-flight counts, the statistics of a
// terminal leaf's path) are written through.  Deeper nodes -- and everything in the table modes, whose arenas are not
// compacted -- are read from the arenas in HBM as before.
constexpr int M0_SEL_CACHE = 2048;
struct TopCache {
    double prior[M0_SEL_CACHE];
    double q[M0_SEL_CACHE];
    int n[M0_SEL_CACHE];
    int vl[M0_SEL_CACHE];
    int cbase[M0_SEL_CACHE];
    int16_t nch[M0_SEL_CACHE];
    uint16_t mv[M0_SEL_CACHE];
};
constexpr int M0_SEL_CACHE_BYTES = M0_SEL_CACHE * 32;     // the launch's dynamic LDS
static_assert(sizeof(TopCache) == M0_SEL_CACHE_BYTES, "32 bytes of select fields per cached node");
// Select field f of node i: from the LDS copy `TC` where the node is cached (`hit`), else from the arena `A`.  A macro on
// purpose: as written here the compiler folds a node's reads into one branch on `hit` (LDS loads | global loads); behind a
// function or lambda, however inlined, each read becomes a select between an LDS and a global address and a flat load, and
// select_kernel measured 25 us (1.5 %) slower per call.
#define TOP(f, hit, i) ((hit) ? TC->f[i] : A.f[i])

// GUMBEL: the instantiation for the Gumbel root search (MODE_GUMBEL, tree_gumbel.h).  Only the root level differs: no
// Dirichlet noise, a pass that ends at the phase boundary of the halving schedule, and at depth 0 the pick by scheduled visit
// count and Gumbel score in place of the PUCT scan (no jitter draw there).  A template parameter, not a field read in the scan:
// the PUCT instantiation is the kernel it was.
// PROOF: the instantiation for the proof search (MODE_PROOF, tree_proof.h, include/m0_proof.h).  The nodes' proofs are read
// through PRF: the tree top's from an LDS copy beside TopCache, the others from the arena.  A terminal leaf is proven at its
// first visit and the proof is combined up its path; a descent stops at a proven node; the scan passes over children that
// are won for their own mover; a pass ends once the root is proven.  While no node is proven it is the PUCT search, draw by draw.
// FORCED: the instantiation for the self-play budget mix (MODE_BUDGET, tree_forced.h, include/m0_budget.h).  The rule is per
// game: in a search with GameDev::forced (a full search with forced playouts; full and fast searches of different games share a
// launch) a descent takes, at depth 0, the lowest root child in deficit where there is one.  A search without the flag is the
// PUCT search, draw by draw.
#define PRF(i) ((i) < ncached ? TP[i] : A.proof[i])
template <SearchMode MODE>
__global__ __launch_bounds__(64) void select_kernel(TreeDev d, TreeCfg c) {
    constexpr bool GUMBEL = MODE == MODE_GUMBEL, PROOF = MODE == MODE_PROOF, FORCED = MODE == MODE_BUDGET;
    extern __shared__ __attribute__((aligned(16))) char sel_cache[];
    TopCache* const TC = reinterpret_cast<TopCache*>(sel_cache);
    __shared__ uint64_t pkey[M0_MAX_DEPTH];
    __shared__ uint8_t pirr[M0_MAX_DEPTH];
    __shared__ Move smoves[M0_MAX_MOVES];
    __shared__ Move spseudo[M0_MAX_MOVES];
    __shared__ double sg[M0_MAX_CHILDREN];
    const int g = blockIdx.x, lane = threadIdx.x;
    GameDev* gd = &d.games[g];
    if (!gd->active) { if (lane == 0) gd->nsamples = 0; return; }
    uint16_t* LM = d.leaf_moves + (size_t)g * (d.L + 1) * M0_MAX_CHILDREN;
    const Arena A = arena_of(d.t, g, gd->arena);
    const int root = gd->root;
    Sample* S = d.samples + (size_t)g * (d.L + 1);
    int* P = d.paths + (size_t)g * (d.L + 1) * M0_MAX_DEPTH;
    int* EP = c.tt_merge ? d.epaths + (size_t)g * (d.L + 1) * M0_MAX_DEPTH : nullptr;
    const uint64_t* TK = c.tt_merge ? d.tt_keys + tt_table_of(d, g, gd) : nullptr;
    const int* TN = c.tt_merge ? d.tt_nodes + tt_table_of(d, g, gd) : nullptr;
    const bool reinfer = gd->reinfer != 0;

    if constexpr (PROOF) {
        // a root that is proven -- by an earlier pass of this search, or in the subtree the search took over -- is searched no
        // further: no sample, no evaluation; expand_kernel declares the search finished
        if (A.proof[root] != 0) { if (lane == 0) { gd->nsamples = 0; gd->reinfer = 0; } return; }
    }
    if (A.nch[root] < 0) { emit_root_init(d, gd, S, P, LM, root, reinfer, smoves, spseudo, lane); return; }
    if constexpr (GUMBEL) {
        if (lane == 0) gd->need_dirichlet = 0;
    } else if (gd->need_dirichlet) {
        apply_dirichlet(A, root, gd, c, sg, lane);
        if (lane == 0) gd->need_dirichlet = 0;
    }
    int nleaf = gd->sims_target - gd->sims_done;
    if (nleaf > d.L) nleaf = d.L;
    // Gumbel: the pass ends with the phase of the halving schedule, where the next phase needs this one's values
    const int g_done = gd->sims_done, g_n = gd->sims_target;
    const int g_m = GUMBEL ? gumbel_m_eff(c.gumbel_cfg.max_considered, A.nch[root]) : 0;
    if constexpr (GUMBEL) {
        if (nleaf > 0) { const int left = gumbel_phase_end(g_m, g_n, g_done) - g_done; if (nleaf > left) nleaf = left; }
    }
    if (nleaf < 0) nleaf = 0;
    // the top of the tree -> LDS (after the Dirichlet noise, which rewrites the root's priors)
    int ncached = 0;
    int16_t* TP = nullptr;                                 // proof search: the proofs of the cached nodes
    if constexpr (PROOF) {
        __shared__ int16_t top_proof[M0_SEL_CACHE];
        TP = top_proof;
    }
    if (!c.tt_merge && nleaf > 0) {
        ncached = gd->next < M0_SEL_CACHE ? gd->next : M0_SEL_CACHE;
        for (int i = lane; i < ncached; i += 64) {
            TC->prior[i] = A.prior[i]; TC->q[i] = A.q[i]; TC->n[i] = A.n[i]; TC->vl[i] = A.vl[i]; TC->cbase[i] = A.cbase[i];
            TC->nch[i] = A.nch[i]; TC->mv[i] = A.mv[i];
            if constexpr (PROOF) TP[i] = A.proof[i];
        }
        __syncthreads();
    }
    int* gcnt = nullptr;                                   // Gumbel: the root children's visit counts as the pass goes
    if constexpr (GUMBEL) {
        __shared__ int gumbel_cnt[M0_MAX_CHILDREN];
        gcnt = gumbel_cnt;
        if (nleaf > 0) gumbel_pass_prologue(d, c, A, gd, g, root, sg, gcnt, lane);
    }
    uint64_t ctrj = gd->ctr_jitter;
    const uint64_t seedj = gd->seed_jitter;
    const double jit = c.selection_jitter > 0.0 ? c.selection_jitter : 0.001;
    const int hist_len = gd->hist_len;
    const uint64_t* H = d.hist + (size_t)g * M0_HIST_CAP;
    const bool forced_search = FORCED && gd->forced != 0;  // wave-uniform
    // proof search: step 2 of the rule needs a node's children to be all of its legal moves
    const bool proof_complete = c.max_children <= 0 && !(c.min_child_prior > 0.0);
    // a node becomes proven: the arena, the LDS copy, and the store made visible to the loads of later descents (see the fence
    // after the terminal backup below)
    auto set_proof = [&](int nd, int16_t pv) {
        if (lane == 0) { A.proof[nd] = pv; if (nd < ncached) TP[nd] = pv; }
    };
    int made = nleaf;                                      // samples of this pass: fewer once the root is proven

    for (int s = 0; s < nleaf; ++s) {
        Pos pos = gd->root_pos;
        int* path = P + (size_t)s * M0_MAX_DEPTH;
        int* epath = c.tt_merge ? EP + (size_t)s * M0_MAX_DEPTH : nullptr;
        int node = root, depth = 0;
        int prev_from = -1, prev_to = -1;
        if (lane == 0) { path[0] = root; if (epath) epath[0] = root; }
        // One round of dependent loads per level: the children scan also fetches every candidate's own node fields
        // (children ARE nodes), and the winner's are broadcast -- the next level starts without loading its node.
        const bool rh = node < ncached;
        int nc = TOP(nch, rh, node), cb = TOP(cbase, rh, node), nn = TOP(n, rh, node);
        double nq = TOP(q, rh, node);
        int16_t stop_proof = 0;                            // proof search: the proven node this descent arrived at
        while (true) {
            if (nc <= 0 || depth >= M0_MAX_DEPTH - 1) break;
            const double sq = sqrt((double)(nn > 1 ? nn : 1));
            const double eff = cpuct_at(c, depth);
            double best = -1e9;
            int bi = -1;
            int b_nch = 0, b_cb = 0, b_n = 0, b_vl = 0;
            double b_q = 0.0;
            Move b_mv = 0;
            bool root_rule = false;
            if constexpr (GUMBEL) root_rule = depth == 0;
            bool forced_root = false;                      // forced playouts: this level is the root of a search with the rule
            int n_sum = 0;                                 // ... and the root children's completed visits
            if constexpr (FORCED) {
                forced_root = forced_search && depth == 0;
                if (forced_root) {
                    int part = 0;
                    for (int i = lane; i < nc; i += 64) { const int ci = cb + i; part += TOP(n, ci < ncached, ci); }
                    n_sum = wave_sum_i(part);
                }
            }
            bool skip_won = false;                         // proof search: some child is not won for its mover -- those that are
            if constexpr (PROOF) {                         // cannot be the arg-max
                bool notwin = false;
                for (int i = lane; i < nc; i += 64) notwin = notwin || proof_state(PRF(cb + i)) != PROOF_WIN;
                skip_won = __any(notwin);
            }
            if (root_rule) {
                // every lane loads the picked child's fields: the broadcast below then reads them from any lane
                bi = gumbel_pick_child(gd, sg, gcnt, nc, gumbel_considered(g_m, g_n, g_done + s), lane);
                const int ci = cb + bi;
                const bool hit = ci < ncached;
                b_n = TOP(n, hit, ci); b_q = TOP(q, hit, ci); b_nch = TOP(nch, hit, ci); b_cb = TOP(cbase, hit, ci);
                b_mv = TOP(mv, hit, ci); b_vl = c.virtual_loss_active ? TOP(vl, hit, ci) : 0;
            } else {
                for (int i = lane; i < nc; i += 64) {
                    const int ci = cb + i;
                    const bool hit = ci < ncached;                  // the children of a node are one block: all lanes agree but at the edge
                    if constexpr (PROOF) { if (skip_won && proof_state(PRF(ci)) == PROOF_WIN) continue; }    // no draw is consumed
                    const int cn = TOP(n, hit, ci);
                    const double cq = TOP(q, hit, ci);
                    const int c_nch = TOP(nch, hit, ci), c_cb = TOP(cbase, hit, ci);
                    const Move m = TOP(mv, hit, ci);
                    const double cprior = TOP(prior, hit, ci);
                    const double qq = cn == 0 ? nq - c.fpu_reduction : cq;
                    const double u = eff * cprior * (sq / (1.0 + (double)cn));
                    double sc = qq + u;
                    if (c.no_instant_backtrack && depth >= 1) {
                        if (mv_from(m) == prev_to && mv_to(m) == prev_from) sc -= 0.01;
                    }
                    const int cvl = c.virtual_loss_active ? TOP(vl, hit, ci) : 0;
                    if (c.virtual_loss_active && c.virtual_loss > 0.0) sc -= (double)cvl * c.virtual_loss;
                    sc += (u01(seedj, ctrj + (uint64_t)i) - 0.5) * jit;
                    if constexpr (FORCED) { if (forced_root) sc = forced_root_score(c.forced_k, cprior, cn, cvl, n_sum, i, sc); }
                    if (sc > best) { best = sc; bi = i; b_nch = c_nch; b_cb = c_cb; b_n = cn; b_q = cq; b_mv = m; b_vl = cvl; }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const double ob = __shfl_xor(best, off);
                    const int oi = __shfl_xor(bi, off);
                    if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
                }
                ctrj += (uint64_t)nc;
                if constexpr (FORCED) { if (forced_root && lane == 0 && budget_score_is_forced(best)) gd->forced_descents++; }
            }
            if (bi < 0) bi = 0;
            const int child = cb + bi;
            // the lane that scanned child bi (i = lane + 64 k) holds its fields iff its own best is bi
            const int wl = bi & 63;
            nc = __shfl(b_nch, wl); cb = __shfl(b_cb, wl); nn = __shfl(b_n, wl); nq = __shfl(b_q, wl);
            const Move m = (Move)__shfl((int)b_mv, wl);
            const uint64_t k = tkey(pos);
            const bool irr = irreversible(pos, m);
            if (lane == 0) { pkey[depth] = k; pirr[depth] = irr ? 1 : 0; }
            make_move(pos, m);
            // the scanned in-flight count + 1 (no second load), and no barrier per level: nothing a level stores
            // (in-flight count, path, position keys) is read before the walk has ended
            const int vlw = __shfl(b_vl, wl);
            if (lane == 0 && c.virtual_loss_active) { A.vl[child] = vlw + 1; if (child < ncached) TC->vl[child] = vlw + 1; }
            prev_from = mv_from(m); prev_to = mv_to(m);
            node = child; ++depth;
            if (c.tt_merge) {
                // mcts.py:919: node = self._tt_get(board._transposition_key()) or best_child -- the walk continues from
                // the node registered LAST for this position; the edge child keeps the statistics its parent scores
                const int tn = tt_lookup(TK, TN, d.tt_cap, tt_key_of(pos), lane);
                if (tn >= 0 && tn != child) {
                    node = tn;
                    nc = A.nch[node]; cb = A.cbase[node]; nn = A.n[node]; nq = A.q[node];
                }
                if (lane == 0) epath[depth] = child;
            }
            if (lane == 0) path[depth] = node;
            if constexpr (PROOF) { stop_proof = PRF(node); if (stop_proof != 0) break; }
        }
        __syncthreads();
        int nlegal = 0;
        double tv = 0.0;
        bool tb_hit = false, term = false;
        if (PROOF && stop_proof != 0) {                  // a terminal sample with the value a table hit of that outcome has
            term = true;
            tv = proof_value(proof_state(stop_proof), c.draw_penalty);
        } else {
            nlegal = gen_legal_wave(pos, smoves, spseudo, lane);
            term = leaf_terminal(d, c, pos, nlegal, depth, pkey, pirr, H, hist_len, lane, tv, tb_hit);
        }
        if (tb_hit && lane == 0) gd->tb_leaves++;
        uint64_t ckey = 0;
        bool cached = false;
        if (!term && c.eval_cache && d.ec.sets > 0 && nlegal <= M0_EC_MAXLEGAL) {
            ckey = ec_key_of(pos);
            cached = ec_probe(d, gd, g, s, ckey, smoves, nlegal, lane);
        }
        emit_leaf(d, c, A, gd, S + s, LM + (size_t)s * M0_MAX_CHILDREN, pos, node, depth, smoves, nlegal, term, cached, ckey, lane);
        __syncthreads();                                 // path[] (lane 0) before the wave reads it
        if (term) {                                      // mcts.py:747-751: terminal leaves back up immediately
            // (the cached copies of the path's statistics follow)
            backprop(A, path, depth, tv, lane, c.tt_merge != 0, [&](int nd, int nn, double qq) {
                if (nd < ncached) { TC->n[nd] = nn; TC->q[nd] = qq; }
            });
            if constexpr (PROOF) {
                // the first visit of a terminal leaf (a proven one is never reached again): its proof, then its ancestors'
                const int16_t pv = stop_proof != 0 ? (int16_t)0 : leaf_proof(d, pos, nlegal, tb_hit);
                if (pv != 0) {
                    set_proof(node, pv);
                    proof_combine_up(A, path, depth, pv, proof_complete, lane, [&](int i) { return PRF(i); }, set_proof);
                }
            }
            __syncthreads();
            // Later descents of this launch read these nodes' statistics again, the uncached ones from the arena: drop this CU's
            // vector-L1 lines so that they come from L2, where the stores above are.  (Round 4: a load of the same addresses
            // issued right after the barrier returned the OLD values from time to time -- the lines were resident from the
            // children scan and a store does not refresh them at once; seen as run-to-run differences in whole games.)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if constexpr (PROOF) {
                if (PRF(root) != 0) { made = s + 1; break; }    // the root is proven: the search ends with this sample
            }
        }
    }
    if (reinfer) emit_root_value(d, gd, S, made, root, lane);
    if (lane == 0) { gd->ctr_jitter = ctrj; gd->nsamples = made + (reinfer ? 1 : 0); }
}
#undef PRF

// one instantiation per TreeCfg::mode, by SearchMode: the list both the dynamic-LDS attribute and the launch are taken from
using SelectKernel = void (*)(TreeDev, TreeCfg);
static constexpr SelectKernel SELECT_KERNELS[] = {select_kernel<MODE_PUCT>, select_kernel<MODE_GUMBEL>, select_kernel<MODE_PROOF>, select_kernel<MODE_BUDGET>};

hipError_t launch_select(const TreeDev& d, const TreeCfg& c, hipStream_t st) {
    static DeviceOnce once;
    hipError_t e = once.run([] {
        for (SelectKernel k : SELECT_KERNELS) {
            hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                M0_SEL_CACHE_BYTES);
            if (e1 != hipSuccess) return e1;
        }
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
    if ((unsigned)c.mode >= sizeof(SELECT_KERNELS) / sizeof(SELECT_KERNELS[0])) return hipErrorInvalidValue;
    if (is_proof(c) && (!d.t.proof || !d.proof_results)) return hipErrorInvalidValue;   // a proof search needs its node array
    hipLaunchKernelGGL(SELECT_KERNELS[c.mode], dim3(d.G), dim3(64), M0_SEL_CACHE_BYTES, st, d, c);
    return hipGetLastError();
}
