// Device-resident search trees: one arena pair per concurrent game, SoA node arrays so a
// node's children (contiguous block) load coalesced, one child per lane.
// Mirrors azchess/mcts.py Node (120-133) / _select (851-925) / _expand (135-225) /
// _backpropagate (946-953) / _add_dirichlet (955-992).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chess_core.h"
namespace m0 { struct TbSet; }   // tb_core.h
// deliberate: the C ABI already fixes M0_POLICY_SIZE (logits per batch row) and M0_PLANES (input planes); one definition
#include "../../include/m0_engine.h"
#include "gumbel_core.h"
#include "proof_core.h"
#include "budget_core.h"

#define M0_MAX_DEPTH 256      // path length cap (nodes)
#define M0_HIST_CAP 192       // reversible-move history window (<= 150 by the 75-move rule)
#define M0_MAX_CHILDREN 256
static_assert(M0_MAX_CHILDREN == m0::M0_GUMBEL_MAX_K, "gumbel_core.h and include/m0_gumbel.h count on 256 root children at most");
static_assert(M0_MAX_CHILDREN == m0::M0_BUDGET_MAX_K, "budget_core.h and include/m0_budget.h count on 256 root children at most");
constexpr int M0_NHWC_C = 32;          // channel stride of the fp16 NHWC network input (M0_PLANES used, the rest zero)

// The searches an engine can run: PUCT, the Gumbel root search (tree_gumbel.h), the proof search (tree_proof.h) and the self-play
// budget mix (tree_forced.h; at the root of a search with GameDev::forced).  All but MODE_PUCT exclude compat.tt_merge.
enum SearchMode : int { MODE_PUCT = 0, MODE_GUMBEL, MODE_PROOF, MODE_BUDGET };

struct TreeCfg {              // MCTSConfig fields the kernels read (mcts.py:61-107)
    double fpu_reduction;
    double draw_penalty;
    double virtual_loss;
    double selection_jitter;
    double cpuct;
    double cpuct_start, cpuct_end;
    int cpuct_plies;          // <=0: constant cpuct
    int use_c_base;
    double cpuct_c_base, cpuct_c_init;
    double dirichlet_alpha, dirichlet_frac;
    int legal_softmax;
    int enable_entropy_noise;
    int no_instant_backtrack;
    int virtual_loss_active;  // 1: apply the in-flight penalty as written (mcts.py:889-890, 922-923)
    int leaves_per_step;      // L = inference_batch_size per tree
    // compatibility switches (include/m0_engine.h, m0_selfplay_cfg)
    int tt_merge;             // mcts.py:919 + 1330-1346: children registered in a position table, select follows the table
    int raw_legal_priors;     // mcts.py:227-256 for non-root expansions
    int max_children;         // mcts.py:806-826
    double min_child_prior;
    int eval_cache;           // 1: leaf evaluations are looked up in / stored to the game's evaluation cache (EvalCache) and a leaf
                              //    reached twice in one pass shares one batch row
    SearchMode mode;          // set through mode_settable (selfplay_engine.h); launch_select runs its select_kernel, expand_kernel reads it
    m0_gumbel_cfg gumbel_cfg; // MODE_GUMBEL: the halving schedule's width and the constants of the improved policy
    double forced_k;          // MODE_BUDGET: forced playouts bring a visited root child up to sqrt(forced_k * prior * sum n) visits
};

M0_HD bool is_gumbel(const TreeCfg& c) { return c.mode == MODE_GUMBEL; }
M0_HD bool is_proof(const TreeCfg& c) { return c.mode == MODE_PROOF; }
M0_HD bool is_budget(const TreeCfg& c) { return c.mode == MODE_BUDGET; }

// select_kernel's cpuct_at (tree_select.hip) at depth 0, for the host: the constant the root's children were scored with
inline double cpuct_at_root(const TreeCfg& c) {
    if (c.use_c_base) return c.cpuct_c_init + log((1.0 + c.cpuct_c_base) / c.cpuct_c_base);
    return c.cpuct_plies <= 0 ? c.cpuct : c.cpuct_start;
}

// Per-game evaluation cache: what the network said about a position (value + the logits of its legal moves, in generation
// order), keyed by everything the network input and the expansion depend on (pieces, turn, castling rights, legal
// en-passant square, the two move counters as the planes encode them).  A repeated position -- a transposition inside the
// search, a position whose node was dropped with a discarded subtree -- is expanded from the cache instead of costing a
// network evaluation.  Same role as the reference's position table, which never evaluates a transposed node twice
// (mcts.py:919), and its nn_cache (mcts.py:44-59); results are unchanged because the 320-wide forward is bitwise batch
// invariant (a fresh evaluation would return the very same numbers).  4-way set associative, least recently used way replaced.
// A match engine (cfg.arena_eval_cache) keeps `sides` = 2 instances per game, one per network, each with its own clock:
// instance (game, GameDev::net_id) holds only what that network said, and the search it evaluates sees no other.
#define M0_EC_MAXLEGAL 64     // positions with more legal moves are not cached
#define M0_EC_WORDS 66        // payload floats per entry: value, nlegal (as int bits), 64 logits
struct EvalCache {
    uint64_t* keys;           // [G][sides][sets * 4], 0 = empty
    uint32_t* stamps;         // [G][sides][sets * 4] last use (the instance's clock, GameDev::cache_clock)
    float* payload;           // [G][sides][sets * 4][M0_EC_WORDS]
    float* hit_stage;         // [G][L + 1][M0_EC_WORDS] payload of this pass's hits (an insert of the same pass may evict the entry)
    int sets;                 // per instance, a power of two; 0 = cache off
    int sides;                // instances per game: 1, or 2 in a match engine (one per network)
};

// Per-game control block (host writes between steps, kernels update counters).
struct GameDev {
    m0::Pos root_pos;
    int root;                 // node index of the root (arena-relative)
    int next;                 // bump allocator
    int arena;                // 0/1: which arena half holds the tree
    int active;               // searching
    int sims_done, sims_target;
    int need_dirichlet;       // apply Dirichlet noise at the next select (run(): mcts.py:374-376)
    int root_q_from_v;        // expanding a reused-but-unexpanded root sets root.q = v (mcts.py:412-413)
    int flip_root_v;          // value_from_white && black to move (mcts.py:1182-1188, root eval only)
    int root_fresh;           // root is a brand-new Node (mcts.py:344-358) rather than a reused child
    int hist_len;
    int nsamples;             // samples produced by the last select
    int overflow;             // arena exhausted at least once
    int finished;             // sims_done >= sims_target after the last expand
    int root_n;
    double root_q;
    double root_v;            // network value of the last root evaluation
    uint64_t seed_jitter, seed_noise, seed_dir;
    uint64_t ctr_jitter, ctr_noise, ctr_dir;
    uint64_t evals;           // network evaluations consumed by this game (counted by the engine)
    int net_id;               // arena: which network evaluates this game's current search (0 / 1); self-play: 0
    int reinfer;              // evaluate the (reused) root once more at the first select of this search (mcts.py:359-371)
    // match engine with compat.tt_merge (TreeDev::tt_sides == 2): arena half s and table s belong to side s for the WHOLE game
    uint64_t cache_hits;      // leaf evaluations served by the evaluation cache
    uint32_t cache_clock[2];  // per cache instance (self-play: [0] only)
    int ec_clear;             // match engine: this slot starts a new game -- advance_kernel empties both of its caches
    int side_next[2];         // bump allocator of each side's half while the other side searches
    int root_found;           // advance_kernel: this search's root was found in the side's table (mcts.py:343, 359-371)
    uint64_t tb_leaves;       // leaves that select_kernel took from the endgame tablebases (TreeDev::tb_set), counted by lane 0
    // Gumbel root search: the game's stream (k draws per search), whether this search has drawn, and how often no root child
    // had the scheduled visit count (0 with a correct schedule)
    uint64_t seed_gumbel, ctr_gumbel;
    int gumbel_drawn;
    int gumbel_miss;
    // self-play budget mix: this search is a full one with forced playouts at its root (arm_search), and the descents the
    // forcing rule has decided in this slot, counted by lane 0
    int forced;
    uint64_t forced_descents;
};

enum SampleKind : int {
    SK_NONE = 0,
    SK_EVAL = 1,              // leaf: network evaluation, expansion, backup
    SK_ROOT_INIT = 2,         // unexpanded root: evaluation + expansion, no backup
    SK_TERMINAL = 3,          // terminal leaf, already backed up by select
    SK_ROOT_VALUE = 4,        // value only: re-evaluation of a reused root
    SK_CACHED = 5,            // leaf whose evaluation the evaluation cache served
    SK_SHARED = 6,            // the same leaf as an earlier sample of this pass (shares its batch row)
};
// the sample reserved a batch row of its own (its planes go to the network)
M0_HD bool sample_owns_row(int kind) { return kind == SK_EVAL || kind == SK_ROOT_INIT || kind == SK_ROOT_VALUE; }
// the sample's descent left in-flight counts on its path, released after the batch
M0_HD bool sample_holds_inflight(int kind) { return kind == SK_EVAL || kind == SK_TERMINAL || kind == SK_CACHED || kind == SK_SHARED; }

struct Sample {
    m0::Pos pos;              // leaf position
    int kind;                 // SampleKind
    uint64_t ckey;            // evaluation-cache key of the leaf (0: not cacheable / cache off)
    int leaf;
    int depth;                // path has depth+1 nodes
    int row;                  // network batch row
    int nlegal;               // legal moves of the leaf (list in TreeDev::leaf_moves), filled by select
};
static_assert(sizeof(Sample) == 104, "the host copies Sample arrays device-to-host: the layout must not move");

struct TreeArrays {           // each [G][2*cap]
    double* prior;
    double* w;
    double* q;
    int* n;
    int* vl;
    int* cbase;
    int16_t* nch;             // -1 not expanded
    uint16_t* mv;
    uint16_t* midx;
    int cap;                  // nodes per arena half
    int16_t* proof;           // proof search: state and plies packed (proof_core.h), 0 = not proven; null = mode off
};

struct RootResult {           // written when a search finishes
    int nchild;
    int root_n;
    double root_q;
    int child_node[M0_MAX_CHILDREN];
    int child_n[M0_MAX_CHILDREN];
    uint16_t child_mv[M0_MAX_CHILDREN];
    uint16_t child_idx[M0_MAX_CHILDREN];
    double child_prior[M0_MAX_CHILDREN];
    double child_q[M0_MAX_CHILDREN];
};

struct GumbelResult {         // Gumbel root search: written beside RootResult when a search finishes
    int pick;                 // the move: index into RootResult's children
    double v_mix;
    double pi[M0_MAX_CHILDREN];   // improved policy over the root children
    double gl[M0_MAX_CHILDREN];   // g + log(prior) of this search
};

struct ProofResult {          // proof search: written beside RootResult when a search finishes
    int state, plies;         // the root's, from the view of its side to move
    int pick;                 // the move: index into RootResult's children
    int16_t child[M0_MAX_CHILDREN];   // every root child's state and plies, packed, from the view of the child's side to move
};

struct TreeDev {
    TreeArrays t;
    GameDev* games;           // [G]
    Sample* samples;          // [G][L+1]
    int* paths;               // [G][L+1][M0_MAX_DEPTH]
    int* epaths;              // tt_merge: [G][L+1][M0_MAX_DEPTH] the edge children chosen at each level (virtual-loss owners)
    uint64_t* tt_keys;        // tt_merge: [G][tt_cap] position keys, 0 = empty (open addressing, linear probing)
    int* tt_nodes;            // tt_merge: [G][tt_cap] node registered LAST under the key
    int tt_cap;               // entries per table, a power of two
    EvalCache ec;
    int search_nodes;         // head-room a per-side half (tt_sides == 2) must have before a search starts there: the nodes one
                              // search can create (~48 per simulation incl. margin); with less the half starts over first
    int tt_sides;             // tables per game: 1, or 2 in a match engine with compat.tt_merge (one per side, kept all game:
                              // the reference keeps one MCTS object, hence one table, per side -- arena.py:157-158)
    uint16_t* leaf_moves;     // [G][L+1][M0_MAX_CHILDREN] legal moves of each sampled leaf, generation order
    uint64_t* hist;           // [G][M0_HIST_CAP]
    RootResult* results;      // [G]
    int* row_counter;         // [2]: rows reserved for network 0 / network 1 (arena); row index = net_row_base*net + count
    int net_row_base;         // first batch row of network 1's region (self-play: unused)
    _Float16* x0;             // network input NHWC [rows][64][M0_NHWC_C]
    const float* logits;      // [rows][M0_POLICY_SIZE]
    const float* values;      // [rows]
    int G;
    int L;
    const m0::TbSet* tb_set;  // endgame tablebases in device memory (m0_selfplay_set_search_tablebase); null = leaves are not probed
    int tb_max_pieces;        // ... for leaves with at most this many men
    double* gumbel_gl;        // Gumbel root search: [G][M0_MAX_CHILDREN] g + log(prior) of the running search; null = mode off
    GumbelResult* gumbel_results;   // [G]
    ProofResult* proof_results;     // proof search: [G]; null = mode off
};

hipError_t launch_select(const TreeDev& d, const TreeCfg& c, hipStream_t st);
hipError_t launch_expand(const TreeDev& d, const TreeCfg& c, hipStream_t st);
// What advance_kernel makes the new root of a game: a value >= 0 keeps that child of the old root with its subtree, a negative
// one is a RootMode.  The two table modes exist with tt_sides == 2 only.
enum RootMode : int {
    ROOT_FRESH = -1,            // a fresh tree (and an empty position table)
    ROOT_FROM_SIDE_TABLE = -2,  // a later search of a game: the root is looked up in the side's table
    ROOT_FIRST_OF_GAME = -3,    // the first search of a game: both tables are cleared first, then a new root
};
hipError_t launch_advance(const TreeDev& d, const int* game_ids_dev, const int* child_slots_dev, int count, hipStream_t st);
// Re-root by moves (tree_reroot.hip).  Entry j: slot slots_dev[j] follows the nmoves_dev[j] <= M0_REROOT_MAX_MOVES moves
// moves_dev[j][0..] (from | to<<6 | promo<<12, as a node's `mv`) from its root through expanded children and keeps the subtree
// of the node it reaches, compacted into the other arena half; where the walk fails the slot gets a fresh root, as ROOT_FRESH.
// out_dev[j]: kept 0/1 and, when kept, the visit count and q of the new root.  The slots must not be searching.
#define M0_REROOT_MAX_MOVES 8
struct RerootOut { int32_t kept, n; double q; };
hipError_t launch_reroot_moves(const TreeDev& d, const int* slots_dev, const int* nmoves_dev, const int* moves_dev /*[count][8]*/,
                               int count, RerootOut* out_dev, hipStream_t st);

// test hooks: position-wise encode / legal move / index kernels (encoding.py on device)
hipError_t launch_encode_positions(const m0::Pos* pos_dev, int n, float* planes_f32_dev /*[n][M0_PLANES][64]*/,
                                   _Float16* nhwc_dev /*[n][64][M0_NHWC_C] or null*/, uint8_t* mask_dev /*[n][M0_POLICY_SIZE]*/,
                                   int32_t* nlegal_dev, uint16_t* moves_dev /*[n][256]*/, int32_t* idx_dev /*[n][256]*/,
                                   hipStream_t st);

// The way back (planes_decode.h): rows of planes f32 [n][M0_PLANES][64] and, nullable, masks u8 [n][M0_POLICY_SIZE] -> per row
// the position (zeroed unless the status is M0_DECODE_OK or M0_DECODE_MASK_MISMATCH), M0_DECODE_* status and flags, legal moves.
hipError_t launch_decode_planes(const float* planes_dev, const uint8_t* mask_dev, int n, m0::Pos* pos_dev, int32_t* status_dev,
                                int32_t* flags_dev, int32_t* nlegal_dev, hipStream_t st);

// Results of the analysis engine (analysis_kernels.hip).  lines: M0_AN_MAX_LINES per entry, nlines: lines written per entry.
// launch_analysis_lines: entry j = the finished search of slot slots_dev[j]: its root children by visits (ties by move order)
// with the most-visited line behind each, at most pv_len moves.
// proof_dev (proof search; null: the ranking above): per entry a m0_proof_lines -- the lines are then ranked as
// m0_tb_root_lines ranks table roots (winning moves, shortest first; unproven and drawn moves by visits; losing moves, longest
// first) and the variation behind a line follows the proof search's pick at every proven node.
hipError_t launch_analysis_lines(const TreeDev& d, const int* slots_dev, int count, int multipv, int pv_len,
                                 m0_analysis_line* lines_dev, int* nlines_dev, hipStream_t st, m0_proof_lines* proof_dev = nullptr);
// launch_root_children: entry j = the finished search of slot slots_dev[j]: (policy index, visits) of every root child in
// move-generation order from the slot's RootResult, zero-padded to M0_MAX_CHILDREN, and their number.
hipError_t launch_root_children(const TreeDev& d, const int* slots_dev, int count, int32_t* policy_idx_dev, int32_t* visits_dev,
                                int32_t* nchild_dev, hipStream_t st);
// launch_policy_lines: entry r = batch row r of a forward over positions that launch_encode_positions prepared (nlegal, moves,
// idx): the legal moves by legal-softmax prior (ties by move order) and the row's value.
hipError_t launch_policy_lines(const float* logits_dev, const float* values_dev, const int32_t* nlegal_dev, const uint16_t* moves_dev,
                               const int32_t* idx_dev, int rows, int multipv, m0_analysis_line* lines_dev, int* nlines_dev,
                               float* value_out_dev, hipStream_t st);

// SSL training targets for recorded positions: out f32 [n][17][64] (piece 13, threat, pin, fork, control)
hipError_t launch_ssl_targets(const m0::Pos* pos_dev, int n, float* out_dev, hipStream_t st);
// ... and for stored planes f32 [n][19][64]: status 0, or 1 for a row the targets cannot be taken from, whose `out` stays unwritten
hipError_t launch_ssl_targets_planes(const float* planes_dev, int n, float* out_dev, int32_t* status_dev, hipStream_t st);

// Replay of written games (replay_kernels.hip, patterns: san_match.h), one wave per game.  Game g owns rows offsets[g] ..
// offsets[g+1] of patterns and of the per-ply outputs and writes the first plies[g] of them: the position before each resolved
// move (input of launch_encode_positions / launch_ssl_targets), the move, its policy index, the legal-move count and the side
// to move.  status: REPLAY_*; end_flags: REPLAY_END_* of the position after the last resolved move.
hipError_t launch_replay_games(const m0::Pos* start_dev, const uint32_t* patterns_dev, const int32_t* offsets_dev /*[n_games+1]*/,
                               int n_games, int max_plies, m0::Pos* pos_dev, uint16_t* moves_dev, int32_t* policy_idx_dev,
                               int32_t* nlegal_dev, int8_t* turn_dev, int32_t* plies_dev, int32_t* status_dev,
                               int32_t* end_flags_dev, hipStream_t st);
