/* libm0engine — C ABI of the MI355X-native Matrix0 self-play hot path.
 *
 * Drop-in boundary for two duck-typed seams of the reference (lukifer23/Matrix0):
 *
 *   1. inference backend  obj.infer_np(np.float32[B,19,8,8]) -> (np.float32[B,4672], np.float32[B])
 *        azchess/mcts.py:618-621, 1021-1023; azchess/selfplay/inference.py:585-645 (InferenceClient.infer_np)
 *        -> m0_net_infer
 *   2. worker entry       selfplay_worker(proc_id, cfg_dict, ckpt_path, games, q, shared_memory_resource)
 *        azchess/selfplay/internal.py:94-95 (called from orchestrator.py:494, selfplay/__main__.py:68)
 *        -> m0_selfplay_create / m0_selfplay_step / m0_selfplay_poll
 *
 *   plus the pure functions of azchess/encoding.py, exposed position-wise for parity tests and
 *   for callers that keep python-chess:  m0_encode_fens, m0_move_to_index_fen.
 *
 * Conventions: every function returns 0 on success or a negative code; the message is
 * available from m0_last_error() (thread-local).  After M0_ERR_HIP from a call on a network or
 * engine handle every later device call on that handle returns M0_ERR_HIP with the first
 * failure's message and starts nothing on the GPU: destroy the handle.  (Calls that only read
 * host state -- m0_selfplay_stats_get, _poll, _running -- still answer.)  No exception crosses the ABI.  All buffers
 * are caller-allocated host memory unless a parameter says "_dev".  Handles are opaque.
 * The library never falls back to a CPU path: without a HIP device m0_net_create fails.
 */
#ifndef M0_ENGINE_H
#define M0_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M0_OK 0
#define M0_ERR_INVALID (-1)
#define M0_ERR_UNSUPPORTED (-2)
#define M0_ERR_HIP (-3)
#define M0_ERR_STATE (-4)
#define M0_ERR_NONFINITE (-5) /* NaN/Inf in network output: mcts.py:1165-1177 raises */

#define M0_POLICY_SIZE 4672
#define M0_PLANES 19

/* activation codes */
#define M0_ACT_RELU 1
#define M0_ACT_SILU 2
#define M0_ACT_LEAKY 3

/* ssl task bits (order = NPZ field order of selfplay/internal.py:647-651) */
#define M0_SSL_PIECE 1
#define M0_SSL_THREAT 2
#define M0_SSL_PIN 4
#define M0_SSL_FORK 8
#define M0_SSL_CONTROL 16

/* NetConfig, azchess/model/resnet.py:247-282 (inference-relevant fields only). */
typedef struct m0_net_cfg {
    int planes;               /* 19 */
    int channels;             /* 320 */
    int blocks;               /* 24 */
    int attention;            /* bool */
    int attention_heads;      /* 20 */
    int attention_every_k;    /* 3 */
    int attention_relbias;    /* bool */
    float attention_unmasked_mix; /* 0.2 */
    int se;                   /* bool */
    float se_ratio;           /* 0.25 */
    int chess_features;       /* bool */
    int piece_square_tables;  /* bool */
    int policy_factor_rank;   /* 128; 0 = dense policy_fc */
    int norm_group;           /* 1 = GroupNorm (supported); 0 = BatchNorm (unsupported on the HIP path) */
    int activation;           /* M0_ACT_SILU | M0_ACT_RELU */
    int value_activation;     /* M0_ACT_SILU | M0_ACT_LEAKY | M0_ACT_RELU */
    int preact;               /* bool; only preact=1 is supported on the HIP path */
    int self_supervised;      /* bool */
    int ssl_tasks;            /* bitmask of M0_SSL_* */
    int infer_attention_stride; /* >=1 */
} m0_net_cfg;

typedef struct m0_net m0_net;

const char* m0_last_error(void);
const char* m0_version(void);
/* hipGetDeviceCount: MI355X visible to this process (0 when there is none; never an error). */
int m0_device_count(void);

/* ---- network (seam 1) ---- */
m0_net* m0_net_create(const m0_net_cfg* cfg, int hip_device);
void m0_net_destroy(m0_net* net);
/* One call per state-dict key (reference key names, resnet.py state_dict()); dtype 0 = f32, 1 = f16.
 * Unknown keys are ignored (load_state_dict(strict=False), selfplay/internal.py:172-174). */
int m0_net_load_weight(m0_net* net, const char* name, const void* data, int dtype, const int64_t* shape, int ndim);
/* Repack to kernel layouts (fp16 MFMA operand tiles), upload; missing keys are an error. */
int m0_net_finalize(m0_net* net);
/* infer_np: planes f32 [B,19,8,8] -> policy logits f32 [B,4672], value f32 [B];
 * ssl (nullable) f32 [B, ssl_channels, 8, 8] in task order piece(13) threat(1) pin(1) fork(1) control(3).
 * Re-entrant: calls on one net are serialised internally (several MCTS objects may share a backend,
 * tests/test_stress.py:221-266).  NaN/Inf in the outputs -> M0_ERR_NONFINITE. */
int m0_net_infer(m0_net* net, const float* planes, int B, float* policy, float* value, float* ssl);
/* Trunk tap (per-layer parity tests; not used by the engines).  Steps of a forward in execution order: 0 = stem (+ positional
 * encoding), 1 = piece-square conv, 2 = interaction conv, 3 + i = tower layer i (residual and attention blocks as the tower
 * lists them).  *steps = their number, *width = the trunk's width in memory (320 for a 288-channel network). */
int m0_net_tap_info(const m0_net* net, int* steps, int* width);
/* m0_net_infer with the tap armed at `step`: besides policy, value and ssl (nullable), `stream` receives the residual stream
 * right after that step and `second` the pre-activated input of the next residual block, act(GroupNorm(stream; its bn1)), when
 * the step wrote one (*has_second = 1; else 0 and `second` is zeroed): both f32 [B][64][width], the kernels' fp16 values
 * widened exactly.  A step the configuration does not have, or an attention layer the inference stride skips, returns the
 * stream of the step before it and no second output.  The tap is off again when the call returns. */
int m0_net_infer_tap(m0_net* net, const float* planes, int B, int step, float* policy, float* value, float* ssl,
                     float* stream, float* second, int* has_second);
int m0_net_ssl_channels(const m0_net* net);
int64_t m0_net_param_count(const m0_net* net);
double m0_net_flops_per_position(const m0_net* net, int with_ssl);
/* Timed forward on synthetic resident inputs (bench/roofline): runs `iters` forwards of batch B on the
 * net's stream and returns the mean milliseconds per forward measured with HIP events on that stream. */
int m0_net_bench_forward(m0_net* net, int B, int iters, int with_ssl, float* ms_per_forward);
/* Roofline instrumentation of the dominant kernel (3x3 C->C implicit-GEMM conv): when enabled, every launch is
 * bracketed by HIP events on the launch stream.  get: accumulated milliseconds, algorithmic FLOP
 * (2 * rows * Cout * Cin * 9 per launch) and launches since the last reset. */
int m0_net_profile_enable(m0_net* net, int on);
int m0_net_profile_get(m0_net* net, double* conv_ms, double* conv_flop, int64_t* launches, int reset);
/* Of those, the milliseconds and launches of the convs that also carry a fused block tail (conv2 of every residual
 * block, the interaction conv); call before a resetting m0_net_profile_get. */
int m0_net_profile_get_tail(m0_net* net, double* tail_ms, int64_t* tail_launches);


/* ---- optional weight broadcast over RCCL / xGMI (the reference has no counterpart: its workers each read the
 * checkpoint, selfplay/internal.py:150-190).  One process per GPU.  Rank 0 calls m0_dist_unique_id and ships the 128 bytes to the
 * other ranks by any out-of-band means (a file, a socket, MPI); every rank calls m0_dist_create (collective: it returns when all
 * `world` ranks have joined).  m0_net_broadcast_weights (collective) overwrites every packed device buffer of a FINALIZED network
 * with the root's: the other ranks finalize a network of the same configuration first, with any weights of the right shapes;
 * networks of different configurations are refused before anything is sent.  librccl is loaded at the first call; without it the
 * functions fail with M0_ERR_UNSUPPORTED / NULL.  (matrix0_amd/dist.py does the same through torch.distributed.) */
typedef struct m0_dist m0_dist;
int m0_dist_unique_id(void* id128);
m0_dist* m0_dist_create(int rank, int world, const void* id128, int hip_device);
void m0_dist_destroy(m0_dist* d);
int m0_dist_rank(const m0_dist* d);
int m0_dist_world(const m0_dist* d);
int m0_net_broadcast_weights(m0_net* net, m0_dist* d, int root);

/* ---- position-wise azchess/encoding.py on the device (batched) ----
 * encode_board (encoding.py:11-46), MoveEncoder.get_legal_actions (:231-243), move_to_index (:80-150).
 * fens: n NUL-terminated strings.  Outputs nullable:
 *   planes f32 [n,19,8,8]; mask u8 [n,4672]; nlegal i32 [n];
 *   moves u16 [n,256] (from | to<<6 | promo<<12, promo 1..4 = N,B,R,Q) in legal_moves order; idx i32 [n,256]. */
int m0_encode_fens(int hip_device, const char* const* fens, int n, float* planes, uint8_t* mask, int32_t* nlegal,
                   uint16_t* moves, int32_t* idx);
/* The network's own input image of the same positions: fp16 bits, NHWC [n][64 squares][32 channels] (19 used, square
 * n = row*8+col of the reference tensor), written by the device function the search's select kernel calls for every
 * leaf (csrc/movegen_wave.h encode_nhwc) -- i.e. encode_board (encoding.py:11-46) as the timed path evaluates it. */
int m0_encode_fens_nhwc(int hip_device, const char* const* fens, int n, uint16_t* nhwc);
/* MoveEncoder.decode_move (encoding.py:174-229): policy index -> UCI (auto-queen, legal fallbacks); "0000" = null move.
 * uci_out: at least 6 bytes. */
int m0_decode_move_fen(int hip_device, const char* fen, int action_idx, char* uci_out);
/* ChessSSLAlgorithms.create_enhanced_ssl_targets (azchess/ssl_algorithms.py:519-543) on the device:
 * out f32 [n,17,8,8] = piece one-hot (13) | threat | pin | fork | control, tensor orientation. */
int m0_ssl_targets_fens(int hip_device, const char* const* fens, int n, float* out);
/* move_to_index for one (fen, uci): raises M0_ERR_INVALID for an illegal move (ValueError in the reference). */
int m0_move_to_index_fen(int hip_device, const char* fen, const char* uci, int32_t* idx);

/* ---- search + self-play (seam 2) ---- */
/* MCTSConfig (azchess/mcts.py:61-107) + the selfplay/draw keys of config.yaml the worker reads
 * (azchess/selfplay/internal.py:269-310, 348-381; azchess/draw.py). */
typedef struct m0_selfplay_cfg {
    /* mcts */
    int num_simulations;          /* selfplay.num_simulations overrides mcts.num_simulations (internal.py:291) */
    double cpuct, cpuct_start, cpuct_end;
    int cpuct_plies;              /* <=0 or missing start/end: constant cpuct */
    int use_c_base; double cpuct_c_base, cpuct_c_init;
    double dirichlet_alpha, dirichlet_frac;
    int dirichlet_plies;          /* <0: always */
    double selection_jitter, fpu_reduction, draw_penalty, virtual_loss;
    int legal_softmax, enable_entropy_noise, no_instant_backtrack, value_from_white;
    int inference_batch_size;     /* leaves collected per tree and step (<= 96 in the reference) */
    double playout_random_frac;
    /* selfplay */
    int max_game_len, min_resign_plies, opening_random_plies;
    double resign_threshold; int resign_window, resign_consecutive_bad; double resign_min_entropy, resign_value_margin;
    double temperature_start, temperature_end; int temperature_moves;
    int low_visit_threshold;
    /* draw adjudication (draw.py) */
    int draw_enabled, draw_min_plies, draw_window, draw_min_unique, draw_halfmove_cap, draw_material_threshold, draw_stalemate;
    /* engine */
    int concurrent_games;         /* trees resident on this GPU */
    int total_games;              /* games to play (<=0: unbounded, slots restart forever) */
    int first_game_index;         /* global index of this engine's first game (multi-GPU sharding) */
    int arena_nodes;              /* nodes per arena half and game (0 = default: (1.3 * num_simulations + 64) * 96); a value
                                     below 4096, the default included, is raised to 4096.  A search that needs more: see
                                     "A full node arena" below */
    uint64_t seed;                /* cfg["seed"] (1234) */
    int virtual_loss_active;      /* 1 = apply mcts.py:889-890/922-923 as written (the reference never does) */
    int ssl_in_forward;           /* run the SSL heads in every leaf evaluation (BASELINE config 4) */
    int ssl_targets;              /* generate ssl_* target maps for every recorded ply (selfplay/internal.py:460-482) */
    int record_games;             /* keep s/pi/legal_mask per ply for m0_selfplay_poll */
    /* evaluation matches (azchess/arena.py:59-126), m0_arena_create only */
    int arena_mode;               /* set by m0_arena_create */
    double arena_temp;            /* move choice: softmax(log(visits+1e-8)/temp) for the first arena_temp_plies plies ... */
    int arena_temp_plies;         /* ... then (or with temp <= 1e-3) the most visited move, first maximum in move order */
    /* compatibility switches (reference behaviours the default engine deviates from; 0 = engine default) */
    int fresh_tree_per_move;      /* 1 = every move starts from a brand-new root (what the reference does with MCTS._tt_get
                                     patched out, the mode tests/golden/ref_worker_*.npz were played in); 0 = keep the played
                                     child's subtree */
    int tt_merge;                 /* 1 = transposition merging inside a search as mcts.py:919 + :1330-1346 (search graph is a DAG).
                                     Self-play: the table lives for one search.  Match engine (m0_arena_create*): one table per
                                     side for the WHOLE game, roots looked up in it, as the reference's per-side MCTS objects do
                                     (arena.py:157-158); arena_nodes must then hold all nodes a side creates in a game */
    int raw_legal_priors;         /* 1 = Node._expand_with_legal_priors (mcts.py:227-256): non-root priors = legal logits / their sum */
    int max_children;             /* MCTS._prune_children (mcts.py:806-826): keep the top-K children by prior; 0 = off */
    double min_child_prior;       /* ... after dropping children with prior < this; 0 = off */
    int root_reinfer;             /* 1 = re-evaluate a reused root as mcts.py:359-371 does (nn_cache of 10 000 positions) */
    /* per-game evaluation cache (csrc/tree.h EvalCache): a leaf whose position was evaluated before -- a transposition inside
     * the search, a position of a discarded subtree -- is expanded from the stored value + legal logits instead of going
     * through the network again.  Games are unchanged (the forward is bitwise batch invariant on the 320-wide path).  Active
     * only with legal_softmax = 1 and without tt_merge / raw_legal_priors.  A hit must also match the stored legal-move count
     * and a checksum of the legal moves; otherwise it is served as a miss.  0 = off.  This field is for self-play engines: a
     * match engine (m0_arena_create*) ignores it -- two networks alternate in one game slot and the key carries no network
     * id -- and has a switch of its own, arena_eval_cache below, which gives every network its own cache. */
    int eval_cache;
    int eval_cache_entries;       /* entries per game (rounded up to a power of two, 4-way sets); 0 = 16384 */
    /* 1 = a pass of >= 2048 rows on the 320-wide network is evaluated as a main part that is a whole number of rounds of
     * workgroups (a multiple of 1024 boards) plus a tail (< 1024 boards) on a second instance over the same weights, on its own
     * stream, at the same time: the tower is board-local, and the tail's workgroups run on the CUs the main launches' partial last
     * round would leave idle.  Results are unchanged (the forward is bitwise batch invariant).  Self-play engines only.
     * 2 = a pass of >= 4096 rows as two halves (the first a multiple of 1024 boards) on the two instances side by side: one
     * half's attention blocks then run beside the other half's power-bound convs instead of behind them (+1.3 % games/s
     * measured); per-launch kernel timings of the two halves overlap.  0 = off (default). */
    int tail_split;
    /* Match engines only (ignored by self-play engines).  1 = every game slot owns TWO evaluation caches of eval_cache_entries
     * entries each, one per network, addressed by the network that evaluates the current search: a position evaluated by
     * network A is never served to a search of network B.  A side's cache lives for the whole game, across that side's
     * fresh-tree searches (its new root's subtree was evaluated by the same network two plies earlier), and both are emptied
     * when the slot starts a new game (colours, hence networks, swap).  Same conditions and hit criteria as eval_cache;
     * outside them the switch is ignored.  Games are unchanged on the bitwise batch-invariant 320-wide path.  0 = off. */
    int arena_eval_cache;
    /* Match engines only.  1 = with an opening book (m0_selfplay_set_openings) games 2k and 2k+1 start from the SAME book
     * position, so every opening is played once with each network as White.  The position is drawn from the counter stream
     * keyed by (seed, k, a purpose of its own), not from either game's stream: the pairing does not depend on the slot or the
     * order in which games start.  0 = every game draws its opening from its own stream, as a self-play engine does. */
    int arena_paired_openings;
} m0_selfplay_cfg;

typedef struct m0_selfplay m0_selfplay;

typedef struct m0_selfplay_stats {
    uint64_t steps, evals, sims, plies, games_finished, games_started;
    double ms_total, ms_net, ms_tree, ms_host;   /* accumulated wall (host) and device (HIP events) times */
    uint64_t arena_overflows;     /* searches that finished with a refused expansion ("A full node arena" below) or, in a game,
                                     without a visit; counted once per search by every way of driving one (m0_selfplay_step,
                                     m0_selfplay_ext_*, m0_search_expand, m0_analysis_*) */
    uint64_t ssl_dropped;         /* finished games emitted WITHOUT ssl_* targets because their staging buffers could not grow */
    uint64_t evals_cached;        /* leaf evaluations served by the evaluation cache (not counted in `evals`) */
    int active_games;
    uint64_t rows_tail;           /* of `evals`: rows evaluated by the tail instance (cfg.tail_split) */
} m0_selfplay_stats;

/* One finished game = one NPZ shard of the reference (selfplay/internal.py:628-651). Arrays stay valid
 * until m0_game_record_free. */
typedef struct m0_game_record {
    int game_index, moves, resigned, resigner /*0 none 1 W 2 B*/, draw, total_plies /*incl. opening*/;
    float result;                 /* z, White POV */
    float avg_policy_entropy, avg_sims;
    double secs;
    const float* s;               /* [T,19,8,8] */
    const float* pi;              /* [T,4672] */
    const float* z;               /* [T] */
    const uint8_t* legal_mask;    /* [T,4672] */
    const float* search_values;   /* [T] root_q per ply */
    const uint16_t* played;       /* [total_plies] moves incl. opening plies */
    const float* ssl;             /* [T,17,8,8] piece(13) threat pin fork control, or NULL */
    void* owner;
    const char* start_fen;        /* the opening-book position the game started from, as given to m0_selfplay_set_openings;
                                     NULL = the initial position.  `played` holds the moves from there on */
} m0_game_record;

m0_selfplay* m0_selfplay_create(m0_net* net, const m0_selfplay_cfg* cfg);
void m0_selfplay_destroy(m0_selfplay* sp);
/* Run `steps` search steps (select -> network -> expand/backup over all resident games), playing moves,
 * finishing and restarting games as searches complete. */
int m0_selfplay_step(m0_selfplay* sp, int steps);
int m0_selfplay_stats_get(m0_selfplay* sp, m0_selfplay_stats* out);
/* Pop one finished game; returns 1 if a record was written, 0 if none pending, <0 on error. */
int m0_selfplay_poll(m0_selfplay* sp, m0_game_record* out);
void m0_game_record_free(m0_game_record* rec);
/* 1 while games remain to be played or are in flight. */
int m0_selfplay_running(m0_selfplay* sp);
/* Opening book (selfplay/internal.py:34-69 load_opening_book / get_opening_position): every new game starts from one of
 * these positions, chosen with the game's own stream as random.choice(OPENING_BOOK) would; n = 0 clears the book
 * (games start from the initial position).  Call before the first step.  A match engine takes a book too (the reference's
 * eval.openings_pgn): cfg->max_game_len then counts the plies played from the book position, and with
 * cfg->arena_paired_openings the two games of a pair share their position. */
int m0_selfplay_set_openings(m0_selfplay* sp, const char* const* fens, int n);
/* The self-play step split at the network, for an external evaluator behind the reference's infer_np seam (net may be
 * NULL): ext_select runs select for all resident games and returns the leaf planes f32 [rows,19,8,8]; ext_expand takes
 * logits f32 [rows,4672] and values f32 [rows], expands / backs up, and does the host part of the step (moves, game
 * ends, restarts) exactly as m0_selfplay_step does.  Parity tests play whole games against golden files this way. */
/* max_rows must be >= concurrent_games * (inference_batch_size + 1) (checked before anything runs). */
int m0_selfplay_ext_select(m0_selfplay* sp, int* rows, float* planes, int max_rows);
int m0_selfplay_ext_expand(m0_selfplay* sp, const float* logits, const float* values, int rows);
/* The network batch the last select (m0_selfplay_ext_select / m0_search_select) wrote on the device: fp16 bits
 * [rows][64][32], row order = the planes rows of that call.  This is what m0_selfplay_step feeds the network. */
int m0_selfplay_last_batch_nhwc(m0_selfplay* sp, uint16_t* nhwc, int max_rows, int* rows);

/* Evaluation match between two networks (azchess/arena.py:59-126 _arena_run_one_game, :305 play_match): game i is played
 * with net_a as White when i is even.  Every search of a game is evaluated by the network of the side to move; each
 * move starts a fresh tree, unless cfg->tt_merge asks for the reference's own structure: one transposition table per side
 * kept for the whole game (arena.py:157-158 keeps one MCTS object per side), roots looked up in it.  With
 * cfg->arena_eval_cache a fresh-tree match engine keeps one evaluation cache per network and game, so what a side's previous
 * search evaluated is not evaluated again (cfg->eval_cache itself stays ignored here); m0_selfplay_stats.evals_cached counts
 * the hits.  Games start from the initial position or from an opening book (m0_selfplay_set_openings,
 * cfg->arena_paired_openings).  The game ends on board.is_game_over(claim_draw=True), on
 * cfg->max_game_len plies or on draw adjudication (draw.py); no resignation.  Step / poll / stats / destroy with the
 * m0_selfplay_* functions; a record's `played` holds the moves, `result` the outcome from White's point of view
 * (0 for unfinished or adjudicated games, as the reference scores them 1/2-1/2). */
m0_selfplay* m0_arena_create(m0_net* net_a, m0_net* net_b, const m0_selfplay_cfg* cfg);
/* The same match engine without networks, for external evaluators behind the reference's infer_np seam (golden tests replay
 * the reference's arena games this way): m0_arena_ext_select returns the leaves of network A's searches and of network B's
 * separately (planes f32 [rows,19,8,8] each; max_rows >= concurrent_games * (inference_batch_size + 1) for both buffers),
 * m0_arena_ext_expand takes the two evaluators' answers and finishes the step exactly as m0_selfplay_step does.  Leaves
 * served by cfg->arena_eval_cache are not handed to the evaluators. */
m0_selfplay* m0_arena_create_ext(const m0_selfplay_cfg* cfg);
int m0_arena_ext_select(m0_selfplay* sp, int* rows_a, int* rows_b, float* planes_a, float* planes_b, int max_rows);
int m0_arena_ext_expand(m0_selfplay* sp, const float* logits_a, const float* values_a, int rows_a, const float* logits_b,
                        const float* values_b, int rows_b);
/* PGN output of arena games (arena.py:281-303 uses chess.pgn): standard algebraic notation, python-chess Board.san().
 * m0_san_legal_fen: the legal moves of `fen` in legal_moves order (moves u16[256]) with their SAN (san char[256][8],
 * NUL-padded).  m0_san_game: movetext "1. e4 e5 2. Nf3 ..." of a game from the start position (moves as in
 * m0_game_record.played); returns its length.  m0_san_game_fen: the same for a game that starts from `fen`
 * (m0_game_record.start_fen), move numbers following the FEN as python-chess writes them: "12... Nf6 13. e4" when Black
 * moves first. */
/* arena.py:73-106 move choice over a visit list in move order; u = the uniform np.random.choice would draw. */
int m0_arena_choose_move(const int32_t* visits, int n, double temp, int ply, int temp_plies, double u);
int m0_san_legal_fen(const char* fen, uint16_t* moves, char* san, int* nlegal);
int m0_san_game(const uint16_t* moves, int n, char* out, int cap);
int m0_san_game_fen(const char* fen, const uint16_t* moves, int n, char* out, int cap);
/* Board.fen() after pushing `n` legal moves (UCI) on the position `fen` (python-chess semantics: cleaned castling rights, the
 * en-passant square only when such a capture is legal); M0_ERR_INVALID for an illegal move.  Host function (no GPU): the PGN
 * opening-book reader (selfplay/internal.py:39-63) and FEN-addressed callers are built on it. */
int m0_fen_after(const char* fen, const char* const* ucis, int n, char* fen_out, int cap);

/* ---- split-step search (external evaluator / parity tests): net may be NULL ----
 * m0_search_begin: reset slot g to `fen` (history-less), sims simulations, optional Dirichlet.
 * m0_search_select: run select for all active slots; returns rows; planes f32 [rows,19,8,8] of the leaves.
 * m0_search_expand: feed logits f32 [rows,4672] and values f32 [rows]; expand + backup.
 * m0_search_result: visits/moves/indices/priors/q of the root children after the search. */
int m0_search_begin(m0_selfplay* sp, int g, const char* fen, int sims, int dirichlet, int game_uid);
int m0_search_select(m0_selfplay* sp, int* rows, float* planes, int max_rows);
int m0_search_expand(m0_selfplay* sp, const float* logits, const float* values, int rows);
int m0_search_result(m0_selfplay* sp, int g, int* nchild, int32_t* child_n, uint16_t* child_mv, int32_t* child_idx,
                     double* child_prior, double* child_q, double* root_q, int* root_n, int* finished);
/* play child slot `slot` of the finished search in g and keep its subtree (tree reuse across moves) */
int m0_search_advance(m0_selfplay* sp, int g, int slot, int sims, int dirichlet);

/* ---- A full node arena ----
 * A slot's tree lives in one half of its arena: arena_nodes nodes (at least 4096).  The root is node 0; an expansion takes one
 * block of consecutive nodes, one per child it keeps after pruning (max_children / min_child_prior), behind the last block.  A
 * search over a kept subtree (tree reuse, m0_search_advance) starts with that subtree copied whole into the other half, children
 * without visits included.
 * An expansion whose block does not fit (nodes in use + block > arena_nodes) is refused.  The test is per expansion: a later
 * leaf with a smaller block may still fit.  After a refusal
 *   - the leaf stays an unexpanded leaf without children; a later descent that reaches it evaluates it and tries again;
 *   - the sample is otherwise an ordinary one: its value is backed up along the path, the simulation counts (the root
 *     children's visits still sum to the simulations run, the search still ends after `sims` of them) and the evaluation
 *     counts in `evals` / `evals_cached`;
 *   - whatever the priors drew from the game's entropy-noise stream before the refusal stays drawn, once per attempt -- with
 *     the evaluation cache too, where a leaf reached again within the pass shares the first sample's row and tries again
 *     from it: games are the same with the cache on and off in a full arena as well;
 *   - the search's overflow flag is set.  It is per search: a fresh root and a kept subtree both clear it, and expansion goes
 *     on in the other half.  It is what m0_analysis_result.overflow reports and what stats.arena_overflows counts.
 * Nothing is written outside the half.  The root's own expansion always fits (1 + 218 < 4096).  The table mode (tt_merge in a
 * match engine) starts a side's half over before a search that might not fit instead (arena_nodes above). */

/* ---- batched position analysis (the reference's MCTS.run(board) for a list of arbitrary positions) ----
 * An analysis engine plays no games: positions are submitted with an id, searched in the engine's tree slots on the device
 * (select -> network -> expand, the kernels of m0_selfplay_step) and answered with the best root moves, the principal
 * variation behind each and the evaluation.  Every analysis is a fresh tree whose random streams are keyed by (cfg->seed, id):
 * a result does not depend on the slot, the number of slots or what else is in flight.  (The streams take the low 32 bits
 * of id.)
 * cfg: concurrent_games = tree slots, inference_batch_size and the MCTS fields as a self-play engine reads them;
 * num_simulations sizes the node arenas (a submission with more simulations may report `overflow`: "A full node arena"
 * above; its lines, PVs -- which end at a refused leaf whatever its visits -- and `sims` are those of the search as it ran).  The self-play, draw and
 * arena fields, eval_cache and tail_split are ignored; tt_merge / raw_legal_priors are refused (NULL, the message starts with
 * "M0_ERR_UNSUPPORTED").  Destroy and stats with m0_selfplay_destroy / m0_selfplay_stats_get.  m0_selfplay_step, _poll,
 * _ext_*, _set_openings and m0_search_* on an analysis engine return M0_ERR_STATE, as m0_analysis_* do on any other engine. */
#define M0_AN_MAX_LINES 8
#define M0_AN_MAX_PV    16
typedef struct m0_analysis_opts { int multipv, pv_len, dirichlet; } m0_analysis_opts;   /* 1..8, 1..16, bool */
typedef struct m0_analysis_line {
    uint16_t move; int32_t policy_index; int32_t visits; float prior; double q;   /* the root child */
    int32_t pv_len; uint16_t pv[M0_AN_MAX_PV];                                    /* pv[0] == move; unused entries 0 */
} m0_analysis_line;
typedef struct m0_analysis_result {
    int64_t id; int32_t status;      /* 0 searched/evaluated, 1 side to move is checkmated, 2 stalemate, 3 answered from the
                                        endgame tablebases (m0_selfplay_set_search_tablebase, m0_tb_root_lines) */
    int32_t nlegal, overflow, sims, root_n; uint64_t evals;
    float value;                     /* network value of the root evaluation (side to move) */
    double root_q; int32_t nlines; m0_analysis_line lines[M0_AN_MAX_LINES];
    /* status 3 only (0 otherwise); appended, every field above keeps its offset */
    int32_t tb_dtm;                  /* distance to mate of the root in plies, 0 for a draw */
    int32_t line_dtm[M0_AN_MAX_LINES];   /* ... of the position after each line's move */
} m0_analysis_result;
m0_selfplay* m0_analysis_create(m0_net* net, const m0_selfplay_cfg* cfg, const m0_analysis_opts* opts);
m0_selfplay* m0_analysis_create_ext(const m0_selfplay_cfg* cfg, const m0_analysis_opts* opts);   /* external evaluator */
/* Queue the position `fen` after the n_moves legal moves `ucis` (nullable when n_moves = 0): the moves go through the
 * repetition window of a game, so the search sees repetitions with the positions before it.  The queue is unbounded.
 * A bad FEN or an illegal move: M0_ERR_INVALID, nothing queued.  A root without legal moves is answered at once (status 1 / 2,
 * nlines 0, no evaluation) and never takes a slot; so is, with tables attached (m0_selfplay_set_search_tablebase), a root inside
 * them (status 3, the lines of m0_tb_root_lines).
 * sims > 0: a search of that many simulations; lines are the root children by visits (ties: move order), each with the
 *           most-visited line behind it (first maximum in move order; it ends at an unexpanded or terminal node, at a node
 *           without visited children, or at opts->pv_len).
 * sims = 0: policy mode, no tree: one network evaluation; lines are the legal moves by legal-softmax prior (ties: move order),
 *           visits 0, pv_len 1, root_n 0, evals 1, value the network's raw value.  Engines with a network only
 *           (m0_analysis_create_ext: M0_ERR_UNSUPPORTED). */
int m0_analysis_submit(m0_selfplay* sp, const char* fen, const char* const* ucis, int n_moves, int sims, int64_t id);
/* `steps` times: evaluate up to concurrent_games * (inference_batch_size + 1) queued policy-mode positions, fill free slots
 * from the queue, run one select -> network -> expand pass, harvest the finished searches (only the compact results cross
 * to the host).  Stops early when nothing is pending. */
int m0_analysis_step(m0_selfplay* sp, int steps);
/* The step split at the network, as m0_selfplay_ext_select / _expand (same buffer rule for max_rows). */
int m0_analysis_ext_select(m0_selfplay* sp, int* rows, float* planes, int max_rows);
int m0_analysis_ext_expand(m0_selfplay* sp, const float* logits, const float* values, int rows);
int m0_analysis_poll(m0_selfplay* sp, m0_analysis_result* out);   /* 1 written, 0 none; completion order */
int m0_analysis_pending(m0_selfplay* sp);                         /* queued + in flight (answered ones not counted) */
size_t m0_analysis_result_size(void);                             /* sizeof(m0_analysis_result), for foreign mirrors */

/* ---- stored training rows back to positions (the inverse of encode_board; csrc/planes_decode.h says what the planes hold) ----
 * Per row a status: 0 or the FIRST of these reasons, in this order. */
#define M0_DECODE_OK 0
#define M0_DECODE_PIECE_VALUE 1         /* a piece-plane value that is not exactly 0.0f or 1.0f (NaN included) */
#define M0_DECODE_SQUARE_CLASH 2        /* two men on one square */
#define M0_DECODE_KINGS 3               /* a side without exactly one king */
#define M0_DECODE_PAWN_RANK 4           /* a pawn on rank 1 or 8 */
#define M0_DECODE_NOT_UNIFORM 5         /* one of the seven constant planes varies over the board */
#define M0_DECODE_FLAG_VALUE 6          /* the turn plane or a castling plane is neither 0 nor 1 */
#define M0_DECODE_CASTLING 7            /* a castling plane set without king and rook on their original squares */
#define M0_DECODE_COUNTER 8             /* a counter plane that is no float32(k / 99.0) resp. float32(k / 199.0) */
#define M0_DECODE_OPPONENT_IN_CHECK 9   /* the side NOT to move is in check */
#define M0_DECODE_TOO_MANY_MOVES 10     /* more pseudo-legal moves than a move list holds (256): no reachable position */
#define M0_DECODE_MASK_MISMATCH 11      /* with a mask: it differs from the legal moves of the decoded position (the audit of
                                           the reference's audit_legal_masks.py); the position and nlegal are still written */
/* per row flags: information, not errors */
#define M0_DECODE_HALFMOVE_SATURATED 1  /* half-move plane exactly 1.0: the clock was 99 OR MORE, the position carries 99 */
#define M0_DECODE_FULLMOVE_SATURATED 2  /* full-move plane exactly 1.0: 199 or more */
#define M0_DECODE_EP_FROM_MASK 4        /* the en-passant square was recovered from the mask */
#define M0_DECODE_NO_MASK 8             /* no mask given: en passant is unknown and set to none */
/* planes f32 [n,19,8,8]; mask u8 [n,4672] or NULL; outputs nullable: status / flags / nlegal i32 [n]; fens n strings of
 * fen_stride bytes each (>= 96), Board.fen() of the decoded position as m0_fen_after writes it, empty for a row whose status
 * leaves no position (every status but OK and MASK_MISMATCH).  One wave per row on the device; M0_ERR_HIP without one. */
int m0_decode_planes(int hip_device, const float* planes, const uint8_t* mask, int n, int32_t* status, int32_t* flags,
                     int32_t* nlegal, char* fens, int fen_stride);
/* The same rows into an analysis engine: decoded on the engine's device and stream, and every row of status 0 queued as
 * m0_analysis_submit queues its FEN (ids[i], or i when ids is NULL; sims = 0: policy mode), with an empty repetition window
 * and without a FEN round trip: the result is bit for bit that of m0_analysis_submit(fen of the row, no moves, sims, id).
 * Rows of another status are reported in status[] (required) and not queued: nothing is answered for them.  Roots without
 * legal moves and, with tables attached, roots inside them are answered at once, as m0_analysis_submit does.  flags nullable. */
int m0_analysis_submit_planes(m0_selfplay* sp, const float* planes, const uint8_t* mask, int n, int sims, const int64_t* ids,
                              int32_t* status, int32_t* flags);
/* Policy targets need every root child, not the 8 best: with keeping on, each harvest also gathers (policy index, visits)
 * of every root child of the finished searches, in move-generation order, and m0_analysis_poll_visits hands them out with the
 * result.  Off (the default) nothing extra is launched or copied and nchild is 0. */
int m0_analysis_keep_visits(m0_selfplay* sp, int on);
/* m0_analysis_poll plus the root's children: nchild, policy_idx[nchild], visits[nchild].  cap = entries of the two arrays,
 * at least 256 (M0_ERR_INVALID otherwise).  nchild = 0 for results answered on the host (mate, stalemate, tablebases), for
 * policy-mode results and for searches harvested while keeping was off. */
int m0_analysis_poll_visits(m0_selfplay* sp, m0_analysis_result* out, int32_t* nchild, int32_t* policy_idx, int32_t* visits,
                            int cap);

/* ---- generated 3- and 4-man endgame tablebases (the reference's tablebases.enabled: selfplay/internal.py:250-260, 559-581) ----
 * The reference ends a self-play game as soon as the position after a move is found in a Syzygy table and takes the sign of
 * its WDL as the result.  Here the tables are computed instead of read: distance-to-mate tables by retrograde analysis on the
 * GPU, ignoring the 50-move rule as Syzygy's WDL does (the reference scores cursed wins as wins), so the verdict is the same.
 * Scope: KK, the five 3-man signatures and every 4-man signature except KPKP (the only one with en passant); a KPKP position
 * is no hit.  Signatures are strings such as "KQK", "KRPK", "KQKR": the greater side first (it is White in the table; a
 * position with the greater side Black is probed through its colour flip), men ordered Q > R > B > N > P.  One byte per entry
 * and 2 * 64^n entries per table: 0 draw, 255 invalid, 1 + d decided in d plies (d even: the side to move is mated in d, d odd:
 * it mates in d); index and encoding are specified in csrc/tb_core.h.  A handle is immutable once made and may be shared by
 * any number of engines and threads; it must outlive the engines it is attached to. */
typedef struct m0_tb m0_tb;
/* Build on the device: every signature in scope with at most max_men (3 or 4) men / the given signatures plus everything
 * their captures and promotions lead into.  NULL on failure (no HIP device, an unknown signature). */
m0_tb* m0_tb_build(int hip_device, int max_men);
m0_tb* m0_tb_build_signatures(int hip_device, const char* const* sigs, int n);
/* Cache file: magic, format version, the list of signatures with a checksum per table, then the tables.  Load needs no GPU and
 * refuses (NULL, message in the last error) a file that is truncated, has another magic or version, or fails a checksum.
 * Save writes a temporary file of a unique name beside `path` and renames it: several processes may save the same tables to
 * the same path at the same time, and a reader never sees a partial file. */
m0_tb* m0_tb_load(const char* path);
int m0_tb_save(const m0_tb* tb, const char* path);
void m0_tb_destroy(m0_tb* tb);
int m0_tb_max_men(const m0_tb* tb);                   /* men of the largest table in the handle */
/* The raw table of a signature (valid while the handle lives); M0_ERR_INVALID when the handle has no such table. */
int m0_tb_table(const m0_tb* tb, const char* sig, const uint8_t** bytes, size_t* n);
/* Table i in build order: signature (sig8: 8 bytes, NUL-padded), largest d (-1: no decided entry), sweeps and milliseconds of
 * its build (0 for a loaded handle's time).  Returns 1, 0 when i is past the last table, M0_ERR_INVALID for a null handle.
 * Not in the reference's interface: tools/bench_tablebase.py and the tests report sweeps and largest d through it. */
int m0_tb_table_info(const m0_tb* tb, int i, char* sig8, int* maxd, int* sweeps, double* build_ms);
/* Per FEN: hit 0/1, wdl -1/0/+1 for the side to move, dtm in plies (0 for draws); outputs nullable.  No hit: more men than the
 * handle covers, a signature it does not hold (KPKP), any castling right left, an illegal placement. */
int m0_tb_probe_fens(const m0_tb* tb, const char* const* fens, int n, uint8_t* hit, int8_t* wdl, int16_t* dtm);
/* Attach to a self-play engine before its first step (tb = NULL detaches): after every played move a position with at most
 * min(max_pieces, m0_tb_max_men) men is probed; on a hit the game ends there with that result (White's point of view,
 * resigned = 0).  Without a tablebase the game loop is unchanged.  Match and analysis engines: M0_ERR_STATE (the reference's
 * arena does not probe). */
int m0_selfplay_set_tablebase(m0_selfplay* sp, const m0_tb* tb, int max_pieces);
uint64_t m0_selfplay_tb_adjudications(m0_selfplay* sp);      /* games ended by a tablebase hit */
/* The tables inside the search (no counterpart in the reference).  Accepted by every engine kind before its first step; tb =
 * NULL detaches.  The handle's tables are copied to the engine's HIP device at the first attach on that device (one copy per
 * handle and device, shared by every engine there, complete before this call returns, freed by m0_tb_destroy: 2.6 MiB for the
 * 3-man set, about 930 MiB for the 4-man set).  From then on select_kernel probes every leaf with at most
 * min(max_pieces, m0_tb_max_men) men after the game-over tests: a hit is a terminal leaf worth +1 / -1 for the side to move
 * (draw_penalty for a table draw), backed up at once, never expanded and never evaluated.  A position with a castling right
 * left is no hit; the half-move clock is ignored, as in adjudication.  A root inside the tables is handled per engine kind:
 *   self-play engines   also adjudicate after every played move, exactly as m0_selfplay_set_tablebase does (same counter);
 *   match engines       adjudicate the same way: the game ends with the table's verdict from White's point of view;
 *   analysis engines    answer a submission whose root is a hit at once from the tables (m0_tb_root_lines): status 3, no slot,
 *                       no evaluation;
 *   m0_search_*         searches whatever root it is given: only leaves are probed.
 * Without an attached handle every engine computes bit for bit what it computed before. */
int m0_selfplay_set_search_tablebase(m0_selfplay* sp, const m0_tb* tb, int max_pieces);
uint64_t m0_selfplay_tb_leaves(m0_selfplay* sp);             /* leaves the search took from the tables */
/* The analysis of a root inside the tables, on the host (no GPU).  1: the root is a hit and `out` is filled (every field but
 * id): status 3, nlegal, root_q = wdl for the side to move, tb_dtm, evals = root_n = sims = 0, value 0 and min(multipv, nlegal)
 * lines.  0: no hit (or a successor without a table), `out` untouched.  M0_ERR_INVALID: a bad FEN, multipv outside [1, 8],
 * pv_len outside [1, 16].
 * Line order: moves whose successor is lost for the opponent first, smallest successor dtm first; then moves to a drawn
 * successor; then moves to a successor won for the opponent, largest dtm first; ties keep the legal-move order.  Per line: q
 * the exact +1 / 0 / -1 from the root mover's view, visits 0, prior 0, policy_index as usual, line_dtm the successor's dtm.
 * A decided line's pv continues with the first-ranked move of each following position and ends at checkmate or at pv_len; a
 * drawn line's pv is the move alone. */
int m0_tb_root_lines(const m0_tb* tb, const char* fen, int multipv, int pv_len, m0_analysis_result* out);

/* ---- host decision functions (selfplay/internal.py), exposed for parity tests ---- */
int m0_sample_move_index(const int32_t* visits, int n, double temperature, double u);
int m0_playout_cap(int sims, double frac, double u);
double m0_temperature_for(int fullmove_number, double t_start, double t_end, int t_moves);
/* position + move list -> flags: bit0 game_over, bit1 game_over(claim_draw), bit2 adjudicate_draw(cfg of sp),
 * bit3 checkmate, bit4 stalemate, bit5 insufficient, bit6 can_claim_fifty, bit7 is_repetition(3),
 * bit8 can_claim_threefold, bit9 fivefold, bit10 seventyfive ; result = game_result(board) */
int m0_rules_probe(const m0_selfplay_cfg* cfg, const char* fen, const char* const* ucis, int n, int* flags, float* result);

/* ---- reading games back in: written moves -> training positions (replaces the python-chess loop of the reference's
 * azchess/tools/process_lichess.py:59-106, and also yields the legal masks its backfill_legal_masks.py adds afterwards) ----
 * A written move becomes a 32-bit pattern without looking at a position (bit layout and matching rule: csrc/san_match.h); a
 * game is an array of patterns, replayed on the device with the engine's own move generator, one wave per game. */
/* One SAN token -> pattern, as python-chess's SAN reader takes it: trailing '!' / '?' and one '+' or '#' dropped; O-O / O-O-O
 * (also written with zeros); [NBRQK]? [a-h]? [1-8]? [-x]? <square> (=?[NBRQ])?.  M0_ERR_INVALID (pattern 0, which matches no
 * move) for anything else, the null moves "--" and "Z0" included.  Host only, no GPU. */
int m0_san_pattern(const char* token, uint32_t* pattern);
/* An exact move -> pattern.  The caller names what it passes ("b1c3" is also a well-formed SAN pawn token): kind M0_MOVE_UCI
 * reads `uci` ("e2e4", "e7e8q"), kind M0_MOVE_RAW reads `raw` = from | to<<6 | promo<<12 (promo 0 none, 1 N, 2 B, 3 R, 4 Q: an
 * engine record's `played`).  Host only. */
#define M0_MOVE_UCI 0
#define M0_MOVE_RAW 1
int m0_move_pattern(int kind, const char* uci, uint32_t raw, uint32_t* pattern);
/* per-game status */
#define M0_REPLAY_OK 0         /* every token resolved to exactly one legal move */
#define M0_REPLAY_ILLEGAL 1    /* the token at index plies[g] fits no legal move (or did not parse) */
#define M0_REPLAY_AMBIGUOUS 2  /* it fits more than one */
#define M0_REPLAY_TOO_LONG 3   /* the game has more than max_plies tokens; its first max_plies are resolved */
/* per-game end flags: the position after the last resolved move */
#define M0_REPLAY_END_CHECKMATE 1
#define M0_REPLAY_END_STALEMATE 2
#define M0_REPLAY_END_INSUFFICIENT 4
#define M0_REPLAY_END_WHITE_TO_MOVE 8
/* Replays n_games games.  Game g starts from start_fens[g] (start_fens or an entry NULL: the initial position) and owns rows
 * offsets[g] .. offsets[g+1] of `patterns` and of every per-ply output (offsets[0] = 0).  It resolves its tokens in order and
 * stops at the first that does not resolve to exactly one legal move, or after max_plies: plies[g] rows are written and the
 * rest of its rows are zero.  Per ply k, for the position BEFORE the move: moves (as M0_MOVE_RAW), policy_idx (move_to_index),
 * nlegal, turn (1 White), planes f32 [19][8][8], mask u8 [4672], ssl f32 [17][8][8] (piece 13, threat, pin, fork, control); each
 * per-ply output may be NULL.  plies, status and end_flags are required.
 * The work is issued in launches of whole games holding at most max_positions_per_launch rows (<= 0: one launch; a game longer
 * than the limit goes alone), which bounds device and staging memory at about 9.5 KB per row for planes and mask; the results
 * do not depend on that number or on the order of the games.  A bad start FEN is M0_ERR_INVALID for the whole call and the
 * message names the game index.  M0_ERR_HIP without a HIP device: there is no CPU path. */
int m0_replay_games(int hip_device, const char* const* start_fens, const uint32_t* patterns, const int32_t* offsets, int n_games,
                    int max_plies, int max_positions_per_launch, int32_t* plies, int32_t* status, int32_t* end_flags,
                    uint16_t* moves, int32_t* policy_idx, int32_t* nlegal, int8_t* turn, float* planes, uint8_t* mask, float* ssl);

#ifdef __cplusplus
}
#endif
/* live searches on an analysis engine (peek, stop, held trees, continue by moves): the calls a UCI front end needs */
#include "m0_analysis_live.h"
/* training loss of stored positions under a network, per row (no trainer, no gradient) */
#include "m0_score.h"
/* ... and its SSL term: the heads' losses per row, targets stored or taken from the stored planes */
#include "m0_ssl_score.h"
/* Gumbel root search for self-play engines: sequential halving and improved-policy targets (opt-in) */
#include "m0_gumbel.h"
/* the trainer's flip and rotate augmentations of stored rows on the device, and the training loss under them */
#include "m0_augment.h"
/* proof search: exact wins, losses and draws backed up the search tree (opt-in) */
#include "m0_proof.h"
/* packed training rows: bitboards and sparse policies, expanded on the device */
#include "m0_rowpack.h"
/* a resident store of packed rows: training batches gathered, expanded and augmented on the device in one launch */
#include "m0_batch.h"
/* ... and the SSL target maps of the augmented rows, written by the same launch */
#include "m0_batch_ssl.h"
/* ... and a weight per resident row: rows drawn in proportion to it and gathered on the device, a prioritised replay buffer */
#include "m0_batch_weighted.h"
/* self-play budget mix: full and fast searches, forced playouts and policy-target pruning (opt-in) */
#include "m0_budget.h"
#endif /* M0_ENGINE_H */
