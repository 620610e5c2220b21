// The self-play engine object and the functions of its game loop (selfplay.hip) that the C-ABI unit (capi_selfplay.hip)
// calls.  Internal: the public face is include/m0_engine.h.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <deque>
#include <list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "chess_core.h"
#include "host_rules.h"
#include "net.h"
#include "tree.h"

namespace m0 {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct GameRecordOwner {
    std::vector<float> s, pi, z, search_values, ssl;
    std::vector<uint8_t> legal_mask;
    std::vector<uint16_t> played;
    std::string start_fen;
    // self-play budget mix (m0_game_record_budget): per recorded ply; `budget` false = a record of an engine without the mode
    bool budget = false;
    std::vector<uint8_t> full;
    std::vector<int32_t> sims;
};

struct HostGame : Line {                  // pos, win, history (all moves incl. opening plies)
    bool in_use = false;
    int game_index = 0;
    std::vector<Pos> rec_pos;             // position of every recorded ply (SSL targets)
    // records
    std::vector<float> states, pis, search_values;
    std::vector<int8_t> turns;
    std::vector<uint8_t> masks;
    std::vector<int> sims_used;
    int nstates = 0;
    double entropy_sum = 0.0;
    int entropy_count = 0;
    ResignState resign;
    HStream rng;                          // PURPOSE_GAME stream: opening plies, playout cap, move sampling
    double t0 = 0.0;
    int cur_sims = 0;
    bool cur_full = true;                 // self-play budget mix: the running search is a full one
    std::vector<uint8_t> full;            // ... and cur_full of every recorded ply, beside sims_used
    bool a_is_white = true;               // arena
    int book_index = -1;                  // the opening-book position the game started from, -1 = the initial position
};

// What one m0_selfplay object is: set once by engine_create and read wherever the three behave differently.  (cfg.arena_mode is
// the same fact in the ABI struct; it is normalised at creation and not read afterwards.)
enum class EngineKind { SelfPlay, Match, Analysis };
// sets of kinds, for the call guard below
constexpr unsigned KIND_SELFPLAY = 1u << (int)EngineKind::SelfPlay, KIND_MATCH = 1u << (int)EngineKind::Match,
                   KIND_ANALYSIS = 1u << (int)EngineKind::Analysis, KIND_GAMES = KIND_SELFPLAY | KIND_MATCH,
                   KIND_ANY = KIND_GAMES | KIND_ANALYSIS;

// The new roots that the next advance_kernel launch sets: per entry a tree slot and either the child of its old root to keep
// or a RootMode (tree.h).  Filled by the host part of a step, launched and emptied by apply_advances.
struct AdvanceList {
    std::vector<int> slots, roots;
    void push(int slot, int root) { slots.push_back(slot); roots.push_back(root); }
    void clear() { slots.clear(); roots.clear(); }
    bool empty() const { return slots.empty(); }
};

// What an analysis engine (capi_analysis.hip) keeps beside the tree slots.  A slot that searches holds its position and
// repetition window in m0_selfplay::games[slot] (in_use) and its search in hg[slot], as a game does.
struct AnalysisJob { Line line; int sims; int nlegal; int64_t id; bool keep = false; };   // keep: m0_analysis_submit_keep / _continue
struct Analysis {
    m0_analysis_opts opts;
    std::deque<AnalysisJob> queue;         // submitted searches that wait for a slot
    std::deque<AnalysisJob> policy_queue;  // submitted policy-mode positions (sims = 0)
    std::deque<m0_analysis_result> done;   // answered, not yet polled
    std::deque<std::vector<int32_t>> done_children;   // beside `done`: the root children of each (answer(), capi_analysis.hip)
    // proof search (m0_selfplay_set_proof on an analysis engine): beside `done` the proofs of each, the proofs of the result
    // handed out last (m0_analysis_last_proof), and the result kernel's output for them
    std::deque<m0_proof_lines> done_proof;
    m0_proof_lines last_proof = {};
    m0_proof_lines* proof_dev = nullptr;   // [G]
    std::vector<m0_proof_lines> hproof;
    std::vector<AnalysisJob> slot_job;     // per slot: what it searches (the Line lives in games[slot])
    // A HELD slot (include/m0_analysis_live.h): its search was answered (finished or stopped) and its tree stays for
    // m0_analysis_continue: games[slot].in_use, hg[slot].active == 0, held[slot]; slot_job[slot].id is the held id.
    std::vector<uint8_t> held;
    int* reroot_in_dev = nullptr;          // m0_analysis_continue: [slot, n_moves, moves x M0_REROOT_MAX_MOVES]
    RerootOut* reroot_out_dev = nullptr;
    std::vector<int> finished;             // scratch: slots harvested by this step
    std::vector<m0_analysis_line> hlines;  // host copies of the result kernels' output
    std::vector<int> hnlines;
    std::vector<float> hvalues;
    std::vector<Pos> hpos;
    m0_analysis_line* lines_dev = nullptr; // [rows_max][M0_AN_MAX_LINES] (searches use the first G entries)
    int* nlines_dev = nullptr;             // [rows_max]
    float* value_out_dev = nullptr;        // [rows_max]
    Pos* pos_dev = nullptr;                // policy mode: [rows_max] positions, their legal moves and policy indices
    int32_t* nlegal_dev = nullptr;
    uint16_t* moves_dev = nullptr;
    int32_t* idx_dev = nullptr;
    bool keep_visits = false;              // m0_analysis_keep_visits: a harvest also fetches every root child's policy index and visits
    int32_t* child_idx_dev = nullptr;      // [G][M0_MAX_CHILDREN] each, allocated when keeping is first turned on
    int32_t* child_n_dev = nullptr;
    int32_t* nchild_dev = nullptr;         // [G]
    std::vector<int32_t> hchild_idx, hchild_n, hnchild;
};

}  // namespace m0

struct m0_selfplay {
    m0::EngineKind kind = m0::EngineKind::SelfPlay;
    m0_selfplay_cfg cfg;
    TreeCfg tc;
    m0_net* nethandle = nullptr;
    m0_net* nethandle_b = nullptr;
    Net* net = nullptr;
    Net* net_b = nullptr;                 // arena: the second network (games with an odd index play it as White)
    Net* net_tail = nullptr;              // cfg.tail_split: a view of `net` (same weights, own stream + workspace) for the partial last round
    hipStream_t stream_tail = nullptr;
    hipEvent_t ev_sel = nullptr, ev_tail = nullptr;
    bool half_split = false;              // cfg.tail_split == 2: two halves instead of main + tail
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int G = 0, L = 0, cap = 0, rows_max = 0;
    TreeDev d;
    std::vector<void*> allocs;
    HipStatus hip;                        // every HIP call made for the engine goes through M0_HIP on it; the first failure stays
    std::vector<GameDev> hg;
    std::vector<m0::HostGame> games;
    std::vector<RootResult> hres;
    float* logits_dev = nullptr;
    float* values_dev = nullptr;
    float* ssl_dev = nullptr;
    m0::Pos* ssl_pos_dev = nullptr;        // staging of one finished game's positions / SSL target maps (ssl_targets)
    float* ssl_out_dev = nullptr;
    int ssl_cap = 0;
    m0::AdvanceList adv;
    int* ids_dev = nullptr;               // the device copy of adv (and of an analysis harvest's slot list)
    int* roots_dev = nullptr;
    std::deque<m0_game_record> done_meta;
    m0_selfplay_stats stats;
    int next_game = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    std::mutex mu;
    std::vector<Sample> hsamples;
    std::vector<int> prev_done;           // per slot: simulations already credited to stats.sims
    int last_rows = 0, last_rows_b = 0;
    int rows2[2] = {0, 0};                // rows of the last select per network
    std::vector<m0::Pos> book;            // opening positions (m0_selfplay_set_openings)
    std::vector<std::string> book_fens;   // ... as the caller wrote them (m0_game_record::start_fen)
    // LRUCache nn_cache of the reference (mcts.py:44-59, 303, 360-371): positions whose root was re-evaluated; 10 000 entries
    std::list<uint64_t> nn_lru;
    std::unordered_map<uint64_t, std::list<uint64_t>::iterator> nn_map;
    bool ext_pending = false;             // ext_select done, ext_expand outstanding
    bool counted = false;                 // registered with the forward gate
    m0::Analysis* an = nullptr;           // the state of an analysis engine (kind == Analysis), null otherwise
    const m0_tb* tb = nullptr;            // endgame tablebase probed on the host: after every played move (m0_selfplay_set_tablebase,
                                          // m0_selfplay_set_search_tablebase), for a submitted root (analysis engines)
    int tb_max_pieces = 0;                // ... for positions with at most this many men (d.tb_set: the probe inside the search)
    uint64_t tb_adjudications = 0;        // games it ended
    bool search_begun = false;            // m0_search_begin was called: the mode (tc.mode, mode_settable) can no longer be set
    std::vector<GumbelResult> hgres;      // host copies of d.gumbel_results, beside hres
    std::vector<ProofResult> hpres;       // host copies of d.proof_results, beside hres
    m0_budget_cfg budget = {1.0, 1, 0.0, 0};
    uint64_t budget_full = 0, budget_fast = 0, budget_pruned = 0;   // searches of either kind, visits pruned from targets
};

namespace m0 {

// Zeroed device memory that lives as long as the engine; null (and the failure in sp->hip) when hipMalloc fails.
template <typename T>
T* dalloc(m0_selfplay* sp, size_t count) {
    void* p = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    if (!M0_HIP(sp->hip, hipMalloc(&p, bytes))) return nullptr;
    sp->allocs.push_back(p);
    M0_HIP(sp->hip, hipMemsetAsync(p, 0, bytes, sp->stream));   // on the engine's own stream: ordered before every kernel that uses it
    return (T*)p;
}
// The creation paths' test after a group of allocations or creations: false, with the error string set, once sp->hip has failed.
inline bool hip_ok(m0_selfplay* sp, const char* context) {
    if (!sp->hip.ok()) m0_hip_error(sp->hip, context);
    return sp->hip.ok();
}

// Head of every engine entry point, in this order: a null handle -> `null_result`; the engine's lock; an engine whose kind is
// not in `kinds` -> M0_ERR_STATE with a message that names the call and the kind; for the calls that touch the device
// (`on_device`; a host-only call must not move the calling thread's current device) an engine whose sp->hip has failed ->
// M0_ERR_HIP with that first failure's message and no further HIP call, else the engine's device.
//
//   call                                                            accepted by
//   m0_selfplay_step, _poll, _set_openings                          self-play, match
//   m0_selfplay_ext_select, _ext_expand, m0_selfplay_set_tablebase   self-play
//   m0_arena_ext_select, _ext_expand                                match
//   m0_search_*                                                     self-play, match (a match engine is accepted as it always
//                                                                   was, although nothing drives one this way)
//   m0_analysis_*                                                   analysis
//   m0_selfplay_stats_get, _running, _last_batch_nhwc,
//   _set_search_tablebase, _tb_leaves, _tb_adjudications            every kind
//   m0_selfplay_set_gumbel, m0_search_gumbel_result,
//   m0_selfplay_set_budget, m0_search_budget_result, _budget_stats  self-play
//   m0_selfplay_set_proof                                           every kind
//   m0_search_proof_result                                          self-play, match
bool kind_accepted(const m0_selfplay* sp, const char* what, unsigned kinds);   // false: the error string is set
#define M0_ENGINE_CALL_OR(null_result, sp, what, kinds, on_device)                    \
    if (!(sp)) { m0_set_error(what ": sp is null"); return null_result; }             \
    std::lock_guard<std::mutex> lk((sp)->mu);                                         \
    if (!m0::kind_accepted(sp, what, kinds)) return M0_ERR_STATE;                     \
    if ((on_device) && !M0_HIP((sp)->hip, hipSetDevice((sp)->device))) return m0_hip_error((sp)->hip)
#define M0_ENGINE_CALL(sp, what, kinds, on_device) M0_ENGINE_CALL_OR(M0_ERR_INVALID, sp, what, kinds, on_device)

// Internal functions set the error string (m0_set_error) where the error happens and return the M0_ERR_* code.
// selfplay.hip
void forward_gate_join(m0_selfplay* sp);        // an engine that owns a network takes part in M0_FORWARD_GATE
void forward_gate_leave(m0_selfplay* sp);
bool sync_games_d2h(m0_selfplay* sp);           // the slots' control blocks: device -> sp->hg, waited for; false: sp->hip has failed
bool sync_games_h2d(m0_selfplay* sp);           // ... sp->hg -> device, on the engine's stream
// Take tree slot `slot` for `line`: a new HostGame, random streams keyed by `uid`, no evaluations counted yet.
HostGame& occupy_slot(m0_selfplay* sp, int slot, Line&& line, int uid);
// Arm a search of the slot's position (MCTS.run prologue) and queue its root (a child of the old root or a RootMode) in sp->adv.
void begin_search(m0_selfplay* sp, int slot, int sims, bool dirichlet, int root);
// ... the arming alone, for a root that is already in place on the device (`fresh`: a brand-new node, not a reused one)
void arm_slot_search(m0_selfplay* sp, int slot, int sims, bool dirichlet, bool fresh);
int apply_advances(m0_selfplay* sp);            // control blocks -> device, advance_kernel over sp->adv, which is empty afterwards
int run_select(m0_selfplay* sp, int* rows_out);
// The search mode (sp->tc.mode).  The guard of the three mode setters: M0_OK when `wanted`, which the messages call `name`, may be
// set or taken back now -- no game or search has started, no compat.tt_merge, no other mode on; else M0_ERR_STATE / _INVALID.
int mode_settable(m0_selfplay* sp, SearchMode wanted, const char* name);
// The shared part of the m0_search_<mode>_result calls: a bad slot g, M0_ERR_STATE with "`what`: <the mode> is not set on this engine",
// M0_OK and *finished false while the search runs; else slot g's RootResult and mode result are copied to their host mirrors.
int mode_result_fetch(m0_selfplay* sp, int g, SearchMode mode, const char* what, bool* finished);
int refill(m0_selfplay* sp);                    // before select: the first games (lazily, at the first step) / queued analyses
int one_step(m0_selfplay* sp);                  // select -> network -> finish_step
// second half of a step: expand / backup on the device, the counters, then the harvest of the finished searches
int finish_step(m0_selfplay* sp, int rows, double t0);

// capi_selfplay.hip
m0_selfplay* engine_create(m0_net* nh, m0_net* nh_b, const m0_selfplay_cfg* cfg, EngineKind kind);
int ext_select_impl(m0_selfplay* sp, int* rows_a, int* rows_b, float* planes_a, float* planes_b, int max_rows);
int ext_expand_impl(m0_selfplay* sp, const float* logits_a, const float* values_a, int rows_a, const float* logits_b,
                    const float* values_b, int rows_b);

// capi_analysis.hip: the two ends of an analysis engine's step, around the select -> network -> expand pass
int analysis_refill(m0_selfplay* sp);       // free slots <- queued searches
int analysis_harvest(m0_selfplay* sp);      // finished searches -> results, slots freed

}  // namespace m0
