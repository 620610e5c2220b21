// extern "C" entry points of the self-play / match engine (include/m0_engine.h): creation and teardown, step / poll / stats,
// the external-evaluator pair and the split-step search API.  The game loop they drive is selfplay.hip.
#include <string.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "selfplay_engine.h"

using namespace m0;

// `match`: a match engine, whose cache switch is arena_eval_cache (eval_cache is ignored there: m0_engine.h)
static void fill_tree_cfg(const m0_selfplay_cfg& c, bool match, TreeCfg& t) {
    t.fpu_reduction = c.fpu_reduction; t.draw_penalty = c.draw_penalty; t.virtual_loss = c.virtual_loss;
    t.selection_jitter = c.selection_jitter; t.cpuct = c.cpuct; t.cpuct_start = c.cpuct_start; t.cpuct_end = c.cpuct_end;
    t.cpuct_plies = c.cpuct_plies; t.use_c_base = c.use_c_base; t.cpuct_c_base = c.cpuct_c_base; t.cpuct_c_init = c.cpuct_c_init;
    t.dirichlet_alpha = c.dirichlet_alpha; t.dirichlet_frac = c.dirichlet_frac; t.legal_softmax = c.legal_softmax;
    t.enable_entropy_noise = c.enable_entropy_noise; t.no_instant_backtrack = c.no_instant_backtrack;
    t.virtual_loss_active = c.virtual_loss_active; t.leaves_per_step = c.inference_batch_size;
    t.tt_merge = c.tt_merge; t.raw_legal_priors = c.raw_legal_priors; t.max_children = c.max_children;
    t.min_child_prior = c.min_child_prior;
    t.mode = MODE_PUCT;                    // m0_selfplay_set_gumbel / _set_proof / _set_budget set another, with its parameters
    t.gumbel_cfg = m0_gumbel_cfg{0, 0.0, 0.0}; t.forced_k = 0.0;
    // the cached payload is the LEGAL logits: only the legal-softmax expansion can be served from it
    t.eval_cache = ((match ? c.arena_eval_cache : c.eval_cache) && c.legal_softmax && !c.raw_legal_priors && !c.tt_merge) ? 1 : 0;
}

static bool alloc_tree_arenas(m0_selfplay* sp) {
    // arena: reused subtree + one search of new children (218 max per expansion is far above the ~35 mean)
    const m0_selfplay_cfg& c = sp->cfg;
    long want = c.arena_nodes > 0 ? c.arena_nodes : (long)(c.num_simulations * 1.3 + 64) * 96;
    if (want < 4096) want = 4096;
    sp->cap = (int)want;
    const size_t N = (size_t)sp->G * 2 * sp->cap;
    TreeArrays& t = sp->d.t;
    t.cap = sp->cap;
    t.prior = dalloc<double>(sp, N); t.w = dalloc<double>(sp, N); t.q = dalloc<double>(sp, N);
    t.n = dalloc<int>(sp, N); t.vl = dalloc<int>(sp, N); t.cbase = dalloc<int>(sp, N);
    t.nch = dalloc<int16_t>(sp, N); t.mv = dalloc<uint16_t>(sp, N); t.midx = dalloc<uint16_t>(sp, N);
    sp->d.games = dalloc<GameDev>(sp, sp->G);
    const size_t LS = (size_t)sp->L + 1;
    sp->d.samples = dalloc<Sample>(sp, (size_t)sp->G * LS);
    sp->d.paths = dalloc<int>(sp, (size_t)sp->G * LS * M0_MAX_DEPTH);
    sp->d.leaf_moves = dalloc<uint16_t>(sp, (size_t)sp->G * LS * M0_MAX_CHILDREN);
    return hip_ok(sp, "hipMalloc failed for the search arenas (lower concurrent_games or arena_nodes)");
}

// cfg.tt_merge: the transposition tables
static bool alloc_position_tables(m0_selfplay* sp) {
    sp->d.tt_sides = 1;
    if (!sp->cfg.tt_merge) return true;
    const size_t LS = (size_t)sp->L + 1;
    int tc = 1024;
    while (tc < 2 * sp->cap) tc <<= 1;
    sp->d.tt_cap = tc;
    // match engine: one table per side, kept for the whole game (the reference keeps one MCTS object per side, arena.py:157-158)
    sp->d.tt_sides = sp->kind == EngineKind::Match ? 2 : 1;
    // a side's half that cannot hold one more search starts over BEFORE that search (advance_kernel), not in the middle of it:
    // ~35 children per expansion on average, 48 with margin, never more than half of the half
    sp->d.search_nodes = (int)std::min<long>((long)sp->cfg.num_simulations * 48 + 4 * M0_MAX_CHILDREN, (long)sp->cap / 2);
    sp->d.epaths = dalloc<int>(sp, (size_t)sp->G * LS * M0_MAX_DEPTH);
    sp->d.tt_keys = dalloc<uint64_t>(sp, (size_t)sp->G * sp->d.tt_sides * tc);
    sp->d.tt_nodes = dalloc<int>(sp, (size_t)sp->G * sp->d.tt_sides * tc);
    return hip_ok(sp, "hipMalloc failed for the position tables (tt_merge): lower concurrent_games or arena_nodes");
}

static bool alloc_eval_cache(m0_selfplay* sp) {
    if (!sp->tc.eval_cache) return true;
    const size_t LS = (size_t)sp->L + 1;
    int entries = sp->cfg.eval_cache_entries > 0 ? sp->cfg.eval_cache_entries : 16384;
    int sets = 64;
    while (sets * 4 < entries) sets <<= 1;
    EvalCache& ec = sp->d.ec;
    ec.sets = sets;
    ec.sides = sp->kind == EngineKind::Match ? 2 : 1;             // match engine: one instance per network
    const size_t entries_all = (size_t)sp->G * ec.sides * sets * 4;
    ec.keys = dalloc<uint64_t>(sp, entries_all);
    ec.stamps = dalloc<uint32_t>(sp, entries_all);
    ec.payload = dalloc<float>(sp, entries_all * M0_EC_WORDS);
    ec.hit_stage = dalloc<float>(sp, (size_t)sp->G * LS * M0_EC_WORDS);
    return hip_ok(sp, "hipMalloc failed for the evaluation cache: lower eval_cache_entries or concurrent_games");
}

// the batch (one region per network), the evaluator's outputs and the small staging buffers
static bool alloc_batch_buffers(m0_selfplay* sp) {
    const int nreg = sp->kind == EngineKind::Match ? 2 : 1;
    sp->d.hist = dalloc<uint64_t>(sp, (size_t)sp->G * M0_HIST_CAP);
    sp->d.results = dalloc<RootResult>(sp, sp->G);
    sp->d.row_counter = dalloc<int>(sp, 4);
    sp->d.x0 = dalloc<_Float16>(sp, (size_t)(nreg * sp->rows_max + 4) * 64 * 32);
    sp->logits_dev = dalloc<float>(sp, (size_t)nreg * sp->rows_max * 4672);
    sp->values_dev = dalloc<float>(sp, (size_t)nreg * sp->rows_max + 4);
    sp->d.net_row_base = sp->rows_max;
    if (sp->cfg.ssl_in_forward && sp->net && sp->net->ssl_channels_total() > 0)
        sp->ssl_dev = dalloc<float>(sp, (size_t)sp->rows_max * sp->net->ssl_channels_total() * 64);
    if (sp->cfg.ssl_targets) {
        sp->ssl_cap = sp->cfg.max_game_len > 0 ? sp->cfg.max_game_len + 1 : 513;
        sp->ssl_pos_dev = dalloc<Pos>(sp, sp->ssl_cap);
        sp->ssl_out_dev = dalloc<float>(sp, (size_t)sp->ssl_cap * 17 * 64);
        if (!hip_ok(sp, "hipMalloc failed for the SSL target staging buffers")) return false;
    }
    sp->ids_dev = dalloc<int>(sp, sp->G);
    sp->roots_dev = dalloc<int>(sp, sp->G);
    sp->d.logits = sp->logits_dev; sp->d.values = sp->values_dev;
    sp->d.G = sp->G; sp->d.L = sp->L;
    return hip_ok(sp, "hipMalloc failed for the batch buffers (lower concurrent_games or inference_batch_size)");
}

// cfg.tail_split: the second instance of the network on a stream of its own (one_step, split_rows)
static bool make_tail_view(m0_selfplay* sp) {
    if (!(sp->cfg.tail_split && sp->net && sp->kind != EngineKind::Match && sp->net->cfg().channels > 256 && sp->net->cfg().channels <= 320 &&
          sp->rows_max >= 2048)) return true;
    // M0_TAIL_CU_MASK=w0,...,w7 (measurement switch, like M0_NET_CU_MASK for the network's own stream): the second instance's
    // stream runs on those CUs only -- with complementary masks every launch of the two halves has a known share of the chip
    M0_HIP(sp->hip, create_stream_cu_mask_env("M0_TAIL_CU_MASK", &sp->stream_tail));
    M0_HIP(sp->hip, hipEventCreateWithFlags(&sp->ev_sel, hipEventDisableTiming));
    M0_HIP(sp->hip, hipEventCreateWithFlags(&sp->ev_tail, hipEventDisableTiming));
    if (!hip_ok(sp, "hipStreamCreate / hipEventCreate failed (tail split)")) return false;
    sp->net_tail = sp->net->shared_view(sp->stream_tail);
    std::string werr;                   // its workspace now, at its largest (a regrowth synchronises the device)
    sp->half_split = sp->cfg.tail_split == 2;
    if (sp->net_tail->ensure_workspace(sp->half_split ? sp->rows_max / 2 + 1024 : 1023, werr) != M0_OK) {
        m0_set_error("tail split: " + werr);
        return false;
    }
    return true;
}

// the device side of a new engine; false with the error string set
static bool build_engine(m0_selfplay* sp) {
    if (!alloc_tree_arenas(sp) || !alloc_position_tables(sp) || !alloc_eval_cache(sp) || !alloc_batch_buffers(sp)) return false;
    sp->hg.assign(sp->G, GameDev());
    for (auto& g : sp->hg) memset(&g, 0, sizeof(GameDev));
    sp->games.assign(sp->G, HostGame());
    sp->hres.resize(sp->G);
    sp->hsamples.resize((size_t)sp->G * (sp->L + 1));
    sp->prev_done.assign(sp->G, 0);
    for (hipEvent_t* e : {&sp->ev0, &sp->ev1, &sp->ev2, &sp->ev3}) M0_HIP(sp->hip, hipEventCreate(e));
    if (!hip_ok(sp, "hipEventCreate failed") || !make_tail_view(sp)) return false;
    std::string err;
    if (sp->net && sp->net->ensure_workspace(sp->rows_max, err) != M0_OK) { m0_set_error(err); return false; }
    if (sp->net && sp->net_b && sp->net_b->ensure_workspace(sp->rows_max, err) != M0_OK) { m0_set_error(err); return false; }
    // the clears ride the engine's stream; wait once so that an allocation / clear failure surfaces here, not in the first step
    M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
    return hip_ok(sp, "clearing the search arenas failed");
}

m0_selfplay* m0::engine_create(m0_net* nh, m0_net* nh_b, const m0_selfplay_cfg* cfg, EngineKind kind) {
    if (!cfg) { m0_set_error("cfg is null"); return nullptr; }
    if (cfg->concurrent_games <= 0 || cfg->inference_batch_size <= 0 || cfg->num_simulations <= 0) {
        m0_set_error("concurrent_games, inference_batch_size and num_simulations must be positive");
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { m0_set_error("no HIP device available (no CPU fallback)"); return nullptr; }
    // a failure below destroys what has been built so far
    std::unique_ptr<m0_selfplay, decltype(&m0_selfplay_destroy)> owner(new m0_selfplay(), &m0_selfplay_destroy);
    m0_selfplay* sp = owner.get();
    sp->cfg = *cfg;
    sp->nethandle = nh;
    sp->nethandle_b = nh_b;
    sp->net = m0_net_impl(nh);
    sp->net_b = m0_net_impl(nh_b);
    sp->kind = kind;
    const bool match = kind == EngineKind::Match;
    sp->cfg.arena_mode = match ? 1 : 0;
    // A match engine alternates two networks in one game slot and the cache key covers the position only (no network id):
    // with ONE cache side B's leaves would be expanded from side A's cached value and logits.  eval_cache is therefore ignored
    // there, whatever the caller asked for; arena_eval_cache gives each network a cache of its own (EvalCache::sides).
    if (match) sp->cfg.eval_cache = 0;
    else { sp->cfg.arena_eval_cache = 0; sp->cfg.arena_paired_openings = 0; }
    fill_tree_cfg(sp->cfg, match, sp->tc);
    sp->device = nh ? m0_net_device(nh) : 0;
    if (nh) forward_gate_join(sp);
    M0_HIP(sp->hip, hipSetDevice(sp->device));
    if (nh) sp->stream = m0_net_stream(nh);
    else { M0_HIP(sp->hip, hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking)); sp->own_stream = true; }
    sp->G = cfg->concurrent_games;
    sp->L = cfg->inference_batch_size;
    sp->rows_max = (sp->G * (sp->L + 1) + 3) & ~3;      // L leaves + the re-evaluation of a reused root, per game
    memset(&sp->stats, 0, sizeof(sp->stats));
    memset(&sp->d, 0, sizeof(sp->d));
    return hip_ok(sp, "engine stream") && build_engine(sp) ? owner.release() : nullptr;
}

// The leaves of the last select as f32 planes for an external evaluator: rows [0, rows_a) into planes_a and, for a match
// engine, rows [net_row_base, net_row_base + rows_b) into planes_b (rows_b = 0 with one network).
static int leaf_planes(m0_selfplay* sp, int rows_a, float* planes_a, int rows_b, float* planes_b) {
    sync_games_d2h(sp);
    if (!M0_HIP(sp->hip, hipMemcpy(sp->hsamples.data(), sp->d.samples, sizeof(Sample) * (size_t)sp->G * (sp->L + 1), hipMemcpyDeviceToHost)))
        return m0_hip_error(sp->hip, "device sync failed");
    const int base = sp->d.net_row_base;
    for (int g = 0; g < sp->G; ++g) {
        if (!sp->hg[g].active) continue;
        for (int s = 0; s < sp->hg[g].nsamples; ++s) {
            const Sample& smp = sp->hsamples[(size_t)g * (sp->L + 1) + s];
            if (!sample_owns_row(smp.kind) || smp.row < 0) continue;
            if (smp.row < rows_a) encode_planes_f32(smp.pos, planes_a + (size_t)smp.row * 19 * 64);
            else if (smp.row >= base && smp.row < base + rows_b) encode_planes_f32(smp.pos, planes_b + (size_t)(smp.row - base) * 19 * 64);
        }
    }
    return M0_OK;
}

// An external evaluator's results for `rows` rows of the batch, starting at row_base, onto the engine's stream (a failure stays
// in sp->hip: the expand that follows is not launched and reports it).
static void upload_eval(m0_selfplay* sp, size_t row_base, const float* logits, const float* values, int rows) {
    if (rows <= 0) return;
    M0_HIP(sp->hip, hipMemcpyAsync(sp->logits_dev + row_base * 4672, logits, (size_t)rows * 4672 * 4, hipMemcpyHostToDevice, sp->stream));
    M0_HIP(sp->hip, hipMemcpyAsync(sp->values_dev + row_base, values, (size_t)rows * 4, hipMemcpyHostToDevice, sp->stream));
}

// first half of a step for an external evaluator: select, then the leaves' planes on the host (region 0 = network A / the only
// network, region 1 = network B of a match engine, whose rows start at d.net_row_base on the device)
int m0::ext_select_impl(m0_selfplay* sp, int* rows_a, int* rows_b, float* planes_a, float* planes_b, int max_rows) {
    if (sp->ext_pending) { m0_set_error("m0_selfplay_ext_expand outstanding"); return M0_ERR_STATE; }
    // select applies virtual losses and reserves batch rows: refuse a buffer that cannot take the worst case BEFORE it runs
    // (an error after it would leave the engine waiting for an ext_expand the caller has no planes for)
    if (!planes_a || (sp->kind == EngineKind::Match && !planes_b) || max_rows < sp->G * (sp->L + 1)) {
        m0_set_error("planes buffer too small: concurrent_games * (inference_batch_size + 1) rows are required");
        return M0_ERR_INVALID;
    }
    int rc = refill(sp);
    if (rc != M0_OK) return rc;
    int r = 0;
    if ((rc = run_select(sp, &r)) != M0_OK) return rc;
    const int rb = sp->kind == EngineKind::Match ? sp->rows2[1] : 0;
    if (r > sp->rows_max || rb > sp->rows_max) { m0_set_error("row counter overflow"); return M0_ERR_STATE; }
    *rows_a = r;
    if (rows_b) *rows_b = rb;
    sp->last_rows = r;
    sp->last_rows_b = rb;
    sp->ext_pending = true;
    if (r + rb > 0) return leaf_planes(sp, r, planes_a, rb, planes_b);
    return M0_OK;
}

int m0::ext_expand_impl(m0_selfplay* sp, const float* logits_a, const float* values_a, int rows_a, const float* logits_b,
                           const float* values_b, int rows_b) {
    if (!sp->ext_pending) { m0_set_error("no m0_selfplay_ext_select outstanding"); return M0_ERR_STATE; }
    if (rows_a != sp->last_rows || rows_b != sp->last_rows_b) { m0_set_error("rows does not match the last select"); return M0_ERR_INVALID; }
    if ((rows_a > 0 && (!logits_a || !values_a)) || (rows_b > 0 && (!logits_b || !values_b))) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    upload_eval(sp, 0, logits_a, values_a, rows_a);
    upload_eval(sp, (size_t)sp->d.net_row_base, logits_b, values_b, rows_b);
    sp->ext_pending = false;
    M0_HIP(sp->hip, hipEventRecord(sp->ev0, sp->stream)); M0_HIP(sp->hip, hipEventRecord(sp->ev1, sp->stream));
    return finish_step(sp, rows_a + rows_b, now_ms());
}

bool m0::kind_accepted(const m0_selfplay* sp, const char* what, unsigned kinds) {
    if (kinds & (1u << (int)sp->kind)) return true;
    static const char* const is_a[] = {"a self-play engine", "a match engine", "an analysis engine"};
    const char* only = kinds == KIND_SELFPLAY ? "self-play engines" : kinds == KIND_MATCH ? "match engines"
                     : kinds == KIND_ANALYSIS ? "analysis engines" : "self-play and match engines";
    m0_set_error(std::string(what) + ": " + only + " only, this is " + is_a[(int)sp->kind]);
    return false;
}

extern "C" {

m0_selfplay* m0_selfplay_create(m0_net* nh, const m0_selfplay_cfg* cfg) { return engine_create(nh, nullptr, cfg, EngineKind::SelfPlay); }

m0_selfplay* m0_arena_create(m0_net* net_a, m0_net* net_b, const m0_selfplay_cfg* cfg) {
    if (!net_a || !net_b) { m0_set_error("m0_arena_create needs two networks"); return nullptr; }
    if (m0_net_device(net_a) != m0_net_device(net_b)) { m0_set_error("both networks must live on the same HIP device"); return nullptr; }
    if (cfg && (cfg->ssl_in_forward || cfg->ssl_targets)) { m0_set_error("arena games carry no SSL outputs"); return nullptr; }
    return engine_create(net_a, net_b, cfg, EngineKind::Match);
}

m0_selfplay* m0_arena_create_ext(const m0_selfplay_cfg* cfg) {
    if (cfg && (cfg->ssl_in_forward || cfg->ssl_targets)) { m0_set_error("arena games carry no SSL outputs"); return nullptr; }
    return engine_create(nullptr, nullptr, cfg, EngineKind::Match);
}

void m0_selfplay_destroy(m0_selfplay* sp) {
    if (!sp) return;
    forward_gate_leave(sp);
    (void)hipSetDevice(sp->device);
    if (sp->stream) (void)hipStreamSynchronize(sp->stream);
    if (sp->stream_tail) (void)hipStreamSynchronize(sp->stream_tail);
    delete sp->net_tail;
    if (sp->ev_sel) (void)hipEventDestroy(sp->ev_sel);
    if (sp->ev_tail) (void)hipEventDestroy(sp->ev_tail);
    if (sp->stream_tail) (void)hipStreamDestroy(sp->stream_tail);
    for (void* p : sp->allocs) (void)hipFree(p);
    for (auto& r : sp->done_meta) delete (GameRecordOwner*)r.owner;
    delete sp->an;
    if (sp->ev0) { (void)hipEventDestroy(sp->ev0); (void)hipEventDestroy(sp->ev1); (void)hipEventDestroy(sp->ev2); (void)hipEventDestroy(sp->ev3); }
    if (sp->own_stream && sp->stream) (void)hipStreamDestroy(sp->stream);
    delete sp;
}

int m0_selfplay_set_openings(m0_selfplay* sp, const char* const* fens, int n) {
    if (!sp || n < 0 || (n > 0 && !fens)) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_set_openings", KIND_GAMES, false);
    if (sp->stats.games_started != 0) { m0_set_error("set the opening book before the first step"); return M0_ERR_STATE; }
    std::vector<Pos> book(n);
    for (int i = 0; i < n; ++i)
        if (!fens[i] || parse_fen(fens[i], book[i]) != 0) { m0_set_error(std::string("bad FEN at index ") + std::to_string(i)); return M0_ERR_INVALID; }
    sp->book.swap(book);
    sp->book_fens.assign(fens, fens + n);
    return M0_OK;
}

int m0_selfplay_ext_select(m0_selfplay* sp, int* rows, float* planes, int max_rows) {
    if (!sp || !rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_ext_select", KIND_SELFPLAY, true);
    return ext_select_impl(sp, rows, nullptr, planes, nullptr, max_rows);
}

int m0_selfplay_ext_expand(m0_selfplay* sp, const float* logits, const float* values, int rows) {
    M0_ENGINE_CALL(sp, "m0_selfplay_ext_expand", KIND_SELFPLAY, true);
    return ext_expand_impl(sp, logits, values, rows, nullptr, nullptr, 0);
}

int m0_arena_ext_select(m0_selfplay* sp, int* rows_a, int* rows_b, float* planes_a, float* planes_b, int max_rows) {
    if (!sp || !rows_a || !rows_b) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_arena_ext_select", KIND_MATCH, true);
    return ext_select_impl(sp, rows_a, rows_b, planes_a, planes_b, max_rows);
}

int m0_arena_ext_expand(m0_selfplay* sp, const float* logits_a, const float* values_a, int rows_a, const float* logits_b,
                        const float* values_b, int rows_b) {
    M0_ENGINE_CALL(sp, "m0_arena_ext_expand", KIND_MATCH, true);
    return ext_expand_impl(sp, logits_a, values_a, rows_a, logits_b, values_b, rows_b);
}

int m0_selfplay_step(m0_selfplay* sp, int steps) {
    M0_ENGINE_CALL(sp, "m0_selfplay_step", KIND_GAMES, true);
    if (sp->ext_pending) { m0_set_error("m0_selfplay_ext_expand outstanding"); return M0_ERR_STATE; }
    int rc = refill(sp);
    for (int i = 0; i < steps && rc == M0_OK; ++i) {
        if (sp->stats.active_games == 0 && sp->stats.steps > 0) break;
        rc = one_step(sp);
    }
    return rc;
}

int m0_selfplay_stats_get(m0_selfplay* sp, m0_selfplay_stats* out) {
    if (!sp || !out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_stats_get", KIND_ANY, false);
    *out = sp->stats;
    return M0_OK;
}

int m0_selfplay_poll(m0_selfplay* sp, m0_game_record* out) {
    if (!sp || !out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_poll", KIND_GAMES, false);
    if (sp->done_meta.empty()) return 0;
    *out = sp->done_meta.front();
    sp->done_meta.pop_front();
    return 1;
}

void m0_game_record_free(m0_game_record* rec) {
    if (rec && rec->owner) { delete (GameRecordOwner*)rec->owner; rec->owner = nullptr; }
}

int m0_selfplay_running(m0_selfplay* sp) {
    M0_ENGINE_CALL_OR(0, sp, "m0_selfplay_running", KIND_ANY, false);
    if (sp->stats.games_started == 0) return 1;
    if (sp->stats.active_games > 0) return 1;
    return (sp->cfg.total_games <= 0 || sp->next_game < sp->cfg.total_games) ? 1 : 0;
}

// ---------------- split-step search ----------------
int m0_search_begin(m0_selfplay* sp, int g, const char* fen, int sims, int dirichlet, int game_uid) {
    if (!sp || !fen || g < 0 || g >= sp->G || sims <= 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_search_begin", KIND_GAMES, true);
    Line line;                             // history-less
    if (parse_fen(fen, line.pos) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    if (!sync_games_d2h(sp)) return m0_hip_error(sp->hip, "device sync failed");
    occupy_slot(sp, g, std::move(line), game_uid);
    sp->search_begun = true;
    begin_search(sp, g, sims, dirichlet != 0, ROOT_FRESH);
    return apply_advances(sp);
}

int m0_search_select(m0_selfplay* sp, int* rows, float* planes, int max_rows) {
    if (!sp || !rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_search_select", KIND_GAMES, true);
    int r = 0;
    { const int rc = run_select(sp, &r); if (rc != M0_OK) return rc; }
    *rows = r;
    sp->last_rows = r;
    if (planes && r > 0) {
        if (r > max_rows) { m0_set_error("planes buffer too small"); return M0_ERR_INVALID; }
        return leaf_planes(sp, r, planes, 0, nullptr);
    }
    return M0_OK;
}

int m0_search_expand(m0_selfplay* sp, const float* logits, const float* values, int rows) {
    if (!sp) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_search_expand", KIND_GAMES, true);
    if (rows != sp->last_rows || rows > sp->rows_max) { m0_set_error("rows does not match the last select"); return M0_ERR_INVALID; }
    if (rows > 0 && (!logits || !values)) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    upload_eval(sp, 0, logits, values, rows);
    std::vector<uint8_t> was_finished(sp->G);
    for (int g = 0; g < sp->G; ++g) was_finished[g] = sp->hg[g].finished ? 1 : 0;
    M0_HIP(sp->hip, launch_expand(sp->d, sp->tc, sp->stream));
    if (!sync_games_d2h(sp)) return m0_hip_error(sp->hip, "expand failed");
    sp->stats.evals += (uint64_t)rows;
    // a search that this expand finished with a refused expansion behind it: counted once, as the fused step does (harvest_games)
    for (int g = 0; g < sp->G; ++g)
        if (sp->hg[g].active && sp->hg[g].finished && !was_finished[g] && sp->hg[g].overflow) sp->stats.arena_overflows++;
    if (sp->tc.eval_cache) {               // as finish_step does
        uint64_t h = 0;
        for (int g = 0; g < sp->G; ++g) h += sp->hg[g].cache_hits;
        sp->stats.evals_cached = h;
    }
    return M0_OK;
}

int m0_search_result(m0_selfplay* sp, int g, int* nchild, int32_t* child_n, uint16_t* child_mv, int32_t* child_idx,
                     double* child_prior, double* child_q, double* root_q, int* root_n, int* finished) {
    if (!sp || g < 0 || g >= sp->G) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_search_result", KIND_GAMES, true);
    if (finished) *finished = sp->hg[g].finished;
    if (!sp->hg[g].finished) { if (nchild) *nchild = 0; return M0_OK; }
    if (!M0_HIP(sp->hip, hipMemcpy(&sp->hres[g], sp->d.results + g, sizeof(RootResult), hipMemcpyDeviceToHost)))
        return m0_hip_error(sp->hip, "result copy failed");
    const RootResult& R = sp->hres[g];
    if (nchild) *nchild = R.nchild;
    for (int i = 0; i < R.nchild; ++i) {
        if (child_n) child_n[i] = R.child_n[i];
        if (child_mv) child_mv[i] = R.child_mv[i];
        if (child_idx) child_idx[i] = R.child_idx[i];
        if (child_prior) child_prior[i] = R.child_prior[i];
        if (child_q) child_q[i] = R.child_q[i];
    }
    if (root_q) *root_q = R.root_n > 0 ? R.root_q : sp->hg[g].root_v;
    if (root_n) *root_n = R.root_n;
    return M0_OK;
}

int m0_search_advance(m0_selfplay* sp, int g, int slot, int sims, int dirichlet) {
    if (!sp || g < 0 || g >= sp->G || sims <= 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_search_advance", KIND_GAMES, true);
    // refresh the mirror first: an earlier advance changed root/next/arena on the device only
    if (!sync_games_d2h(sp)) return m0_hip_error(sp->hip, "device sync failed");
    if (!sp->hg[g].finished) { m0_set_error("search not finished"); return M0_ERR_STATE; }
    if (!M0_HIP(sp->hip, hipMemcpy(&sp->hres[g], sp->d.results + g, sizeof(RootResult), hipMemcpyDeviceToHost)))
        return m0_hip_error(sp->hip, "result copy failed");
    const RootResult& R = sp->hres[g];
    if (slot < 0 || slot >= R.nchild) { m0_set_error("child slot out of range"); return M0_ERR_INVALID; }
    sp->games[g].play(R.child_mv[slot]);
    const bool fresh = sp->cfg.fresh_tree_per_move || sp->cfg.tt_merge || is_gumbel(sp->tc);
    begin_search(sp, g, sims, dirichlet != 0, fresh ? ROOT_FRESH : slot);
    return apply_advances(sp);
}

int m0_selfplay_last_batch_nhwc(m0_selfplay* sp, uint16_t* out, int max_rows, int* rows) {
    if (!sp || !out || !rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    M0_ENGINE_CALL(sp, "m0_selfplay_last_batch_nhwc", KIND_ANY, true);
    const int r = sp->last_rows;
    if (r > max_rows) { m0_set_error("output buffer too small"); return M0_ERR_INVALID; }
    *rows = r;
    if (r > 0) {
        M0_HIP(sp->hip, hipMemcpyAsync(out, sp->d.x0, (size_t)r * 64 * 32 * 2, hipMemcpyDeviceToHost, sp->stream));
        if (!M0_HIP(sp->hip, hipStreamSynchronize(sp->stream))) return m0_hip_error(sp->hip, "copy failed");
    }
    return M0_OK;
}

}  // extern "C"
