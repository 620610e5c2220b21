// Host engine: drives the device trees and the network, plays the games.
// Mirrors the per-game loop of selfplay_worker (azchess/selfplay/internal.py:326-679) for many
// concurrent games: opening plies, draw adjudication, temperature, MCTS.run bookkeeping
// (mcts.py:318-512), move sampling, resign logic, result and record assembly.
// The engine's C-ABI (creation, step, poll, external evaluators, split-step search) is capi_selfplay.hip.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include "selfplay_engine.h"
#include "tb.h"

namespace m0 {

// mcts.py:359-371: a root that run() finds already in its table is evaluated again unless the position sits in nn_cache
// (which only this branch fills).  Returns true when the evaluation has to be made; updates the LRU either way.
static bool nn_cache_miss(m0_selfplay* sp, uint64_t key) {
    auto it = sp->nn_map.find(key);
    if (it != sp->nn_map.end()) {
        sp->nn_lru.splice(sp->nn_lru.end(), sp->nn_lru, it->second);
        return false;
    }
    sp->nn_lru.push_back(key);
    sp->nn_map[key] = std::prev(sp->nn_lru.end());
    if (sp->nn_lru.size() > 10000) { sp->nn_map.erase(sp->nn_lru.front()); sp->nn_lru.pop_front(); }
    return true;
}

static void seed_game_dev(GameDev& g, uint64_t base, int uid) {
    g.seed_jitter = derive_seed(base, uid, PURPOSE_JITTER);
    g.seed_noise = derive_seed(base, uid, PURPOSE_NOISE);
    g.seed_dir = derive_seed(base, uid, PURPOSE_DIRICHLET);
    g.seed_gumbel = derive_seed(base, uid, PURPOSE_GUMBEL);
    g.ctr_jitter = g.ctr_noise = g.ctr_dir = g.ctr_gumbel = 0;
    g.gumbel_miss = 0;
}

bool sync_games_d2h(m0_selfplay* sp) {
    M0_HIP(sp->hip, hipMemcpyAsync(sp->hg.data(), sp->d.games, sizeof(GameDev) * sp->G, hipMemcpyDeviceToHost, sp->stream));
    return M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
}
bool sync_games_h2d(m0_selfplay* sp) {
    return M0_HIP(sp->hip, hipMemcpyAsync(sp->d.games, sp->hg.data(), sizeof(GameDev) * sp->G, hipMemcpyHostToDevice, sp->stream));
}
static void push_hist(m0_selfplay* sp, int slot, const RepWindow& w) {
    int n = (int)w.keys.size();
    const uint64_t* src = w.keys.data();
    if (n > M0_HIST_CAP) { src += n - M0_HIST_CAP; n = M0_HIST_CAP; }
    sp->hg[slot].hist_len = n;
    if (n > 0) M0_HIP(sp->hip, hipMemcpyAsync(sp->d.hist + (size_t)slot * M0_HIST_CAP, src, (size_t)n * 8, hipMemcpyHostToDevice, sp->stream));
}

static const char* const MODE_NAMES[] = {"the PUCT search", "the Gumbel root search", "the proof search", "the self-play budget mix"};
int mode_settable(m0_selfplay* sp, SearchMode wanted, const char* name) {
    // stats.steps counts for the engines that start no games (analysis); where games are played one has started before a step ends
    if (sp->stats.games_started != 0 || sp->stats.steps != 0 || sp->search_begun) {
        m0_set_error(std::string("set ") + name + " before the first step or search"); return M0_ERR_STATE;
    }
    const char* other = sp->cfg.tt_merge ? "compat.tt_merge"
                        : sp->tc.mode != MODE_PUCT && sp->tc.mode != wanted ? MODE_NAMES[sp->tc.mode] : nullptr;
    if (other) { m0_set_error(std::string(name) + " does not go with " + other); return M0_ERR_INVALID; }
    return M0_OK;
}
// The results of slots [first, first + count), device -> host mirrors: RootResult and what the engine's mode writes beside it when a
// search finishes, described by its device array, host mirror and element size (PUCT and the budget mix write nothing more).
static bool results_d2h(m0_selfplay* sp, int first, int count) {
    struct { const void* dev; void* host; size_t size; } m = {nullptr, nullptr, 0};
    if (is_gumbel(sp->tc)) m = {sp->d.gumbel_results, sp->hgres.data(), sizeof(GumbelResult)};
    if (is_proof(sp->tc)) m = {sp->d.proof_results, sp->hpres.data(), sizeof(ProofResult)};
    return M0_HIP(sp->hip, hipMemcpy(&sp->hres[first], sp->d.results + first, sizeof(RootResult) * count, hipMemcpyDeviceToHost)) &&
           (!m.size || M0_HIP(sp->hip, hipMemcpy((char*)m.host + first * m.size, (const char*)m.dev + first * m.size, m.size * count,
                                                 hipMemcpyDeviceToHost)));
}
int mode_result_fetch(m0_selfplay* sp, int g, SearchMode mode, const char* what, bool* finished) {
    *finished = false;
    if (g < 0 || g >= sp->G) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    if (sp->tc.mode != mode) { m0_set_error(std::string(what) + ": " + MODE_NAMES[mode] + " is not set on this engine"); return M0_ERR_STATE; }
    if (!sp->hg[g].finished) return M0_OK;
    if (!results_d2h(sp, g, 1)) return m0_hip_error(sp->hip, "result copy failed");
    *finished = true;
    return M0_OK;
}

// configure a search on slot for the host position (MCTS.run prologue, mcts.py:342-396)
static void arm_search(m0_selfplay* sp, int slot, const Pos& pos, const RepWindow& win, int sims, bool dirichlet, bool fresh) {
    GameDev& g = sp->hg[slot];
    g.root_pos = pos;
    g.active = 1; g.sims_done = 0; g.sims_target = sims;
    g.need_dirichlet = dirichlet && !is_gumbel(sp->tc) ? 1 : 0;    // the Gumbel root takes no Dirichlet noise
    g.gumbel_drawn = 0;
    // budget mix: forced playouts at the root of a full search (every split-step search of such an engine is a full one)
    g.forced = is_budget(sp->tc) && sp->budget.forced_k > 0.0 && sp->games[slot].cur_full ? 1 : 0;
    g.root_q_from_v = 0;
    g.root_fresh = fresh ? 1 : 0;
    g.flip_root_v = (sp->cfg.value_from_white && pos.turn == BLACK) ? 1 : 0;
    g.finished = 0; g.nsamples = 0;
    g.reinfer = (sp->cfg.root_reinfer && !fresh && nn_cache_miss(sp, tkey(pos))) ? 1 : 0;
    sp->prev_done[slot] = 0;
    push_hist(sp, slot, win);
}

HostGame& occupy_slot(m0_selfplay* sp, int slot, Line&& line, int uid) {
    HostGame& hgm = sp->games[slot];
    hgm = HostGame();
    static_cast<Line&>(hgm) = std::move(line);
    hgm.in_use = true;
    hgm.game_index = uid;
    seed_game_dev(sp->hg[slot], sp->cfg.seed, uid);
    sp->hg[slot].evals = 0;
    return hgm;
}

void arm_slot_search(m0_selfplay* sp, int slot, int sims, bool dirichlet, bool fresh) {
    const HostGame& hgm = sp->games[slot];
    arm_search(sp, slot, hgm.pos, hgm.win, sims, dirichlet, fresh);
}

void begin_search(m0_selfplay* sp, int slot, int sims, bool dirichlet, int root) {
    arm_slot_search(sp, slot, sims, dirichlet, root < 0);
    sp->adv.push(slot, root);
}

static void finish_game(m0_selfplay* sp, int slot, bool resigned, int resigner, bool have_z, float z_in) {
    HostGame& hgm = sp->games[slot];
    const m0_selfplay_cfg& c = sp->cfg;
    const bool match = sp->kind == EngineKind::Match;
    float z = z_in;
    if (!have_z) {
        // internal.py:587-599 computed per game (SURVEY B-8: the reference's stale-z reuse is not reproduced)
        if (is_game_over(hgm.pos, hgm.win, true)) z = game_result(hgm.pos);
        else if (match) z = 0.f;                                     // arena.py:121-123: unfinished = 1/2-1/2
        else z = hgm.search_values.empty() ? 0.f : hgm.search_values.back();
    }
    sp->stats.games_finished++;
    if ((c.record_games && hgm.nstates > 0) || match) {
        GameRecordOwner* o = new GameRecordOwner();
        o->s.swap(hgm.states); o->pi.swap(hgm.pis); o->legal_mask.swap(hgm.masks);
        o->search_values = hgm.search_values;
        o->z.resize(hgm.nstates);
        for (int i = 0; i < hgm.nstates; ++i) o->z[i] = z * (float)hgm.turns[i];
        o->played.assign(hgm.history.begin(), hgm.history.end());
        if (is_budget(sp->tc)) { o->budget = true; o->full = hgm.full; o->sims.assign(hgm.sims_used.begin(), hgm.sims_used.end()); }
        if (hgm.book_index >= 0) o->start_fen = sp->book_fens[hgm.book_index];
        if (c.ssl_targets && (int)hgm.rec_pos.size() == hgm.nstates) {
            // targets for all plies of the game in one launch on the engine stream
            const int T = hgm.nstates;
            if (T > sp->ssl_cap) {             // a game longer than the staging buffers (max_game_len <= 0): grow them
                Pos* np = dalloc<Pos>(sp, (size_t)T + 64);
                float* no = dalloc<float>(sp, ((size_t)T + 64) * 17 * 64);
                if (np && no) { sp->ssl_pos_dev = np; sp->ssl_out_dev = no; sp->ssl_cap = T + 64; }   // the old pair is freed with the engine
                else sp->stats.ssl_dropped++;
            }
            if (T <= sp->ssl_cap) {
                o->ssl.resize((size_t)T * 17 * 64);
                M0_HIP(sp->hip, hipMemcpyAsync(sp->ssl_pos_dev, hgm.rec_pos.data(), sizeof(Pos) * T, hipMemcpyHostToDevice, sp->stream));
                M0_HIP(sp->hip, launch_ssl_targets(sp->ssl_pos_dev, T, sp->ssl_out_dev, sp->stream));
                M0_HIP(sp->hip, hipMemcpyAsync(o->ssl.data(), sp->ssl_out_dev, (size_t)T * 17 * 64 * 4, hipMemcpyDeviceToHost, sp->stream));
                if (!M0_HIP(sp->hip, hipStreamSynchronize(sp->stream))) o->ssl.clear();   // no targets in the record; the step fails
            }
        }
        m0_game_record r;
        memset(&r, 0, sizeof(r));
        r.game_index = hgm.game_index; r.moves = hgm.nstates; r.resigned = resigned ? 1 : 0; r.resigner = resigner;
        r.draw = z == 0.0f ? 1 : 0; r.total_plies = (int)hgm.history.size(); r.result = z;
        r.avg_policy_entropy = (float)(hgm.entropy_sum / (double)(hgm.entropy_count > 0 ? hgm.entropy_count : 1));
        double ss = 0; for (int v : hgm.sims_used) ss += v;
        r.avg_sims = hgm.sims_used.empty() ? 0.f : (float)(ss / (double)hgm.sims_used.size());
        r.secs = (now_ms() - hgm.t0) / 1000.0;
        r.s = o->s.data(); r.pi = o->pi.data(); r.z = o->z.data(); r.legal_mask = o->legal_mask.data();
        r.search_values = o->search_values.data(); r.played = o->played.data(); r.owner = o;
        r.ssl = o->ssl.empty() ? nullptr : o->ssl.data();
        r.start_fen = hgm.book_index >= 0 ? o->start_fen.c_str() : nullptr;
        sp->done_meta.push_back(r);
    }
    hgm.in_use = false;
    sp->hg[slot].active = 0;
}

// top of the per-ply loop (internal.py:382-408): termination tests, then arm the search
static void begin_move(m0_selfplay* sp, int slot, int child_slot) {
    HostGame& hgm = sp->games[slot];
    const m0_selfplay_cfg& c = sp->cfg;
    const bool match = sp->kind == EngineKind::Match;
    DrawCfg dc = draw_cfg_from(c);
    // self-play: internal.py:382-408; arena: `while not board.is_game_over(claim_draw=True) and moves < max_moves`
    // then the adjudication test (arena.py:68-72)
    if (is_game_over(hgm.pos, hgm.win, match) || hgm.nstates >= c.max_game_len ||
        should_adjudicate_draw(hgm.pos, hgm.win, hgm.history, dc)) {
        finish_game(sp, slot, false, 0, false, 0.f);
        return;
    }
    int root = child_slot;
    if (match) {
        root = ROOT_FRESH;                                         // a fresh tree per move (see m0_arena_create)
        sp->hg[slot].net_id = ((hgm.pos.turn == WHITE) == hgm.a_is_white) ? 0 : 1;
    }
    // mcts.py:378-387 draws random.randint only when the cap is configured
    const bool cap_draws = c.playout_random_frac > 0.0 && c.num_simulations > 0;
    // budget mix (include/m0_budget.h): the ply's draw of the game's budget stream decides between a full and a fast search
    hgm.cur_full = !is_budget(sp->tc) || budget_is_full(c.seed, hgm.game_index, hgm.nstates, sp->budget.full_prob);
    if (is_budget(sp->tc)) ++(hgm.cur_full ? sp->budget_full : sp->budget_fast);
    const int budget = hgm.cur_full ? c.num_simulations : sp->budget.fast_simulations;
    int sims = playout_cap(budget, c.playout_random_frac, cap_draws ? hgm.rng.next() : 0.0);
    hgm.cur_sims = sims;
    if (c.fresh_tree_per_move || c.tt_merge) root = ROOT_FRESH;   // tt_merge: the table lives for one search (see m0_engine.h)
    if (is_gumbel(sp->tc)) root = ROOT_FRESH;                      // the halving schedule assumes unvisited root children
    // ... except in a match engine, where each side's table lives for the whole game
    if (match && c.tt_merge) root = hgm.nstates == 0 ? ROOT_FIRST_OF_GAME : ROOT_FROM_SIDE_TABLE;
    const bool dir = (c.dirichlet_plies < 0 || hgm.nstates < c.dirichlet_plies) && hgm.cur_full;   // a fast search takes no noise
    begin_search(sp, slot, sims, dir, root);
}

static void start_game(m0_selfplay* sp, int slot) {
    const bool match = sp->kind == EngineKind::Match;
    Line start;
    parse_fen(START_FEN, start.pos);
    HostGame& hgm = occupy_slot(sp, slot, std::move(start), sp->cfg.first_game_index + sp->next_game++);
    sp->stats.games_started++;
    hgm.rng = HStream(derive_seed(sp->cfg.seed, hgm.game_index, PURPOSE_GAME));
    if (!sp->book.empty()) {               // get_opening_position (internal.py:65-69): random.choice(OPENING_BOOK)
        // a paired match: games 2k and 2k+1 share the draw of pair k's own stream (and leave their own streams alone), so each
        // opening is played with both colours whichever slot takes the games and whenever they start
        const bool paired = match && sp->cfg.arena_paired_openings;
        const double u = paired ? HStream(derive_seed(sp->cfg.seed, hgm.game_index / 2, PURPOSE_PAIR_OPENING)).next() : hgm.rng.next();
        size_t k = (size_t)(u * (double)sp->book.size());
        if (k >= sp->book.size()) k = sp->book.size() - 1;
        hgm.pos = sp->book[k];
        hgm.book_index = (int)k;
    }
    hgm.t0 = now_ms();
    hgm.a_is_white = (hgm.game_index % 2) == 0;               // arena.py:66
    // a match engine's caches hold what each NETWORK said; the next game of the slot swaps the colours (advance_kernel clears)
    if (match && sp->tc.eval_cache) sp->hg[slot].ec_clear = 1;
    // opening diversity: uniform random legal plies (internal.py:366-379; random.choice -> injected stream)
    for (int i = 0; i < sp->cfg.opening_random_plies; ++i) {
        if (is_game_over(hgm.pos, hgm.win, false)) break;
        Move mv[M0_MAX_MOVES];
        int n = gen_legal(hgm.pos, mv);
        if (n <= 0) break;
        int k = (int)(hgm.rng.next() * n);
        if (k >= n) k = n - 1;
        hgm.play(mv[k]);
    }
    begin_move(sp, slot, ROOT_FRESH);
}

// What a finished search gives the game loop -- the only part of a ply's end that knows the search modes.
// target: per root child its share of the policy target (recorded as float); visits: the counts the move is sampled from; pick: the
// move the search picked itself (index into the root children), -1: it is sampled
struct SearchOutcome { std::vector<double> target; std::vector<int32_t> visits; int pick; };
static SearchOutcome search_outcome(m0_selfplay* sp, int slot, long total) {
    const HostGame& hgm = sp->games[slot];
    const RootResult& R = sp->hres[slot];
    const int k = R.nchild;
    SearchOutcome out{std::vector<double>(k), std::vector<int32_t>(R.child_n, R.child_n + k), -1};
    for (int i = 0; i < k; ++i) out.target[i] = (double)R.child_n[i] / (double)total;     // mcts.py:828-837: visits over their sum
    auto own = [k](int pick) { return pick >= 0 && pick < k ? pick : 0; };
    if (is_gumbel(sp->tc)) {
        // the improved policy and the search's own pick: no temperature, no low_visit_threshold, the Gumbel draw is the sampling
        out.target.assign(sp->hgres[slot].pi, sp->hgres[slot].pi + k);
        out.pick = own(sp->hgres[slot].pick);
    } else if (is_budget(sp->tc) && hgm.cur_full && sp->budget.prune_targets && sp->budget.forced_k > 0.0) {
        // a full search with forced playouts and target pruning: the visits that only the forcing brought are taken out of the
        // target again, and the move is sampled from what is left (include/m0_budget.h)
        sp->budget_pruned += (uint64_t)budget_prune(k, R.child_prior, R.child_q, R.child_n, R.root_n, cpuct_at_root(sp->tc),
                                                    sp->budget.forced_k, out.visits.data(), out.target.data(), nullptr);
    } else if (is_proof(sp->tc) && sp->kind == EngineKind::Match) {
        // a match engine plays the search's own move -- the shortest proven win, the longest defence, never a move that is proven
        // lost while another is not; most visits with nothing proven -- but a sampled opening ply stays sampled till then
        const ProofResult& PR = sp->hpres[slot];
        if (PR.state != PROOF_NONE || !(sp->cfg.arena_temp > 1e-3 && hgm.nstates < sp->cfg.arena_temp_plies)) out.pick = own(PR.pick);
    }
    return out;
}

// The searched position becomes a row of the game's record (planes, policy target, legal mask) and an entry of its entropy window.
static void record_ply(m0_selfplay* sp, HostGame& hgm, const RootResult& R, const std::vector<double>& target) {
    const m0_selfplay_cfg& c = sp->cfg;
    const int k = R.nchild;
    const size_t T = (size_t)hgm.nstates;
    if (c.record_games) {
        hgm.pis.resize((T + 1) * 4672, 0.f);
        float* pi = hgm.pis.data() + T * 4672;
        for (int i = 0; i < k; ++i) pi[R.child_idx[i]] = (float)target[i];
        hgm.states.resize((T + 1) * 19 * 64);
        encode_planes_f32(hgm.pos, hgm.states.data() + T * 19 * 64);
        if (c.ssl_targets) hgm.rec_pos.push_back(hgm.pos);
        hgm.masks.resize((T + 1) * 4672, 0);
        uint8_t* mk = hgm.masks.data() + T * 4672;
        if (c.max_children > 0 || c.min_child_prior > 0.0) {          // pruned roots: the mask is still ALL legal moves
            Move lm[M0_MAX_MOVES];
            const int nl = gen_legal(hgm.pos, lm);
            for (int i = 0; i < nl; ++i) mk[move_to_index(hgm.pos, lm[i])] = 1;
        } else {
            for (int i = 0; i < k; ++i) mk[R.child_idx[i]] = 1;
        }
    }
    // entropy of pi (internal.py:430-436)
    double ent = 0.0;
    for (int i = 0; i < k; ++i) { const double p = std::max((double)(float)target[i], 1e-12); ent -= p * log(p); }   // of the recorded share
    ent -= (double)(4672 - k) * (1e-12 * log(1e-12));
    hgm.entropy_sum += ent; hgm.entropy_count++;
    hgm.resign.recent_entropies.push_back(ent);
    if ((int)hgm.resign.recent_entropies.size() > c.resign_window) hgm.resign.recent_entropies.erase(hgm.resign.recent_entropies.begin());
}

// MCTS.run epilogue + the rest of the per-ply loop body (mcts.py:431-507, internal.py:408-539): search_outcome, record_ply, then --
// here, knowing no mode -- the move (the search's own or sampled), resignation, the tablebase verdict and the next search.
static void finish_search(m0_selfplay* sp, int slot) {
    HostGame& hgm = sp->games[slot];
    const m0_selfplay_cfg& c = sp->cfg;
    const RootResult& R = sp->hres[slot];
    const int k = R.nchild;
    long total = 0;
    for (int i = 0; i < k; ++i) total += R.child_n[i];
    if (k <= 0 || total <= 0) {        // mcts.py:435-463 raises RuntimeError: the game is dropped (no record), counted
        sp->stats.arena_overflows++;   // in stats.arena_overflows, which the worker logs
        hgm.nstates = 0;               // no rows -> finish_game emits no training record
        hgm.states.clear(); hgm.pis.clear(); hgm.masks.clear(); hgm.search_values.clear(); hgm.turns.clear();
        hgm.sims_used.clear(); hgm.full.clear(); hgm.rec_pos.clear();
        finish_game(sp, slot, false, 0, true, 0.f);
        return;
    }
    const SearchOutcome out = search_outcome(sp, slot, total);
    record_ply(sp, hgm, R, out.target);
    // temperature + move choice (internal.py:386-394, 418-427, 690-735)
    int pick = out.pick;
    if (pick < 0 && sp->kind == EngineKind::Match) {  // arena.py:73-106 (the uniform is drawn only on the sampling branch, as np.random.choice is)
        const bool sampling = c.arena_temp > 1e-3 && hgm.nstates < c.arena_temp_plies;
        pick = arena_choose_move(out.visits.data(), k, c.arena_temp, hgm.nstates, c.arena_temp_plies, sampling ? hgm.rng.next() : 0.0);
    } else if (pick < 0) {
        double temp = temperature_for(hgm.pos.fullmove, c.temperature_start, c.temperature_end, c.temperature_moves);
        const int maxv = *std::max_element(R.child_n, R.child_n + k);
        if (c.low_visit_threshold > 0 && maxv < c.low_visit_threshold && temp < 0.8) temp = 0.8;
        pick = sample_move_index(out.visits.data(), k, temp, sample_move_draws(out.visits.data(), k, temp) ? hgm.rng.next() : 0.0);
    }
    const double root_q = R.root_n > 0 ? R.root_q : sp->hg[slot].root_v;
    hgm.search_values.push_back((float)root_q); hgm.turns.push_back(hgm.pos.turn == WHITE ? 1 : -1);
    hgm.sims_used.push_back(hgm.cur_sims); hgm.full.push_back(hgm.cur_full ? 1 : 0);
    hgm.nstates++; sp->stats.plies++;
    // resign (internal.py:507-536)
    if (sp->kind != EngineKind::Match && resign_update(hgm.resign, root_q, hgm.nstates, c)) {
        const bool white = hgm.pos.turn == WHITE;
        finish_game(sp, slot, true, white ? 1 : 2, true, white ? -1.f : 1.f);
        return;
    }
    hgm.play(R.child_mv[pick]);
    // tablebase hit after the move (internal.py:559-581): the game ends with the table's verdict, from White's point of view
    // (a match engine too, once the tables are attached through m0_selfplay_set_search_tablebase)
    int wdl = 0, dtm = 0;
    if (sp->tb && tb_probe(sp->tb->set, hgm.pos, sp->tb_max_pieces, wdl, dtm)) {
        sp->tb_adjudications++;
        finish_game(sp, slot, false, 0, true, (float)(hgm.pos.turn == WHITE ? wdl : -wdl));
        return;
    }
    begin_move(sp, slot, pick);
}

int run_select(m0_selfplay* sp, int* rows_out) {
    M0_HIP(sp->hip, hipMemsetAsync(sp->d.row_counter, 0, 8, sp->stream));
    M0_HIP(sp->hip, launch_select(sp->d, sp->tc, sp->stream));
    M0_HIP(sp->hip, hipMemcpyAsync(sp->rows2, sp->d.row_counter, 8, hipMemcpyDeviceToHost, sp->stream));
    if (!M0_HIP(sp->hip, hipStreamSynchronize(sp->stream))) return m0_hip_error(sp->hip, "select failed");
    *rows_out = sp->rows2[0];              // network 0's rows; network 1's (arena) start at d.net_row_base
    return M0_OK;
}

static bool launch_advances(m0_selfplay* sp) {
    const std::vector<int>& ids = sp->adv.slots;
    const std::vector<int>& roots = sp->adv.roots;
    if (!sync_games_h2d(sp)) return false;
    if (!ids.empty()) {
        M0_HIP(sp->hip, hipMemcpyAsync(sp->ids_dev, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, sp->stream));
        M0_HIP(sp->hip, hipMemcpyAsync(sp->roots_dev, roots.data(), roots.size() * 4, hipMemcpyHostToDevice, sp->stream));
        M0_HIP(sp->hip, launch_advance(sp->d, sp->ids_dev, sp->roots_dev, (int)ids.size(), sp->stream));
        if (!M0_HIP(sp->hip, hipStreamSynchronize(sp->stream))) return false;   // the list is reused by the next step
        if (sp->d.tt_sides == 2) {
            // per-side tables: only the device knows whether a root was found in its side's table.  A found root is evaluated
            // once more unless nn_cache holds the position (mcts.py:359-371; the cache belongs to the side's MCTS object).
            if (!sync_games_d2h(sp)) return false;
            bool any = false;
            for (size_t k = 0; k < ids.size(); ++k) {
                if (roots[k] > ROOT_FROM_SIDE_TABLE) continue;
                GameDev& g = sp->hg[ids[k]];
                const uint64_t salt = (g.net_id & 1) ? 0x9E3779B97F4A7C15ull : 0ull;
                const uint64_t gsalt = (uint64_t)(uint32_t)sp->games[ids[k]].game_index * 0xD6E8FEB86659FD93ull;
                g.reinfer = (g.root_found && nn_cache_miss(sp, tkey(g.root_pos) ^ salt ^ gsalt)) ? 1 : 0;
                any = any || g.reinfer;
            }
            if (any && !sync_games_h2d(sp)) return false;
        }
    }
    return true;
}

int apply_advances(m0_selfplay* sp) {
    const bool ok = launch_advances(sp);
    sp->adv.clear();
    return ok ? M0_OK : m0_hip_error(sp->hip, "advance failed");
}

static void count_active_games(m0_selfplay* sp) {
    int act = 0;
    for (int s = 0; s < sp->G; ++s) act += sp->games[s].in_use ? 1 : 0;
    sp->stats.active_games = act;
}

// a game in every free slot, as long as games remain to be played; their roots are queued in sp->adv
static void start_games(m0_selfplay* sp) {
    for (int s = 0; s < sp->G; ++s) {
        if (sp->games[s].in_use) continue;
        if (sp->cfg.total_games > 0 && sp->next_game >= sp->cfg.total_games) break;
        start_game(sp, s);
    }
}

static int start_first_games(m0_selfplay* sp) {         // lazily, at the first step
    if (sp->stats.games_started != 0) return M0_OK;
    if (!sync_games_d2h(sp)) return m0_hip_error(sp->hip, "device sync failed");
    start_games(sp);
    const int rc = apply_advances(sp);
    if (rc != M0_OK) return rc;
    count_active_games(sp);
    return M0_OK;
}

int refill(m0_selfplay* sp) {
    switch (sp->kind) {
    case EngineKind::Analysis: return analysis_refill(sp);
    default: return start_first_games(sp);
    }
}

// The searches that the last expand finished become moves; games end, free slots start the next ones.
static int harvest_games(m0_selfplay* sp) {
    if (!results_d2h(sp, 0, sp->G)) return m0_hip_error(sp->hip, "harvest failed");
    for (int s = 0; s < sp->G; ++s) {
        if (!(sp->hg[s].active && sp->hg[s].finished)) continue;
        if (sp->hg[s].overflow) sp->stats.arena_overflows++;
        finish_search(sp, s);
    }
    start_games(sp);
    return apply_advances(sp);
}

// after expand, when a search has finished
static int harvest(m0_selfplay* sp) {
    switch (sp->kind) {
    case EngineKind::Analysis: return analysis_harvest(sp);
    default: return harvest_games(sp);
    }
}

// Several engines on one GPU (engine.SelfplayPool).  By default their forwards simply overlap on the chip.  With
// M0_FORWARD_GATE=1 (read once) the forwards of engines that own a network on the same device take turns instead: what the
// second engine then adds is that its tree kernels and host work run while the other engine's forward owns the chip, and a
// conv launch's event-bracketed time stays a measurement of that kernel alone.  Measured: gated 1.098
// against 1.121 games/s with one engine in round 3 -- the gate is a measurement aid, not a speed-up, hence opt-in.  It is held
// from the first launch of a forward until its last kernel has finished and is skipped by a step without rows.
static constexpr int M0_MAX_DEVICES = 16;
static std::mutex g_forward_gate[M0_MAX_DEVICES];
static std::atomic<int> g_engines_with_net[M0_MAX_DEVICES];
static bool forward_gate_enabled() {
    static const bool on = [] { const char* v = getenv("M0_FORWARD_GATE"); return v && v[0] == '1'; }();
    return on;
}

struct ForwardGate {
    std::mutex* m = nullptr;
    hipStream_t st = nullptr;
    ForwardGate(int device, hipStream_t stream, bool has_rows) : st(stream) {
        if (has_rows && forward_gate_enabled() && (unsigned)device < (unsigned)M0_MAX_DEVICES &&
            g_engines_with_net[device].load(std::memory_order_relaxed) > 1) {
            m = &g_forward_gate[device];
            m->lock();
        }
    }
    void release() {
        if (m) { (void)hipStreamSynchronize(st); m->unlock(); m = nullptr; }
    }
    ~ForwardGate() { release(); }
};

void forward_gate_join(m0_selfplay* sp) {
    if ((unsigned)sp->device < (unsigned)M0_MAX_DEVICES) { g_engines_with_net[sp->device].fetch_add(1); sp->counted = true; }
}
void forward_gate_leave(m0_selfplay* sp) {
    if (sp->counted) g_engines_with_net[sp->device].fetch_sub(1);
}

// second half of a step: expand / backup on the device, then the host part (counters, the harvest of the finished searches)
int finish_step(m0_selfplay* sp, int rows, double t0) {
    M0_HIP(sp->hip, hipEventRecord(sp->ev2, sp->stream));
    M0_HIP(sp->hip, launch_expand(sp->d, sp->tc, sp->stream));
    M0_HIP(sp->hip, hipEventRecord(sp->ev3, sp->stream));
    if (!sync_games_d2h(sp)) return m0_hip_error(sp->hip, "step failed");
    if (sp->net) sp->net->harvest_profile();
    if (sp->net_b) sp->net_b->harvest_profile();
    float ms_sel = 0, ms_net = 0, ms_exp = 0;
    M0_HIP(sp->hip, hipEventElapsedTime(&ms_sel, sp->ev0, sp->ev1));
    M0_HIP(sp->hip, hipEventElapsedTime(&ms_net, sp->ev1, sp->ev2));
    if (!M0_HIP(sp->hip, hipEventElapsedTime(&ms_exp, sp->ev2, sp->ev3))) return m0_hip_error(sp->hip, "step failed");
    sp->stats.ms_net += ms_net; sp->stats.ms_tree += ms_sel + ms_exp;
    sp->stats.steps++; sp->stats.evals += (uint64_t)rows;
    const double t1 = now_ms();
    bool any = false;                      // a search has finished
    if (sp->tc.eval_cache) {
        uint64_t h = 0;
        for (int s = 0; s < sp->G; ++s) h += sp->hg[s].cache_hits;
        sp->stats.evals_cached = h;
    }
    for (int s = 0; s < sp->G; ++s) {
        if (!sp->hg[s].active) continue;
        const int delta = sp->hg[s].sims_done - sp->prev_done[s];
        if (delta > 0) { sp->stats.sims += (uint64_t)delta; sp->prev_done[s] = sp->hg[s].sims_done; }
        if (sp->hg[s].finished) any = true;
    }
    if (any) { const int rc = harvest(sp); if (rc != M0_OK) return rc; }
    count_active_games(sp);
    const double t2 = now_ms();
    sp->stats.ms_host += t2 - t1;
    sp->stats.ms_total += t2 - t0;
    return M0_OK;
}

// How one_step divides the rows of a pass between the network and its tail view (cfg.tail_split).
// Tail split: the rows beyond the last whole round of workgroups (1024 boards = 256 four-board tiles) go to the second instance
// on its own stream, behind the select kernel and in front of the expand kernel by events; the main launches then have no
// partial last round and the tail's workgroups fill CUs as they come free.
// tail_split = 2: the pass as two halves (the first one a whole number of rounds) on the two streams.  Two forwards side by
// side keep the chip's power draw even -- one half's attention blocks (latency-bound, low power) fall beside the other
// half's convs (power-bound) instead of running behind them at the clock they leave: +1.3 % games/s
struct RowSplit { int main_rows, tail_rows; };
static RowSplit split_rows(int rows, bool have_tail, bool half_split) {
    int main_rows = rows;
    if (have_tail && rows >= 2048 && (rows & 1023) != 0) main_rows = rows & ~1023;
    if (have_tail && half_split && rows >= 4096) main_rows = ((rows / 2) + 1023) & ~1023;
    return {main_rows, rows - main_rows};
}

int one_step(m0_selfplay* sp) {
    std::string err;                         // Net::forward's
    const double t0 = now_ms();
    M0_HIP(sp->hip, hipEventRecord(sp->ev0, sp->stream));
    int rows = 0;
    if (run_select(sp, &rows) != M0_OK) return M0_ERR_HIP;
    if (!M0_HIP(sp->hip, hipEventRecord(sp->ev1, sp->stream))) return m0_hip_error(sp->hip, "step failed");
    if (rows > sp->rows_max || sp->rows2[1] > sp->rows_max) { m0_set_error("row counter overflow"); return M0_ERR_STATE; }
    ForwardGate gate(sp->device, sp->stream, rows > 0 || sp->rows2[1] > 0);
    if (rows > 0) {
        if (!sp->net) { m0_set_error("m0_selfplay_step needs a network (use the split-step API without one)"); return M0_ERR_STATE; }
        const auto [main_rows, tail_rows] = split_rows(rows, sp->net_tail != nullptr, sp->half_split);
        float* ssl = sp->cfg.ssl_in_forward ? sp->ssl_dev : nullptr;
        if (tail_rows > 0 && !M0_HIP(sp->hip, hipEventRecord(sp->ev_sel, sp->stream)))   // the select kernel has written the batch
            return m0_hip_error(sp->hip, "step failed");
        m0_net_lock(sp->nethandle);          // an infer_np on the same backend from another thread waits here
        // main part first: its launches start at once, the tail's are enqueued while they run
        int rc = sp->net->forward(nullptr, sp->d.x0, main_rows, sp->logits_dev, sp->values_dev, ssl, sp->stream, err);
        if (rc == M0_OK && tail_rows > 0 && M0_HIP(sp->hip, hipStreamWaitEvent(sp->stream_tail, sp->ev_sel, 0))) {
            const size_t sslw = ssl ? (size_t)sp->net->ssl_channels_total() * 64 : 0;
            rc = sp->net_tail->forward(nullptr, sp->d.x0 + (size_t)main_rows * 64 * 32, tail_rows, sp->logits_dev + (size_t)main_rows * 4672,
                                       sp->values_dev + main_rows, ssl ? ssl + (size_t)main_rows * sslw : nullptr, sp->stream_tail, err);
            M0_HIP(sp->hip, hipEventRecord(sp->ev_tail, sp->stream_tail));
            M0_HIP(sp->hip, hipStreamWaitEvent(sp->stream, sp->ev_tail, 0));
        }
        m0_net_unlock(sp->nethandle);
        if (rc != M0_OK) { sp->hip.check(sp->net->hip()); m0_set_error(err); return rc; }   // a network's HIP failure is the engine's too
        if (!sp->hip.ok()) return m0_hip_error(sp->hip, "step failed");
        sp->stats.rows_tail += (uint64_t)tail_rows;
    }
    if (sp->rows2[1] > 0) {                 // arena: the other network's leaves, in their own region of the batch
        if (!sp->net_b) { m0_set_error("rows for a second network without one"); return M0_ERR_STATE; }
        const size_t b = (size_t)sp->d.net_row_base;
        m0_net_lock(sp->nethandle_b);
        int rc = sp->net_b->forward(nullptr, sp->d.x0 + b * 64 * 32, sp->rows2[1], sp->logits_dev + b * 4672,
                                    sp->values_dev + b, nullptr, sp->stream, err);
        m0_net_unlock(sp->nethandle_b);
        if (rc != M0_OK) { sp->hip.check(sp->net_b->hip()); m0_set_error(err); return rc; }
        rows += sp->rows2[1];
    }
    gate.release();
    return finish_step(sp, rows, t0);
}

}  // namespace m0
