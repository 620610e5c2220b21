// extern "C" entry points of the analysis engine (include/m0_engine.h): a list of arbitrary positions in, the best moves, the
// lines behind them and the evaluation out.  The engine is a self-play engine object that plays no games: its tree slots are
// filled from a host queue (analysis_refill, the engine's `refill`), searched by the pass of m0_selfplay_step (one_step / the
// external-evaluator pair) and emptied by the result kernel (analysis_harvest, its `harvest`); positions that ask for no search go through the position
// encoder, one forward and the policy kernel (policy_pass).
// Live searches (include/m0_analysis_live.h): a running search is read with the result kernel on its one slot (live_result:
// peek, and stop, which answers with that very readout), a search submitted with keep leaves its tree in its slot (held), and
// m0_analysis_continue re-roots a held tree by moves on the device (tree_reroot.hip) and searches on in place.
#include <string.h>
#include <algorithm>
#include <string>
#include <memory>
#include "selfplay_engine.h"
#include "planes_decode.h"
#include "tb.h"

using namespace m0;

namespace m0 {

static int searches_pending(const m0_selfplay* sp) {          // queued or searched in a slot (a held slot searches nothing)
    int n = (int)sp->an->queue.size();
    for (int s = 0; s < sp->G; ++s) n += sp->games[s].in_use && !sp->an->held[s] ? 1 : 0;
    return n;
}
static int pending_count(const m0_selfplay* sp) { return searches_pending(sp) + (int)sp->an->policy_queue.size(); }

static m0_analysis_result blank_result(const AnalysisJob& job) {
    m0_analysis_result r;
    memset(&r, 0, sizeof(r));
    r.id = job.id; r.nlegal = job.nlegal; r.sims = job.sims;
    return r;
}

// A result joins the answered ones with its root children ((policy index, visits) pairs, empty unless a harvest kept them).
static void answer(Analysis& a, const m0_analysis_result& r, std::vector<int32_t>&& children = std::vector<int32_t>(),
                   const m0_proof_lines& proof = m0_proof_lines{}) {
    a.done.push_back(r);
    a.done_children.push_back(std::move(children));
    a.done_proof.push_back(proof);
}
// the result kernel's proof output, where the engine runs the proof search
static m0_proof_lines* proof_out(const m0_selfplay* sp) { return is_proof(sp->tc) ? sp->an->proof_dev : nullptr; }
// the front of the answered results leaves: its proofs are what m0_analysis_last_proof returns from now on
static void pop_done(Analysis& a) {
    a.last_proof = a.done_proof.front();
    a.done.pop_front();
    a.done_children.pop_front();
    a.done_proof.pop_front();
}

// What m0_analysis_submit does with a position once it stands in job.line and job.nlegal is known: roots without legal moves
// and roots inside the attached tables are answered here, on the host (answered_on_host); every other one waits for a slot (or
// a policy pass).
static bool answered_on_host(m0_selfplay* sp, const AnalysisJob& job) {
    if (job.nlegal == 0) {                 // no search, no evaluation, no slot
        m0_analysis_result r = blank_result(job);
        r.status = in_check(job.line.pos) ? 1 : 2;
        answer(*sp->an, r);
        return true;
    }
    if (sp->tb) {                          // a root inside the attached tables: answered from them, as the two cases above
        m0_analysis_result r = blank_result(job);
        if (tb_root_lines(sp->tb, sp->tb_max_pieces, job.line.pos, sp->an->opts.multipv, sp->an->opts.pv_len, &r)) {
            answer(*sp->an, r);
            return true;
        }
    }
    return false;
}
static void queue_job(m0_selfplay* sp, AnalysisJob&& job) {
    if (answered_on_host(sp, job)) return;
    (job.sims == 0 ? sp->an->policy_queue : sp->an->queue).push_back(std::move(job));
}

// entry j of what a result kernel wrote (hlines / hnlines) -> the lines of r
static void copy_lines(const Analysis& a, int j, m0_analysis_result& r) {
    r.nlines = a.hnlines[j] < 0 ? 0 : (a.hnlines[j] > M0_AN_MAX_LINES ? M0_AN_MAX_LINES : a.hnlines[j]);
    for (int l = 0; l < r.nlines; ++l) r.lines[l] = a.hlines[(size_t)j * M0_AN_MAX_LINES + l];
}

// An answered search leaves its slot: free for the next one, or held with its tree (submitted with keep).
static void leave_slot(m0_selfplay* sp, int s) {
    sp->an->held[s] = sp->an->slot_job[s].keep ? 1 : 0;
    sp->games[s].in_use = sp->an->slot_job[s].keep;
}

// Free slots take the next queued searches: a fresh tree each, random streams keyed by the submission's id (not by the slot).
int analysis_refill(m0_selfplay* sp) {
    Analysis& a = *sp->an;
    for (int s = 0; s < sp->G && !a.queue.empty(); ++s) {
        if (sp->games[s].in_use) continue;
        AnalysisJob& job = a.queue.front();
        occupy_slot(sp, s, std::move(job.line), (int)job.id);
        a.slot_job[s] = AnalysisJob{Line(), job.sims, job.nlegal, job.id, job.keep};
        a.queue.pop_front();
        sp->hg[s].net_id = 0;
        sp->hg[s].root_n = 0; sp->hg[s].root_q = 0.0; sp->hg[s].root_v = 0.0;   // what a peek before the first pass reports
        begin_search(sp, s, a.slot_job[s].sims, a.opts.dirichlet != 0, ROOT_FRESH);
    }
    return sp->adv.empty() ? M0_OK : apply_advances(sp);
}

// The searches that the last expand finished: their lines from the result kernel (the trees stay on the device), the rest
// from the slots' control blocks, which the step has just mirrored.  The slots are free afterwards (or held: leave_slot).
int analysis_harvest(m0_selfplay* sp) {
    Analysis& a = *sp->an;
    a.finished.clear();
    for (int s = 0; s < sp->G; ++s)
        if (sp->hg[s].active && sp->hg[s].finished) a.finished.push_back(s);
    const int nf = (int)a.finished.size();
    if (nf == 0) return M0_OK;
    HipStatus& hs = sp->hip;
    M0_HIP(hs, hipMemcpyAsync(sp->ids_dev, a.finished.data(), (size_t)nf * 4, hipMemcpyHostToDevice, sp->stream));
    M0_HIP(hs, launch_analysis_lines(sp->d, sp->ids_dev, nf, a.opts.multipv, a.opts.pv_len, a.lines_dev, a.nlines_dev, sp->stream,
                                     proof_out(sp)));
    M0_HIP(hs, hipMemcpyAsync(a.hlines.data(), a.lines_dev, sizeof(m0_analysis_line) * M0_AN_MAX_LINES * nf, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hnlines.data(), a.nlines_dev, (size_t)nf * 4, hipMemcpyDeviceToHost, sp->stream));
    if (proof_out(sp))
        M0_HIP(hs, hipMemcpyAsync(a.hproof.data(), a.proof_dev, sizeof(m0_proof_lines) * nf, hipMemcpyDeviceToHost, sp->stream));
    if (a.keep_visits) {           // the root children of the same searches, in the same trip
        M0_HIP(hs, launch_root_children(sp->d, sp->ids_dev, nf, a.child_idx_dev, a.child_n_dev, a.nchild_dev, sp->stream));
        M0_HIP(hs, hipMemcpyAsync(a.hchild_idx.data(), a.child_idx_dev, (size_t)nf * M0_MAX_CHILDREN * 4, hipMemcpyDeviceToHost, sp->stream));
        M0_HIP(hs, hipMemcpyAsync(a.hchild_n.data(), a.child_n_dev, (size_t)nf * M0_MAX_CHILDREN * 4, hipMemcpyDeviceToHost, sp->stream));
        M0_HIP(hs, hipMemcpyAsync(a.hnchild.data(), a.nchild_dev, (size_t)nf * 4, hipMemcpyDeviceToHost, sp->stream));
    }
    if (!M0_HIP(hs, hipStreamSynchronize(sp->stream))) return m0_hip_error(hs, "analysis harvest failed");
    for (int j = 0; j < nf; ++j) {
        const int s = a.finished[j];
        GameDev& g = sp->hg[s];
        m0_analysis_result r = blank_result(a.slot_job[s]);
        r.overflow = g.overflow; r.root_n = g.root_n; r.evals = g.evals;
        r.value = (float)g.root_v;
        r.root_q = g.root_n > 0 ? g.root_q : g.root_v;
        copy_lines(a, j, r);
        if (g.overflow) sp->stats.arena_overflows++;
        std::vector<int32_t> children;
        if (a.keep_visits) {               // [policy index x k | visits x k]
            const int k = a.hnchild[j] < 0 ? 0 : (a.hnchild[j] > M0_MAX_CHILDREN ? M0_MAX_CHILDREN : a.hnchild[j]);
            const int32_t* ci = a.hchild_idx.data() + (size_t)j * M0_MAX_CHILDREN;
            const int32_t* cn = a.hchild_n.data() + (size_t)j * M0_MAX_CHILDREN;
            children.assign(ci, ci + k);
            children.insert(children.end(), cn, cn + k);
        }
        answer(a, r, std::move(children), proof_out(sp) ? a.hproof[j] : m0_proof_lines{});
        g.active = 0; g.finished = 0;
        leave_slot(sp, s);
    }
    return sync_games_h2d(sp) ? M0_OK : m0_hip_error(hs, "releasing the slots failed");
}

// Policy mode: up to rows_max queued positions -> network input, legal moves and policy indices (the position encoder), one
// forward, the policy kernel; the compact lines come back.
static int policy_pass(m0_selfplay* sp) {
    Analysis& a = *sp->an;
    const int n = (int)std::min<size_t>(a.policy_queue.size(), (size_t)sp->rows_max);
    if (n <= 0) return M0_OK;
    const double t0 = now_ms();
    for (int i = 0; i < n; ++i) a.hpos[i] = a.policy_queue[i].line.pos;
    HipStatus& hs = sp->hip;
    M0_HIP(hs, hipMemcpyAsync(a.pos_dev, a.hpos.data(), sizeof(Pos) * n, hipMemcpyHostToDevice, sp->stream));
    if (!M0_HIP(hs, launch_encode_positions(a.pos_dev, n, nullptr, sp->d.x0, nullptr, a.nlegal_dev, a.moves_dev, a.idx_dev, sp->stream)))
        return m0_hip_error(hs, "position encode failed");
    std::string err;
    m0_net_lock(sp->nethandle);
    const int rc = sp->net->forward(nullptr, sp->d.x0, n, sp->logits_dev, sp->values_dev, nullptr, sp->stream, err);
    m0_net_unlock(sp->nethandle);
    if (rc != M0_OK) { hs.check(sp->net->hip()); m0_set_error(err); return rc; }
    M0_HIP(hs, launch_policy_lines(sp->logits_dev, sp->values_dev, a.nlegal_dev, a.moves_dev, a.idx_dev, n, a.opts.multipv, a.lines_dev,
                                   a.nlines_dev, a.value_out_dev, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hlines.data(), a.lines_dev, sizeof(m0_analysis_line) * M0_AN_MAX_LINES * n, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hnlines.data(), a.nlines_dev, (size_t)n * 4, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hvalues.data(), a.value_out_dev, (size_t)n * 4, hipMemcpyDeviceToHost, sp->stream));
    if (!M0_HIP(hs, hipStreamSynchronize(sp->stream))) return m0_hip_error(hs, "policy pass failed");
    for (int i = 0; i < n; ++i) {
        m0_analysis_result r = blank_result(a.policy_queue.front());
        r.evals = 1;
        r.value = a.hvalues[i];
        r.root_q = (double)r.value;
        copy_lines(a, i, r);
        answer(a, r);
        a.policy_queue.pop_front();
    }
    sp->stats.evals += (uint64_t)n;
    sp->stats.ms_total += now_ms() - t0;
    return M0_OK;
}

// Queued searches that can never start: none is in a slot and every slot is held.  Sets the error string.
static bool blocked_by_held(const m0_selfplay* sp) {
    if (sp->an->queue.empty()) return false;
    for (int s = 0; s < sp->G; ++s) if (!sp->games[s].in_use || !sp->an->held[s]) return false;
    m0_set_error("searches are queued but every slot is held: m0_analysis_release or m0_analysis_continue one");
    return true;
}

// ---- live searches (include/m0_analysis_live.h)
static bool live_call_ok(const m0_selfplay* sp, const char* what) {
    if (!sp->ext_pending) return true;
    m0_set_error(std::string(what) + ": m0_analysis_ext_expand outstanding");
    return false;
}
static int slot_of(const m0_selfplay* sp, int64_t id, bool held) {      // the slot that searches / holds `id`, -1: none
    for (int s = 0; s < sp->G; ++s)
        if (sp->games[s].in_use && (sp->an->held[s] != 0) == held && sp->an->slot_job[s].id == id) return s;
    return -1;
}
template <typename Q> static typename Q::iterator queued(Q& q, int64_t id) {
    return std::find_if(q.begin(), q.end(), [id](const AnalysisJob& j) { return j.id == id; });
}

// The result of the search in slot s as it stands: the lines from the result kernel on that one slot (it reads the tree, not
// the block a finished search writes), the rest from the slot's control block, read back first.
static int live_result(m0_selfplay* sp, int s, m0_analysis_result& r, m0_proof_lines& proof) {
    Analysis& a = *sp->an;
    HipStatus& hs = sp->hip;
    proof = m0_proof_lines{};
    M0_HIP(hs, hipMemcpyAsync(sp->ids_dev, &s, 4, hipMemcpyHostToDevice, sp->stream));
    M0_HIP(hs, launch_analysis_lines(sp->d, sp->ids_dev, 1, a.opts.multipv, a.opts.pv_len, a.lines_dev, a.nlines_dev, sp->stream,
                                     proof_out(sp)));
    if (proof_out(sp)) M0_HIP(hs, hipMemcpyAsync(&proof, a.proof_dev, sizeof(m0_proof_lines), hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hlines.data(), a.lines_dev, sizeof(m0_analysis_line) * M0_AN_MAX_LINES, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(a.hnlines.data(), a.nlines_dev, 4, hipMemcpyDeviceToHost, sp->stream));
    if (!sync_games_d2h(sp)) return m0_hip_error(hs, "reading a running search failed");
    const GameDev& g = sp->hg[s];
    r = blank_result(a.slot_job[s]);
    r.sims = g.sims_done;
    r.overflow = g.overflow; r.root_n = g.root_n; r.evals = g.evals;
    r.value = (float)g.root_v;
    r.root_q = g.root_n > 0 ? g.root_q : g.root_v;
    copy_lines(a, 0, r);
    return M0_OK;
}

static m0_selfplay* analysis_create_impl(m0_net* nh, const m0_selfplay_cfg* cfg, const m0_analysis_opts* opts) {
    if (!cfg || !opts) { m0_set_error("cfg / opts is null"); return nullptr; }
    if (opts->multipv < 1 || opts->multipv > M0_AN_MAX_LINES || opts->pv_len < 1 || opts->pv_len > M0_AN_MAX_PV) {
        m0_set_error("multipv must be in [1, 8] and pv_len in [1, 16]");
        return nullptr;
    }
    if (cfg->tt_merge || cfg->raw_legal_priors) {
        m0_set_error("M0_ERR_UNSUPPORTED: an analysis engine searches plain trees (tt_merge / raw_legal_priors are refused)");
        return nullptr;
    }
    m0_selfplay_cfg c = *cfg;
    // no games are played: every analysis is a fresh tree of exactly the simulations it asks for
    c.total_games = 0; c.record_games = 0; c.ssl_in_forward = 0; c.ssl_targets = 0; c.opening_random_plies = 0;
    c.playout_random_frac = 0.0; c.fresh_tree_per_move = 1; c.root_reinfer = 0;
    c.arena_mode = 0; c.arena_eval_cache = 0; c.arena_paired_openings = 0; c.eval_cache = 0; c.tail_split = 0;
    std::unique_ptr<m0_selfplay, decltype(&m0_selfplay_destroy)> owner(engine_create(nh, nullptr, &c, EngineKind::Analysis), &m0_selfplay_destroy);
    m0_selfplay* sp = owner.get();
    if (!sp) return nullptr;
    Analysis* a = sp->an = new Analysis();
    a->opts = *opts;
    const size_t R = (size_t)sp->rows_max;
    a->slot_job.resize(sp->G);
    a->held.assign(sp->G, 0);
    a->reroot_in_dev = dalloc<int>(sp, 2 + M0_REROOT_MAX_MOVES);
    a->reroot_out_dev = dalloc<RerootOut>(sp, 1);
    a->hlines.resize(R * M0_AN_MAX_LINES);
    a->hnlines.resize(R);
    a->hvalues.resize(R);
    a->hpos.resize(R);
    a->lines_dev = dalloc<m0_analysis_line>(sp, R * M0_AN_MAX_LINES);
    a->nlines_dev = dalloc<int>(sp, R);
    a->value_out_dev = dalloc<float>(sp, R);
    if (sp->net) {                         // policy mode needs the engine's own network
        a->pos_dev = dalloc<Pos>(sp, R);
        a->nlegal_dev = dalloc<int32_t>(sp, R);
        a->moves_dev = dalloc<uint16_t>(sp, R * M0_MAX_MOVES);
        a->idx_dev = dalloc<int32_t>(sp, R * M0_MAX_MOVES);
    }
    M0_HIP(sp->hip, hipStreamSynchronize(sp->stream));
    return hip_ok(sp, "hipMalloc failed for the analysis result buffers") ? owner.release() : nullptr;
}

}  // namespace m0

extern "C" {

m0_selfplay* m0_analysis_create(m0_net* net, const m0_selfplay_cfg* cfg, const m0_analysis_opts* opts) {
    if (!net) { m0_set_error("m0_analysis_create needs a network (m0_analysis_create_ext takes an external evaluator)"); return nullptr; }
    return analysis_create_impl(net, cfg, opts);
}

m0_selfplay* m0_analysis_create_ext(const m0_selfplay_cfg* cfg, const m0_analysis_opts* opts) {
    return analysis_create_impl(nullptr, cfg, opts);
}

// m0_analysis_submit / _submit_keep behind the call guard
static int submit_impl(m0_selfplay* sp, const char* fen, const char* const* ucis, int n_moves, int sims, int64_t id, bool keep) {
    if (!fen || sims < (keep ? 1 : 0) || n_moves < 0 || (n_moves > 0 && !ucis)) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    if (sims == 0 && !sp->net) { m0_set_error("policy mode (sims = 0) needs an engine with a network"); return M0_ERR_UNSUPPORTED; }
    AnalysisJob job;
    job.sims = sims; job.id = id; job.keep = keep;
    if (parse_fen(fen, job.line.pos) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    Move legal[M0_MAX_MOVES];
    int n = 0;
    for (int i = 0; i < n_moves; ++i) {
        if (!job.line.play_if_legal(ucis[i] ? parse_uci(ucis[i]) : (Move)0xFFFF, legal, n)) {
            m0_set_error(std::string("Illegal move: ") + (ucis[i] ? ucis[i] : "(null)"));
            return M0_ERR_INVALID;
        }
    }
    job.nlegal = gen_legal(job.line.pos, legal);
    queue_job(sp, std::move(job));
    return M0_OK;
}

int m0_analysis_submit(m0_selfplay* sp, const char* fen, const char* const* ucis, int n_moves, int sims, int64_t id) {
    M0_ENGINE_CALL(sp, "m0_analysis_submit", KIND_ANALYSIS, true);
    return submit_impl(sp, fen, ucis, n_moves, sims, id, false);
}

int m0_analysis_submit_planes(m0_selfplay* sp, const float* planes, const uint8_t* mask, int n, int sims, const int64_t* ids,
                              int32_t* status, int32_t* flags) {
    M0_ENGINE_CALL(sp, "m0_analysis_submit_planes", KIND_ANALYSIS, true);
    if (!planes || !status || n <= 0 || sims < 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    if (sims == 0 && !sp->net) { m0_set_error("policy mode (sims = 0) needs an engine with a network"); return M0_ERR_UNSUPPORTED; }
    // decoded on the engine's device and stream; the buffers live for this call
    const size_t N = (size_t)n;
    DevBuf<float> dpl; DevBuf<uint8_t> dm; DevBuf<Pos> dp; DevBuf<int32_t> dst, dfl, dnl;
    HipStatus& hs = sp->hip; HipStatus as;   // `as`: a batch too large for the call's own buffers is refused, the engine lives on
    if (!dpl.alloc(as, N * M0_PLANES * 64) || (mask && !dm.alloc(as, N * M0_POLICY_SIZE)) || !dp.alloc(as, N) || !dst.alloc(as, N) ||
        !dfl.alloc(as, N) || !dnl.alloc(as, N)) return m0_hip_error(as, "hipMalloc failed");
    std::vector<Pos> hp(N);
    std::vector<int32_t> hfl(N), hnl(N);
    M0_HIP(hs, hipMemcpyAsync(dpl.p, planes, N * M0_PLANES * 64 * sizeof(float), hipMemcpyHostToDevice, sp->stream));
    if (mask) M0_HIP(hs, hipMemcpyAsync(dm.p, mask, N * M0_POLICY_SIZE, hipMemcpyHostToDevice, sp->stream));
    M0_HIP(hs, launch_decode_planes(dpl.p, dm.p, n, dp.p, dst.p, dfl.p, dnl.p, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(hp.data(), dp.p, N * sizeof(Pos), hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(status, dst.p, N * 4, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(hfl.data(), dfl.p, N * 4, hipMemcpyDeviceToHost, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(hnl.data(), dnl.p, N * 4, hipMemcpyDeviceToHost, sp->stream));
    if (!M0_HIP(hs, hipStreamSynchronize(sp->stream))) return m0_hip_error(hs, "decoding the planes failed");
    if (flags) memcpy(flags, hfl.data(), N * 4);
    for (int i = 0; i < n; ++i) {
        if (status[i] != M0_DECODE_OK) continue;             // reported, not queued
        AnalysisJob job;
        job.sims = sims; job.id = ids ? ids[i] : (int64_t)i;
        job.line.pos = hp[i];                                // an empty repetition window: the planes hold no history
        job.nlegal = hnl[i];
        queue_job(sp, std::move(job));
    }
    return M0_OK;
}

int m0_analysis_keep_visits(m0_selfplay* sp, int on) {
    M0_ENGINE_CALL(sp, "m0_analysis_keep_visits", KIND_ANALYSIS, true);
    Analysis& a = *sp->an;
    if (on && !a.child_idx_dev) {          // the first time: one entry per slot, as the lines of a harvest
        const size_t G = (size_t)sp->G;
        a.child_idx_dev = dalloc<int32_t>(sp, G * M0_MAX_CHILDREN);
        a.child_n_dev = dalloc<int32_t>(sp, G * M0_MAX_CHILDREN);
        a.nchild_dev = dalloc<int32_t>(sp, G);
        if (!sp->hip.ok()) { a.child_idx_dev = nullptr; return m0_hip_error(sp->hip, "hipMalloc failed for the root-children buffers"); }
        a.hchild_idx.resize(G * M0_MAX_CHILDREN);
        a.hchild_n.resize(G * M0_MAX_CHILDREN);
        a.hnchild.resize(G);
    }
    a.keep_visits = on != 0;
    return M0_OK;
}

int m0_analysis_step(m0_selfplay* sp, int steps) {
    M0_ENGINE_CALL(sp, "m0_analysis_step", KIND_ANALYSIS, true);
    if (!sp->net) { m0_set_error("m0_analysis_step needs a network (use m0_analysis_ext_select / _expand without one)"); return M0_ERR_STATE; }
    if (sp->ext_pending) { m0_set_error("m0_analysis_ext_expand outstanding"); return M0_ERR_STATE; }
    for (int i = 0; i < steps && pending_count(sp) > 0; ++i) {
        int rc = policy_pass(sp);
        if (rc == M0_OK && blocked_by_held(sp)) return M0_ERR_STATE;
        if (rc == M0_OK) rc = refill(sp);
        if (rc == M0_OK && searches_pending(sp) > 0) rc = one_step(sp);      // the pass and the harvest
        if (rc != M0_OK) return rc;
    }
    return M0_OK;
}

int m0_analysis_ext_select(m0_selfplay* sp, int* rows, float* planes, int max_rows) {
    M0_ENGINE_CALL(sp, "m0_analysis_ext_select", KIND_ANALYSIS, true);
    if (!rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (!sp->ext_pending && blocked_by_held(sp)) return M0_ERR_STATE;
    return ext_select_impl(sp, rows, nullptr, planes, nullptr, max_rows);
}

int m0_analysis_ext_expand(m0_selfplay* sp, const float* logits, const float* values, int rows) {
    M0_ENGINE_CALL(sp, "m0_analysis_ext_expand", KIND_ANALYSIS, true);
    return ext_expand_impl(sp, logits, values, rows, nullptr, nullptr, 0);
}

int m0_analysis_poll(m0_selfplay* sp, m0_analysis_result* out) {
    M0_ENGINE_CALL(sp, "m0_analysis_poll", KIND_ANALYSIS, true);
    if (!out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (sp->an->done.empty()) return 0;
    *out = sp->an->done.front();
    pop_done(*sp->an);
    return 1;
}

int m0_analysis_poll_visits(m0_selfplay* sp, m0_analysis_result* out, int32_t* nchild, int32_t* policy_idx, int32_t* visits,
                            int cap) {
    M0_ENGINE_CALL(sp, "m0_analysis_poll_visits", KIND_ANALYSIS, true);
    if (!out || !nchild || !policy_idx || !visits) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (cap < M0_MAX_CHILDREN) { m0_set_error("cap must be at least 256 (M0_MAX_CHILDREN)"); return M0_ERR_INVALID; }
    if (sp->an->done.empty()) return 0;
    *out = sp->an->done.front();
    const std::vector<int32_t>& ch = sp->an->done_children.front();
    const int k = (int)(ch.size() / 2);
    *nchild = k;
    if (k > 0) { memcpy(policy_idx, ch.data(), (size_t)k * 4); memcpy(visits, ch.data() + k, (size_t)k * 4); }
    pop_done(*sp->an);
    return 1;
}

int m0_analysis_last_proof(m0_selfplay* sp, m0_proof_lines* out) {
    M0_ENGINE_CALL(sp, "m0_analysis_last_proof", KIND_ANALYSIS, false);
    if (!out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (!is_proof(sp->tc)) { m0_set_error("m0_analysis_last_proof: the proof search is not set on this engine"); return M0_ERR_STATE; }
    *out = sp->an->last_proof;
    return M0_OK;
}

int m0_analysis_pending(m0_selfplay* sp) {
    M0_ENGINE_CALL(sp, "m0_analysis_pending", KIND_ANALYSIS, true);
    return pending_count(sp);
}

size_t m0_analysis_result_size(void) { return sizeof(m0_analysis_result); }

// ---- live searches (include/m0_analysis_live.h)
int m0_analysis_submit_keep(m0_selfplay* sp, const char* fen, const char* const* ucis, int n_moves, int sims, int64_t id) {
    M0_ENGINE_CALL(sp, "m0_analysis_submit_keep", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_submit_keep")) return M0_ERR_STATE;
    return submit_impl(sp, fen, ucis, n_moves, sims, id, true);
}

int m0_analysis_peek(m0_selfplay* sp, int64_t id, m0_analysis_result* out) {
    M0_ENGINE_CALL(sp, "m0_analysis_peek", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_peek")) return M0_ERR_STATE;
    if (!out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    Analysis& a = *sp->an;
    const int s = slot_of(sp, id, false);
    if (s < 0) {
        if (queued(a.queue, id) != a.queue.end()) return 0;
        m0_set_error("m0_analysis_peek: no search with this id is queued or running");
        return M0_ERR_INVALID;
    }
    m0_analysis_result r;
    const int rc = live_result(sp, s, r, a.last_proof);
    if (rc != M0_OK) return rc;
    *out = r;
    return 1;
}

int m0_analysis_stop(m0_selfplay* sp, int64_t id) {
    M0_ENGINE_CALL(sp, "m0_analysis_stop", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_stop")) return M0_ERR_STATE;
    Analysis& a = *sp->an;
    const int s = slot_of(sp, id, false);
    if (s < 0) {
        auto it = queued(a.queue, id);
        if (it == a.queue.end()) { m0_set_error("m0_analysis_stop: no search with this id is queued or running"); return M0_ERR_INVALID; }
        m0_analysis_result r = blank_result(*it);      // never searched: no slot, nothing held
        r.sims = 0;
        a.queue.erase(it);
        answer(a, r);
        return M0_OK;
    }
    m0_analysis_result r;
    m0_proof_lines proof;
    const int rc = live_result(sp, s, r, proof);
    if (rc != M0_OK) return rc;
    if (r.overflow) sp->stats.arena_overflows++;
    answer(a, r, std::vector<int32_t>(), proof);
    sp->hg[s].active = 0; sp->hg[s].finished = 0;
    leave_slot(sp, s);
    sync_games_h2d(sp);
    return M0_HIP(sp->hip, hipStreamSynchronize(sp->stream)) ? M0_OK : m0_hip_error(sp->hip, "stopping a search failed");
}

int m0_analysis_continue(m0_selfplay* sp, int64_t held_id, const char* const* ucis, int n_moves, int sims, int64_t id, int keep,
                         int32_t* reused_n) {
    M0_ENGINE_CALL(sp, "m0_analysis_continue", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_continue")) return M0_ERR_STATE;
    if (sims < 1 || n_moves < 0 || n_moves > M0_REROOT_MAX_MOVES || (n_moves > 0 && !ucis)) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    Analysis& a = *sp->an;
    const int s = slot_of(sp, held_id, true);
    if (s < 0) { m0_set_error("m0_analysis_continue: this id is not held"); return M0_ERR_INVALID; }
    AnalysisJob job;
    job.line = static_cast<const Line&>(sp->games[s]);
    job.sims = sims; job.id = id; job.keep = keep != 0;
    int in[2 + M0_REROOT_MAX_MOVES] = {s, n_moves};
    Move legal[M0_MAX_MOVES];
    int n = 0;
    for (int i = 0; i < n_moves; ++i) {
        const Move m = ucis[i] ? parse_uci(ucis[i]) : (Move)0xFFFF;
        if (!job.line.play_if_legal(m, legal, n)) {
            m0_set_error(std::string("Illegal move: ") + (ucis[i] ? ucis[i] : "(null)"));
            return M0_ERR_INVALID;
        }
        in[2 + i] = (int)m;
    }
    job.nlegal = gen_legal(job.line.pos, legal);
    if (reused_n) *reused_n = 0;
    a.held[s] = 0; sp->games[s].in_use = false;        // held_id is held no longer, whatever follows
    // a final position that needs no search: answered as m0_analysis_submit answers it, the slot is free
    if (answered_on_host(sp, job)) return M0_OK;
    // the tree: follow the moves on the device and keep what is behind them
    HipStatus& hs = sp->hip;
    RerootOut out = {0, 0, 0.0};
    M0_HIP(hs, hipMemcpyAsync(a.reroot_in_dev, in, sizeof(in), hipMemcpyHostToDevice, sp->stream));
    M0_HIP(hs, launch_reroot_moves(sp->d, a.reroot_in_dev, a.reroot_in_dev + 1, a.reroot_in_dev + 2, 1, a.reroot_out_dev, sp->stream));
    M0_HIP(hs, hipMemcpyAsync(&out, a.reroot_out_dev, sizeof(out), hipMemcpyDeviceToHost, sp->stream));
    if (!sync_games_d2h(sp)) return m0_hip_error(hs, "re-rooting the held tree failed");    // root / arena / next as the kernel left them
    const bool kept = out.kept != 0;
    occupy_slot(sp, s, std::move(job.line), (int)id);
    a.slot_job[s] = AnalysisJob{Line(), sims, job.nlegal, id, job.keep};
    GameDev& g = sp->hg[s];
    g.net_id = 0;
    arm_slot_search(sp, s, sims, a.opts.dirichlet != 0, !kept);
    g.reinfer = kept ? 1 : 0;                          // a kept root: its value once more, as MCTS.run on a root found again
    g.root_n = kept ? out.n : 0; g.root_q = kept ? out.q : 0.0; g.root_v = 0.0;
    sync_games_h2d(sp);
    if (!M0_HIP(hs, hipStreamSynchronize(sp->stream))) return m0_hip_error(hs, "re-rooting the held tree failed");
    if (reused_n) *reused_n = kept ? out.n : 0;
    return M0_OK;
}

int m0_analysis_release(m0_selfplay* sp, int64_t held_id) {
    M0_ENGINE_CALL(sp, "m0_analysis_release", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_release")) return M0_ERR_STATE;
    const int s = slot_of(sp, held_id, true);
    if (s < 0) { m0_set_error("m0_analysis_release: this id is not held"); return M0_ERR_INVALID; }
    sp->an->held[s] = 0;
    sp->games[s].in_use = false;
    return M0_OK;
}

int m0_analysis_held(m0_selfplay* sp) {
    M0_ENGINE_CALL(sp, "m0_analysis_held", KIND_ANALYSIS, true);
    if (!live_call_ok(sp, "m0_analysis_held")) return M0_ERR_STATE;
    int n = 0;
    for (int s = 0; s < sp->G; ++s) n += sp->games[s].in_use && sp->an->held[s] ? 1 : 0;
    return n;
}

}  // extern "C"
