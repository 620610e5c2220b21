// extern "C" entry points of the endgame tablebases (include/m0_engine.h, m0_tb_*): build, cache file, probing, the analysis
// of a root inside the tables, and the two attachments to an engine: the host probe after a played move
// (m0_selfplay_set_tablebase) and the probe inside the search (m0_selfplay_set_search_tablebase), for which the handle keeps
// one copy of its tables per HIP device.  The build and that copy touch the GPU; everything else runs on the host.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <memory>
#include <mutex>
#include "selfplay_engine.h"
#include "tb.h"

using namespace m0;

namespace {

// Cache file: header, one record per table, then the tables' bytes in the same order.  Little endian.
constexpr char TB_MAGIC[8] = {'M', '0', 'T', 'B', 'A', 'S', 'E', '\n'};
constexpr uint32_t TB_FORMAT = 1;
struct FileHeader { char magic[8]; uint32_t format, ntables; };
struct FileRecord { char sig[8]; uint64_t bytes, checksum; int32_t maxd, sweeps; };

// sum over the 64-bit words w_i of mix64(w_i + (i + 1) * golden): any changed word changes the sum
uint64_t tb_checksum(const uint8_t* p, size_t n) {
    uint64_t h = 0;
    for (size_t i = 0; i < n / 8; ++i) {
        uint64_t w;
        memcpy(&w, p + 8 * i, 8);
        h += mix64(w + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull);
    }
    return h;
}

m0_tb* build(int hip_device, const std::vector<std::string>& sigs) {
    std::vector<std::string> order;
    std::string bad, err;
    if (!tb_build_order(sigs, order, bad)) { m0_set_error("not a tablebase signature in scope: " + bad); return nullptr; }
    std::unique_ptr<m0_tb> tb(new m0_tb());
    if (tb_build_on_device(hip_device, order, tb.get(), err) != M0_OK) { m0_set_error("tablebase build failed: " + err); return nullptr; }
    return tb.release();
}

// ---- the analysis of a root inside the tables ----
struct RankedMove { Move mv; int wdl, dtm; };      // wdl / dtm of the successor, for the side to move there

// The legal moves of p, best first for the mover: successors lost for the opponent by ascending dtm, drawn ones, successors
// won for the opponent by descending dtm; ties in legal-move order.  false: a successor is not in the tables.
bool rank_moves(const m0_tb* tb, int max_men, const Pos& p, std::vector<RankedMove>& out) {
    Move mv[M0_MAX_MOVES];
    const int n = gen_legal(p, mv);
    out.clear();
    for (int i = 0; i < n; ++i) {
        Pos q = p;
        make_move(q, mv[i]);
        RankedMove r{mv[i], 0, 0};
        if (!tb_probe(tb->set, q, max_men, r.wdl, r.dtm)) return false;
        out.push_back(r);
    }
    auto cls = [](const RankedMove& r) { return r.wdl < 0 ? 0 : (r.wdl == 0 ? 1 : 2); };
    std::stable_sort(out.begin(), out.end(), [&](const RankedMove& a, const RankedMove& b) {
        if (cls(a) != cls(b)) return cls(a) < cls(b);
        return cls(a) == 0 ? a.dtm < b.dtm : (cls(a) == 2 ? a.dtm > b.dtm : false);
    });
    return true;
}

}  // namespace

bool m0::tb_root_lines(const m0_tb* tb, int max_men, const Pos& root, int multipv, int pv_len, m0_analysis_result* out) {
    int wdl = 0, dtm = 0;
    if (!tb_probe(tb->set, root, max_men, wdl, dtm)) return false;
    std::vector<RankedMove> ranked, next;
    if (!rank_moves(tb, max_men, root, ranked)) return false;
    std::vector<m0_analysis_line> lines;
    for (size_t l = 0; l < ranked.size() && (int)l < multipv; ++l) {
        const RankedMove& r = ranked[l];
        m0_analysis_line ln;
        memset(&ln, 0, sizeof(ln));
        ln.move = r.mv; ln.policy_index = move_to_index(root, r.mv); ln.q = (double)-r.wdl;
        ln.pv[ln.pv_len++] = r.mv;
        Pos p = root;
        make_move(p, r.mv);
        while (r.wdl != 0 && ln.pv_len < pv_len) {            // a decided line: the first-ranked move of every position on it
            if (!rank_moves(tb, max_men, p, next)) return false;
            if (next.empty()) break;                          // checkmate
            ln.pv[ln.pv_len++] = next[0].mv;
            make_move(p, next[0].mv);
        }
        lines.push_back(ln);
    }
    const int64_t id = out->id;
    memset(out, 0, sizeof(*out));
    out->id = id; out->status = 3; out->nlegal = (int32_t)ranked.size(); out->root_q = (double)wdl; out->tb_dtm = dtm;
    out->nlines = (int32_t)lines.size();
    for (size_t l = 0; l < lines.size(); ++l) { out->lines[l] = lines[l]; out->line_dtm[l] = ranked[l].dtm; }
    return true;
}

// ---- the device copy ----
int m0::tb_device_set(const m0_tb* tb, int hip_device, const TbSet** set_dev, std::string& err) {
    std::lock_guard<std::mutex> lk(tb->dev_mu);
    for (const auto& c : tb->dev_copies)
        if (c.device == hip_device) { *set_dev = c.set; return M0_OK; }
    m0_tb_device_copy c;
    c.device = hip_device;
    TbSet host;
    for (auto& t : host.tab) t = nullptr;
    HipStatus hs;
    M0_HIP(hs, hipSetDevice(hip_device));
    for (const TbTable& t : tb->tables) {
        void* p = nullptr;
        if (!M0_HIP(hs, hipMalloc(&p, t.bytes.size()))) break;
        c.allocs.push_back(p);
        host.tab[tb_material_code(t.sig)] = (const uint8_t*)p;
        M0_HIP(hs, hipMemcpy(p, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice));
    }
    void* sd = nullptr;
    if (M0_HIP(hs, hipMalloc(&sd, sizeof(TbSet)))) c.allocs.push_back(sd);
    M0_HIP(hs, hipMemcpy(sd, &host, sizeof(TbSet), hipMemcpyHostToDevice));
    if (!M0_HIP(hs, hipDeviceSynchronize())) {                // nothing of the upload is left in flight when the caller goes on
        err = "copying the tables to the device failed: " + hs.message();
        for (void* p : c.allocs) (void)hipFree(p);            // no kernel has seen them
        return M0_ERR_HIP;
    }
    c.set = (const TbSet*)sd;
    *set_dev = c.set;
    tb->dev_copies.push_back(std::move(c));
    return M0_OK;
}

void m0::tb_free_device_copies(m0_tb* tb) {
    std::lock_guard<std::mutex> lk(tb->dev_mu);
    for (auto& c : tb->dev_copies) {
        if (hipSetDevice(c.device) != hipSuccess) continue;
        for (void* p : c.allocs) (void)hipFree(p);
    }
    tb->dev_copies.clear();
}

extern "C" {

m0_tb* m0_tb_build(int hip_device, int max_men) {
    if (max_men != 3 && max_men != 4) { m0_set_error("max_men must be 3 or 4"); return nullptr; }
    return build(hip_device, tb_all_signatures(max_men));
}

m0_tb* m0_tb_build_signatures(int hip_device, const char* const* sigs, int n) {
    if (!sigs || n <= 0) { m0_set_error("no signatures given"); return nullptr; }
    std::vector<std::string> v;
    for (int i = 0; i < n; ++i) v.push_back(sigs[i] ? sigs[i] : "");
    return build(hip_device, v);
}

void m0_tb_destroy(m0_tb* tb) {
    if (!tb) return;
    tb_free_device_copies(tb);
    delete tb;
}

int m0_tb_max_men(const m0_tb* tb) { return tb ? tb->max_men : 0; }

int m0_tb_table(const m0_tb* tb, const char* sig, const uint8_t** bytes, size_t* n) {
    if (!tb || !sig) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    for (const auto& t : tb->tables)
        if (t.name == sig) {
            if (bytes) *bytes = t.bytes.data();
            if (n) *n = t.bytes.size();
            return M0_OK;
        }
    m0_set_error(std::string("no table ") + sig);
    return M0_ERR_INVALID;
}

int m0_tb_table_info(const m0_tb* tb, int i, char* sig8, int* maxd, int* sweeps, double* build_ms) {
    if (!tb) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (i < 0 || i >= (int)tb->tables.size()) return 0;
    const TbTable& t = tb->tables[i];
    if (sig8) { memset(sig8, 0, 8); memcpy(sig8, t.name.c_str(), std::min<size_t>(7, t.name.size())); }
    if (maxd) *maxd = t.maxd;
    if (sweeps) *sweeps = t.sweeps;
    if (build_ms) *build_ms = t.build_ms;
    return 1;
}

int m0_tb_save(const m0_tb* tb, const char* path) {
    if (!tb || !path) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    // a name of its own per save: workers that share a cache path build the same tables at the same time
    std::string tmp = std::string(path) + ".tmpXXXXXX";
    const int fd = mkstemp(&tmp[0]);
    FILE* f = fd >= 0 ? fdopen(fd, "wb") : nullptr;
    if (!f) { if (fd >= 0) { close(fd); remove(tmp.c_str()); } m0_set_error("cannot write " + tmp); return M0_ERR_INVALID; }
    (void)fchmod(fd, 0644);
    FileHeader h;
    memcpy(h.magic, TB_MAGIC, 8);
    h.format = TB_FORMAT; h.ntables = (uint32_t)tb->tables.size();
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1;
    for (const auto& t : tb->tables) {
        FileRecord r;
        memset(&r, 0, sizeof(r));
        memcpy(r.sig, t.name.c_str(), std::min<size_t>(7, t.name.size()));
        r.bytes = t.bytes.size(); r.checksum = tb_checksum(t.bytes.data(), t.bytes.size());
        r.maxd = t.maxd; r.sweeps = t.sweeps;
        ok = ok && fwrite(&r, sizeof(r), 1, f) == 1;
    }
    for (const auto& t : tb->tables) ok = ok && fwrite(t.bytes.data(), 1, t.bytes.size(), f) == t.bytes.size();
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); m0_set_error(std::string("writing ") + path + " failed"); return M0_ERR_INVALID; }
    return M0_OK;
}

m0_tb* m0_tb_load(const char* path) {
    if (!path) { m0_set_error("null argument"); return nullptr; }
    FILE* f = fopen(path, "rb");
    if (!f) { m0_set_error(std::string("cannot open ") + path); return nullptr; }
    std::unique_ptr<FILE, int (*)(FILE*)> closer(f, fclose);
    const std::string where = std::string("tablebase file ") + path + ": ";
    FileHeader h;
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, TB_MAGIC, 8) != 0) { m0_set_error(where + "wrong magic"); return nullptr; }
    if (h.format != TB_FORMAT) { m0_set_error(where + "unknown format version"); return nullptr; }
    if (h.ntables == 0 || h.ntables > 64) { m0_set_error(where + "bad table count"); return nullptr; }
    std::unique_ptr<m0_tb> tb(new m0_tb());
    std::vector<FileRecord> recs(h.ntables);
    if (fread(recs.data(), sizeof(FileRecord), h.ntables, f) != h.ntables) { m0_set_error(where + "truncated header"); return nullptr; }
    for (auto& r : recs) {
        TbTable t;
        r.sig[7] = 0;
        t.name = r.sig;
        if (!tb_parse_sig(r.sig, t.sig) || r.bytes != tb_entries(t.sig.n)) { m0_set_error(where + "bad table record " + t.name); return nullptr; }
        for (const auto& o : tb->tables) if (o.name == t.name) { m0_set_error(where + "table listed twice: " + t.name); return nullptr; }
        t.maxd = r.maxd; t.sweeps = r.sweeps;
        tb->tables.push_back(std::move(t));
    }
    for (size_t i = 0; i < recs.size(); ++i) {
        TbTable& t = tb->tables[i];
        t.bytes.resize(recs[i].bytes);
        if (fread(t.bytes.data(), 1, t.bytes.size(), f) != t.bytes.size()) { m0_set_error(where + "truncated at table " + t.name); return nullptr; }
        if (tb_checksum(t.bytes.data(), t.bytes.size()) != recs[i].checksum) { m0_set_error(where + "checksum mismatch in table " + t.name); return nullptr; }
    }
    if (fgetc(f) != EOF) { m0_set_error(where + "trailing bytes"); return nullptr; }
    tb->index_tables();
    return tb.release();
}

int m0_tb_probe_fens(const m0_tb* tb, const char* const* fens, int n, uint8_t* hit, int8_t* wdl, int16_t* dtm) {
    if (!tb || n < 0 || (n > 0 && !fens)) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    for (int i = 0; i < n; ++i) {
        Pos p;
        if (!fens[i] || parse_fen(fens[i], p) != 0) { m0_set_error("bad FEN at index " + std::to_string(i)); return M0_ERR_INVALID; }
        int w = 0, d = 0;
        const bool h = tb_probe(tb->set, p, tb->max_men, w, d);
        if (hit) hit[i] = h ? 1 : 0;
        if (wdl) wdl[i] = (int8_t)w;
        if (dtm) dtm[i] = (int16_t)d;
    }
    return M0_OK;
}

int m0_tb_root_lines(const m0_tb* tb, const char* fen, int multipv, int pv_len, m0_analysis_result* out) {
    if (!tb || !fen || !out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (multipv < 1 || multipv > M0_AN_MAX_LINES || pv_len < 1 || pv_len > M0_AN_MAX_PV) {
        m0_set_error("multipv must be in [1, 8] and pv_len in [1, 16]");
        return M0_ERR_INVALID;
    }
    Pos p;
    if (parse_fen(fen, p) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    return tb_root_lines(tb, tb->max_men, p, multipv, pv_len, out) ? 1 : 0;
}

// Both attachments.  `in_search`: also the device copy that select_kernel probes, and the stricter rule for "nothing has run yet".
static int attach_tablebase(m0_selfplay* sp, const m0_tb* tb, int max_pieces, bool in_search) {
    bool started = sp->stats.games_started != 0;
    if (in_search) {
        const bool queued = sp->an && (!sp->an->queue.empty() || !sp->an->policy_queue.empty() || !sp->an->done.empty());
        started = started || sp->stats.steps != 0 || sp->stats.evals != 0 || sp->ext_pending || queued;
    }
    if (started) { m0_set_error("attach the tablebase before the first step"); return M0_ERR_STATE; }
    if (tb && max_pieces < 2) { m0_set_error("max_pieces must be at least 2"); return M0_ERR_INVALID; }
    const TbSet* set_dev = nullptr;
    if (tb && in_search) {
        std::string err;
        const int rc = tb_device_set(tb, sp->device, &set_dev, err);
        if (rc != M0_OK) { m0_set_error("m0_selfplay_set_search_tablebase: " + err); return rc; }
        if (!M0_HIP(sp->hip, hipSetDevice(sp->device))) return m0_hip_error(sp->hip, "m0_selfplay_set_search_tablebase");
    }
    // the host probe of a root (after a played move; of a submission) and the leaf probe of select_kernel read the same limit
    sp->tb = tb;
    sp->tb_max_pieces = tb ? std::min(max_pieces, tb->max_men) : 0;
    if (in_search) { sp->d.tb_set = set_dev; sp->d.tb_max_pieces = sp->tb_max_pieces; }
    return M0_OK;
}

int m0_selfplay_set_tablebase(m0_selfplay* sp, const m0_tb* tb, int max_pieces) {
    M0_ENGINE_CALL(sp, "m0_selfplay_set_tablebase", KIND_SELFPLAY, false);      // matches and analysis do not probe after a move
    return attach_tablebase(sp, tb, max_pieces, false);
}

int m0_selfplay_set_search_tablebase(m0_selfplay* sp, const m0_tb* tb, int max_pieces) {
    M0_ENGINE_CALL(sp, "m0_selfplay_set_search_tablebase", KIND_ANY, false);
    return attach_tablebase(sp, tb, max_pieces, true);
}

uint64_t m0_selfplay_tb_leaves(m0_selfplay* sp) {
    M0_ENGINE_CALL_OR(0, sp, "m0_selfplay_tb_leaves", KIND_ANY, false);
    uint64_t n = 0;
    for (const GameDev& g : sp->hg) n += g.tb_leaves;         // the mirror the last step copied
    return n;
}

uint64_t m0_selfplay_tb_adjudications(m0_selfplay* sp) {
    M0_ENGINE_CALL_OR(0, sp, "m0_selfplay_tb_adjudications", KIND_ANY, false);
    return sp->tb_adjudications;
}

}  // extern "C"
