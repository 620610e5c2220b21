// TEST INFRASTRUCTURE: host (g++) build of matrix0_amd/csrc/tb_core.h.  The init pass and the sweeps that the GPU build
// runs one thread per entry run here in a plain loop, so the tablebase logic can be checked against the independent
// generator (tests/tb_ref) and debugged without a GPU.  Not part of libm0engine.so.
// With -DTB_SHIM_MAIN the file is a stand-alone program (the one to build with -fsanitize=address,undefined).
#include <stdio.h>
#include <string.h>
#include <map>
#include <thread>
#include "../../matrix0_amd/csrc/tb.h"
using namespace m0;

namespace {

// f(thread, first, last) over [0, total) in contiguous slices, one per thread.  tb_step's result does not depend on the order
// in which entries are visited (it only uses entries with d < n), so the slices may run side by side.  The slices read and
// write the table's bytes through plain accesses at the same time, as the GPU's threads do: formally a C++ data race (a
// thread sanitizer will flag it), harmless because a byte written during sweep n is 1 + n and every reader treats that value
// as not yet decided.
template <typename F>
void parallel_slices(size_t total, F f) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(f, t, total * t / nt, total * (t + 1) / nt);
    for (auto& x : th) x.join();
}
constexpr unsigned MAX_THREADS = 16;

struct Shim {
    std::map<std::string, TbTable> tables;
    TbSet set;
    Shim() { for (auto& t : set.tab) t = nullptr; }
};

// one table; its dependencies must be there.  Returns the number of sweeps, < 0 on failure.
int generate(Shim& S, const std::string& name) {
    TbTable T;
    T.name = name;
    if (!tb_parse_sig(name.c_str(), T.sig)) return -1;
    int max_sub_d = -1;
    for (const auto& d : tb_dependencies(name)) {
        auto it = S.tables.find(d);
        if (it == S.tables.end()) return -2;
        max_sub_d = std::max(max_sub_d, it->second.maxd);
    }
    const uint32_t total = tb_entries(T.sig.n);
    T.bytes.resize(total);
    parallel_slices(total, [&](unsigned, size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) T.bytes[i] = tb_init_entry(T.sig, (uint32_t)i);
    });
    std::vector<uint32_t> open;                      // entries still 0 (tb_step returns at once for the others)
    for (uint32_t i = 0; i < total; ++i) {
        if (T.bytes[i] == 1) T.maxd = 0;
        if (T.bytes[i] == TB_DRAW) open.push_back(i);
    }
    TbTable& dst = S.tables[name] = std::move(T);
    S.set.tab[tb_material_code(dst.sig)] = dst.bytes.data();
    int quiet = 0, n = 0;
    for (;;) {
        ++n;
        if (n + 1 >= TB_INVALID) return -3;
        int missing = 0;
        int miss[MAX_THREADS] = {0};
        std::vector<uint32_t> rest[MAX_THREADS];
        parallel_slices(open.size(), [&](unsigned t, size_t a, size_t b) {
            for (size_t k = a; k < b; ++k)
                if (!tb_step(dst.sig, S.set, dst.bytes.data(), open[k], n, &miss[t])) rest[t].push_back(open[k]);
        });
        const size_t before = open.size();
        open.clear();
        for (unsigned t = 0; t < MAX_THREADS; ++t) { open.insert(open.end(), rest[t].begin(), rest[t].end()); missing |= miss[t]; }
        const size_t changed = before - open.size();
        if (missing) return -4;
        if (changed) { quiet = 0; dst.maxd = n; } else ++quiet;
        if (quiet >= 2 && n > max_sub_d + 1) break;
    }
    dst.sweeps = n;
    return n;
}

}  // namespace

extern "C" {

void* tbs_new() { return new Shim(); }
void tbs_free(void* h) { delete (Shim*)h; }

// `sig` and everything it depends on (tables already there are kept).  0, or < 0 on failure.
int tbs_generate(void* h, const char* sig) {
    Shim& S = *(Shim*)h;
    std::vector<std::string> order;
    std::string bad;
    if (!tb_build_order({sig}, order, bad)) return -1;
    for (const auto& name : order)
        if (!S.tables.count(name)) { const int rc = generate(S, name); if (rc < 0) return rc; }
    return 0;
}

const uint8_t* tbs_table(void* h, const char* sig, uint64_t* n, int* maxd, int* sweeps) {
    Shim& S = *(Shim*)h;
    auto it = S.tables.find(sig);
    if (it == S.tables.end()) return nullptr;
    if (n) *n = it->second.bytes.size();
    if (maxd) *maxd = it->second.maxd;
    if (sweeps) *sweeps = it->second.sweeps;
    return it->second.bytes.data();
}

// decode -> locate round trip over every entry of `sig`: the number of valid entries, or -(idx + 1) of the first entry
// whose position does not come back to the same table and index.
int64_t tbs_roundtrip(const char* sig) {
    TbSig s;
    if (!tb_parse_sig(sig, s)) return INT64_MIN;
    int64_t valid = 0;
    for (uint32_t i = 0; i < tb_entries(s.n); ++i) {
        Pos p;
        if (!tb_decode(s, i, p)) continue;
        int code;
        uint32_t idx;
        if (!tb_locate(p, code, idx) || code != tb_material_code(s) || idx != i) return -((int64_t)i + 1);
        ++valid;
    }
    return valid;
}

// material code and index of a FEN; 0 when it cannot be located
int tbs_locate(const char* fen, int* code, uint32_t* idx) {
    Pos p;
    if (parse_fen(fen, p) != 0) return 0;
    return tb_locate(p, *code, *idx) ? 1 : 0;
}

int tbs_sig_code(const char* sig) { TbSig s; return tb_parse_sig(sig, s) ? tb_material_code(s) : -1; }

// the build order of `sig`'s closure as "KK KQK ..." (cap bytes)
int tbs_order(const char* sig, char* out, int cap) {
    std::vector<std::string> order;
    std::string bad, s;
    if (!tb_build_order({sig}, order, bad)) return -1;
    for (const auto& o : order) s += (s.empty() ? "" : " ") + o;
    if ((int)s.size() + 1 > cap) return -2;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)order.size();
}

int tbs_all_signatures(int max_men, char* out, int cap) {
    std::string s;
    const auto all = tb_all_signatures(max_men);
    for (const auto& o : all) s += (s.empty() ? "" : " ") + o;
    if ((int)s.size() + 1 > cap) return -2;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)all.size();
}

}  // extern "C"

#ifdef TB_SHIM_MAIN
int main(int argc, char** argv) {
    void* h = tbs_new();
    int rc = 0;
    for (int i = 1; i < argc && rc == 0; ++i) {
        rc = tbs_generate(h, argv[i]);
        uint64_t n = 0;
        int maxd = 0, sweeps = 0;
        if (rc == 0 && tbs_table(h, argv[i], &n, &maxd, &sweeps))
            printf("%s entries %llu largest d %d sweeps %d round trip %lld\n", argv[i], (unsigned long long)n, maxd, sweeps,
                   (long long)tbs_roundtrip(argv[i]));
    }
    tbs_free(h);
    return rc == 0 ? 0 : 1;
}
#endif
