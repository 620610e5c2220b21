// The tablebase handle of the C-ABI (include/m0_engine.h, m0_tb_*) and the host helpers around tb_core.h: the tables a
// signature depends on, the build order, the GPU build (tb_build.hip).  Internal.
#pragma once
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "tb_core.h"

namespace m0 {

struct TbTable {
    std::string name;              // "KQKR"
    TbSig sig;
    std::vector<uint8_t> bytes;    // 2 * 64^n entries
    int maxd = -1;                 // largest d of a decided entry, -1 when there is none
    int sweeps = 0;                // sweeps the build ran (0: loaded from a file written before it was known)
    double build_ms = 0.0;
};

}  // namespace m0

// The tables once more in the memory of one HIP device, for the probe inside select_kernel (tree_select.hip): `set` is a
// TbSet in device memory whose pointers are device pointers.  Made on first use (m0::tb_device_set), shared by every engine
// on that device, freed with the handle and never before: a hipFree synchronises the whole device.
struct m0_tb_device_copy {
    int device = -1;
    const m0::TbSet* set = nullptr;
    std::vector<void*> allocs;          // the tables and the set
};

struct m0_tb {
    std::vector<m0::TbTable> tables;    // in build order
    m0::TbSet set;                      // host pointers into tables[i].bytes
    int max_men = 0;
    mutable std::mutex dev_mu;          // guards dev_copies (the handle itself is immutable)
    mutable std::vector<m0_tb_device_copy> dev_copies;
    void index_tables() {
        for (auto& t : set.tab) t = nullptr;
        max_men = 0;
        for (auto& t : tables) {
            set.tab[m0::tb_material_code(t.sig)] = t.bytes.data();
            max_men = std::max(max_men, (int)t.sig.n);
        }
    }
};

namespace m0 {

inline std::string tb_sig_name(int nw, const int* wt, int nb, const int* bt) {
    static const char L[] = "PNBRQ";
    std::string s = "K";
    for (int i = 0; i < nw; ++i) s += L[wt[i]];
    s += 'K';
    for (int i = 0; i < nb; ++i) s += L[bt[i]];
    return s;
}

// Canonical name of the material (w, b), men in any order: sides sorted, the greater side first.
inline std::string tb_canonical(std::vector<int> w, std::vector<int> b) {
    std::sort(w.begin(), w.end(), std::greater<int>());
    std::sort(b.begin(), b.end(), std::greater<int>());
    if (b.size() > w.size() || (b.size() == w.size() && b > w)) w.swap(b);
    return tb_sig_name((int)w.size(), w.data(), (int)b.size(), b.data());
}

// The tables the moves of `name` lead into: one man captured, one pawn promoted, or both.
inline std::vector<std::string> tb_dependencies(const std::string& name) {
    TbSig s;
    std::vector<std::string> out;
    if (!tb_parse_sig(name.c_str(), s)) return out;
    const std::vector<int> side[2] = {std::vector<int>(s.wt, s.wt + s.nw), std::vector<int>(s.bt, s.bt + s.nb)};
    auto add = [&](const std::vector<int>& w, const std::vector<int>& b) {
        const std::string d = tb_canonical(w, b);
        if (d != name && std::find(out.begin(), out.end(), d) == out.end()) out.push_back(d);
    };
    for (int c = 0; c < 2; ++c) {
        for (size_t i = 0; i < side[c].size(); ++i) {                 // a man of side c is captured
            std::vector<int> mine = side[c];
            mine.erase(mine.begin() + i);
            c == 0 ? add(mine, side[1]) : add(side[0], mine);
        }
        for (size_t i = 0; i < side[c].size(); ++i) {                 // a pawn of side c promotes, with or without a capture
            if (side[c][i] != PAWN) continue;
            for (int promo = KNIGHT; promo <= QUEEN; ++promo) {
                std::vector<int> mine = side[c];
                mine[i] = promo;
                c == 0 ? add(mine, side[1]) : add(side[0], mine);
                const std::vector<int>& other = side[c ^ 1];
                for (size_t j = 0; j < other.size(); ++j) {
                    std::vector<int> rest = other;
                    rest.erase(rest.begin() + j);
                    c == 0 ? add(mine, rest) : add(rest, mine);
                }
            }
        }
    }
    return out;
}

inline int tb_pawns(const TbSig& s) {
    int n = 0;
    for (int i = 0; i < s.nw; ++i) n += s.wt[i] == PAWN;
    for (int i = 0; i < s.nb; ++i) n += s.bt[i] == PAWN;
    return n;
}

// `sigs` plus everything they depend on, in an order in which every table comes after its dependencies: by number of men,
// then by number of pawns (captures lose a man, promotions a pawn), then by name.  false: a name that is not in scope.
inline bool tb_build_order(const std::vector<std::string>& sigs, std::vector<std::string>& order, std::string& bad) {
    order.clear();
    std::vector<std::string> todo = sigs;
    while (!todo.empty()) {
        const std::string s = todo.back();
        todo.pop_back();
        TbSig sig;
        if (!tb_parse_sig(s.c_str(), sig)) { bad = s; return false; }
        if (std::find(order.begin(), order.end(), s) != order.end()) continue;
        order.push_back(s);
        for (const auto& d : tb_dependencies(s)) todo.push_back(d);
    }
    auto rank = [](const std::string& s) {
        TbSig sig;
        tb_parse_sig(s.c_str(), sig);
        return sig.n * 8 + tb_pawns(sig);
    };
    std::sort(order.begin(), order.end(), [&](const std::string& a, const std::string& b) {
        const int ra = rank(a), rb = rank(b);
        return ra != rb ? ra < rb : a < b;
    });
    return true;
}

// Every signature in scope with at most max_men men (max_men 2..4).
inline std::vector<std::string> tb_all_signatures(int max_men) {
    std::vector<std::string> out{"KK"};
    for (int a = QUEEN; a >= PAWN && max_men >= 3; --a) out.push_back(tb_canonical({a}, {}));
    for (int a = QUEEN; a >= PAWN && max_men >= 4; --a)
        for (int b = a; b >= PAWN; --b) {
            out.push_back(tb_canonical({a, b}, {}));
            if (!(a == PAWN && b == PAWN)) out.push_back(tb_canonical({a}, {b}));
        }
    return out;
}

// capi_tb.hip: the device copy of tb's tables on `hip_device`, uploaded (and the upload waited for) at the first call.
int tb_device_set(const m0_tb* tb, int hip_device, const TbSet** set_dev, std::string& err);
// ... all of them freed (m0_tb_destroy)
void tb_free_device_copies(m0_tb* tb);

// capi_tb.hip: m0_tb_root_lines for a parsed position and a probe limit; false (out untouched) when the root is no hit.
// out->id is kept.
bool tb_root_lines(const m0_tb* tb, int max_men, const Pos& root, int multipv, int pv_len, m0_analysis_result* out);

// tb_build.hip: builds the tables `order` (a tb_build_order result) on the device and leaves them in tb->tables.
int tb_build_on_device(int hip_device, const std::vector<std::string>& order, m0_tb* tb, std::string& err);

}  // namespace m0
