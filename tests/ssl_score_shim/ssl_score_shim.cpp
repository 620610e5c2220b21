// matrix0_amd/csrc/ssl_score_core.h and ssl_targets_core.h under g++: a row scored exactly as ssl_score_kernel scores it, the 64
// lanes as a loop.  Lane `sq` scores tensor square sq, the lanes are merged by the kernel's tree (lane i takes lane i + 32, then
// + 16, ... + 1), and lane 0 finishes.  The core carries its own exp and log, so nothing here depends on the host's libm.
#include <stdint.h>
#include <vector>
#include "../../matrix0_amd/csrc/ssl_score_core.h"

using namespace m0sslscore;

namespace {

constexpr size_t PLANES_ROW = (size_t)M0_PLANES * 64, TARGETS_ROW = (size_t)m0ssl::TARGET_CH * 64;

// the board of a row of planes; false when the row is not usable
bool board_of(const float* prow, m0ssl::Board4& board, bool& white) {
    bool unusable = false;
    for (int sq = 0; sq < 64; ++sq) {
        bool bad;
        board.set(sq, m0ssl::plane_piece(prow, sq, &bad));
        unusable = unusable || bad || m0ssl::side_bad(prow[12 * 64 + sq], prow[12 * 64]);
    }
    white = prow[12 * 64] == 1.f;
    return !unusable;
}

void score_row(const float* hrow, int tasks, const float* prow, const float* trow, float* out) {
    m0ssl::Board4 board;
    bool white;
    const bool unusable = !board_of(prow, board, white), stored = trow != nullptr;
    std::vector<Cell> cell(LANES);
    bool poisoned = false, differ = false;
    for (int sq = 0; sq < LANES; ++sq) {
        const Logits z = load_logits(tasks, hrow, sq);
        poisoned = poisoned || !(poison_of(z) == 0.f);
        Targets own = {};
        if (!unusable) own = targets_of(m0ssl::square_targets(board, sq, white));
        Targets t = own;
        if (stored) {
            t = stored_targets(trow, sq);
            differ = differ || classes_differ(tasks, t, own);
        }
        if (stored || !unusable) cell[sq] = score_square(tasks, z, t);
    }
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int lane = 0; lane < off; ++lane) cell[lane].merge(cell[lane + off]);
    finish(cell[0], unusable, poisoned, stored, differ, out);
}

}  // namespace

extern "C" {

// as m0_ssl_score_rows, on the host; -1 for the arguments it refuses
int sss_score_rows(const float* heads, int tasks, const float* planes, const float* targets, int B, float* rows) {
    if (!heads || !planes || !rows || B <= 0 || bad_tasks(tasks)) return -1;
    const size_t head_row = (size_t)channels(tasks) * 64;
    for (int b = 0; b < B; ++b)
        score_row(heads + b * head_row, tasks, planes + b * PLANES_ROW, targets ? targets + b * TARGETS_ROW : nullptr,
                  rows + (size_t)b * M0_SSL_SCORE_COLS);
    return 0;
}

// as m0_ssl_targets_planes, on the host
int sss_targets_planes(const float* planes, int n, float* out, int32_t* status) {
    if (!planes || !out || !status || n <= 0) return -1;
    for (int i = 0; i < n; ++i) {
        m0ssl::Board4 board;
        bool white;
        status[i] = board_of(planes + i * PLANES_ROW, board, white) ? 0 : 1;
        if (status[i]) continue;
        for (int sq = 0; sq < 64; ++sq) m0ssl::store_square(m0ssl::square_targets(board, sq, white), out + i * TARGETS_ROW, sq);
    }
    return 0;
}

// the core's own exp (x <= 0), log (x >= 1) and log(1 + f), element by element, for the tests of their accuracy
void sss_math(const float* x, int n, int which, float* y) {
    for (int i = 0; i < n; ++i) y[i] = which == 0 ? exp_le0(x[i]) : which == 1 ? log_ge1(x[i]) : log1p_series(x[i]);
}

}  // extern "C"

#ifdef SSL_SCORE_SHIM_MAIN
// Stand-alone run for the sanitizers: seeded rows of every kind the core branches on, every task set, targets from the planes
// and stored; prints a checksum.
#include <math.h>
#include <stdio.h>
int main() {
    const int B = 24;
    std::vector<float> p(B * PLANES_ROW, 0.f), t(B * TARGETS_ROW, 0.f), rows((size_t)B * M0_SSL_SCORE_COLS);
    std::vector<int32_t> st(B);
    uint64_t s = 88172645463325252ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int b = 0; b < B; ++b) {
        float* prow = p.data() + b * PLANES_ROW;
        for (int sq = 0; sq < 64; ++sq) {
            if (next() % 3 == 0) prow[(next() % 12) * 64 + sq] = 1.f;
            prow[12 * 64 + sq] = (float)(b % 2);
        }
        if (b % 8 == 5) prow[3 * 64 + 9] = 0.5f;
        if (b % 8 == 6) prow[12 * 64 + 63] = 1.f - prow[12 * 64];
        if (b % 8 == 7) prow[0 * 64 + 1] = prow[7 * 64 + 1] = 1.f;
    }
    if (sss_targets_planes(p.data(), B, t.data(), st.data())) return 1;
    double sum = 0;
    for (int tasks : {31, 1, 17, 14}) {
        std::vector<float> h((size_t)B * channels(tasks) * 64);
        for (auto& x : h) x = (float)((double)(next() % 80001) / 1000.0 - 40.0);
        h[5] = NAN; h[h.size() - 1] = INFINITY;
        for (const float* targets : {(const float*)nullptr, (const float*)t.data()}) {
            if (sss_score_rows(h.data(), tasks, p.data(), targets, B, rows.data())) return 1;
            for (float x : rows) sum += x;
        }
    }
    if (sss_score_rows(p.data(), 0, p.data(), nullptr, B, rows.data()) != -1) return 1;
    printf("ssl_score_shim ok: checksum %.6f\n", sum);
    return sum == sum ? 0 : 1;
}
#endif
