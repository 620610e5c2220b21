// matrix0_amd/csrc/score_core.h under g++: a row scored exactly as score_rows_kernel scores it, the 64 lanes as a loop.  Lane
// `lane` folds the 16-byte pieces k * 64 + lane (k = 0..18) in that order, the lanes are merged by the kernel's tree (lane i takes
// lane i + 32, then + 16, ... + 1), and lane 0 finishes.  Only expf / logf differ from the device (the host's libm).
#include <stdint.h>
#include <vector>
#include "../../matrix0_amd/csrc/score_core.h"

using namespace m0score;

static void score_row(const float* logits, const float* pi, const uint8_t* mask, float value, float z, const m0_score_opts& o,
                      float* out) {
    const bool masked = o.mask_mode == M0_SCORE_MASK_LEGAL;
    auto each_column = [&](int lane, auto&& f) {
        for (int k = 0; k < SWEEPS; ++k) {
            const int piece = k * LANES + lane;
            if (piece >= F4) continue;
            for (int c = piece * 4; c < piece * 4 + 4; ++c) f(c, logits[c], pi[c], masked && mask[c] != 0);
        }
    };
    std::vector<Scan> scan(LANES);
    for (int lane = 0; lane < LANES; ++lane) {
        scan[lane].mode = o.mask_mode;
        each_column(lane, [&](int c, float l, float p, bool m) { scan[lane].add(c, l, p, m); });
    }
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int lane = 0; lane < off; ++lane) scan[lane].merge(scan[lane + off]);
    const Plan plan(o, scan[0]);
    std::vector<Tail> tail(LANES);
    for (int lane = 0; lane < LANES; ++lane) each_column(lane, [&](int, float l, float p, bool m) { tail[lane].add(plan, l, p, m); });
    for (int off = LANES / 2; off > 0; off >>= 1)
        for (int lane = 0; lane < off; ++lane) tail[lane].merge(tail[lane + off]);
    finish(o, scan[0], plan, tail[0], value, z, out);
}

extern "C" {

// as m0_score_rows, on the host; -1 for the arguments it refuses
int ss_score_rows(const float* logits, const float* value, const float* pi, const float* z, const uint8_t* mask, int B,
                  const m0_score_opts* opts, float* rows) {
    if (!logits || !value || !pi || !z || !rows || B <= 0 || bad_opts(opts, mask != nullptr)) return -1;
    for (int b = 0; b < B; ++b)
        score_row(logits + (size_t)b * COLS, pi + (size_t)b * COLS, mask ? mask + (size_t)b * COLS : nullptr, value[b], z[b], *opts,
                  rows + (size_t)b * M0_SCORE_COLS);
    return 0;
}

}  // extern "C"

#ifdef SCORE_SHIM_MAIN
// Stand-alone run for the sanitizers: seeded rows of every kind the core branches on, every mode; prints a checksum.
#include <stdio.h>
int main() {
    const int B = 24;
    std::vector<float> l((size_t)B * COLS), p((size_t)B * COLS, 0.f), v(B), zz(B), rows((size_t)B * M0_SCORE_COLS);
    std::vector<uint8_t> m((size_t)B * COLS, 0);
    uint64_t s = 88172645463325252ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (auto& x : l) x = (float)((double)(next() % 20001) / 1000.0 - 10.0);
    for (int b = 0; b < B; ++b) {
        const int nlegal = b % 6 == 5 ? 0 : 1 + (int)(next() % 218);
        for (int k = 0; k < nlegal; ++k) m[(size_t)b * COLS + next() % COLS] = 1;
        if (b % 4 != 3) for (int k = 0; k < 1 + b % 7; ++k) p[(size_t)b * COLS + next() % COLS] = 1.f / (float)(1 + b % 7);
        if (b % 8 == 1) l[(size_t)b * COLS + 17] = 3e4f, l[(size_t)b * COLS + 4000] = -3e4f;
        if (b % 8 == 2) l[(size_t)b * COLS + 4671] = NAN;
        v[b] = b % 8 == 6 ? INFINITY : (float)(b % 5) * 0.5f - 1.f;
        zz[b] = (float)(b % 3 - 1);
    }
    double sum = 0;
    for (int mode = M0_SCORE_MASK_LEGAL; mode <= M0_SCORE_MASK_NONE; ++mode)
        for (int huber = 0; huber < 2; ++huber) {
            const m0_score_opts o{mode, huber ? 0.05f : 0.f, huber, 0.5f};
            if (ss_score_rows(l.data(), v.data(), p.data(), zz.data(), mode == M0_SCORE_MASK_LEGAL ? m.data() : nullptr, B, &o, rows.data()))
                return 1;
            for (float x : rows) sum += x;
        }
    const m0_score_opts bad{M0_SCORE_MASK_LEGAL, 0.f, 0, 1.f};
    if (ss_score_rows(l.data(), v.data(), p.data(), zz.data(), nullptr, B, &bad, rows.data()) != -1) return 1;
    printf("score_shim ok: checksum %.6f\n", sum);
    return sum == sum ? 0 : 1;
}
#endif
