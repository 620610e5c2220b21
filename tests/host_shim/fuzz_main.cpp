// TEST INFRASTRUCTURE: a stand-alone host program over malformed rows for sanitizer builds (-fsanitize=address,undefined) of
// the planes decode: whatever a row holds, decode_planes_host reads inside the row, writes inside its outputs and answers a
// status from the header.  Deterministic (a fixed counter-based stream); prints the histogram of statuses.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../matrix0_amd/csrc/planes_decode.h"
using namespace m0;

static uint64_t ctr = 0;
static uint64_t rnd() { return mix64(0x9E3779B97F4A7C15ull * ++ctr); }

int main() {
    // exactly-sized heap rows: an access past either end is the sanitizer's to report
    std::vector<float> planes(19 * 64);
    std::vector<uint8_t> mask(M0_POLICY_SIZE);
    Pos start;
    parse_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", start);
    const float odd[] = {0.5f, -0.0f, 2.0f, NAN, INFINITY, -1.0f, 1e-45f, 0.99999994f};
    int hist[M0_DECODE_MASK_MISMATCH + 1] = {0};
    for (int it = 0; it < 20000; ++it) {
        const int kind = it % 5;
        if (kind == 0) {                                   // a board of random men: one king each, no two on a square
            for (auto& v : planes) v = 0.f;
            const int wk = (int)(rnd() % 64), bk = (int)(rnd() % 64);
            planes[5 * 64 + wk] = 1.f; planes[11 * 64 + bk] = 1.f;
            const int density = 2 + (int)(rnd() % 6);
            for (int s = 0; s < 64; ++s) {
                const uint64_t r = rnd();
                if (s == wk || s == bk || r % density) continue;
                int pl = (int)((r >> 8) % 10);             // 0..4 white P..Q, 5..9 black p..q
                pl = pl < 5 ? pl : pl + 1;
                if ((pl % 6 == 0) && (s < 8 || s >= 56) && (r >> 20) % 8) continue;
                planes[pl * 64 + s] = 1.f;
            }
            for (int k = 12; k < 19; ++k) {
                float v = (rnd() & 1) ? 1.f : 0.f;
                if (k >= 13 && k < 17 && rnd() % 4) v = 0.f;
                if (k == 17) v = (float)((double)(rnd() % 100) / 99.0);
                if (k == 18) v = (float)((double)(rnd() % 200) / 199.0);
                for (int s = 0; s < 64; ++s) planes[k * 64 + s] = v;
            }
        } else if (kind == 1) {                            // random bits
            for (auto& v : planes) { const uint32_t u = (uint32_t)rnd(); memcpy(&v, &u, 4); }
        } else if (kind == 2) {                            // the initial position with a few values replaced
            encode_planes_f32(start, planes.data());
            for (int j = 0, m = 1 + (int)(rnd() % 4); j < m; ++j) planes[rnd() % planes.size()] = odd[rnd() % 8];
        } else {                                           // ... with queens on its empty squares, up to a board full of them
            encode_planes_f32(start, planes.data());
            const int every = 1 + (int)(rnd() % 4);
            for (int s = 16; s < 48; ++s) if (rnd() % every == 0) planes[(kind == 3 ? 4 : 10) * 64 + s] = 1.f;
        }
        if (it % 3 == 0) for (auto& m : mask) m = (rnd() % 16 == 0) ? 1 : 0;
        else {                                             // the mask the row would carry, if the row is a position at all
            memset(mask.data(), 0, mask.size());
            Pos q;
            int f0 = 0, n0 = 0;
            const int s0 = decode_planes_host(planes.data(), nullptr, q, f0, n0);
            if (s0 == M0_DECODE_OK) {
                Move mv[M0_MAX_MOVES];
                const int k = gen_legal(q, mv);
                for (int j = 0; j < k; ++j) mask[move_to_index(q, mv[j])] = 1;
            }
        }
        Pos p;
        int fl = 0, nl = 0;
        const int st = decode_planes_host(planes.data(), (it & 1) ? mask.data() : nullptr, p, fl, nl);
        if (st < 0 || st > M0_DECODE_MASK_MISMATCH || nl < 0 || nl > M0_MAX_MOVES) { printf("bad answer %d %d\n", st, nl); return 1; }
        hist[st]++;
    }
    for (int s = 0; s <= M0_DECODE_MASK_MISMATCH; ++s) printf("status %d: %d\n", s, hist[s]);
    return 0;
}
