// TEST INFRASTRUCTURE: host (g++) build of matrix0_amd/csrc/rowpack_core.h with the lane split of rowpack_kernels.hip written as
// loops -- a wave's 64 lanes are the inner loop, a ballot is a loop that collects a bit per lane, a readlane an array read -- so
// that the split can be compared on the CPU with the straight loops of rowpack_host.h (m0_rowpack_*_host), and run under the
// sanitizers as a stand-alone program.  Not part of libm0engine.so.
#include <stdio.h>
#include <stdlib.h>
#include "../../matrix0_amd/csrc/rowpack_host.h"

using namespace m0rowpack;

namespace {

void load_piece(const void* row, int piece, int pieces, uint32_t w[4]) {
    if (piece < pieces) memcpy(w, (const uint8_t*)row + (size_t)piece * 16, 16);
    else w[0] = w[1] = w[2] = w[3] = 0u;
}

// rowpack_count_kernel of one row
void count_row(const float* prow, const uint8_t* mrow, const Pos& p, int status, m0_rowpack_pos* out, int32_t* counts) {
    bool other = false;
    int mcount = 0, pcount = 0;
    uint32_t w[4];
    for (int k = 0; mrow && k < MASK_SWEEPS; ++k)
        for (int lane = 0; lane < LANES; ++lane) {
            load_piece(mrow, k * LANES + lane, MASK_PIECES, w);
            mcount += __builtin_popcount(mask_piece_bits(w, other));
        }
    int rk, mk;
    row_kinds(status, mrow != nullptr, !other, rk, mk);
    for (int k = 0; rk == M0_ROWPACK_PACKED && k < PI_SWEEPS; ++k)
        for (int lane = 0; lane < LANES; ++lane) {
            load_piece(prow, k * LANES + lane, PI_PIECES, w);
            pcount += __builtin_popcount(pi_piece_bits(w[0], w[1], w[2], w[3]));
        }
    for (int lane = 0; lane < 13; ++lane) ((uint64_t*)out)[lane] = rk == M0_ROWPACK_PACKED ? packed_word(p, mk, lane) : raw_word(mk, lane);
    counts[0] = pcount;
    counts[1] = rk == M0_ROWPACK_PACKED && mk == M0_ROWPACK_MASK_LIST ? mcount : 0;
}

// rowpack_fill_kernel of one PACKED row
void fill_row(const float* prow, const uint8_t* mrow, int mk, int64_t base, int64_t mbase, uint16_t* pi_idx, float* pi_val,
              uint16_t* mask_idx) {
    for (int k = 0; k < PI_SWEEPS; ++k) {
        uint32_t w[LANES][4];
        int bits[LANES];
        uint64_t ballot[4] = {0, 0, 0, 0};
        for (int lane = 0; lane < LANES; ++lane) {
            load_piece(prow, k * LANES + lane, PI_PIECES, w[lane]);
            bits[lane] = pi_piece_bits(w[lane][0], w[lane][1], w[lane][2], w[lane][3]);
            for (int j = 0; j < 4; ++j) ballot[j] |= (uint64_t)(bits[lane] >> j & 1) << lane;
        }
        for (int lane = 0; lane < LANES; ++lane)
            for (int j = 0; j < 4; ++j)
                if (bits[lane] >> j & 1) {
                    const int64_t at = base + pi_slot(ballot, bits[lane], lane, j);
                    pi_idx[at] = (uint16_t)((k * LANES + lane) * 4 + j);
                    memcpy(&pi_val[at], &w[lane][j], 4);
                }
        for (int j = 0; j < 4; ++j) base += __builtin_popcountll(ballot[j]);
    }
    if (mk != M0_ROWPACK_MASK_LIST) return;
    for (int k = 0; k < MASK_SWEEPS; ++k) {
        int prefix = 0;                                                       // wave_prefix: the lanes below
        for (int lane = 0; lane < LANES; ++lane) {
            uint32_t w[4];
            bool other = false;
            load_piece(mrow, k * LANES + lane, MASK_PIECES, w);
            int bits = mask_piece_bits(w, other);
            int64_t at = mbase + prefix;
            prefix += __builtin_popcount(bits);
            while (bits) {
                const int j = __builtin_ctz(bits);
                bits &= bits - 1;
                mask_idx[at++] = (uint16_t)((k * LANES + lane) * 16 + j);
            }
        }
        mbase += prefix;
    }
}

// expand_row of rowpack_kernels.hip: the wave's current 64 entries in ci / cv, an entry taken by the lane that owns its piece
template <int PER, int PIECES>
void expand_row(const uint16_t* idx, const float* val, int64_t e, const int64_t end, void* out) {
    constexpr int SWEEPS = (PIECES + LANES - 1) / LANES;
    int64_t cb = e;
    int ci[LANES];
    uint32_t cv[LANES];
    auto load_chunk = [&]() {
        for (int lane = 0; lane < LANES; ++lane) {
            ci[lane] = cb + lane < end ? (int)idx[cb + lane] : 65535;
            cv[lane] = 0;
            if (PER == 4 && cb + lane < end) memcpy(&cv[lane], &val[cb + lane], 4);
        }
    };
    load_chunk();
    for (int k = 0; k < SWEEPS; ++k) {
        const int hi = (k + 1) * LANES * PER;
        uint32_t o[LANES][4];
        memset(o, 0, sizeof(o));
        while (e < end) {
            if (e - cb >= LANES) { cb += LANES; load_chunk(); }
            const int j = (int)(e - cb), c = ci[j];
            if (c >= hi) break;
            const int lane = entry_lane(c, PER);
            if (PER == 4) o[lane][c & 3] = cv[j];
            else o[lane][(c & 15) >> 2] |= 1u << ((c & 3) * 8);
            ++e;
        }
        for (int lane = 0; lane < LANES; ++lane)
            if (k * LANES + lane < PIECES) memcpy((uint8_t*)out + (size_t)(k * LANES + lane) * 16, o[lane], 16);
    }
}

}  // namespace

extern "C" {

// m0_rowpack_pack_host with the kernels' lane split: 0, or -1 with sizes set when the capacity does not do
int rs_pack_lanes(const float* planes, const float* pi, const float* z, const uint8_t* mask, int n, m0_rowpack_arrays* out,
                  int64_t* sizes) {
    const size_t N = (size_t)n;
    std::vector<m0_rowpack_pos> pos(N);
    std::vector<int32_t> counts(2 * N), raw_slot;
    std::vector<int64_t> pi_off, mask_off;
    for (size_t i = 0; i < N; ++i) {
        Pos p;
        int flags = 0, nlegal = 0;
        const uint8_t* mrow = mask ? mask + i * COLS : nullptr;
        const int st = m0::decode_planes_host(planes + i * PLANE_FLOATS, mrow, p, flags, nlegal);
        count_row(pi + i * COLS, mrow, p, st, &pos[i], &counts[2 * i]);
    }
    scan_counts(pos.data(), counts.data(), N, pi_off, mask_off, raw_slot, sizes);
    if (!check_capacity(out, sizes, mask != nullptr).empty()) return -1;
    for (size_t i = 0; i < N; ++i) {
        const uint8_t* mrow = mask ? mask + i * COLS : nullptr;
        if (pos[i].row_kind == M0_ROWPACK_RAW) {
            const size_t r = (size_t)raw_slot[i];
            memcpy(out->raw_planes + r * PLANE_FLOATS, planes + i * PLANE_FLOATS, PLANE_FLOATS * sizeof(float));
            memcpy(out->raw_pi + r * COLS, pi + i * COLS, COLS * sizeof(float));
            if (mrow) memcpy(out->raw_mask + r * COLS, mrow, COLS);
        } else {
            fill_row(pi + i * COLS, mrow, pos[i].mask_kind, pi_off[i], mask_off[i], out->pi_idx, out->pi_val, out->mask_idx);
        }
    }
    memcpy(out->pos, pos.data(), N * sizeof(m0_rowpack_pos));
    memcpy(out->z, z, N * sizeof(float));
    memcpy(out->pi_off, pi_off.data(), (N + 1) * sizeof(int64_t));
    memcpy(out->mask_off, mask_off.data(), (N + 1) * sizeof(int64_t));
    out->n = n; out->pi_n = sizes[0]; out->mask_n = sizes[1]; out->raw_n = sizes[2];
    return 0;
}

// m0_rowpack_unpack_host with the kernels' lane split for pi and LIST masks (planes and LEGAL masks: the encoder, as there)
int rs_unpack_lanes(const m0_rowpack_arrays* in, float* planes, float* pi, float* z, uint8_t* mask) {
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    if (!check_arrays(in, positions, raw_slot).empty() || (mask != nullptr) != has_masks(*in)) return -1;
    unpack_host(*in, positions, raw_slot, planes, pi, z, mask);
    for (size_t i = 0; i < (size_t)in->n; ++i) {
        if (in->pos[i].row_kind == M0_ROWPACK_RAW) continue;
        memset(pi + i * COLS, 0xEE, COLS * sizeof(float));                    // every piece is written again, zeros included
        expand_row<4, PI_PIECES>(in->pi_idx, in->pi_val, in->pi_off[i], in->pi_off[i + 1], pi + i * COLS);
        if (mask && in->pos[i].mask_kind == M0_ROWPACK_MASK_LIST) {
            memset(mask + i * COLS, 0xEE, COLS);
            expand_row<16, MASK_PIECES>(in->mask_idx, nullptr, in->mask_off[i], in->mask_off[i + 1], mask + i * COLS);
        }
    }
    return 0;
}

}  // extern "C"

#ifdef ROWPACK_SHIM_MAIN
// 20 000 seeded rows in batches of 500 through both packers and both unpackers, every buffer a vector of exactly the size
// asked for: positions after seeded legal moves from the start, soft pi on seeded columns; some rows malformed (RAW), some with
// every column an entry, some with edited masks (LIST) or a mask byte of 2 (RAW).
static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }

int main() {
    const int BATCH = 500, TOTAL = 20000;
    long kinds[2] = {0, 0}, masks[3] = {0, 0, 0}, full = 0;
    for (int done = 0; done < TOTAL; done += BATCH) {
        const bool with_mask = (done / BATCH) % 4 != 3;
        std::vector<float> planes((size_t)BATCH * PLANE_FLOATS), pi((size_t)BATCH * COLS, 0.f), z(BATCH);
        std::vector<uint8_t> mask((size_t)BATCH * COLS, 0);
        Pos p;
        m0::parse_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", p);
        for (int i = 0; i < BATCH; ++i) {
            m0::Move mv[M0_MAX_MOVES];
            int k = m0::gen_legal(p, mv);
            if (k == 0 || p.halfmove > 90) { m0::parse_fen("rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", p); k = m0::gen_legal(p, mv); }
            float* srow = &planes[(size_t)i * PLANE_FLOATS];
            float* prow = &pi[(size_t)i * COLS];
            uint8_t* mrow = &mask[(size_t)i * COLS];
            m0::encode_planes_f32(p, srow);
            for (int j = 0; j < k; ++j) {
                const int idx = m0::move_to_index(p, mv[j]);
                mrow[idx] = 1;
                if (next() % 3) prow[idx] = (float)(1 + next() % 100) / 128.f;
            }
            z[i] = (float)((int)(next() % 3) - 1);
            const int what = (int)(next() % 16);
            if (what == 0) srow[next() % PLANE_FLOATS] = 0.5f;                                   // RAW
            if (what == 1) { for (int c = 0; c < COLS; ++c) prow[c] = (float)(1 + next() % 7); ++full; }
            if (what == 2) mrow[next() % COLS] ^= 1;                                             // LIST
            if (what == 3) mrow[next() % COLS] = 2;                                              // RAW with a mask
            if (what == 4) { const uint32_t odd[3] = {0x80000000u, 1u, 0x7FC00001u}; memcpy(&prow[next() % COLS], &odd[next() % 3], 4); }
            if (what == 5) memset(prow, 0, COLS * sizeof(float));
            m0::make_move(p, mv[next() % k]);
        }
        const uint8_t* mk = with_mask ? mask.data() : nullptr;
        int64_t sizes[3], sizes2[3];
        m0_rowpack_arrays none = {};
        none.n = BATCH;
        if (pack_host(planes.data(), pi.data(), z.data(), mk, BATCH, &none, sizes).empty()) { printf("a capacity of 0 was taken\n"); return 1; }
        struct Store {
            std::vector<m0_rowpack_pos> pos; std::vector<float> z, pi_val, raw_planes, raw_pi; std::vector<int64_t> pi_off, mask_off;
            std::vector<uint16_t> pi_idx, mask_idx; std::vector<uint8_t> raw_mask;
            m0_rowpack_arrays a;
            Store(int n, const int64_t* s, bool m) : pos(n), z(n), pi_val(s[0]), raw_planes(s[2] * PLANE_FLOATS), raw_pi(s[2] * COLS),
                pi_off(n + 1), mask_off(n + 1), pi_idx(s[0]), mask_idx(s[1]), raw_mask(m ? s[2] * COLS : 0) {
                a = {n, s[0], s[1], s[2], pos.data(), z.data(), pi_off.data(), pi_idx.data(), pi_val.data(), mask_off.data(),
                     mask_idx.data(), raw_planes.data(), raw_pi.data(), m ? raw_mask.data() : nullptr};
            }
        } a(BATCH, sizes, with_mask), b(BATCH, sizes, with_mask);
        if (!pack_host(planes.data(), pi.data(), z.data(), mk, BATCH, &a.a, sizes).empty()) { printf("pack_host refused its own sizes\n"); return 1; }
        if (rs_pack_lanes(planes.data(), pi.data(), z.data(), mk, BATCH, &b.a, sizes2) != 0 || memcmp(sizes, sizes2, sizeof(sizes))) { printf("lane sizes differ\n"); return 1; }
        if (memcmp(a.pos.data(), b.pos.data(), BATCH * sizeof(m0_rowpack_pos)) || a.pi_off != b.pi_off || a.mask_off != b.mask_off ||
            a.pi_idx != b.pi_idx || memcmp(a.pi_val.data(), b.pi_val.data(), a.pi_val.size() * 4) || a.mask_idx != b.mask_idx ||
            memcmp(a.raw_planes.data(), b.raw_planes.data(), a.raw_planes.size() * 4) || memcmp(a.raw_pi.data(), b.raw_pi.data(), a.raw_pi.size() * 4) ||
            a.raw_mask != b.raw_mask) { printf("the lane split packs other bytes (batch at %d)\n", done); return 1; }
        for (int way = 0; way < 2; ++way) {
            std::vector<float> s2(planes.size()), pi2(pi.size()), z2(BATCH);
            std::vector<uint8_t> m2(with_mask ? mask.size() : 0);
            std::vector<Pos> positions;
            std::vector<int32_t> raw_slot;
            if (way == 0) {
                const std::string why = check_arrays(&a.a, positions, raw_slot);
                if (!why.empty()) { printf("check_arrays: %s\n", why.c_str()); return 1; }
                unpack_host(a.a, positions, raw_slot, s2.data(), pi2.data(), z2.data(), with_mask ? m2.data() : nullptr);
            } else if (rs_unpack_lanes(&a.a, s2.data(), pi2.data(), z2.data(), with_mask ? m2.data() : nullptr) != 0) { printf("lane unpack refused\n"); return 1; }
            if (memcmp(s2.data(), planes.data(), planes.size() * 4) || memcmp(pi2.data(), pi.data(), pi.size() * 4) ||
                memcmp(z2.data(), z.data(), BATCH * 4) || (with_mask && memcmp(m2.data(), mask.data(), mask.size()))) {
                printf("round trip differs (way %d, batch at %d)\n", way, done);
                return 1;
            }
        }
        for (int i = 0; i < BATCH; ++i) { ++kinds[a.pos[i].row_kind]; ++masks[a.pos[i].mask_kind]; }
    }
    printf("rows %ld packed %ld raw %ld mask_none %ld mask_legal %ld mask_list %ld full_pi %ld\n", kinds[0] + kinds[1], kinds[0], kinds[1],
           masks[0], masks[1], masks[2], full);
    return kinds[1] > 0 && full > 0 && masks[2] > 0 ? 0 : 1;
}
#endif
