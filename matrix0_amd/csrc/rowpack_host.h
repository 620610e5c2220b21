// Host side of the packed training rows (include/m0_rowpack.h), plain C++ without HIP: the checks every unpacking call runs on
// the arrays it is given, the scan between the two packing passes, and packing and unpacking themselves with straight loops
// over rowpack_core.h.  Used by capi_rowpack.hip (m0_rowpack_*_host and the device calls' host halves) and, under g++, by
// tests/rowpack_shim.
#pragma once
#include <limits.h>
#include <string.h>
#include <string>
#include <vector>
#include "rowpack_core.h"

namespace m0rowpack {

inline bool has_masks(const m0_rowpack_arrays& a) { return a.n > 0 && a.pos && a.pos[0].mask_kind != M0_ROWPACK_MASK_NONE; }

// What the encoder runs on for a RAW row before the row's own planes replace its output: any position will do
inline Pos filler_pos() {
    Pos p;
    m0::parse_fen("4k3/8/8/8/8/8/8/4K3 w - - 0 1", p);
    return p;
}

// The arrays of packed rows as m0_rowpack_unpack* and m0_net_score_packed take them.  Empty when they are fine, with
// positions [n] (the filler for RAW rows) and raw_slot [n] (-1 for PACKED rows) filled; otherwise why not.
inline std::string check_arrays(const m0_rowpack_arrays* a, std::vector<Pos>& positions, std::vector<int32_t>& raw_slot) {
    if (!a) return "null argument";
    if (a->n <= 0 || a->n > INT_MAX) return "the number of rows must be positive";
    if (!a->pos || !a->z || !a->pi_off || !a->mask_off) return "null array";
    if (a->pi_n < 0 || a->mask_n < 0 || a->raw_n < 0) return "negative count";
    if ((a->pi_n > 0 && (!a->pi_idx || !a->pi_val)) || (a->mask_n > 0 && !a->mask_idx)) return "null entry array";
    const size_t n = (size_t)a->n;
    const bool masks = has_masks(*a);
    if (a->raw_n > 0 && (!a->raw_planes || !a->raw_pi || (masks && !a->raw_mask))) return "null raw array";
    if (a->pi_off[0] != 0 || a->mask_off[0] != 0 || a->pi_off[n] != a->pi_n || a->mask_off[n] != a->mask_n)
        return "offsets do not run from 0 to the counts";
    positions.assign(n, filler_pos());
    raw_slot.assign(n, -1);
    int64_t raw = 0;
    for (size_t i = 0; i < n; ++i) {
        const std::string at = " (row " + std::to_string(i) + ")";
        const m0_rowpack_pos& q = a->pos[i];
        const int64_t p0 = a->pi_off[i], p1 = a->pi_off[i + 1], m0_ = a->mask_off[i], m1 = a->mask_off[i + 1];
        if (p1 < p0 || p1 - p0 > COLS || p1 > a->pi_n || m1 < m0_ || m1 - m0_ > COLS || m1 > a->mask_n) return "offsets do not ascend" + at;
        if (q.row_kind > M0_ROWPACK_RAW || q.mask_kind > M0_ROWPACK_MASK_LIST) return "kind out of range" + at;
        if ((q.mask_kind != M0_ROWPACK_MASK_NONE) != masks) return "rows with and without masks" + at;
        if (m1 != m0_ && !(q.row_kind == M0_ROWPACK_PACKED && q.mask_kind == M0_ROWPACK_MASK_LIST)) return "mask entries of a row that lists none" + at;
        if (q.row_kind == M0_ROWPACK_RAW) {
            if (p1 != p0 || q.mask_kind == M0_ROWPACK_MASK_LEGAL) return "a raw row with entries" + at;
            if (raw >= a->raw_n) return "more raw rows than raw_n" + at;
            raw_slot[i] = (int32_t)raw++;
            continue;
        }
        if (unpack_pos(q, positions[i]) != M0_DECODE_OK) { positions[i] = filler_pos(); return "no position" + at; }
        for (int64_t e = p0; e < p1; ++e)
            if (a->pi_idx[e] >= COLS || (e > p0 && a->pi_idx[e] <= a->pi_idx[e - 1])) return "pi columns do not ascend below 4672" + at;
        for (int64_t e = m0_; e < m1; ++e)
            if (a->mask_idx[e] >= COLS || (e > m0_ && a->mask_idx[e] <= a->mask_idx[e - 1])) return "mask columns do not ascend below 4672" + at;
    }
    if (raw != a->raw_n) return "fewer raw rows than raw_n";
    return "";
}

// Between the passes: counts i32 [n][2] (pi entries, LIST entries) and the rows' kinds -> offsets [n + 1], raw slots, sizes [3]
inline void scan_counts(const m0_rowpack_pos* pos, const int32_t* counts, size_t n, std::vector<int64_t>& pi_off,
                        std::vector<int64_t>& mask_off, std::vector<int32_t>& raw_slot, int64_t* sizes) {
    pi_off.assign(n + 1, 0); mask_off.assign(n + 1, 0); raw_slot.assign(n, -1);
    int32_t raw = 0;
    for (size_t i = 0; i < n; ++i) {
        pi_off[i + 1] = pi_off[i] + counts[2 * i];
        mask_off[i + 1] = mask_off[i] + counts[2 * i + 1];
        if (pos[i].row_kind == M0_ROWPACK_RAW) raw_slot[i] = raw++;
    }
    sizes[0] = pi_off[n]; sizes[1] = mask_off[n]; sizes[2] = raw;
}

// the caller's arrays against the sizes; empty when they hold them
inline std::string check_capacity(const m0_rowpack_arrays* out, const int64_t* sizes, bool masks) {
    if (out->pi_n < sizes[0] || out->mask_n < sizes[1] || out->raw_n < sizes[2]) return "capacity too small (see sizes)";
    if (!out->pos || !out->z || !out->pi_off || !out->mask_off || (sizes[0] > 0 && (!out->pi_idx || !out->pi_val)) ||
        (sizes[1] > 0 && !out->mask_idx) || (sizes[2] > 0 && (!out->raw_planes || !out->raw_pi || (masks && !out->raw_mask))))
        return "null output array";
    return "";
}

inline uint32_t bits_of(float x) { return m0::f32_bits(x); }

// m0_rowpack_pack_host without the argument checks; pi null: rows without a policy (no entries, zero raw_pi rows).  Empty, or why the capacity does not do (sizes are set either way).
inline std::string pack_host(const float* planes, const float* pi, const float* z, const uint8_t* mask, size_t n,
                             m0_rowpack_arrays* out, int64_t* sizes) {
    std::vector<m0_rowpack_pos> pos(n);
    std::vector<int32_t> counts(2 * n, 0), raw_slot;
    std::vector<int64_t> pi_off, mask_off;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* mrow = mask ? mask + i * COLS : nullptr;
        const float* prow = pi ? pi + i * COLS : nullptr;
        Pos p;
        int flags = 0, nlegal = 0, rk, mk, set = 0;
        const int st = m0::decode_planes_host(planes + i * PLANE_FLOATS, mrow, p, flags, nlegal);
        bool binary = true;
        for (int c = 0; mrow && c < COLS; ++c) { binary = binary && mrow[c] <= 1; set += mrow[c] != 0; }
        row_kinds(st, mrow != nullptr, binary, rk, mk);
        uint64_t* w = (uint64_t*)&pos[i];
        for (int k = 0; k < 13; ++k) w[k] = rk == M0_ROWPACK_PACKED ? packed_word(p, mk, k) : raw_word(mk, k);
        if (rk != M0_ROWPACK_PACKED) continue;
        for (int c = 0; prow && c < COLS; ++c) counts[2 * i] += bits_of(prow[c]) != 0u;
        if (mk == M0_ROWPACK_MASK_LIST) counts[2 * i + 1] = set;
    }
    scan_counts(pos.data(), counts.data(), n, pi_off, mask_off, raw_slot, sizes);
    const std::string why = check_capacity(out, sizes, mask != nullptr);
    if (!why.empty()) return why;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* mrow = mask ? mask + i * COLS : nullptr;
        const float* prow = pi ? pi + i * COLS : nullptr;
        if (pos[i].row_kind == M0_ROWPACK_RAW) {
            const size_t r = (size_t)raw_slot[i];
            memcpy(out->raw_planes + r * PLANE_FLOATS, planes + i * PLANE_FLOATS, PLANE_FLOATS * sizeof(float));
            if (prow) memcpy(out->raw_pi + r * COLS, prow, COLS * sizeof(float));
            else memset(out->raw_pi + r * COLS, 0, COLS * sizeof(float));
            if (mrow) memcpy(out->raw_mask + r * COLS, mrow, COLS);
            continue;
        }
        int64_t e = pi_off[i];
        for (int c = 0; prow && c < COLS; ++c)
            if (bits_of(prow[c]) != 0u) { out->pi_idx[e] = (uint16_t)c; out->pi_val[e] = prow[c]; ++e; }
        if (pos[i].mask_kind != M0_ROWPACK_MASK_LIST) continue;
        e = mask_off[i];
        for (int c = 0; c < COLS; ++c)
            if (mrow[c]) out->mask_idx[e++] = (uint16_t)c;
    }
    memcpy(out->pos, pos.data(), n * sizeof(m0_rowpack_pos));
    memcpy(out->z, z, n * sizeof(float));
    memcpy(out->pi_off, pi_off.data(), (n + 1) * sizeof(int64_t));
    memcpy(out->mask_off, mask_off.data(), (n + 1) * sizeof(int64_t));
    out->n = (int64_t)n; out->pi_n = sizes[0]; out->mask_n = sizes[1]; out->raw_n = sizes[2];
    return "";
}

// m0_rowpack_unpack_host behind check_arrays: planes and a LEGAL mask come from the encoder and the move generator of
// chess_core.h, as encode_positions_kernel makes them.  mask null: not written.
inline void unpack_host(const m0_rowpack_arrays& a, const std::vector<Pos>& positions, const std::vector<int32_t>& raw_slot,
                        float* planes, float* pi, float* z, uint8_t* mask) {
    const size_t n = (size_t)a.n;
    for (size_t i = 0; i < n; ++i) {
        float* srow = planes + i * PLANE_FLOATS;
        float* prow = pi + i * COLS;
        uint8_t* mrow = mask ? mask + i * COLS : nullptr;
        if (a.pos[i].row_kind == M0_ROWPACK_RAW) {
            const size_t r = (size_t)raw_slot[i];
            memcpy(srow, a.raw_planes + r * PLANE_FLOATS, PLANE_FLOATS * sizeof(float));
            memcpy(prow, a.raw_pi + r * COLS, COLS * sizeof(float));
            if (mrow) memcpy(mrow, a.raw_mask + r * COLS, COLS);
            continue;
        }
        const Pos& p = positions[i];
        m0::encode_planes_f32(p, srow);
        memset(prow, 0, COLS * sizeof(float));
        for (int64_t e = a.pi_off[i]; e < a.pi_off[i + 1]; ++e) prow[a.pi_idx[e]] = a.pi_val[e];
        if (!mrow) continue;
        memset(mrow, 0, COLS);
        if (a.pos[i].mask_kind == M0_ROWPACK_MASK_LIST) {
            for (int64_t e = a.mask_off[i]; e < a.mask_off[i + 1]; ++e) mrow[a.mask_idx[e]] = 1;
        } else {
            m0::Move mv[M0_MAX_MOVES];
            const int k = m0::gen_legal(p, mv);
            for (int j = 0; j < k; ++j) {
                const int idx = m0::move_to_index(p, mv[j]);
                if (idx >= 0 && idx < COLS) mrow[idx] = 1;
            }
        }
    }
    memcpy(z, a.z, n * sizeof(float));
}

}  // namespace m0rowpack
