// Host side of the resident row store (include/m0_batch.h), plain C++ without HIP: a segment laid out as one block of memory
// behind rowpack_host.h's check_arrays, and a batch filled on the CPU with straight loops over batch_core.h.  Used by
// capi_batch.hip (the host store, m0_rowstore_batch_host, and the block a device segment is uploaded from) and, under g++, by
// tests/batch_san.
#pragma once
#include <string.h>
#include <string>
#include <type_traits>
#include <vector>
#include "batch_core.h"
#include "rowpack_host.h"

namespace m0batch {

using m0rowpack::check_arrays;
using m0rowpack::has_masks;

// A segment as one block: a SegView first, then its arrays, each on a 16-byte boundary.  The pointers of the SegView point into
// the block where it lies; rebase_segment turns them for the address of a copy (a device segment).
struct SegBlock {
    std::vector<uint8_t> bytes;
    int64_t rows = 0, raw_rows = 0;
};

// Empty when the arrays are fine and of the store's sort, with `block` built; otherwise why not, with `block` untouched.
inline std::string build_segment(const m0_rowpack_arrays* a, bool with_mask, SegBlock& block) {
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    const std::string why = check_arrays(a, positions, raw_slot);
    if (!why.empty()) return why;
    if (has_masks(*a) != with_mask) return with_mask ? "rows without masks for a store with masks" : "rows with masks for a store without masks";
    const size_t n = (size_t)a->n, npi = (size_t)a->pi_n, nmk = (size_t)a->mask_n, raw = (size_t)a->raw_n;
    std::vector<uint8_t> meta(n);
    for (size_t i = 0; i < n; ++i) meta[i] = make_meta(a->pos[i].row_kind, a->pos[i].mask_kind);
    struct Part { const void* src; size_t bytes; size_t at; };
    Part parts[12] = {{positions.data(), n * sizeof(Pos), 0},       {meta.data(), n, 0},
                      {a->z, n * sizeof(float), 0},                 {a->pi_off, (n + 1) * sizeof(int64_t), 0},
                      {a->pi_idx, npi * sizeof(uint16_t), 0},       {a->pi_val, npi * sizeof(float), 0},
                      {a->mask_off, (n + 1) * sizeof(int64_t), 0},  {a->mask_idx, nmk * sizeof(uint16_t), 0},
                      {raw_slot.data(), n * sizeof(int32_t), 0},    {a->raw_planes, raw * PLANE_FLOATS * sizeof(float), 0},
                      {a->raw_pi, raw * COLS * sizeof(float), 0},   {a->raw_mask, with_mask ? raw * COLS : 0, 0}};
    size_t total = (sizeof(SegView) + 15) / 16 * 16;
    for (Part& p : parts) { p.at = total; total += (p.bytes + 15) / 16 * 16; }
    std::vector<uint8_t> bytes(total, 0);
    for (const Part& p : parts)
        if (p.bytes) memcpy(bytes.data() + p.at, p.src, p.bytes);
    const uint8_t* at = bytes.data();
    SegView v;
    v.n = a->n;
    v.pos = (const Pos*)(at + parts[0].at);             v.meta = at + parts[1].at;
    v.z = (const float*)(at + parts[2].at);             v.pi_off = (const int64_t*)(at + parts[3].at);
    v.pi_idx = (const uint16_t*)(at + parts[4].at);     v.pi_val = (const float*)(at + parts[5].at);
    v.mask_off = (const int64_t*)(at + parts[6].at);    v.mask_idx = (const uint16_t*)(at + parts[7].at);
    v.raw_slot = (const int32_t*)(at + parts[8].at);    v.raw_planes = (const float*)(at + parts[9].at);
    v.raw_pi = (const float*)(at + parts[10].at);       v.raw_mask = with_mask ? at + parts[11].at : nullptr;
    memcpy(bytes.data(), &v, sizeof(SegView));
    block.bytes.swap(bytes);
    block.rows = a->n;
    block.raw_rows = a->raw_n;
    return "";
}

// The block's SegView for a copy of the block at `base`
inline void rebase_segment(SegBlock& block, const uint8_t* base) {
    SegView v;
    memcpy(&v, block.bytes.data(), sizeof(SegView));
    const uint8_t* old = reinterpret_cast<const uint8_t*>(v.pos) - (sizeof(SegView) + 15) / 16 * 16;      // pos is the first array
    auto move = [&](auto*& p) {
        if (p) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + (reinterpret_cast<const uint8_t*>(p) - old));
    };
    move(v.pos); move(v.meta); move(v.z); move(v.pi_off); move(v.pi_idx); move(v.pi_val); move(v.mask_off); move(v.mask_idx);
    move(v.raw_slot); move(v.raw_planes); move(v.raw_pi); move(v.raw_mask);
    memcpy(block.bytes.data(), &v, sizeof(SegView));
}

// The maps of one output row from the pieces of its 64 output cells (batch_core.h): status 0; an unusable row: zeros, status 1
inline void ssl_row_host(const int* cells, bool usable, bool stm_white, float* ssl, int32_t* ssl_status) {
    m0ssl::Board4 board;
    for (int t = 0; t < 64; ++t) board.set(t, cells[t]);
    for (int t = 0; t < 64; ++t) {
        if (usable) target_cell(board, t, stm_white, ssl);
        else zero_cell(ssl, t);
    }
    *ssl_status = usable ? 0 : 1;
}

// One output row on the CPU: what batch_rows_kernel writes for the same reference.  mask null: not written; ssl and ssl_status
// both null: not written.
inline void batch_row_host(const SegView& g, int row, int kind, float* planes, float* pi, float* z, uint8_t* mask, float* ssl = nullptr,
                           int32_t* ssl_status = nullptr) {
    *z = g.z[row];
    const uint8_t meta = g.meta[row];
    int cells[64];
    if (meta_raw(meta)) {
        const size_t slot = (size_t)g.raw_slot[row];
        const float* stored = g.raw_planes + slot * PLANE_FLOATS;
        m0aug::augment_row(kind, (const uint32_t*)stored, M0_PLANES, (const uint32_t*)(g.raw_pi + slot * COLS),
                           mask ? g.raw_mask + slot * COLS : nullptr, (uint32_t*)planes, (uint32_t*)pi, mask);
        if (ssl) {
            bool unusable = false;
            for (int t = 0; t < 64; ++t) {
                bool bad;
                cells[t] = raw_cell(stored, kind, t, &bad);
                unusable = unusable || bad;
            }
            ssl_row_host(cells, !unusable, raw_white(stored, kind), ssl, ssl_status);
        }
        return;
    }
    const Pos& p = g.pos[row];
    float c7[7];
    m0::plane_consts(p, c7);
    for (int t = 0; t < 64; ++t) {
        const int pl = cells[t] = m0::piece_plane(p, cell_square(kind, t));
        for (int k = 0; k < M0_PLANES; ++k) planes[k * 64 + t] = plane_cell(pl, c7, k);
    }
    if (ssl) ssl_row_host(cells, true, p.turn == m0::WHITE, ssl, ssl_status);
    memset(pi, 0, COLS * sizeof(float));
    for (int64_t e = g.pi_off[row]; e < g.pi_off[row + 1]; ++e) pi[dest_column(kind, g.pi_idx[e])] = g.pi_val[e];
    if (!mask) return;
    memset(mask, 0, COLS);
    if (meta_mask_kind(meta) == M0_ROWPACK_MASK_LIST) {
        for (int64_t e = g.mask_off[row]; e < g.mask_off[row + 1]; ++e) mask[dest_column(kind, g.mask_idx[e])] = 1;
    } else {
        m0::Move mv[M0_MAX_MOVES];
        const int k = m0::gen_legal(p, mv);
        for (int j = 0; j < k; ++j) {
            const int idx = m0::move_to_index(p, mv[j]);
            if (idx >= 0 && idx < COLS) mask[dest_column(kind, idx)] = 1;
        }
    }
}

// refs [B] -> the dense outputs; ssl [B][17][64] and ssl_status [B], or both null
inline void batch_rows_host(const RowRef* refs, int B, float* planes, float* pi, float* z, uint8_t* mask, float* ssl = nullptr,
                            int32_t* ssl_status = nullptr) {
    for (int b = 0; b < B; ++b)
        batch_row_host(*refs[b].seg, refs[b].row, refs[b].kind, planes + (size_t)b * PLANE_FLOATS, pi + (size_t)b * COLS, z + b,
                       mask ? mask + (size_t)b * COLS : nullptr, ssl ? ssl + (size_t)b * SSL_FLOATS : nullptr,
                       ssl ? ssl_status + b : nullptr);
}

}  // namespace m0batch
