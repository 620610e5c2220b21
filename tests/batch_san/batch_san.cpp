// Stand-alone check of the host side of the resident row store (matrix0_amd/csrc/batch_core.h, batch_host.h, and
// rowpack_host.h's check_arrays) under the sanitizers: built by `make sanitize` with -fsanitize=address,undefined and run on the
// CPU; never loaded into Python.  2 000 seeded rows in batches of 250 -- positions after seeded legal moves from the start, soft
// pi, some rows malformed (RAW), some with every column an entry, some with edited masks (LIST) or a mask byte of 2 (RAW) -- are
// packed, laid out as a segment and read back as batches of seeded ids under every kind, into vectors of exactly the size asked
// for; each output row must equal unpack_host followed by augment_row.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../matrix0_amd/csrc/batch_host.h"

using namespace m0batch;
using m0rowpack::pack_host;
using m0rowpack::unpack_host;

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }

int main() {
    const int BATCH = 250, TOTAL = 2000;
    const char* start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
    long raw_rows = 0, rows_out = 0;
    for (int done = 0; done < TOTAL; done += BATCH) {
        const bool with_mask = (done / BATCH) % 4 != 3;
        std::vector<float> planes((size_t)BATCH * PLANE_FLOATS), pi((size_t)BATCH * COLS, 0.f), z(BATCH);
        std::vector<uint8_t> mask((size_t)BATCH * COLS, 0);
        Pos p;
        m0::parse_fen(start, p);
        for (int i = 0; i < BATCH; ++i) {
            m0::Move mv[M0_MAX_MOVES];
            int k = m0::gen_legal(p, mv);
            if (k == 0 || p.halfmove > 90) { m0::parse_fen(start, p); k = m0::gen_legal(p, mv); }
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
            const int what = (int)(next() % 12);
            if (what == 0) srow[next() % PLANE_FLOATS] = 0.5f;                                   // RAW
            if (what == 1) for (int c = 0; c < COLS; ++c) prow[c] = (float)(1 + next() % 7);     // every column an entry
            if (what == 2) mrow[next() % COLS] ^= 1;                                             // LIST
            if (what == 3) mrow[next() % COLS] = 2;                                              // RAW with a mask
            if (what == 4) { const uint32_t odd[3] = {0x80000000u, 1u, 0x7FC00001u}; memcpy(&prow[next() % COLS], &odd[next() % 3], 4); }
            m0::make_move(p, mv[next() % k]);
        }
        const uint8_t* mk = with_mask ? mask.data() : nullptr;
        int64_t sizes[3];
        m0_rowpack_arrays a = {};
        a.n = BATCH;
        (void)pack_host(planes.data(), pi.data(), z.data(), mk, BATCH, &a, sizes);
        std::vector<m0_rowpack_pos> pos(BATCH);
        std::vector<float> pz(BATCH), pi_val(sizes[0]), raw_planes(sizes[2] * PLANE_FLOATS), raw_pi(sizes[2] * COLS);
        std::vector<int64_t> pi_off(BATCH + 1), mask_off(BATCH + 1);
        std::vector<uint16_t> pi_idx(sizes[0]), mask_idx(sizes[1]);
        std::vector<uint8_t> raw_mask(with_mask ? sizes[2] * COLS : 0);
        a = {BATCH, sizes[0], sizes[1], sizes[2], pos.data(), pz.data(), pi_off.data(), pi_idx.data(), pi_val.data(), mask_off.data(),
             mask_idx.data(), raw_planes.data(), raw_pi.data(), with_mask ? raw_mask.data() : nullptr};
        if (!pack_host(planes.data(), pi.data(), z.data(), mk, BATCH, &a, sizes).empty()) { printf("pack_host refused its own sizes\n"); return 1; }
        raw_rows += sizes[2];
        // the reference: the rows unpacked
        std::vector<Pos> positions;
        std::vector<int32_t> raw_slot;
        if (!check_arrays(&a, positions, raw_slot).empty()) { printf("check_arrays refused packed rows\n"); return 1; }
        std::vector<float> us((size_t)BATCH * PLANE_FLOATS), upi((size_t)BATCH * COLS), uz(BATCH);
        std::vector<uint8_t> um(with_mask ? (size_t)BATCH * COLS : 0);
        unpack_host(a, positions, raw_slot, us.data(), upi.data(), uz.data(), with_mask ? um.data() : nullptr);
        // a segment of the other sort is refused and leaves the block alone
        SegBlock block;
        if (build_segment(&a, !with_mask, block).empty() || !block.bytes.empty()) { printf("a segment of the other sort was taken\n"); return 1; }
        if (!build_segment(&a, with_mask, block).empty()) { printf("build_segment refused packed rows\n"); return 1; }
        const SegView* view = reinterpret_cast<const SegView*>(block.bytes.data());
        for (int B : {1, 7, 64}) {
            std::vector<RowRef> refs(B);
            for (int b = 0; b < B; ++b) refs[b] = RowRef{view, (int32_t)(next() % BATCH), (int32_t)(next() % 3)};
            std::vector<float> os((size_t)B * PLANE_FLOATS), opi((size_t)B * COLS), oz(B);
            std::vector<uint8_t> om(with_mask ? (size_t)B * COLS : 0);
            batch_rows_host(refs.data(), B, os.data(), opi.data(), oz.data(), with_mask ? om.data() : nullptr);
            for (int b = 0; b < B; ++b) {
                const size_t r = (size_t)refs[b].row;
                std::vector<uint32_t> ws(PLANE_FLOATS), wpi(COLS);
                std::vector<uint8_t> wm(with_mask ? COLS : 0);
                m0aug::augment_row(refs[b].kind, (const uint32_t*)&us[r * PLANE_FLOATS], M0_PLANES, (const uint32_t*)&upi[r * COLS],
                                   with_mask ? &um[r * COLS] : nullptr, ws.data(), wpi.data(), with_mask ? wm.data() : nullptr);
                if (memcmp(ws.data(), &os[(size_t)b * PLANE_FLOATS], PLANE_FLOATS * 4) || memcmp(wpi.data(), &opi[(size_t)b * COLS], COLS * 4) ||
                    memcmp(&uz[r], &oz[b], 4) || (with_mask && memcmp(wm.data(), &om[(size_t)b * COLS], COLS))) {
                    printf("row %zu under kind %d differs (batch at %d)\n", r, refs[b].kind, done);
                    return 1;
                }
                ++rows_out;
            }
        }
        // a copy of the block elsewhere, rebased to where it lies, reads the same
        SegBlock copy = block;
        rebase_segment(copy, copy.bytes.data());
        block = SegBlock();
        float s1[PLANE_FLOATS], p1[COLS], z1;
        std::vector<uint8_t> m1(with_mask ? COLS : 0);
        batch_row_host(*reinterpret_cast<const SegView*>(copy.bytes.data()), BATCH - 1, 2, s1, p1, &z1, with_mask ? m1.data() : nullptr);
    }
    printf("ok: %ld batch rows of %d packed rows (%ld raw) equal unpack then augment\n", rows_out, TOTAL, raw_rows);
    return 0;
}
