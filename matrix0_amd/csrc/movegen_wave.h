// Wave-wide move generation and input encoding, one position per wavefront: used by select_kernel (tree_select.hip) and by
// the position-wise test-hook kernel (position_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "tree.h"

using namespace m0;

// Exclusive prefix sum over the wave's lanes (lane 0 first) of three packed 10-bit counters; `total` = wave sum.
__device__ __forceinline__ uint32_t wave_excl_scan3(uint32_t v, int lane, uint32_t& total) {
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off);
        if (lane >= off) incl += u;
    }
    total = __shfl(incl, 63);
    return incl - v;
}

// Pseudo-legal moves in python-chess generation order (chess_core.h gen_moves<false>), one SQUARE per lane:
// lane L works square 63 - L, so ascending lanes are python-chess's scan_reversed order.  Per category (piece moves by
// from-square; pawn captures by from-square; single pushes, double pushes by to-square; en passant by from-square)
// every lane counts its moves, three packed prefix sums give its output offsets, and it writes its own moves; the
// check-evasion king moves (first) and castling (after the pieces) are uniform work.  gen_moves<false> on every lane was
// 33 k cycles per leaf (the pseudo-legal list built 64 times over, sequentially).
static __device__ int gen_pseudo_wave(const Pos& p, Move* out, int lane) {
    const int us = p.turn, them = us ^ 1;
    const uint64_t own = occ_of(p, us), theirs = occ_of(p, them), o = own | theirs;
    const int ksq = king_sq(p, us);
    const bool chk = ksq >= 0 && attacked(p, ksq, them);
    const int s = 63 - lane;
    const uint64_t sb = bit(s);
    const uint64_t pawns = p.bb[PAWN] & own;
    // --- check evasion: the king's moves come first and the king leaves the piece scan
    int n0 = 0;
    if (chk) {
        uint64_t t = king_att(ksq) & ~own;
        n0 = popc(t);
        if (lane == 0) { int j = 0; while (t) { const int to = msb(t); t &= ~bit(to); out[j++] = mk_move(ksq, to, 0); } }
    }
    // --- category A: non-pawn pieces
    uint64_t tA = 0;
    if ((own & ~p.bb[PAWN] & sb) && !(chk && s == ksq)) tA = piece_targets(p, s, piece_type_at(p, s));
    const uint32_t cA = (uint32_t)popc(tA);
    // --- castling (uniform), after the pieces
    Move cz[2];
    int ncz = 0;
    if (!chk && ksq >= 0) {
        const int cr = clean_cr(p);
        const int base = us == WHITE ? 0 : 56;
        if (ksq == base + 4) {
            const int kbit = us == WHITE ? CR_WK : CR_BK, qbit = us == WHITE ? CR_WQ : CR_BQ;
            if ((cr & kbit) && !(o & (bit(base + 5) | bit(base + 6))) && !attacked(p, base + 5, them) &&
                !attacked(p, base + 6, them))
                cz[ncz++] = mk_move(ksq, base + 6, 0);
            if ((cr & qbit) && !(o & (bit(base + 1) | bit(base + 2) | bit(base + 3))) && !attacked(p, base + 3, them) &&
                !attacked(p, base + 2, them))
                cz[ncz++] = mk_move(ksq, base + 2, 0);
        }
    }
    // --- category C: pawn captures (from-square s), promotions expand to 4
    const uint64_t tC = (pawns & sb) ? (pawn_att(s, us) & theirs) : 0;
    const uint64_t promo_rank = RANK_1 | RANK_8;
    const uint32_t cC = (uint32_t)(popc(tC & ~promo_rank) + 4 * popc(tC & promo_rank));
    // --- category D / E: single and double pushes (to-square s)
    const uint64_t single = (us == WHITE ? pawns << 8 : pawns >> 8) & ~o;
    const uint64_t dbl = (us == WHITE ? single << 8 : single >> 8) & ~o & (us == WHITE ? (RANK_1 << 24) : (RANK_1 << 32));
    const uint32_t cD = (single & sb) ? ((sb & promo_rank) ? 4u : 1u) : 0u;
    const uint32_t cE = (dbl & sb) ? 1u : 0u;
    // --- category F: en passant (from-square s)
    uint64_t epc = 0;
    if (p.ep >= 0 && !(o & bit(p.ep))) epc = pawns & pawn_att(p.ep, them) & (us == WHITE ? (RANK_1 << 32) : (RANK_1 << 24));
    const uint32_t cF = (epc & sb) ? 1u : 0u;
    // --- offsets
    uint32_t tot1, tot2;
    const uint32_t ex1 = wave_excl_scan3(cA | (cC << 10) | (cD << 20), lane, tot1);
    const uint32_t ex2 = wave_excl_scan3(cE | (cF << 10), lane, tot2);
    const int nA = tot1 & 1023, nC = (tot1 >> 10) & 1023, nD = (tot1 >> 20) & 1023, nE = tot2 & 1023, nF = (tot2 >> 10) & 1023;
    const int baseA = n0, baseZ = baseA + nA, baseC = baseZ + ncz, baseD = baseC + nC, baseE = baseD + nD, baseF = baseE + nE;
    {
        int j = baseA + (int)(ex1 & 1023);
        uint64_t t = tA;
        while (t) { const int to = msb(t); t &= ~bit(to); out[j++] = mk_move(s, to, 0); }
    }
    if (lane == 0) for (int i = 0; i < ncz; ++i) out[baseZ + i] = cz[i];
    {
        int j = baseC + (int)((ex1 >> 10) & 1023);
        uint64_t t = tC;
        while (t) {
            const int to = msb(t); t &= ~bit(to);
            if (bit(to) & promo_rank) { out[j++] = mk_move(s, to, 4); out[j++] = mk_move(s, to, 3); out[j++] = mk_move(s, to, 2); out[j++] = mk_move(s, to, 1); }
            else out[j++] = mk_move(s, to, 0);
        }
    }
    if (cD) {
        int j = baseD + (int)((ex1 >> 20) & 1023);
        const int from = s + (us == WHITE ? -8 : 8);
        if (cD == 4) { out[j++] = mk_move(from, s, 4); out[j++] = mk_move(from, s, 3); out[j++] = mk_move(from, s, 2); out[j++] = mk_move(from, s, 1); }
        else out[j] = mk_move(from, s, 0);
    }
    if (cE) out[baseE + (int)(ex2 & 1023)] = mk_move(s + (us == WHITE ? -16 : 16), s, 0);
    if (cF) out[baseF + (int)((ex2 >> 10) & 1023)] = mk_move(s, p.ep, 0);
    return baseF + nF;
}

// Legal moves in generation order: the pseudo-legal list (one square per lane, above), then the legality test
// (make + king-attack) spread one move per lane and an order-preserving ballot compaction.  Same list as gen_legal()
// (tests/test_chess_core_host.py pins gen_legal; tests/test_encoding_gpu.py compares this one on 10 000 positions).
static __device__ int gen_legal_wave(const Pos& p, Move* out_lds, Move* tmp_lds, int lane) {
    const int np = gen_pseudo_wave(p, tmp_lds, lane);
    __syncthreads();
    int base = 0;
    for (int k0 = 0; k0 < np; k0 += 64) {
        const int i = k0 + lane;
        const Move m = i < np ? tmp_lds[i] : (Move)0;
        const bool ok = i < np && legal_after(p, m);
        const unsigned long long mask = __ballot(ok);
        if (ok) out_lds[base + __popcll(mask & ((1ull << lane) - 1ull))] = m;
        base += __popcll(mask);
    }
    __syncthreads();
    return base;
}

// lane = tensor square n (row-major, row 0 = rank 8): M0_NHWC_C fp16 channels (M0_PLANES used)
static __device__ void encode_nhwc(const Pos& p, _Float16* dst /*[64][M0_NHWC_C]*/, int lane) {
    static_assert(M0_PLANES == 12 + 7 && M0_PLANES <= M0_NHWC_C && M0_NHWC_C == 32, "12 piece planes + plane_consts, stored as four 16-byte pieces");
    const int s = (7 - (lane >> 3)) * 8 + (lane & 7);
    float c7[7];
    plane_consts(p, c7);
    const int pl = piece_plane(p, s);
    __attribute__((aligned(16))) _Float16 h[M0_NHWC_C];
#pragma unroll
    for (int i = 0; i < M0_NHWC_C; ++i) h[i] = (_Float16)0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) h[i] = (_Float16)(pl == i ? 1.f : 0.f);
#pragma unroll
    for (int i = 0; i < 7; ++i) h[12 + i] = (_Float16)c7[i];
    uint4* o = reinterpret_cast<uint4*>(dst + lane * M0_NHWC_C);
    const uint4* hv = reinterpret_cast<const uint4*>(h);
    o[0] = hv[0]; o[1] = hv[1]; o[2] = hv[2]; o[3] = hv[3];
}
// batch row `row` of the network input
__device__ __forceinline__ _Float16* nhwc_row(_Float16* x0, int row) { return x0 + (size_t)row * 64 * M0_NHWC_C; }
