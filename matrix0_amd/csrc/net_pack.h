// The weight layouts of the network's kernels, host-only: plain arrays and dimensions in, a std::vector in the consuming kernel's
// order out.  No HIP and no Net here, so every index below can be exercised on a CPU (tests/host_shim/pack_shim.cpp,
// tests/test_net_pack.py); net_pack.hip fetches, checks, calls these and uploads.  The function templates take the element
// types as parameters: the product instantiates float -> _Float16, the tests int32 -> int32 with each element holding its own
// index, which turns a packed buffer into a map from position to source element.
//
// Every layout is the LDS image of its kernel, so that staging is a linear copy.  Rows are output
// channels, k is the input channel; a row is cut into 16-byte chunks (8 fp16) whose index is XOR-swizzled by the row so that the
// kernel's fragment reads are conflict-free.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace net_pack {

// ---- the two 16-byte-chunk swizzles: position of element k within its row
// 128-byte rows (64 k): chunk index ^ (row >> 1) & 7 -- conv_big_kernel, the qkv pieces of attn_block_kernel
inline int swizzle_row64(int row, int k) { return (((k >> 3) ^ ((row >> 1) & 7)) << 3) | (k & 7); }
// 64-byte rows (32 k): chunk index ^ (4 - (row >> 2)) & 3 -- conv_zs_kernel, the proj pieces of attn_block_kernel
inline int swizzle_row32(int row, int k) { return (((k >> 3) ^ ((4 - ((row >> 2) & 3)) & 3)) << 3) | (k & 7); }

// ---- the two row maps of the GEMM packer
// qkv output rows (type, head, dim 16) -> the same with the padded head count (a padded trunk carries all-zero heads)
inline int qkv_row_padded(int row, int heads, int heads_pad) {
    const int d = row % 16, th = row / 16;
    return ((th / heads) * heads_pad + th % heads) * 16 + d;
}
// input index of an FC behind a flatten: the reference's NCHW c * 64 + sq -> NHWC sq * ch + c
inline int flatten_k(int k, int ch) { return (k % 64) * ch + k / 64; }

// ---- GEMM weights [N_real][Cin_real][taps] -> the layout of the consuming kernel, zero-padded to Cin_pad x N_pad
enum GemmLayout {
    GEMM_SMALL,     // conv_gemm_kernel: [tap][Cin/32][N][32]
    GEMM_BIG_1X1,   // conv_big_kernel:  [tap][Cin/64][N][64], swizzle_row64
    GEMM_BIG_3X3,   // conv_zs_kernel:   [chunk*9+tap][N/320][k half][320][32] (chunk = 64 k), swizzle_row32
};
struct GemmShape {
    int taps, Cin_real, Cin_pad, N_real, N_pad;
    int flatten_ch = 0;                     // > 0: k goes through flatten_k(k, flatten_ch)
    int qkv_heads = 0, qkv_heads_pad = 0;   // qkv_heads > 0: rows go through qkv_row_padded
};

inline size_t gemm_index(GemmLayout layout, const GemmShape& s, int n, int k, int tap) {
    if (layout == GEMM_BIG_3X3) {
        const int chunk = k >> 6, half = (k >> 5) & 1, nl = n % 320;
        return ((((size_t)(chunk * 9 + tap) * (s.N_pad / 320) + n / 320) * 2 + half) * 320 + nl) * 32 + swizzle_row32(nl, k & 31);
    }
    if (layout == GEMM_BIG_1X1)
        return (((size_t)tap * (s.Cin_pad / 64) + (k >> 6)) * s.N_pad + n) * 64 + swizzle_row64(n, k & 63);
    return (((size_t)tap * (s.Cin_pad / 32) + (k >> 5)) * s.N_pad + n) * 32 + (k & 31);
}

template <class Out, class In>
std::vector<Out> gemm_weights(const In* w, GemmLayout layout, const GemmShape& s) {
    std::vector<Out> p((size_t)s.taps * s.Cin_pad * s.N_pad, (Out)0);
    for (int nr = 0; nr < s.N_real; ++nr) {
        const int n = s.qkv_heads > 0 ? qkv_row_padded(nr, s.qkv_heads, s.qkv_heads_pad) : nr;
        for (int k = 0; k < s.Cin_real; ++k) {
            const int kk = s.flatten_ch > 0 ? flatten_k(k, s.flatten_ch) : k;
            for (int t = 0; t < s.taps; ++t)
                p[gemm_index(layout, s, n, kk, t)] = (Out)w[((size_t)nr * s.Cin_real + k) * s.taps + t];
        }
    }
    return p;
}

// ---- attn_block_kernel operands (attn_block.hip), 320-wide trunk: 20 heads of 16 in 10 groups of two
// The block's qkv [3 C][C] and proj [C][C] weights (C = 16 heads <= 320) as one stream of 12 KB pieces in LDS image order.  Per
// group g of two heads: five pieces [96 cols = (q, k, v) x 2 heads x 16][64 k] (swizzle_row64) and two pieces [160 output
// channels][32 k = 2 heads x 16] (swizzle_row32, half a piece, padded to 12 KB); three zero pieces end the stream (the kernel's
// prefetch runs past the last group).  Padded heads and channels are zero.
constexpr int kAttnGroups = 10, kAttnPiecesPerGroup = 7, kAttnPadPieces = 3;
constexpr size_t kAttnPiece = 6144;         // elements: 12 KB of fp16
constexpr size_t kAttnPackElems = (size_t)(kAttnGroups * kAttnPiecesPerGroup + kAttnPadPieces) * kAttnPiece;

template <class Out, class In>
std::vector<Out> attn_block_weights(const In* wq, const In* wp, int heads) {
    const int C = heads * 16;
    std::vector<Out> buf(kAttnPackElems, (Out)0);
    for (int g = 0; g < kAttnGroups; ++g) {
        for (int pc = 0; pc < 5; ++pc) {
            Out* piece = &buf[(size_t)(g * kAttnPiecesPerGroup + pc) * kAttnPiece];
            for (int col = 0; col < 96; ++col) {
                const int type = col >> 5, h = 2 * g + ((col >> 4) & 1), d = col & 15;
                for (int k = 0; k < 64; ++k)
                    if (h < heads && 64 * pc + k < C)
                        piece[col * 64 + swizzle_row64(col, k)] = (Out)wq[(size_t)((type * heads + h) * 16 + d) * C + 64 * pc + k];
            }
        }
        for (int hh = 0; hh < 2; ++hh) {
            Out* piece = &buf[(size_t)(g * kAttnPiecesPerGroup + 5 + hh) * kAttnPiece];
            for (int cl = 0; cl < 160; ++cl)
                for (int k = 0; k < 32; ++k) {
                    const int oc = 160 * hh + cl, h = 2 * g + (k >> 4);
                    if (oc < C && h < heads) piece[cl * 32 + swizzle_row32(cl, k)] = (Out)wp[(size_t)oc * C + h * 16 + (k & 15)];
                }
        }
    }
    return buf;
}

// The relative-position bias in MFMA accumulator order, [20 heads][2 query halves][64 lanes][32]: element e of lane holds
// query 32 qt + (lane & 31), key 32 (e >> 4) + 8 (r >> 2) + 4 (lane >> 5) + (r & 3) with r = e & 15.  `rel_bias_log2` is
// rel_bias * log2(e) [heads][64][64] (the kernels exponentiate with exp2), or null: no bias, all zero.
template <class Out, class In>
std::vector<Out> attn_block_bias(const In* rel_bias_log2, int heads) {
    std::vector<Out> bb((size_t)20 * 2 * 64 * 32, (Out)0);
    if (!rel_bias_log2) return bb;
    for (int h = 0; h < heads; ++h)
        for (int qt = 0; qt < 2; ++qt)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 32; ++e) {
                    const int r = e & 15;
                    const int q = qt * 32 + (lane & 31), key = (e >> 4) * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                    bb[(((size_t)h * 2 + qt) * 64 + lane) * 32 + e] = (Out)rel_bias_log2[((size_t)h * 64 + q) * 64 + key];
                }
    return bb;
}

// ---- small tables
// v[n] -> [n_pad], zeros behind: a bias or norm vector of a padded width, the split attention path's rel_bias with padded heads
template <class Out, class In>
std::vector<Out> zero_padded(const In* v, size_t n, size_t n_pad) {
    std::vector<Out> p(n_pad, (Out)0);
    for (size_t i = 0; i < n; ++i) p[i] = (Out)v[i];
    return p;
}

// src [rows][cols] -> [out_rows][out_cols] with out[c][r] = src[r][c], zeros elsewhere: the positional encoding [C][64] ->
// [64][P], squeeze-excite W1 [hd][C] -> [P][hd] and W2 [C][hd] -> [hd][P]
template <class Out, class In>
std::vector<Out> transposed(const In* src, int rows, int cols, int out_rows, int out_cols) {
    std::vector<Out> t((size_t)out_rows * out_cols, (Out)0);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) t[(size_t)c * out_cols + r] = (Out)src[(size_t)r * cols + c];
    return t;
}

// attention visibility mask, resnet.py:104-130: bit j of word i = square i sees square j (same row, column or diagonal, a
// knight's move, or adjacent)
inline std::vector<uint64_t> attn_mask() {
    std::vector<uint64_t> m(64, 0);
    for (int i = 0; i < 64; ++i)
        for (int j = 0; j < 64; ++j) {
            const int dr = i / 8 - j / 8, dc = i % 8 - j % 8, adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
            const bool vis = adr == 0 || adc == 0 || adr == adc || (adr == 2 && adc == 1) || (adr == 1 && adc == 2) ||
                             (adr <= 1 && adc <= 1);
            if (vis) m[i] |= 1ull << j;
        }
    return m;
}

// ---- squeeze-excite FCs as fp16 MFMA fragment pieces for conv_zs_kernel's tail (conv_zs_tail.h), 320-wide trunk
// B-fragment pieces of v_mfma_f32_16x16x32_f16, 512 elements each: lane (c15 = lane & 15, q = lane >> 4) holds column c15,
// k = 8 q .. 8 q + 7 of its tile.  From the transposed matrices w1t [320][hd] and w2t [hd][320]:
//   W1 piece (nt, ks) at piece nt * 10 + ks:                w1t[channel 32 ks + 8 q + e][hidden 16 nt + c15]    nt < ceil(hd/16), ks < 10
//   W2 piece (nt, ks) at piece 10 ceil(hd/16) + nt * KS2 + ks:  w2t[hidden 32 ks + 8 q + e][channel 16 nt + c15]    nt < 20, ks < KS2 = ceil(hd/32)
// hidden units >= hd are zero.
template <class Out, class In>
std::vector<Out> se_fragments(const In* w1t, const In* w2t, int hd) {
    const int P = 320, NT1 = (hd + 15) / 16, KS2 = (hd + 31) / 32;
    std::vector<Out> wf((size_t)(10 * NT1 + 20 * KS2) * 512, (Out)0);
    for (int nt = 0; nt < NT1; ++nt)
        for (int ks = 0; ks < 10; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int c = 32 * ks + 8 * (l >> 4) + e, j = 16 * nt + (l & 15);
                    if (j < hd) wf[((size_t)(nt * 10 + ks) * 64 + l) * 8 + e] = (Out)w1t[(size_t)c * hd + j];
                }
    for (int nt = 0; nt < 20; ++nt)
        for (int ks = 0; ks < KS2; ++ks)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int j = 32 * ks + 8 * (l >> 4) + e, c = 16 * nt + (l & 15);
                    if (j < hd) wf[((size_t)(10 * NT1 + nt * KS2 + ks) * 64 + l) * 8 + e] = (Out)w2t[(size_t)j * P + c];
                }
    return wf;
}

// ---- joint policy / value head: policy_head.0 (Na = 64 columns) and value_head.0 (Nb = 128) read the same trunk and run as one
// GEMM with N = Na + Nb, columns [policy | value]: the two small-tile images [Cin/32][N][32] interleaved chunk by chunk
template <class T>
std::vector<T> joint_columns(const std::vector<T>& a, int Na, const std::vector<T>& b, int Nb, int Cin) {
    std::vector<T> c;
    c.reserve(a.size() + b.size());
    for (int ch = 0; ch < Cin / 32; ++ch) {
        c.insert(c.end(), a.begin() + (size_t)ch * Na * 32, a.begin() + (size_t)(ch + 1) * Na * 32);
        c.insert(c.end(), b.begin() + (size_t)ch * Nb * 32, b.begin() + (size_t)(ch + 1) * Nb * 32);
    }
    return c;
}
template <class T>
std::vector<T> joined(const std::vector<T>& a, const std::vector<T>& b) {   // their GroupNorm parameters, the same way
    std::vector<T> c(a);
    c.insert(c.end(), b.begin(), b.end());
    return c;
}

}  // namespace net_pack
