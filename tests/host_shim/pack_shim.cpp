// Host build of csrc/net_pack.h, the weight layouts, instantiated int32 -> int32: the caller fills every input tensor with its
// elements' own flat index + 1, so a packed buffer is a map from position to source element and 0 means padding
// (tests/test_net_pack.py).  Every pk_* function writes its result to `out` when it fits in `cap` elements and returns its length.
// With -DPACK_SHIM_MAIN the file is a stand-alone program (the one to build with -fsanitize=address,undefined) that runs the
// test's list of cases over exactly-sized buffers and checks that every source element lands exactly once.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../matrix0_amd/csrc/net_pack.h"
namespace pk = net_pack;

namespace {
int64_t give(const std::vector<int32_t>& v, int32_t* out, int64_t cap) {
    if ((int64_t)v.size() <= cap) memcpy(out, v.data(), v.size() * sizeof(int32_t));
    return (int64_t)v.size();
}
}  // namespace

extern "C" {

// layout: 0 small tile, 1 1x1 big tile, 2 3x3 big tile (pk::GemmLayout)
int64_t pk_gemm(const int32_t* w, int layout, int taps, int Cin_real, int Cin_pad, int N_real, int N_pad, int flatten_ch,
                int qkv_heads, int qkv_heads_pad, int32_t* out, int64_t cap) {
    const pk::GemmShape s = {taps, Cin_real, Cin_pad, N_real, N_pad, flatten_ch, qkv_heads, qkv_heads_pad};
    return give(pk::gemm_weights<int32_t>(w, (pk::GemmLayout)layout, s), out, cap);
}
int64_t pk_attn_weights(const int32_t* wq, const int32_t* wp, int heads, int32_t* out, int64_t cap) {
    return give(pk::attn_block_weights<int32_t>(wq, wp, heads), out, cap);
}
int64_t pk_attn_bias(const int32_t* rel_bias, int heads, int32_t* out, int64_t cap) {
    return give(pk::attn_block_bias<int32_t>(rel_bias, heads), out, cap);
}
int64_t pk_zero_padded(const int32_t* v, int64_t n, int64_t n_pad, int32_t* out, int64_t cap) {
    return give(pk::zero_padded<int32_t>(v, (size_t)n, (size_t)n_pad), out, cap);
}
int64_t pk_transposed(const int32_t* src, int rows, int cols, int out_rows, int out_cols, int32_t* out, int64_t cap) {
    return give(pk::transposed<int32_t>(src, rows, cols, out_rows, out_cols), out, cap);
}
// w1 [hd][C], w2 [C][hd] -> the fragment pieces, through the two transposes as the intake does (trunk 320 wide in memory)
int64_t pk_se_fragments(const int32_t* w1, const int32_t* w2, int hd, int C, int32_t* out, int64_t cap) {
    const std::vector<int32_t> w1t = pk::transposed<int32_t>(w1, hd, C, 320, hd), w2t = pk::transposed<int32_t>(w2, C, hd, hd, 320);
    return give(pk::se_fragments<int32_t>(w1t.data(), w2t.data(), hd), out, cap);
}
void pk_attn_mask(uint64_t* out) {
    const std::vector<uint64_t> m = pk::attn_mask();
    memcpy(out, m.data(), 64 * sizeof(uint64_t));
}
int64_t pk_joint_columns(const int32_t* a, int Na, const int32_t* b, int Nb, int Cin, int32_t* out, int64_t cap) {
    const std::vector<int32_t> va(a, a + (size_t)Cin * Na), vb(b, b + (size_t)Cin * Nb);
    return give(pk::joint_columns(va, Na, vb, Nb, Cin), out, cap);
}

}  // extern "C"

#ifdef PACK_SHIM_MAIN
namespace {
int failures = 0;
std::vector<int32_t> iota(size_t n, int32_t first = 1) {
    std::vector<int32_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = first + (int32_t)i;
    return v;
}
// every value 1 .. sources exactly once, everything else 0, and the length as expected
void check(const char* what, const std::vector<int32_t>& packed, size_t sources, size_t length) {
    std::vector<char> seen(sources + 1, 0);
    size_t bad = packed.size() != length;
    for (int32_t v : packed) {
        if (v < 0 || (size_t)v > sources || (v && seen[v]++)) ++bad;
    }
    for (size_t i = 1; i <= sources; ++i) bad += !seen[i];
    printf("%-50s %9zu elements %s\n", what, packed.size(), bad ? "WRONG" : "ok");
    failures += bad != 0;
}
void gemm_case(const char* what, pk::GemmLayout layout, const pk::GemmShape& s) {
    const size_t n = (size_t)s.N_real * s.Cin_real * s.taps;
    check(what, pk::gemm_weights<int32_t>(iota(n).data(), layout, s), n, (size_t)s.taps * s.Cin_pad * s.N_pad);
}
}  // namespace

int main() {
    gemm_case("small tile 3x3 19->32 x 64 (stem)", pk::GEMM_SMALL, {9, 19, 32, 64, 64});
    gemm_case("small tile 1x1 96 x 1->32", pk::GEMM_SMALL, {1, 96, 96, 1, 32});
    gemm_case("big tile 1x1 320 x 320", pk::GEMM_BIG_1X1, {1, 320, 320, 320, 320});
    gemm_case("big tile 1x1 288->320 x 864->960, heads 18->20", pk::GEMM_BIG_1X1, {1, 288, 320, 864, 960, 0, 18, 20});
    gemm_case("big tile 3x3 320 x 320", pk::GEMM_BIG_3X3, {9, 320, 320, 320, 320});
    gemm_case("big tile 3x3 288->320 x 288->320", pk::GEMM_BIG_3X3, {9, 288, 320, 288, 320});
    gemm_case("flatten 64 ch, small tile 4096 x 40->64", pk::GEMM_SMALL, {1, 4096, 4096, 40, 64, 64});
    gemm_case("flatten 128 ch, big tile 8192 x 640", pk::GEMM_BIG_1X1, {1, 8192, 8192, 640, 640, 128});
    for (int heads : {20, 18}) {
        const int C = heads * 16;
        const size_t nq = (size_t)3 * C * C, np = (size_t)C * C, nb = (size_t)heads * 4096;
        check("attention block weight pieces", pk::attn_block_weights<int32_t>(iota(nq).data(), iota(np, 1 + (int32_t)nq).data(), heads),
              nq + np, pk::kAttnPackElems);
        check("attention block bias table", pk::attn_block_bias<int32_t>(iota(nb).data(), heads), nb, (size_t)20 * 2 * 64 * 32);
        check("split-path rel_bias", pk::zero_padded<int32_t>(iota(nb).data(), nb, (size_t)20 * 4096), nb, (size_t)20 * 4096);
        for (int hd : {8, 20, 80, 96}) {
            const size_t n = (size_t)hd * C;
            std::vector<int32_t> wf((size_t)(10 * ((hd + 15) / 16) + 20 * ((hd + 31) / 32)) * 512);
            const int64_t len = pk_se_fragments(iota(n).data(), iota(n, 1 + (int32_t)n).data(), hd, C, wf.data(), (int64_t)wf.size());
            check("squeeze-excite fragment pieces", wf, 2 * n, (size_t)len);
        }
        check("positional encoding", pk::transposed<int32_t>(iota((size_t)C * 64).data(), C, 64, 64, 320), (size_t)C * 64, 64 * 320);
    }
    {
        const int Cin = 320;
        const std::vector<int32_t> a = iota((size_t)Cin * 64), b = iota((size_t)Cin * 128, 1 + Cin * 64);
        std::vector<int32_t> c((size_t)Cin * 192);
        const int64_t len = pk_joint_columns(a.data(), 64, b.data(), 128, Cin, c.data(), (int64_t)c.size());
        check("joint head columns", c, c.size(), (size_t)len);
    }
    uint64_t m[64];
    pk_attn_mask(m);
    int bits = 0;
    for (uint64_t w : m) bits += __builtin_popcountll(w);
    printf("visibility mask: %d visible pairs\n", bits);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
