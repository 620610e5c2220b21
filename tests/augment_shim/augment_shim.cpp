// matrix0_amd/csrc/augment_core.h under g++: rows transformed by the core's own maps, as augment_rows_kernel moves them, and the
// core's constexpr tables handed out for tests/test_augment.py to compare with the reference's.
#include <stdint.h>
#include <string.h>
#include "../../matrix0_amd/csrc/augment_core.h"

using namespace m0aug;

extern "C" {

// as m0_augment_rows, on the host; -1 for the arguments it refuses (the outputs then stay untouched)
int as_augment_rows(const uint32_t* planes, int P, const uint32_t* pi, const uint8_t* mask, const uint8_t* kinds, int B,
                    uint32_t* planes_out, uint32_t* pi_out, uint8_t* mask_out) {
    if (!planes || !pi || !kinds || !planes_out || !pi_out || B <= 0 || P <= 0) return -1;
    if ((mask != nullptr) != (mask_out != nullptr)) return -1;
    if (planes == planes_out || pi == pi_out || (mask && mask == mask_out)) return -1;
    for (int b = 0; b < B; ++b)
        if (!valid_kind(kinds[b])) return -1;
    for (int b = 0; b < B; ++b)
        augment_row(kinds[b], planes + (size_t)b * P * SQUARES, P, pi + (size_t)b * COLS, mask ? mask + (size_t)b * COLS : nullptr,
                    planes_out + (size_t)b * P * SQUARES, pi_out + (size_t)b * COLS, mask ? mask_out + (size_t)b * COLS : nullptr);
    return 0;
}

// PERM[kind] as 73 ints and the square map as 64 ints; -1 for no kind
int as_tables(int kind, int32_t* perm, int32_t* squares) {
    if (!valid_kind(kind)) return -1;
    for (int c = 0; c < CHANNELS; ++c) perm[c] = PERM[kind].at[c];
    for (int sq = 0; sq < SQUARES; ++sq) squares[sq] = sq ^ SQUARE_XOR[kind];
    return 0;
}

int as_source_column(int kind, int col) { return valid_kind(kind) && col >= 0 && col < COLS ? source_column(kind, col) : -1; }

}  // extern "C"

#ifdef AUGMENT_SHIM_MAIN
// Stand-alone run for the sanitizers: seeded rows, every kind with and without a mask, twice (a kind is an involution).
#include <stdio.h>
#include <vector>
int main() {
    const int B = 7, P = 19;
    std::vector<uint32_t> s((size_t)B * P * SQUARES), p((size_t)B * COLS), s1(s.size()), p1(p.size()), s2(s.size()), p2(p.size());
    std::vector<uint8_t> m((size_t)B * COLS), m1(m.size()), m2(m.size()), k(B);
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (auto& v : s) v = (uint32_t)next();
    for (auto& v : p) v = (uint32_t)next();
    for (auto& v : m) v = (uint8_t)(next() & 1);
    for (int b = 0; b < B; ++b) k[b] = (uint8_t)(b % KINDS);
    uint64_t sum = 0;
    for (int masked = 0; masked < 2; ++masked) {
        uint8_t* mm = masked ? m.data() : nullptr;
        if (as_augment_rows(s.data(), P, p.data(), mm, k.data(), B, s1.data(), p1.data(), masked ? m1.data() : nullptr)) return 1;
        if (as_augment_rows(s1.data(), P, p1.data(), masked ? m1.data() : nullptr, k.data(), B, s2.data(), p2.data(), masked ? m2.data() : nullptr)) return 1;
        if (s2 != s || p2 != p || (masked && m2 != m)) return 1;
        for (uint32_t v : p1) sum += v;
    }
    k[3] = 3;
    if (as_augment_rows(s.data(), P, p.data(), nullptr, k.data(), B, s1.data(), p1.data(), nullptr) != -1) return 1;
    printf("augment_shim ok: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
