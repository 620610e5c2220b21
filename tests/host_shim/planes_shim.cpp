// TEST INFRASTRUCTURE: host (g++) build of matrix0_amd/csrc/planes_decode.h, the planes -> position decode that
// decode_planes_kernel runs one wave per row, so that it can be checked on the CPU against the golden encodings and serve as
// the expectation of the kernel's GPU test.  Not part of libm0engine.so.
#include <string.h>
#include "../../matrix0_amd/csrc/planes_decode.h"
#include "../../matrix0_amd/csrc/fen_text.h"
using namespace m0;

extern "C" {

// n rows: planes f32 [n][19][64], mask u8 [n][4672] or null.  Outputs nullable but status / flags / nlegal: fens [n][stride]
// (empty unless the row left a position), moves u16 [n][256] and idx i32 [n][256] of the decoded position's legal moves in
// order, planes_out f32 [n][19][64] = the decoded position encoded again.
int pd_decode(const float* planes, const uint8_t* mask, int n, int32_t* status, int32_t* flags, int32_t* nlegal, char* fens,
              int stride, uint16_t* moves, int32_t* idx, float* planes_out) {
    for (int i = 0; i < n; ++i) {
        Pos p;
        int fl = 0, nl = 0;
        const int st = decode_planes_host(planes + (size_t)i * 19 * 64, mask ? mask + (size_t)i * M0_POLICY_SIZE : nullptr, p, fl, nl);
        status[i] = st; flags[i] = fl; nlegal[i] = nl;
        const bool valid = st == M0_DECODE_OK || st == M0_DECODE_MASK_MISMATCH;
        if (fens) {
            memset(fens + (size_t)i * stride, 0, stride);
            if (valid) {
                const std::string f = fen_of(p);
                memcpy(fens + (size_t)i * stride, f.c_str(), (int)f.size() < stride ? f.size() : (size_t)stride - 1);
            }
        }
        if (!valid) continue;
        Move mv[M0_MAX_MOVES];
        const int k = gen_legal(p, mv);
        for (int j = 0; j < k; ++j) {
            if (moves) moves[(size_t)i * M0_MAX_MOVES + j] = mv[j];
            if (idx) idx[(size_t)i * M0_MAX_MOVES + j] = move_to_index(p, mv[j]);
        }
        if (planes_out) encode_planes_f32(p, planes_out + (size_t)i * 19 * 64);
    }
    return 0;
}

}
