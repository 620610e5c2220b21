// extern "C" device hooks that take FEN strings and need no engine (include/m0_engine.h): encoding.py on the device and the
// SSL target maps; and the way back, stored planes to positions.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "chess_core.h"
#include "fen_text.h"
#include "tree.h"

using namespace m0;

namespace {

// selects the device, parses the n FENs and puts the positions on it
int upload_fens(HipStatus& hs, int hip_device, const char* const* fens, int n, DevBuf<Pos>& dp) {
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    std::vector<Pos> hp(n);
    for (int i = 0; i < n; ++i)
        if (!fens[i] || parse_fen(fens[i], hp[i]) != 0) { m0_set_error(std::string("bad FEN at index ") + std::to_string(i)); return M0_ERR_INVALID; }
    dp.alloc(hs, n);
    return M0_HIP(hs, hipMemcpy(dp.p, hp.data(), sizeof(Pos) * n, hipMemcpyHostToDevice)) ? M0_OK : m0_hip_error(hs, "position upload failed");
}

}  // namespace

extern "C" {

int m0_encode_fens(int hip_device, const char* const* fens, int n, float* planes, uint8_t* mask, int32_t* nlegal,
                   uint16_t* moves, int32_t* idx) {
    if (!fens || n <= 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    DevBuf<Pos> dp;
    HipStatus hs;
    const int rc = upload_fens(hs, hip_device, fens, n, dp);
    if (rc != M0_OK) return rc;
    const size_t N = (size_t)n;
    DevBuf<float> dpl; DevBuf<uint8_t> dm; DevBuf<int32_t> dn; DevBuf<uint16_t> dmv; DevBuf<int32_t> di;
    if ((planes && !dpl.alloc(hs, N * 19 * 64)) || (mask && !dm.alloc(hs, N * 4672)) || (nlegal && !dn.alloc(hs, N)) ||
        (moves && !dmv.alloc(hs, N * M0_MAX_MOVES)) || (idx && !di.alloc(hs, N * M0_MAX_MOVES))) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_encode_positions(dp.p, n, dpl.p, nullptr, dm.p, dn.p, dmv.p, di.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "encode kernel failed");
    if (planes) dpl.download(hs, planes, N * 19 * 64);
    if (mask) dm.download(hs, mask, N * 4672);
    if (nlegal) dn.download(hs, nlegal, N);
    if (moves) dmv.download(hs, moves, N * M0_MAX_MOVES);
    if (idx) di.download(hs, idx, N * M0_MAX_MOVES);
    return hs.ok() ? M0_OK : m0_hip_error(hs, "download failed");
}

int m0_encode_fens_nhwc(int hip_device, const char* const* fens, int n, uint16_t* out) {
    if (!fens || n <= 0 || !out) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    DevBuf<Pos> dp;
    HipStatus hs;
    const int rc = upload_fens(hs, hip_device, fens, n, dp);
    if (rc != M0_OK) return rc;
    DevBuf<_Float16> dx;
    if (!dx.alloc(hs, (size_t)n * 64 * 32)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_encode_positions(dp.p, n, nullptr, dx.p, nullptr, nullptr, nullptr, nullptr, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "encode kernel failed");
    return dx.download(hs, (_Float16*)out, (size_t)n * 64 * 32) ? M0_OK : m0_hip_error(hs, "download failed");
}

int m0_ssl_targets_fens(int hip_device, const char* const* fens, int n, float* out) {
    if (!fens || n <= 0 || !out) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    DevBuf<Pos> dp;
    HipStatus hs;
    const int rc = upload_fens(hs, hip_device, fens, n, dp);
    if (rc != M0_OK) return rc;
    DevBuf<float> dout;
    if (!dout.alloc(hs, (size_t)n * 17 * 64)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_ssl_targets(dp.p, n, dout.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "ssl kernel failed");
    return dout.download(hs, out, (size_t)n * 17 * 64) ? M0_OK : m0_hip_error(hs, "download failed");
}

int m0_decode_planes(int hip_device, const float* planes, const uint8_t* mask, int n, int32_t* status, int32_t* flags,
                     int32_t* nlegal, char* fens, int fen_stride) {
    if (!planes || n <= 0 || (fens && fen_stride < 96)) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t N = (size_t)n;
    DevBuf<float> dpl; DevBuf<uint8_t> dm; DevBuf<Pos> dp; DevBuf<int32_t> dst, dfl, dnl;
    if (!dpl.upload(hs, planes, N * M0_PLANES * 64) || (mask && !dm.upload(hs, mask, N * M0_POLICY_SIZE)) || !dp.alloc(hs, N) || !dst.alloc(hs, N) ||
        !dfl.alloc(hs, N) || !dnl.alloc(hs, N)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_decode_planes(dpl.p, dm.p, n, dp.p, dst.p, dfl.p, dnl.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "decode kernel failed");
    std::vector<int32_t> hst(N);
    std::vector<Pos> hp(fens ? N : 0);
    dst.download(hs, hst.data(), N);
    if (flags) dfl.download(hs, flags, N);
    if (nlegal) dnl.download(hs, nlegal, N);
    if (fens) dp.download(hs, hp.data(), N);
    if (!hs.ok()) return m0_hip_error(hs, "download failed");
    if (status) memcpy(status, hst.data(), N * sizeof(int32_t));
    if (fens) {
        memset(fens, 0, N * (size_t)fen_stride);
        for (size_t i = 0; i < N; ++i) {
            if (hst[i] != M0_DECODE_OK && hst[i] != M0_DECODE_MASK_MISMATCH) continue;
            const std::string f = fen_of(hp[i]);
            memcpy(fens + i * (size_t)fen_stride, f.c_str(), f.size() < (size_t)fen_stride ? f.size() : (size_t)fen_stride - 1);
        }
    }
    return M0_OK;
}

int m0_move_to_index_fen(int hip_device, const char* fen, const char* uci, int32_t* out) {
    if (!fen || !uci || !out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    const Move want = parse_uci(uci);
    if (want == 0xFFFF) { m0_set_error(std::string("Illegal move: ") + uci); return M0_ERR_INVALID; }
    std::vector<uint16_t> mv(M0_MAX_MOVES);
    std::vector<int32_t> id(M0_MAX_MOVES);
    int32_t n = 0;
    const char* fens[1] = {fen};
    int rc = m0_encode_fens(hip_device, fens, 1, nullptr, nullptr, &n, mv.data(), id.data());
    if (rc != M0_OK) return rc;
    for (int i = 0; i < n; ++i)
        if (mv[i] == want) { *out = id[i]; return M0_OK; }
    m0_set_error(std::string("Illegal move: ") + uci);     // encoding.py:120-121 raises ValueError
    return M0_ERR_INVALID;
}

int m0_decode_move_fen(int hip_device, const char* fen, int action_idx, char* uci_out) {
    if (!fen || !uci_out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (action_idx < 0 || action_idx >= M0_POLICY_SIZE) { m0_set_error("action_idx out of range"); return M0_ERR_INVALID; }
    Pos p;
    if (parse_fen(fen, p) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    std::vector<uint16_t> mv(M0_MAX_MOVES);
    int32_t n = 0;
    const char* fens[1] = {fen};
    int rc = m0_encode_fens(hip_device, fens, 1, nullptr, nullptr, &n, mv.data(), nullptr);   // legal moves from the device
    if (rc != M0_OK) return rc;
    static const int RAY[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    static const int KN[8][2] = {{-2, -1}, {-2, 1}, {-1, -2}, {-1, 2}, {1, -2}, {1, 2}, {2, -1}, {2, 1}};
    const int from = action_idx / 73, off = action_idx % 73;
    const int fr = from >> 3, ff = from & 7;
    int dr, df, steps = 1, promo = 0;
    bool under = false;
    if (off < 56) { dr = RAY[off / 7][0]; df = RAY[off / 7][1]; steps = off % 7 + 1; }
    else if (off < 64) { dr = KN[off - 56][0]; df = KN[off - 56][1]; }
    else {
        const int u = off - 64, d = u % 3;
        static const int DW[3][2] = {{1, 0}, {1, -1}, {1, 1}}, DB[3][2] = {{-1, 0}, {-1, 1}, {-1, -1}};
        dr = p.turn == WHITE ? DW[d][0] : DB[d][0]; df = p.turn == WHITE ? DW[d][1] : DB[d][1];
        promo = u / 3 + 1; under = true;
    }
    const int tr = fr + dr * steps, tf = ff + df * steps;
    int to = -1;
    Move want = 0xFFFF;
    if (tr >= 0 && tr < 8 && tf >= 0 && tf < 8) {
        to = tr * 8 + tf;
        if (!under && piece_type_at(p, from) == PAWN && (p.occ[0] | p.occ[1]) & bit(from) && (tr == 0 || tr == 7)) promo = 4;
        want = mk_move(from, to, promo);
    }
    Move pick = 0xFFFF;
    for (int i = 0; i < n && pick == 0xFFFF; ++i) if (mv[i] == want) pick = mv[i];
    if (to >= 0) for (int i = 0; i < n && pick == 0xFFFF; ++i) if (mv_from(mv[i]) == from && mv_to(mv[i]) == to) pick = mv[i];
    if (to < 0) for (int i = 0; i < n && pick == 0xFFFF; ++i) if (mv_from(mv[i]) == from && mv_to(mv[i]) == 0) pick = mv[i];   // null move target a1 (python Move.null().to_square == 0)
    for (int i = 0; i < n && pick == 0xFFFF; ++i) if (mv_from(mv[i]) == from) pick = mv[i];
    if (pick == 0xFFFF) { strcpy(uci_out, "0000"); return M0_OK; }
    const int f = mv_from(pick), t = mv_to(pick), pr = mv_promo(pick);
    uci_out[0] = (char)('a' + (f & 7)); uci_out[1] = (char)('1' + (f >> 3));
    uci_out[2] = (char)('a' + (t & 7)); uci_out[3] = (char)('1' + (t >> 3));
    uci_out[4] = pr ? " nbrq"[pr] : '\0'; uci_out[5] = '\0';
    return M0_OK;
}

}  // extern "C"
