// extern "C" entry points for reading games back in (include/m0_engine.h): written moves -> patterns on the host, and whole games
// -> training positions on the device (replay_kernels.hip, then the position-wise encoder and the SSL target kernel).
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "chess_core.h"
#include "san_match.h"
#include "tree.h"

using namespace m0;

static_assert(M0_REPLAY_OK == REPLAY_OK && M0_REPLAY_ILLEGAL == REPLAY_ILLEGAL && M0_REPLAY_AMBIGUOUS == REPLAY_AMBIGUOUS &&
              M0_REPLAY_TOO_LONG == REPLAY_TOO_LONG, "status codes of the ABI are the kernel's");
static_assert(M0_REPLAY_END_CHECKMATE == REPLAY_END_CHECKMATE && M0_REPLAY_END_STALEMATE == REPLAY_END_STALEMATE &&
              M0_REPLAY_END_INSUFFICIENT == REPLAY_END_INSUFFICIENT && M0_REPLAY_END_WHITE_TO_MOVE == REPLAY_END_WHITE_TO_MOVE,
              "end flags of the ABI are the kernel's");

namespace {

const char* const START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";

// Consecutive games [g0, g1) issued as one launch; rows = pattern and output rows it holds on the device.
struct ReplayLaunch {
    int g0, g1;
    size_t rows;
};

// copies the first plies[g] rows of every game of a launch from the staging buffer to the caller's flat array
template <typename T>
void scatter_rows(HipStatus& hs, const DevBuf<T>& dev, std::vector<T>& staging, const ReplayLaunch& L, const std::vector<int32_t>& local_off,
                  const int32_t* offsets, const int32_t* plies, size_t width, T* out) {
    if (!out) return;
    staging.resize(L.rows * width);
    if (!dev.download(hs, staging.data(), L.rows * width)) return;
    for (int g = L.g0; g < L.g1; ++g)
        memcpy(out + (size_t)offsets[g] * width, staging.data() + (size_t)local_off[g - L.g0] * width,
               (size_t)plies[g] * width * sizeof(T));
}

}  // namespace

extern "C" {

int m0_san_pattern(const char* token, uint32_t* pattern) {
    if (!token || !pattern) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (!san_parse_token(token, pattern)) { m0_set_error(std::string("not a SAN move: ") + token); return M0_ERR_INVALID; }
    return M0_OK;
}

int m0_move_pattern(int kind, const char* uci, uint32_t raw, uint32_t* pattern) {
    if (!pattern) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    bool ok = false;
    if (kind == M0_MOVE_UCI) ok = san_parse_uci(uci, pattern);
    else if (kind == M0_MOVE_RAW) ok = san_parse_raw(raw, pattern);
    if (!ok) { *pattern = 0; m0_set_error("not a move (kind M0_MOVE_UCI: a UCI string, M0_MOVE_RAW: from | to<<6 | promo<<12)"); return M0_ERR_INVALID; }
    return M0_OK;
}

int m0_replay_games(int hip_device, const char* const* start_fens, const uint32_t* patterns, const int32_t* offsets, int n_games,
                    int max_plies, int max_positions_per_launch, int32_t* plies, int32_t* status, int32_t* end_flags,
                    uint16_t* moves, int32_t* policy_idx, int32_t* nlegal, int8_t* turn, float* planes, uint8_t* mask, float* ssl) {
    if (!patterns || !offsets || n_games <= 0 || max_plies <= 0 || !plies || !status || !end_flags) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    if (offsets[0] != 0) { m0_set_error("offsets[0] must be 0"); return M0_ERR_INVALID; }
    for (int g = 0; g < n_games; ++g)
        if (offsets[g + 1] < offsets[g]) { m0_set_error(std::string("offsets decrease at game ") + std::to_string(g)); return M0_ERR_INVALID; }
    std::vector<Pos> hstart(n_games);
    for (int g = 0; g < n_games; ++g) {
        const char* fen = start_fens && start_fens[g] ? start_fens[g] : START_FEN;
        if (parse_fen(fen, hstart[g]) != 0) { m0_set_error(std::string("bad FEN at index ") + std::to_string(g)); return M0_ERR_INVALID; }
    }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;

    // A game puts min(tokens, max_plies + 1) rows on the device: the tokens it may resolve, and one more for a game past the
    // cap so that the kernel sees it is longer.  A launch takes whole games while they fit; a game larger than the limit goes alone.
    auto rows_of = [&](int g) { return (size_t)std::min<int64_t>((int64_t)offsets[g + 1] - offsets[g], (int64_t)max_plies + 1); };
    const size_t limit = max_positions_per_launch > 0 ? (size_t)max_positions_per_launch : ~(size_t)0;
    std::vector<ReplayLaunch> launches;
    for (int g = 0; g < n_games;) {
        ReplayLaunch L{g, g, 0};
        while (L.g1 < n_games && (L.g1 == L.g0 || L.rows + rows_of(L.g1) <= limit)) { L.rows += rows_of(L.g1); ++L.g1; }
        launches.push_back(L);
        g = L.g1;
    }
    size_t max_rows = 1, max_games = 1;
    for (const ReplayLaunch& L : launches) { max_rows = std::max(max_rows, L.rows); max_games = std::max(max_games, (size_t)(L.g1 - L.g0)); }

    const size_t total = (size_t)offsets[n_games];
    if (moves) memset(moves, 0, total * sizeof(uint16_t));
    if (policy_idx) memset(policy_idx, 0, total * sizeof(int32_t));
    if (nlegal) memset(nlegal, 0, total * sizeof(int32_t));
    if (turn) memset(turn, 0, total);
    if (planes) memset(planes, 0, total * M0_PLANES * 64 * sizeof(float));
    if (mask) memset(mask, 0, total * M0_POLICY_SIZE);
    if (ssl) memset(ssl, 0, total * 17 * 64 * sizeof(float));

    DevBuf<Pos> dstart, dpos;
    DevBuf<uint32_t> dpat;
    DevBuf<int32_t> doff, dplies, dstatus, dend, didx, dnl;
    DevBuf<uint16_t> dmv;
    DevBuf<int8_t> dturn;
    DevBuf<float> dplanes, dssl;
    DevBuf<uint8_t> dmask;
    if (!dstart.alloc(hs, max_games) || !dpos.alloc(hs, max_rows) || !dpat.alloc(hs, max_rows) || !doff.alloc(hs, max_games + 1) ||
        !dplies.alloc(hs, max_games) || !dstatus.alloc(hs, max_games) || !dend.alloc(hs, max_games) || !didx.alloc(hs, max_rows) ||
        !dnl.alloc(hs, max_rows) || !dmv.alloc(hs, max_rows) || !dturn.alloc(hs, max_rows) ||
        (planes && !dplanes.alloc(hs, max_rows * M0_PLANES * 64)) || (mask && !dmask.alloc(hs, max_rows * M0_POLICY_SIZE)) ||
        (ssl && !dssl.alloc(hs, max_rows * 17 * 64))) return m0_hip_error(hs, "hipMalloc failed");

    std::vector<uint32_t> hpat;
    std::vector<int32_t> local_off, s_i32;
    std::vector<uint16_t> s_u16;
    std::vector<int8_t> s_i8;
    std::vector<float> s_f32;
    std::vector<uint8_t> s_u8;
    for (const ReplayLaunch& L : launches) {
        const int ng = L.g1 - L.g0;
        hpat.clear();
        local_off.assign(1, 0);
        for (int g = L.g0; g < L.g1; ++g) {
            hpat.insert(hpat.end(), patterns + offsets[g], patterns + offsets[g] + rows_of(g));
            local_off.push_back((int32_t)hpat.size());
        }
        M0_HIP(hs, hipMemcpy(dstart.p, hstart.data() + L.g0, sizeof(Pos) * ng, hipMemcpyHostToDevice));
        M0_HIP(hs, hipMemcpy(doff.p, local_off.data(), sizeof(int32_t) * (ng + 1), hipMemcpyHostToDevice));
        if (L.rows) M0_HIP(hs, hipMemcpy(dpat.p, hpat.data(), sizeof(uint32_t) * L.rows, hipMemcpyHostToDevice));
        // rows a game does not resolve are encoded too (and not copied back): they must hold a defined position
        if (L.rows) M0_HIP(hs, hipMemset(dpos.p, 0, sizeof(Pos) * L.rows));
        M0_HIP(hs, launch_replay_games(dstart.p, dpat.p, doff.p, ng, max_plies, dpos.p, dmv.p, didx.p, dnl.p, dturn.p, dplies.p,
                                       dstatus.p, dend.p, nullptr));
        if (planes || mask)
            M0_HIP(hs, launch_encode_positions(dpos.p, (int)L.rows, dplanes.p, nullptr, dmask.p, nullptr, nullptr, nullptr, nullptr));
        if (ssl) M0_HIP(hs, launch_ssl_targets(dpos.p, (int)L.rows, dssl.p, nullptr));
        if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "replay kernels failed");
        dplies.download(hs, plies + L.g0, ng);
        dstatus.download(hs, status + L.g0, ng);
        dend.download(hs, end_flags + L.g0, ng);
        if (!hs.ok()) return m0_hip_error(hs, "replay download failed");      // scatter_rows reads plies
        scatter_rows(hs, dmv, s_u16, L, local_off, offsets, plies, 1, moves);
        scatter_rows(hs, didx, s_i32, L, local_off, offsets, plies, 1, policy_idx);
        scatter_rows(hs, dnl, s_i32, L, local_off, offsets, plies, 1, nlegal);
        scatter_rows(hs, dturn, s_i8, L, local_off, offsets, plies, 1, turn);
        scatter_rows(hs, dplanes, s_f32, L, local_off, offsets, plies, (size_t)M0_PLANES * 64, planes);
        scatter_rows(hs, dmask, s_u8, L, local_off, offsets, plies, (size_t)M0_POLICY_SIZE, mask);
        scatter_rows(hs, dssl, s_f32, L, local_off, offsets, plies, (size_t)17 * 64, ssl);
        if (!hs.ok()) return m0_hip_error(hs, "replay download failed");
    }
    return M0_OK;
}

}  // extern "C"
