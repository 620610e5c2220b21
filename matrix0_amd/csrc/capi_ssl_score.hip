// extern "C" entry points of the SSL score that need no network (include/m0_ssl_score.h): the kernel on host arrays, the
// targets of stored planes, and the kernel's timing on resident inputs.  m0_net_score_ssl, which runs the kernel behind a
// forward, lives with the network handle in capi_net.hip.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "ssl_score_core.h"
#include "ssl_score_kernels.h"
#include "tree.h"

using namespace m0sslscore;

namespace {

constexpr size_t PLANES_ROW = (size_t)M0_PLANES * 64, TARGETS_ROW = (size_t)m0ssl::TARGET_CH * 64;

}  // namespace

extern "C" {

int m0_ssl_score_rows(int hip_device, const float* heads, int tasks, const float* planes, const float* targets, int B,
                      float* rows) {
    if (!heads || !planes || !rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    if (bad_tasks(tasks)) { m0_set_error("tasks must be a non-empty set of M0_SSL_* bits"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t N = (size_t)B, head_row = (size_t)channels(tasks) * 64;
    DevBuf<float> dh, dp, dt, dr;
    if (!dh.upload(hs, heads, N * head_row) || !dp.upload(hs, planes, N * PLANES_ROW) || (targets && !dt.upload(hs, targets, N * TARGETS_ROW)) ||
        !dr.alloc(hs, N * M0_SSL_SCORE_COLS)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_ssl_score(dh.p, tasks, dp.p, dt.p, B, dr.p, nullptr));
    M0_HIP(hs, hipDeviceSynchronize());
    if (!hs.ok()) return m0_hip_error(hs, "ssl score kernel failed");
    return dr.download(hs, rows, N * M0_SSL_SCORE_COLS) ? M0_OK : m0_hip_error(hs, "download failed");
}

int m0_ssl_targets_planes(int hip_device, const float* planes, int n, float* out, int32_t* status) {
    if (!planes || !out || !status || n <= 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t N = (size_t)n;
    DevBuf<float> dp, dout;
    DevBuf<int32_t> dst;
    if (!dp.upload(hs, planes, N * PLANES_ROW) || !dout.alloc(hs, N * TARGETS_ROW) || !dst.alloc(hs, N)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_ssl_targets_planes(dp.p, n, dout.p, dst.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "ssl kernel failed");
    std::vector<float> got(N * TARGETS_ROW);
    std::vector<int32_t> st(N);
    if (!dout.download(hs, got.data(), got.size()) || !dst.download(hs, st.data(), N)) return m0_hip_error(hs, "download failed");
    for (size_t i = 0; i < N; ++i) {                   // the kernel wrote nothing for an unusable row: the caller's stays
        status[i] = st[i];
        if (st[i] == 0) memcpy(out + i * TARGETS_ROW, got.data() + i * TARGETS_ROW, TARGETS_ROW * 4);
    }
    return M0_OK;
}

int m0_ssl_score_bench(int hip_device, int B, int tasks, int from_planes, int iters, float* us_per_launch, double* bytes_per_launch) {
    if (B <= 0 || iters <= 0 || bad_tasks(tasks) || !us_per_launch || !bytes_per_launch) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    // synthetic rows: about 24 pieces on random squares, either side to move, head outputs of a few units; stored targets are
    // the planes' own
    const size_t N = (size_t)B, head_row = (size_t)channels(tasks) * 64;
    std::vector<float> hh(N * head_row), hp(N * PLANES_ROW, 0.f), ht(from_planes ? 0 : N * TARGETS_ROW);
    BenchRng rng;
    for (auto& x : hh) x = (float)((double)(rng.next() % 16384) / 2048.0 - 4.0);
    for (size_t b = 0; b < N; ++b) {
        float* prow = hp.data() + b * PLANES_ROW;
        m0ssl::Board4 board;
        for (int sq = 0; sq < 64; ++sq) {
            if (rng.next() % 8 >= 3) continue;
            const int piece = (int)(rng.next() % 12);
            prow[piece * 64 + sq] = 1.f;
            board.set(sq, piece);
        }
        const bool white = rng.next() % 2 == 0;
        for (int sq = 0; sq < 64; ++sq) prow[12 * 64 + sq] = white ? 1.f : 0.f;
        if (!from_planes)
            for (int sq = 0; sq < 64; ++sq) m0ssl::store_square(m0ssl::square_targets(board, sq, white), ht.data() + b * TARGETS_ROW, sq);
    }
    DevBuf<float> dh, dp, dt, dr;
    if (!dh.upload(hs, hh.data(), hh.size()) || !dp.upload(hs, hp.data(), hp.size()) || (!from_planes && !dt.upload(hs, ht.data(), ht.size())) ||
        !dr.alloc(hs, N * M0_SSL_SCORE_COLS)) return m0_hip_error(hs, "hipMalloc failed");
    auto launch = [&]() { return M0_HIP(hs, launch_ssl_score(dh.p, tasks, dp.p, dt.p, B, dr.p, nullptr)); };
    launch();                                                                           // warm-up
    const float ms = m0_time_iterations(hs, nullptr, iters, launch);
    if (!hs.ok()) return m0_hip_error(hs, "ssl score bench failed");
    *us_per_launch = ms * 1000.f;
    *bytes_per_launch = (double)B * (4.0 * (double)head_row + 256.0 * m0ssl::PLANES_READ +
                                     (from_planes ? 0.0 : 4.0 * (double)TARGETS_ROW) + 4.0 * M0_SSL_SCORE_COLS);
    return M0_OK;
}

}  // extern "C"
