// extern "C" entry points of the training-loss score that need no network (include/m0_score.h): the kernel on host arrays, and
// its timing on resident inputs.  m0_net_score, which runs it behind a forward, lives with the network handle in capi_net.hip.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "score_core.h"
#include "score_kernels.h"

using namespace m0score;

extern "C" {

int m0_score_rows(int hip_device, const float* logits, const float* value, const float* pi, const float* z,
                  const uint8_t* legal_mask, int B, const m0_score_opts* opts, float* rows) {
    if (!logits || !value || !pi || !z || !rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    if (const char* why = bad_opts(opts, legal_mask != nullptr)) { m0_set_error(why); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const bool masked = opts->mask_mode == M0_SCORE_MASK_LEGAL;
    const size_t cells = (size_t)B * COLS;
    DevBuf<float> dl, dv, dp, dz, dr;
    DevBuf<uint8_t> dm;
    if (!dl.upload(hs, logits, cells) || !dp.upload(hs, pi, cells) || !dv.upload(hs, value, B) || !dz.upload(hs, z, B) ||
        !dr.alloc(hs, (size_t)B * M0_SCORE_COLS) || (masked && !dm.upload(hs, legal_mask, cells))) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_score_rows(dl.p, dv.p, dp.p, dz.p, dm.p, B, *opts, dr.p, nullptr));
    M0_HIP(hs, hipDeviceSynchronize());
    dr.download(hs, rows, (size_t)B * M0_SCORE_COLS);
    if (!hs.ok()) return m0_hip_error(hs, "score kernel failed");
    return M0_OK;
}

int m0_score_bench(int hip_device, int B, int iters, float* us_per_launch, double* bytes_per_launch) {
    if (B <= 0 || iters <= 0 || !us_per_launch || !bytes_per_launch) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    // one synthetic row shape repeated with different numbers: about 35 legal moves, soft pi on them, logits of a few units
    const size_t cells = (size_t)B * COLS;
    std::vector<float> hl(cells), hp(cells, 0.f), hv(B), hz(B);
    std::vector<uint8_t> hm(cells, 0);
    BenchRng rng;
    for (size_t i = 0; i < cells; ++i) hl[i] = (float)((double)(rng.next() % 16384) / 2048.0 - 4.0);
    for (int b = 0; b < B; ++b) {
        float sum = 0.f;
        for (int k = 0; k < 35; ++k) {
            const size_t c = (size_t)b * COLS + rng.next() % COLS;
            hm[c] = 1;
            hp[c] = (float)(1 + rng.next() % 100);
        }
        for (int c = 0; c < COLS; ++c) sum += hp[(size_t)b * COLS + c];
        for (int c = 0; c < COLS; ++c) hp[(size_t)b * COLS + c] /= sum;
        hv[b] = (float)((double)(rng.next() % 2001) / 1000.0 - 1.0);
        hz[b] = (float)((int)(rng.next() % 3) - 1);
    }
    DevBuf<float> dl, dv, dp, dz, dr;
    DevBuf<uint8_t> dm;
    if (!dl.upload(hs, hl.data(), cells) || !dp.upload(hs, hp.data(), cells) || !dv.upload(hs, hv.data(), B) || !dz.upload(hs, hz.data(), B) ||
        !dr.alloc(hs, (size_t)B * M0_SCORE_COLS) || !dm.upload(hs, hm.data(), cells)) return m0_hip_error(hs, "hipMalloc failed");
    const m0_score_opts opts{M0_SCORE_MASK_LEGAL, 0.05f, 1, 1.0f};
    auto launch = [&]() { return M0_HIP(hs, launch_score_rows(dl.p, dv.p, dp.p, dz.p, dm.p, B, opts, dr.p, nullptr)); };
    launch();                                                                           // warm-up
    const float ms = m0_time_iterations(hs, nullptr, iters, launch);
    if (!hs.ok()) return m0_hip_error(hs, "score bench failed");
    *us_per_launch = ms * 1000.f;
    *bytes_per_launch = (double)B * ((double)COLS * (4 + 4 + 1) + 4 + 4 + 4.0 * M0_SCORE_COLS);
    return M0_OK;
}

}  // extern "C"
