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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { m0_set_error("no HIP device available (no CPU fallback)"); return M0_ERR_HIP; }
    HipStatus hs;
    if (!M0_HIP(hs, hipSetDevice(hip_device))) return m0_hip_error(hs);
    const bool masked = opts->mask_mode == M0_SCORE_MASK_LEGAL;
    const size_t cells = (size_t)B * COLS;
    DevBuf<float> dl, dv, dp, dz, dr;
    DevBuf<uint8_t> dm;
    if (!dl.alloc(hs, cells) || !dp.alloc(hs, cells) || !dv.alloc(hs, B) || !dz.alloc(hs, B) ||
        !dr.alloc(hs, (size_t)B * M0_SCORE_COLS) || (masked && !dm.alloc(hs, cells))) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, hipMemcpy(dl.p, logits, cells * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dp.p, pi, cells * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dv.p, value, (size_t)B * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dz.p, z, (size_t)B * 4, hipMemcpyHostToDevice));
    if (masked) M0_HIP(hs, hipMemcpy(dm.p, legal_mask, cells, hipMemcpyHostToDevice));
    M0_HIP(hs, launch_score_rows(dl.p, dv.p, dp.p, dz.p, dm.p, B, *opts, dr.p, nullptr));
    M0_HIP(hs, hipDeviceSynchronize());
    dr.download(hs, rows, (size_t)B * M0_SCORE_COLS);
    if (!hs.ok()) return m0_hip_error(hs, "score kernel failed");
    return M0_OK;
}

int m0_score_bench(int hip_device, int B, int iters, float* us_per_launch, double* bytes_per_launch) {
    if (B <= 0 || iters <= 0 || !us_per_launch || !bytes_per_launch) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { m0_set_error("no HIP device available (no CPU fallback)"); return M0_ERR_HIP; }
    HipStatus hs;
    if (!M0_HIP(hs, hipSetDevice(hip_device))) return m0_hip_error(hs);
    // one synthetic row shape repeated with different numbers: about 35 legal moves, soft pi on them, logits of a few units
    const size_t cells = (size_t)B * COLS;
    std::vector<float> hl(cells), hp(cells, 0.f), hv(B), hz(B);
    std::vector<uint8_t> hm(cells, 0);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (size_t i = 0; i < cells; ++i) hl[i] = (float)((double)(next() % 16384) / 2048.0 - 4.0);
    for (int b = 0; b < B; ++b) {
        float sum = 0.f;
        for (int k = 0; k < 35; ++k) {
            const size_t c = (size_t)b * COLS + next() % COLS;
            hm[c] = 1;
            hp[c] = (float)(1 + next() % 100);
        }
        for (int c = 0; c < COLS; ++c) sum += hp[(size_t)b * COLS + c];
        for (int c = 0; c < COLS; ++c) hp[(size_t)b * COLS + c] /= sum;
        hv[b] = (float)((double)(next() % 2001) / 1000.0 - 1.0);
        hz[b] = (float)((int)(next() % 3) - 1);
    }
    DevBuf<float> dl, dv, dp, dz, dr;
    DevBuf<uint8_t> dm;
    if (!dl.alloc(hs, cells) || !dp.alloc(hs, cells) || !dv.alloc(hs, B) || !dz.alloc(hs, B) ||
        !dr.alloc(hs, (size_t)B * M0_SCORE_COLS) || !dm.alloc(hs, cells)) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, hipMemcpy(dl.p, hl.data(), cells * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dp.p, hp.data(), cells * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dv.p, hv.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dz.p, hz.data(), (size_t)B * 4, hipMemcpyHostToDevice));
    M0_HIP(hs, hipMemcpy(dm.p, hm.data(), cells, hipMemcpyHostToDevice));
    const m0_score_opts opts{M0_SCORE_MASK_LEGAL, 0.05f, 1, 1.0f};
    M0_HIP(hs, launch_score_rows(dl.p, dv.p, dp.p, dz.p, dm.p, B, opts, dr.p, nullptr));         // warm-up
    struct Events {                          // destroyed on every way out
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    M0_HIP(hs, hipEventCreate(&ev.e0)); M0_HIP(hs, hipEventCreate(&ev.e1));
    M0_HIP(hs, hipEventRecord(ev.e0, nullptr));
    for (int i = 0; i < iters; ++i) M0_HIP(hs, launch_score_rows(dl.p, dv.p, dp.p, dz.p, dm.p, B, opts, dr.p, nullptr));
    M0_HIP(hs, hipEventRecord(ev.e1, nullptr));
    M0_HIP(hs, hipEventSynchronize(ev.e1));
    float ms = 0.f;
    if (!M0_HIP(hs, hipEventElapsedTime(&ms, ev.e0, ev.e1))) return m0_hip_error(hs, "score bench failed");
    *us_per_launch = ms * 1000.f / (float)iters;
    *bytes_per_launch = (double)B * ((double)COLS * (4 + 4 + 1) + 4 + 4 + 4.0 * M0_SCORE_COLS);
    return M0_OK;
}

}  // extern "C"
