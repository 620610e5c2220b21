// extern "C" entry points of the augmentations that need no network (include/m0_augment.h): the kernel on host arrays, and its
// timing on resident inputs.  m0_net_score_aug, which runs it before a forward, lives with the network handle in capi_net.hip.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "augment_core.h"
#include "augment_kernels.h"

using namespace m0aug;

// the argument checks m0_augment_rows and m0_net_score_aug share on the kinds; nullptr when they are fine
const char* m0_bad_kinds(const uint8_t* kinds, int B) {
    if (!kinds) return "null argument";
    for (int b = 0; b < B; ++b)
        if (!valid_kind(kinds[b])) return "augmentation kind out of range";
    return nullptr;
}

extern "C" {

int m0_augment_rows(int hip_device, const float* planes, int P, const float* pi, const uint8_t* legal_mask, const uint8_t* kinds, int B,
                    float* planes_out, float* pi_out, uint8_t* mask_out) {
    if (!planes || !pi || !kinds || !planes_out || !pi_out) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    if (P <= 0) { m0_set_error("planes must be positive"); return M0_ERR_INVALID; }
    if ((legal_mask != nullptr) != (mask_out != nullptr)) { m0_set_error("legal_mask and mask_out come together or not at all"); return M0_ERR_INVALID; }
    if (planes == planes_out || pi == pi_out || (legal_mask && legal_mask == mask_out)) {
        m0_set_error("the transform is out of place: an output is its own input");
        return M0_ERR_INVALID;
    }
    if (const char* why = m0_bad_kinds(kinds, B)) { m0_set_error(why); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t cells = (size_t)B * COLS, pcells = (size_t)B * P * SQUARES;
    DevBuf<float> ds, dp, dso, dpo;
    DevBuf<uint8_t> dm, dmo, dk;
    if (!ds.upload(hs, planes, pcells) || !dso.alloc(hs, pcells) || !dp.upload(hs, pi, cells) || !dpo.alloc(hs, cells) || !dk.upload(hs, kinds, B) ||
        (legal_mask && (!dm.upload(hs, legal_mask, cells) || !dmo.alloc(hs, cells)))) return m0_hip_error(hs, "hipMalloc failed");
    M0_HIP(hs, launch_augment_rows(ds.p, dp.p, dm.p, dk.p, M0_AUG_NONE, B, P, dso.p, dpo.p, dmo.p, nullptr));
    M0_HIP(hs, hipDeviceSynchronize());
    if (!hs.ok()) return m0_hip_error(hs, "augment kernel failed");          // the outputs stay untouched
    dso.download(hs, planes_out, pcells);
    dpo.download(hs, pi_out, cells);
    if (legal_mask) dmo.download(hs, mask_out, cells);
    if (!hs.ok()) return m0_hip_error(hs, "augment kernel failed");
    return M0_OK;
}

int m0_augment_bench(int hip_device, int B, int iters, float* us_per_launch, double* bytes_per_launch) {
    if (B <= 0 || iters <= 0 || !us_per_launch || !bytes_per_launch) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    // what is moved does not depend on the values: seeded floats and bytes, the three kinds in turn
    const int P = M0_PLANES;
    const size_t cells = (size_t)B * COLS, pcells = (size_t)B * P * SQUARES;
    std::vector<float> hp(cells), hplanes(pcells);
    std::vector<uint8_t> hm(cells), hk(B);
    BenchRng rng;
    for (auto& x : hp) x = (float)((double)(rng.next() % 16384) / 16384.0);
    for (auto& x : hplanes) x = (float)(rng.next() % 2);
    for (auto& x : hm) x = (uint8_t)(rng.next() % 128 == 0);
    for (int b = 0; b < B; ++b) hk[b] = (uint8_t)(b % KINDS);
    DevBuf<float> ds, dp, dso, dpo;
    DevBuf<uint8_t> dm, dmo, dk;
    if (!ds.upload(hs, hplanes.data(), pcells) || !dso.alloc(hs, pcells) || !dp.upload(hs, hp.data(), cells) || !dpo.alloc(hs, cells) ||
        !dk.upload(hs, hk.data(), B) || !dm.upload(hs, hm.data(), cells) || !dmo.alloc(hs, cells)) return m0_hip_error(hs, "hipMalloc failed");
    auto launch = [&]() { return M0_HIP(hs, launch_augment_rows(ds.p, dp.p, dm.p, dk.p, M0_AUG_NONE, B, P, dso.p, dpo.p, dmo.p, nullptr)); };
    launch();                                                                           // warm-up
    const float ms = m0_time_iterations(hs, nullptr, iters, launch);
    if (!hs.ok()) return m0_hip_error(hs, "augment bench failed");
    *us_per_launch = ms * 1000.f;
    *bytes_per_launch = (double)B * (2.0 * ((double)COLS * (4 + 1) + (double)P * SQUARES * 4) + 1.0);
    return M0_OK;
}

}  // extern "C"
