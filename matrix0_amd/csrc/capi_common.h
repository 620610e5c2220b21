// Shared between the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "hip_check.h"

class Net;
Net* m0_net_impl(m0_net* n);
hipStream_t m0_net_stream(m0_net* n);
int m0_net_device(m0_net* n);
// The handle's mutex: every forward on a network (m0_net_infer from any thread, an engine stepping on it) runs under it --
// the workspace and the stream belong to the handle.
void m0_net_lock(m0_net* n);
void m0_net_unlock(m0_net* n);
// A non-blocking stream; when the environment variable env_name holds w0,w1,...,w7 (hex words, bit b = CU b in the driver's
// numbering) the stream runs on those CUs only (hipExtStreamCreateWithCUMask).  Measurement switch; read at every call.
hipError_t create_stream_cu_mask_env(const char* env_name, hipStream_t* stream);
// The check m0_augment_rows and m0_net_score_aug share on kinds u8 [B] (include/m0_augment.h): nullptr when every row holds a kind,
// otherwise why not (capi_augment.hip).
const char* m0_bad_kinds(const uint8_t* kinds, int B);
// Packed rows (include/m0_rowpack.h) checked, uploaded and unpacked on `st` into device arrays planes f32 [n][19][64],
// pi f32 [n][4672] and mask u8 [n][4672] (null: no mask wanted); returns with the stream drained.  M0_ERR_INVALID with nothing
// launched for arrays that fail the checks (capi_rowpack.hip).
int m0_rowpack_unpack_to_device(HipStatus& hs, const m0_rowpack_arrays* in, float* planes_dev, float* pi_dev, uint8_t* mask_dev,
                                hipStream_t st);
// The seeded rows that m0_rowpack_bench and m0_rowstore_bench run on: planes f32 [N][19][64], pi f32 [N][4672], mask u8 [N][4672];
// every row packs as a position with a LEGAL mask (capi_rowpack.hip).
void m0_rowpack_bench_rows(size_t N, std::vector<float>& planes, std::vector<float>& pi, std::vector<uint8_t>& mask);

// What every stateless device call does first: M0_OK with hip_device current, or M0_ERR_HIP and the error string set.
inline int m0_select_device(HipStatus& hs, int hip_device, const char* hint = "no CPU fallback") {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        m0_set_error(std::string("no HIP device available (") + hint + ")");
        return M0_ERR_HIP;
    }
    return M0_HIP(hs, hipSetDevice(hip_device)) ? M0_OK : m0_hip_error(hs);
}

// device memory for the length of one call
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(HipStatus& st, size_t count) { return M0_HIP(st, hipMalloc((void**)&p, count * sizeof(T))); }
    // alloc, then the host array copied in on `stream`; an empty array still gets one element, so that p is never null
    bool upload(HipStatus& st, const T* host, size_t count, hipStream_t stream = nullptr) {
        if (!alloc(st, count ? count : 1)) return false;
        return count == 0 || M0_HIP(st, hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, stream));
    }
    bool download(HipStatus& st, T* host, size_t count) const { return M0_HIP(st, hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost)); }
};

// The seeded xorshift64 behind the synthetic inputs of the *_bench calls: one sequence, so those inputs are reproducible.
struct BenchRng {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
};

// Milliseconds per iteration of `enqueue()` issued `iters` times on `stream`, between two events that are destroyed on every way
// out.  enqueue returns whether to go on (an M0_HIP line does): after a false nothing more is issued and the answer is 0.  The
// caller tests `st` afterwards.
template <typename F>
float m0_time_iterations(HipStatus& st, hipStream_t stream, int iters, F&& enqueue) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    M0_HIP(st, hipEventCreate(&ev.e0)); M0_HIP(st, hipEventCreate(&ev.e1));
    if (!M0_HIP(st, hipEventRecord(ev.e0, stream))) return 0.f;
    for (int i = 0; i < iters; ++i)
        if (!enqueue()) return 0.f;
    M0_HIP(st, hipEventRecord(ev.e1, stream));
    M0_HIP(st, hipEventSynchronize(ev.e1));
    float ms = 0.f;
    M0_HIP(st, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms / (float)iters;
}
