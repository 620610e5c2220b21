// Shared between the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
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

// device memory for the length of one call
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(HipStatus& st, size_t count) { return M0_HIP(st, hipMalloc((void**)&p, count * sizeof(T))); }
    bool download(HipStatus& st, T* host, size_t count) const { return M0_HIP(st, hipMemcpy(host, p, count * sizeof(T), hipMemcpyDeviceToHost)); }
};
