// ssl_score_kernel (ssl_score_kernels.hip): the SSL losses of stored rows on the device, behind a forward or on its own.
#pragma once
#include <hip/hip_runtime.h>

// heads f32 [B][C][64] for the C channels of `tasks`, planes f32 [B][19][64], targets f32 [B][17][64] or nullptr (taken from the
// planes) -> rows f32 [B][M0_SSL_SCORE_COLS] (include/m0_ssl_score.h); all device pointers
hipError_t launch_ssl_score(const float* heads, int tasks, const float* planes, const float* targets, int B, float* rows,
                            hipStream_t stream);
