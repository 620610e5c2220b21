// Launch of augment_rows_kernel (augment_kernels.hip), on device pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// B rows (s [B][P][64], pi [B][4672], mask [B][4672] u8 or null with mask_out null) transformed into s_out, pi_out, mask_out on
// `stream`: row b by kinds[b] (device, u8 [B]; a value above M0_AUG_ROT180 is taken as M0_AUG_NONE), or every row by uniform_kind
// when kinds is null.  Out of place: hipErrorInvalidValue, and nothing launched, when an output is its own input, a required
// pointer is null, a mask comes without mask_out or the reverse, B <= 0, P <= 0 or uniform_kind is no kind.  Every pointer is
// 16-byte aligned (rows are whole multiples of 16 bytes).
hipError_t launch_augment_rows(const float* s, const float* pi, const uint8_t* mask, const uint8_t* kinds, int uniform_kind, int B, int P,
                               float* s_out, float* pi_out, uint8_t* mask_out, hipStream_t stream);
