// The per-wave attention arithmetic of ChessAttention.forward (resnet.py:142-179), shared by attn_core_kernel
// (attn_core.hip) and phase 2 of attn_block_kernel (attn_block.hip): both kernels must give the same bits.
//   S = QK^T/sqrt(D) (+rel_bias[h]) clamp +-50 ; masked branch fill -1e4 ;   (rel_bias arrives times log2 e)
//   out = (1-mix)*softmax(S_masked)V + mix*softmax(S)V     (mix in (0,1))
//   mix >= 1: masked only ; mix <= 0: unmasked only.
// One wave handles 32 queries of one (board, head) against its 64 keys, head dim 16, both matrix products on MFMA 32x32x16
// (r31 = lane & 31 = query, half = lane >> 5):
//   S^T = K Q^T  (A = K rows = keys, B = Q^T cols = queries; K = head_dim = 16: one MFMA per 32x32 tile) -> a lane owns one
//                 query column and 16 keys per tile in registers, so the softmax sums need a single cross-half shuffle;
//   O^T = V^T P^T (A = V^T rows = head dims (16 of the 32 used), B = P^T cols = queries): the B operand IS the
//                 lane's register block of probabilities -- the contraction index may be enumerated in any order as
//                 long as A agrees, so A is gathered from a transposed LDS copy of V in the accumulator's key order.
// Accumulator order: register r of S^T tile kt is key kt*32 + 8(r>>2) + 4 half + (r&3).  Bias and visibility reach the core
// through accessors (kt, g) -> the half4v of registers 4g..4g+3 of tile kt (keys kt*32 + 8g + 4 half + {0..3}): one 8-byte
// LDS read in attn_core_kernel, a slice of registers in attn_block_kernel.  kt and g arrive as integral_constants.
#pragma once
#include "kernel_common.h"

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.44269504088896f;        // scores in log2 units: exp(x) = exp2(x log2 e)

// output weights of the masked / unmasked branch (resnet.py:154-174)
__device__ __forceinline__ void attn_branch_weights(float mix, float& wm, float& wu) {
    if (mix > 0.f && mix < 1.f) { wm = 1.f - mix; wu = 1.f - (1.f - mix); }
    else if (mix >= 1.f) { wm = 1.f; wu = 0.f; }
    else { wm = 0.f; wu = 1.f; }
}

// A operand of the PV product for S^T tile kt, register block jb (regs 8jb..8jb+7): V[key][d], d = lane & 15,
// keys kt*32 + 16 jb + 4 half + {0..3} and + 8 more (the accumulator's row order).  vrow = row d of the transposed V copy.
__device__ __forceinline__ void attn_v_frags(const _Float16* vrow, int half, half8 (&vf)[2][2]) {
    static_for<0, 2>([&](auto kt_) __attribute__((always_inline)) {
        static_for<0, 2>([&](auto jb_) __attribute__((always_inline)) {
            constexpr int kt = decltype(kt_)::value, jb = decltype(jb_)::value;
            const half4v lo = *reinterpret_cast<const half4v*>(vrow + kt * 32 + 16 * jb + 4 * half);
            const half4v hi = *reinterpret_cast<const half4v*>(vrow + kt * 32 + 16 * jb + 8 + 4 * half);
            vf[kt][jb] = half8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        });
    });
}

// S^T tiles of one query tile: row (key) = (r&3)+8*(r>>2)+4*half (+32 for the 2nd), col (query) = lane&31
__device__ __forceinline__ void attn_scores(half8 kf0, half8 kf1, half8 qf, float16v (&st)[2]) {
    const float16v zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    st[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf0, qf, zero, 0, 0, 0);
    st[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf1, qf, zero, 0, 0, 0);
}

// scores -> probabilities -> O^T.  isd = log2(e)/sqrt(D), clampv = 50 log2(e); wm, wu from attn_branch_weights.
template <typename Bias, typename Vis>
__device__ __forceinline__ float16v attn_softmax_pv(const float16v (&st)[2], Bias&& bias, Vis&& vis, const half8 (&vf)[2][2],
                                                    float isd, float clampv, float wm, float wu) {
    // scores clamped to [-50,50]: exp needs no max subtraction; masked fill -1e4 underflows to exactly 0
    float e[2][16];
    float su = 0.f, sm = 0.f;
    static_for<0, 2>([&](auto kt_) __attribute__((always_inline)) {
        static_for<0, 4>([&](auto g_) __attribute__((always_inline)) {
            constexpr int kt = decltype(kt_)::value, g = decltype(g_)::value;
            const half4v b4 = bias(kt_, g_);
            const half4v v4 = vis(kt_, g_);          // 1 where the mask lets the query see the key, as an fp16 multiplicand
            static_for<0, 4>([&](auto j_) __attribute__((always_inline)) {
                constexpr int j = decltype(j_)::value;
                float d = st[kt][4 * g + j] * isd + (float)b4[j];
                d = __builtin_amdgcn_fmed3f(d, -clampv, clampv);
                const float eu = __builtin_amdgcn_exp2f(d);
                e[kt][4 * g + j] = eu;
                su += eu;
                sm += eu * (float)v4[j];
            });
        });
    });
    su += __shfl_xor(su, 32);
    sm += __shfl_xor(sm, 32);
    const float cu = wu / su, cm = wm / sm;
    // probabilities (both branches folded into one weight) as the B operand, O^T accumulated over the 4 key blocks
    float16v oacc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    static_for<0, 2>([&](auto kt_) __attribute__((always_inline)) {
        static_for<0, 2>([&](auto jb_) __attribute__((always_inline)) {
            constexpr int kt = decltype(kt_)::value, jb = decltype(jb_)::value;
            // regs 8jb..8jb+3 = keys kt*32 + 16 jb + 4 half + {0..3}, regs +4..+7 = the same + 8
            const half4v v0 = vis(kt_, std::integral_constant<int, 2 * jb>{});
            const half4v v1 = vis(kt_, std::integral_constant<int, 2 * jb + 1>{});
            half8 pf;
            static_for<0, 8>([&](auto u_) __attribute__((always_inline)) {
                constexpr int u = decltype(u_)::value;
                constexpr int r = 8 * jb + u;                          // key = kt*32 + (r&3) + 8*(r>>2) + 4*half
                const float vs = (float)(u < 4 ? v0[u & 3] : v1[u & 3]);
                pf[u] = (_Float16)(e[kt][r] * (vs * cm + cu));
            });
            oacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[kt][jb], pf, oacc, 0, 0, 0);
        });
    });
    return oacc;
}

// O^T: lane = query, regs 0..7 = head dims (r&3) + 8*(r>>2) + 4*half -> 16 contiguous bytes per lane (dims 8 half .. 8 half + 7)
// after one exchange with the other half
__device__ __forceinline__ uint4v attn_pack_o(const float16v& oacc, int half) {
    union { half2v h2[2]; uint32_t u[2]; } lo4, hi4, rcv;
    lo4.h2[0] = half2v{(_Float16)oacc[0], (_Float16)oacc[1]}; lo4.h2[1] = half2v{(_Float16)oacc[2], (_Float16)oacc[3]};
    hi4.h2[0] = half2v{(_Float16)oacc[4], (_Float16)oacc[5]}; hi4.h2[1] = half2v{(_Float16)oacc[6], (_Float16)oacc[7]};
    rcv.u[0] = __shfl_xor(half ? lo4.u[0] : hi4.u[0], 32);
    rcv.u[1] = __shfl_xor(half ? lo4.u[1] : hi4.u[1], 32);
    if (half == 0) return uint4v{lo4.u[0], lo4.u[1], rcv.u[0], rcv.u[1]};      // d 0..3 own, 4..7 from the partner
    return uint4v{rcv.u[0], rcv.u[1], hi4.u[0], hi4.u[1]};                     // d 8..11 from the partner, 12..15 own
}
