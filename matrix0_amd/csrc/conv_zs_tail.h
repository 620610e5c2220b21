// Residual-block tail fused into conv2's epilogue (EPI_TAIL; PRE = EPI_TAIL_PRE), for conv_zs_kernel's accumulator layout
// (conv_zs_epilogue.h; the arithmetic is conv_tail.h's):
//   t      = conv2 output (the workgroup holds 4 whole boards x all 320 channels in its accumulators)
//   gate   = sigmoid(W2 act(W1 mean_squares(t) + b1) + b2)            squeeze-excite, resnet.py:59-68 (optional)
//   y      = x + gate * t                                             the residual stream          -> a.out
//   y2     = act(GroupNorm16(y; next block's bn1))                    the next conv1's operand     -> a.y2 (optional)
// A wave = (board pair wp, channel quarter wn): 2 boards x 80 channels, accumulators in the activation-as-operand-A layout
// (conv_zs_epilogue.h, zsa_* helpers): lane (c15, q) holds board q >> 1, square 8 mi + 4 (q & 1) + r, channel 16 ni + c15.
//
// Squeeze-excite on the matrix cores.  The two small FCs used to be scalar loops over LDS (5 barriers, ~7 us per tile, most
// of it the 100 KB of fp32->fp16 weights arriving from L2).  Here:
//   A  channel means of t from the accumulators (in-lane sums + one shuffle), written as fp16 hi + lo parts (the pair
//      carries ~22 mantissa bits) in A-fragment order: poolA[hi|lo][board][320]
//   B  FC1 as 16x16x32 MFMAs: rows = boards, K = 320 channels, N = hidden units; wave nt computes hidden units 16 nt..16 nt+15
//      (B fragments = host-packed pieces of W1, GemmArgs::se_wf), adds b1, activates, writes hidden as hi + lo fp16
//   C  FC2 per wave for its own 80 channels: rows = boards ordered so that accumulator row 4q + r is board q >> 1 of the
//      wave's pair -- the gate of (board, channel) comes out in exactly the lane that scales that accumulator column.
// Three workgroup barriers.  The weight pieces are one stream of 1-KiB DMA pieces (se_wf): 10 x ceil(Hd/16) of W1, then
// 20 x ceil(Hd/32) of W2, at most 60 + 60 for Hd <= TAIL_SE_HMAX (net_kernels.h).
//
// D  gate * t staged as fp16 in the wave's private image [64 squares][2 boards][80 ch]; the loads of x are issued between
//    the tile columns into the registers the staged accumulators free
// E, F  conv_tail.h: tail_residual (lane = (16-byte channel chunk of a board, square mod 3)), tail_gn_stats (a board has
//    an even number of chunks, so chunk ^ 1 is in the same board), tail_y2.
// D-F touch only the wave's own image: no workgroup barrier after C.
#pragma once
#include "conv_zs_epilogue.h"
#include "conv_tail.h"

constexpr int ZS_SE_WOFF = 8192;          // LDS offset of the weight pieces during the squeeze-excite phase

// number of 1-KiB pieces of GemmArgs::se_wf for Hd hidden units (net_pack.h lays them out, se_fragments)
__host__ __device__ inline int zs_se_pieces_w1(int Hd) { return 10 * ((Hd + 15) >> 4); }
__host__ __device__ inline int zs_se_pieces_w2(int Hd) { return 20 * ((Hd + 31) >> 5); }

#ifdef SW_STAMP
__device__ unsigned long long* g_zs_tail_stamp;    // [blocks][8] realtime stamps of the tail's phases (tools/ubench)
#define ZS_TAIL_STAMP(k) do { if (tid == 0) g_zs_tail_stamp[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ZS_TAIL_STAMP(k) do {} while (0)
#endif

// PRE: t is first normalised and activated, t <- act(GroupNorm16(t; a.pre_gamma, a.pre_beta)) -- the chess-feature
// convs (resnet.py:229-244: x += act(norm(conv(x)))); no squeeze-excite in that case.
template <int ACT, bool PRE = false>
__device__ __forceinline__ void zs_tail_epilogue(float4v (&acc)[8][5], const GemmArgs& a, char* smem, int m0, int wp, int wn,
                                                 int wave, int lane) {
    constexpr int NG = 5, MT = 8;
    const int tid = wave * 64 + lane;
    const int c15 = lane & 15, q = lane >> 4;
    const bool se = a.se_w1 != nullptr;
    // phase E/F lane mapping and the second output's GroupNorm parameters (fetched now: a late load is an exposed
    // global-memory latency in a kernel with one workgroup per CU)
    const int c20 = lane % TAIL_NCH, rsub = lane / TAIL_NCH;
    const bool lane_on = rsub < 3;
    const int bd = c20 >= 10 ? 1 : 0, ch = c20 - 10 * bd;        // board of the pair, chunk of its 80 channels
    float gg[8], bb[8];
    if (a.y2 != nullptr) tail_gn_params(a, wn * 80 + ch * 8, gg, bb);
    float gv[NG];
    ZS_TAIL_STAMP(0);
    if (se && !PRE) {
        const int Hd = a.se_hidden;
        const int NT1 = (Hd + 15) >> 4, KS2 = (Hd + 31) >> 5;
        const int n1 = 10 * NT1, npieces = n1 + 20 * KS2;
        _Float16* poolA = reinterpret_cast<_Float16*>(smem);           // [2][4][320]  5120 B
        _Float16* hidA = reinterpret_cast<_Float16*>(smem + 5120);     // [2][4][128]  2048 B, zero beyond the hidden units
        const char* wf = smem + ZS_SE_WOFF;
        for (int p = wave; p < npieces; p += 8)
            glds16(reinterpret_cast<const char*>(a.se_wf) + (size_t)p * 1024 + lane * 16, smem + ZS_SE_WOFF + p * 1024);
        if (tid < 128) reinterpret_cast<uint4*>(hidA)[tid] = make_uint4(0, 0, 0, 0);
        const int j1 = 16 * wave + c15;
        const float b1v = (wave < NT1 && j1 < Hd) ? a.se_b1[j1] : 0.f;
        float b2v[NG];
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            b2v[decltype(ni_)::value] = a.se_b2[wn * 80 + decltype(ni_)::value * 16 + c15];
        });
        // A: channel means of the lane's (board, 5 channels)
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            constexpr int ni = decltype(ni_)::value;
            float s = 0.f;
            static_for<0, MT>([&](auto mi_) __attribute__((always_inline)) {
                static_for<0, 4>([&](auto r_) __attribute__((always_inline)) { s += acc[decltype(mi_)::value][ni][decltype(r_)::value]; });
            });
            s += __shfl_xor(s, 16);
            const float mean = s * (1.f / 64.f);
            const _Float16 hi = (_Float16)mean;
            const _Float16 lo = (_Float16)(mean - (float)hi);
            if ((q & 1) == 0) {
                const int o = (2 * wp + (q >> 1)) * 320 + wn * 80 + ni * 16 + c15;
                poolA[o] = hi; poolA[4 * 320 + o] = lo;
            }
        });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // B: hidden units 16 wave .. 16 wave + 15 of the 4 boards (A rows: board = row & 3)
        if (wave < NT1) {
            float4v h0 = {0.f, 0.f, 0.f, 0.f}, h1 = {0.f, 0.f, 0.f, 0.f};
            const _Float16* pa = poolA + (c15 & 3) * 320 + 8 * q;
            const char* wb = wf + (size_t)(wave * 10) * 1024 + lane * 16;
#pragma unroll
            for (int ks = 0; ks < 10; ++ks) {
                const half8 ah = *reinterpret_cast<const half8*>(pa + 32 * ks);
                const half8 al = *reinterpret_cast<const half8*>(pa + 4 * 320 + 32 * ks);
                const half8 bw = *reinterpret_cast<const half8*>(wb + ks * 1024);
                h0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw, h0, 0, 0, 0);
                h1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw, h1, 0, 0, 0);
            }
            if (q == 0) {                                            // rows 0..3 = boards 0..3, column c15 = hidden unit j1
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float hv = act_fast<ACT>(h0[r] + h1[r] + b1v);
                    const _Float16 hi = (_Float16)hv;
                    hidA[r * 128 + j1] = hi;
                    hidA[4 * 128 + r * 128 + j1] = (_Float16)(hv - (float)hi);
                }
            }
        }
        __syncthreads();
        // C: gate of this wave's 2 boards x 80 channels (A rows 0..7: board a of the pair, 8..15: board b)
        {
            float4v g0[NG], g1[NG];
            static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
                g0[decltype(ni_)::value] = float4v{0.f, 0.f, 0.f, 0.f}; g1[decltype(ni_)::value] = float4v{0.f, 0.f, 0.f, 0.f};
            });
            const _Float16* ha = hidA + (2 * wp + (c15 >> 3)) * 128 + 8 * q;
            const char* wb = wf + (size_t)n1 * 1024 + (size_t)(5 * wn * KS2) * 1024 + lane * 16;
            for (int ks = 0; ks < KS2; ++ks) {
                const half8 ah = *reinterpret_cast<const half8*>(ha + 32 * ks);
                const half8 al = *reinterpret_cast<const half8*>(ha + 4 * 128 + 32 * ks);
                static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
                    constexpr int ni = decltype(ni_)::value;
                    const half8 bw = *reinterpret_cast<const half8*>(wb + (size_t)(ni * KS2 + ks) * 1024);
                    g0[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw, g0[ni], 0, 0, 0);
                    g1[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw, g1[ni], 0, 0, 0);
                });
            }
            static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
                constexpr int ni = decltype(ni_)::value;
                gv[ni] = __builtin_amdgcn_rcpf(1.f + __expf(-(g0[ni][0] + g1[ni][0] + b2v[ni])));
            });
        }
        __syncthreads();                                          // the images below overwrite the pools and the weights
    } else {
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) { gv[decltype(ni_)::value] = 1.f; });
    }
    float pv[NG];                                                 // PRE: per-column shift (gv = scale)
    if constexpr (PRE) {
        // GroupNorm(16 channels x 64 squares) of t on the accumulators: a board's group is 32 lanes of this wave
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            constexpr int ni = decltype(ni_)::value;
            const int col = wn * 80 + ni * 16 + c15;
            float s = 0.f, ss = 0.f;
            static_for<0, MT>([&](auto mi_) __attribute__((always_inline)) {
                const float4v av = acc[decltype(mi_)::value][ni];
                static_for<0, 4>([&](auto r_) __attribute__((always_inline)) { const float v = av[decltype(r_)::value]; s += v; ss += v * v; });
            });
            s = zsa_sum_board(s); ss = zsa_sum_board(ss);
            float mean, rstd;
            gn16_mean_rstd(s, ss, mean, rstd);
            gn16_affine(mean, rstd, a.pre_gamma[col], a.pre_beta[col], gv[ni], pv[ni]);
        });
    }

    ZS_TAIL_STAMP(1);
    // D: gate * t -> the wave's fp16 image; the loads of x are issued between the tile columns, into the registers
    // the staged accumulators free (x is 2-3 us away and nothing else runs on this CU)
    char* img = smem + wave * 20480;
    char* wbase = zsa_stage_base(img, lane);
    const uint32_t ldo2 = (uint32_t)a.ldo * 2u;
    const size_t tile_off = ((size_t)(m0 + wp * 128) * a.ldo + wn * 80) * 2;      // wave-uniform
    const char* xin = reinterpret_cast<const char*>(a.res) + tile_off;
    char* yout = reinterpret_cast<char*>(a.out) + tile_off;
    const int rows_valid = a.Mvalid - (m0 + wp * 128 + bd * 64);                  // of this lane's board
    const uint32_t lane_goff = (uint32_t)(bd * 64 + rsub) * ldo2 + (uint32_t)ch * 16u;
    const uint32_t lane_loff = (uint32_t)(rsub * TAIL_NCH + c20) * 16u;
    half8 xv[TAIL_NIT];
    static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
        constexpr int ni = decltype(ni_)::value;
        static_for<0, MT>([&](auto mi_) __attribute__((always_inline)) {
            constexpr int mi = decltype(mi_)::value;
            float v[4];
            static_for<0, 4>([&](auto r_) __attribute__((always_inline)) {
                constexpr int r = decltype(r_)::value;
                if constexpr (PRE) v[r] = act_fast<ACT>(acc[mi][ni][r] * gv[ni] + pv[ni]);
                else v[r] = acc[mi][ni][r] * gv[ni];
            });
            zsa_stage_tile<mi, ni>(v, wbase, lane);
        });
        __builtin_amdgcn_sched_barrier(0);
        // the 22 loads of x spread over the 5 channel tiles (5 after each of the first two, 4 after the others)
        static_for<(ni < 2 ? ni * 5 : 10 + (ni - 2) * 4), (ni < 2 ? ni * 5 + 5 : 10 + (ni - 1) * 4)>([&](auto it_) __attribute__((always_inline)) {
            constexpr int it = decltype(it_)::value;
            const int row = rsub + 3 * it;
            xv[it] = (lane_on && row < 64) ? *reinterpret_cast<const half8*>(xin + (lane_goff + (uint32_t)(3 * it) * ldo2))
                                           : half8{0, 0, 0, 0, 0, 0, 0, 0};
        });
        __builtin_amdgcn_sched_barrier(0);
    });

    ZS_TAIL_STAMP(2);
    float gs, gss;
    tail_residual(img, lane_loff, yout, lane_goff, ldo2, rows_valid, xv, lane, gs, gss);
    ZS_TAIL_STAMP(3);
    if (a.y2 == nullptr) return;
    tail_gn_stats(gs, gss, lane);
    tail_y2<ACT>(img, lane_loff, reinterpret_cast<char*>(a.y2) + tile_off, lane_goff, ldo2, rows_valid, gs, gss, gg, bb, lane);
    ZS_TAIL_STAMP(4);
}
