// The residual-block tail (conv_tail.h) for conv_pp16_kernel's accumulator layout (4 x 10 tiles of 16x16, conv_epilogue16.h),
// all 8 waves together (LDS is free once the main loop is over):
//   A  per-board channel means of t from the accumulators                         -> LDS pool[4][C]
//   B  W1, W2 (fp16) by global_load_lds -> LDS, hidden = act(W1 pool + b1), gate = sigmoid(W2 hidden + b2) -> LDS;
//      B5: each lane picks up the gate values of its accumulator columns
//   C  gate * t staged as fp16 in the wave's private LDS image [64 rows][160 ch]   (conv_stage_tile16)
//   D, E  conv_tail.h: tail_residual, tail_gn_stats, tail_y2
// Phases C-E touch only the wave's own image: no workgroup barrier after B.
#pragma once
#include "conv_epilogue16.h"
#include "conv_tail.h"

// C == 320 (one N block), 8 waves: wave = (board wm, channel half wn), NT == 5.
// PRE: t is first normalised and activated, t <- act(GroupNorm16(t; a.pre_gamma, a.pre_beta)) -- the chess-feature
// convs (resnet.py:229-244: x += act(norm(conv(x)))); no squeeze-excite in that case.
#ifdef SW_STAMP
__device__ unsigned long long* g_tail_stamp;    // [blocks][8] realtime stamps of the tail's phases (tools/ubench)
#define TAIL_STAMP(k) do { if (tid == 0) g_tail_stamp[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TAIL_STAMP(k) do {} while (0)
#endif

template <int ACT, bool PRE = false>
__device__ __forceinline__ void conv_tail_epilogue16(float4v (&acc)[4][10], const GemmArgs& a, char* smem, int m0, int wm,
                                                     int wn, int wave, int lane) {
    constexpr int NT = 5, C = 320, NG = 10;
    const int tid = wave * 64 + lane;
    const int c15 = lane & 15;
    float* pool = reinterpret_cast<float*>(smem);              // [C][4 boards]   5120 B (one 16-byte read per channel)
    float* gate = pool + 4 * C;                                // [4][C]          5120 B
    float* hid = gate + 4 * C;                                 // [Hd<=128][4]    2048 B
    float* part = hid + 4 * 128;                               // [parts<=8][4][Hd<=128] 16384 B
    float* wst = reinterpret_cast<float*>(smem + 32768);       // staged W1 / W2: C*Hd*4 <= 131072 B - 32768
    const int Hd = a.se_hidden;
    const bool se = a.se_w1 != nullptr;
    // phase D/E lane mapping and the second output's GroupNorm parameters (fetched now: a late load is an exposed
    // global-memory latency in a kernel with one workgroup per CU)
    const int chunk = lane % TAIL_NCH, rsub = lane / TAIL_NCH;
    const bool lane_on = rsub < 3;
    float gg[8], bb[8];
    if (a.y2 != nullptr) tail_gn_params(a, wn * 160 + chunk * 8, gg, bb);
    float gv[NG];
    TAIL_STAMP(0);
    if (se && !PRE) {
        // B1 (issued first, lands while phase A runs): W1 and W2 as fp16 -> LDS, both at once (C*Hd*2 bytes each, a
        // multiple of 1024 for C = 320 and Hd a multiple of 8, which the launcher checks)
        const int wbytes = C * Hd * 2;
        const int npieces = wbytes >> 10;
        _Float16* wsth = reinterpret_cast<_Float16*>(wst);
        for (int p = wave; p < npieces; p += 8)
            glds16(reinterpret_cast<const char*>(a.se_w1h) + p * 1024 + lane * 16, reinterpret_cast<char*>(wsth) + p * 1024);
        for (int p = wave; p < npieces; p += 8)
            glds16(reinterpret_cast<const char*>(a.se_w2h) + p * 1024 + lane * 16, reinterpret_cast<char*>(wsth) + wbytes + p * 1024);
        const _Float16* w1l = wsth;                             // [C][Hd]
        const _Float16* w2l = wsth + C * Hd;                    // [Hd][C]
        // A: channel means of this wave's board / channel half
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            constexpr int ni = decltype(ni_)::value;
            float s = 0.f;
            static_for<0, 4>([&](auto mi_) __attribute__((always_inline)) {
                static_for<0, 4>([&](auto r_) __attribute__((always_inline)) { s += acc[decltype(mi_)::value][ni][decltype(r_)::value]; });
            });
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (lane < 16) pool[(wn * 160 + ni * 16 + c15) * 4 + wm] = s * (1.f / 64.f);
        });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // B2: hidden = act(W1 pool + b1); thread = (hidden unit j, channel part), the 4 boards at once; w1 is [C][Hd]
        const int parts = 512 / Hd > 8 ? 8 : 512 / Hd;
        {
            const int j = tid % Hd, p = tid / Hd;
            if (p < parts) {
                const int cpp = (C + parts - 1) / parts;
                const int cbeg = p * cpp, cend = cbeg + cpp < C ? cbeg + cpp : C;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 6
                for (int c = cbeg; c < cend; ++c) {
                    const float w = (float)w1l[c * Hd + j];
                    const float4 pv = *reinterpret_cast<const float4*>(pool + c * 4);
                    s0 = __builtin_fmaf(w, pv.x, s0); s1 = __builtin_fmaf(w, pv.y, s1); s2 = __builtin_fmaf(w, pv.z, s2); s3 = __builtin_fmaf(w, pv.w, s3);   // explicit: all four boards alike (se_gate_kernel's header)
                }
                float* pp = part + (p * 4) * 128 + j;
                pp[0] = s0; pp[128] = s1; pp[256] = s2; pp[384] = s3;
            }
        }
        __syncthreads();
        // B3: the hidden units
        for (int i = tid; i < 4 * Hd; i += 512) {
            const int b = i / Hd, j = i - b * Hd;
            float s = a.se_b1[j];
            for (int p = 0; p < parts; ++p) s += part[(p * 4 + b) * 128 + j];
            hid[j * 4 + b] = act_fast<ACT>(s);
        }
        __syncthreads();
        // B4: gate = sigmoid(W2 hidden + b2); thread = channel (first 320 threads), the 4 boards at once; w2 is [Hd][C]
        if (tid < C) {
            const float b2 = a.se_b2[tid];
            float s0 = b2, s1 = b2, s2 = b2, s3 = b2;
#pragma unroll 8
            for (int j = 0; j < Hd; ++j) {
                const float w = (float)w2l[j * C + tid];
                const float4 hv = *reinterpret_cast<const float4*>(hid + j * 4);
                s0 = __builtin_fmaf(w, hv.x, s0); s1 = __builtin_fmaf(w, hv.y, s1); s2 = __builtin_fmaf(w, hv.z, s2); s3 = __builtin_fmaf(w, hv.w, s3);
            }
            gate[tid] = __builtin_amdgcn_rcpf(1.f + __expf(-s0));
            gate[C + tid] = __builtin_amdgcn_rcpf(1.f + __expf(-s1));
            gate[2 * C + tid] = __builtin_amdgcn_rcpf(1.f + __expf(-s2));
            gate[3 * C + tid] = __builtin_amdgcn_rcpf(1.f + __expf(-s3));
        }
        __syncthreads();
        // B5: the gate values of this lane's accumulator columns
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            constexpr int ni = decltype(ni_)::value;
            gv[ni] = gate[wm * C + wn * 160 + ni * 16 + c15];
        });
        __syncthreads();                                          // the images below overwrite pool / gate / wst
    } else {
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) { gv[decltype(ni_)::value] = 1.f; });
    }
    float pv[NG];                                                 // PRE: per-column shift (gv = scale)
    if constexpr (PRE) {
        // GroupNorm(16 channels x 64 squares) of t on the accumulators: the wave owns whole groups (as EPI 1)
        static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
            constexpr int ni = decltype(ni_)::value;
            const int col = wn * 160 + ni * 16 + c15;
            float s = 0.f, ss = 0.f;
            static_for<0, 4>([&](auto mi_) __attribute__((always_inline)) {
                const float4v av = acc[decltype(mi_)::value][ni];
                static_for<0, 4>([&](auto r_) __attribute__((always_inline)) { const float v = av[decltype(r_)::value]; s += v; ss += v * v; });
            });
            s = wave_sum64(s); ss = wave_sum64(ss);
            const float mean = s * (1.f / 1024.f);
            float var = ss * (1.f / 1024.f) - mean * mean;
            var = var > 0.f ? var : 0.f;
            gv[ni] = rsqrtf(var + 1e-5f) * a.pre_gamma[col];
            pv[ni] = a.pre_beta[col] - mean * gv[ni];
        });
    }

    TAIL_STAMP(1);
    // C: gate * t -> the wave's fp16 image; the loads of x are issued between the tile columns, into the registers
    // the staged accumulators free (x is 2-3 us away and nothing else runs on this CU)
    char* img = smem + wave * (NT * 64 * 64);
    char* wbase = conv_stage_base16(img, lane);
    const uint32_t ldo2 = (uint32_t)a.ldo * 2u;
    const size_t tile_off = ((size_t)(m0 + wm * 64) * a.ldo + wn * 160) * 2;      // wave-uniform
    const char* xin = reinterpret_cast<const char*>(a.res) + tile_off;
    char* yout = reinterpret_cast<char*>(a.out) + tile_off;
    const int rows_valid = a.Mvalid - (m0 + wm * 64);
    const uint32_t lane_goff = (uint32_t)rsub * ldo2 + (uint32_t)chunk * 16u;
    const uint32_t lane_loff = (uint32_t)(rsub * TAIL_NCH + chunk) * 16u;
    half8 xv[TAIL_NIT];
    static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
        constexpr int ni = decltype(ni_)::value;
        static_for<0, 4>([&](auto mi_) __attribute__((always_inline)) {
            constexpr int mi = decltype(mi_)::value;
            float v[4];
            static_for<0, 4>([&](auto r_) __attribute__((always_inline)) {
                constexpr int r = decltype(r_)::value;
                if constexpr (PRE) v[r] = act_fast<ACT>(acc[mi][ni][r] * gv[ni] + pv[ni]);
                else v[r] = acc[mi][ni][r] * gv[ni];
            });
            conv_stage_tile16<mi, ni>(v, wbase, lane);
        });
        __builtin_amdgcn_sched_barrier(0);
        // the 22 loads of x spread over the 10 channel tiles (3 after each of the first two, 2 after the others)
        static_for<(ni < 2 ? ni * 3 : 6 + (ni - 2) * 2), (ni < 2 ? ni * 3 + 3 : 6 + (ni - 1) * 2)>([&](auto it_) __attribute__((always_inline)) {
            constexpr int it = decltype(it_)::value;
            const int row = rsub + 3 * it;
            xv[it] = (lane_on && row < 64) ? *reinterpret_cast<const half8*>(xin + (lane_goff + (uint32_t)(3 * it) * ldo2))
                                           : half8{0, 0, 0, 0, 0, 0, 0, 0};
        });
        __builtin_amdgcn_sched_barrier(0);
    });

    TAIL_STAMP(2);
    float gs, gss;
    tail_residual(img, lane_loff, yout, lane_goff, ldo2, rows_valid, xv, lane, gs, gss);
    TAIL_STAMP(3);
    if (a.y2 == nullptr) return;
    tail_gn_stats(gs, gss, lane);
    tail_y2<ACT>(img, lane_loff, reinterpret_cast<char*>(a.y2) + tile_off, lane_goff, ldo2, rows_valid, gs, gss, gg, bb, lane);
    TAIL_STAMP(4);
}
