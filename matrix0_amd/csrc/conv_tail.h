// Residual-block tails fused into a conv's epilogue (the workgroup holds 4 whole boards x all 320 channels in its
// accumulators):
//   t      = conv output
//   gate   = sigmoid(W2 act(W1 mean_squares(t) + b1) + b2)            squeeze-excite, resnet.py:59-68 (optional)
//   or PRE: t <- act(GroupNorm16(t; a.pre_gamma, a.pre_beta))          the chess-feature convs, resnet.py:229-244
//   y      = x + gate * t                                             the residual stream          -> a.out
//   y2     = act(GroupNorm16(y; next block's bn1))                    the next conv1's operand     -> a.y2 (optional)
// i.e. what conv2's plain epilogue + se_gate_kernel + ew_board_kernel did with three launches and two more trips of
// the tensor through HBM.  Everything a board needs is inside the workgroup, so the only new global traffic is the
// read of x.  Each accumulator layout has its own tail: conv_tail_epilogue below (conv_big_kernel, EPI_TAIL_PRE only)
// and conv_zs_tail.h (conv_zs_kernel, EPI_TAIL and EPI_TAIL_PRE).  Each reads its accumulators (channel means,
// squeeze-excite gate, PRE statistics) and stages gate * t as fp16 in the wave's private LDS image, 64 rows of 20
// 16-byte chunks, issuing the loads of x between the tile columns.  The rest works on that image and is shared:
//   tail_gn_params  the second GroupNorm's parameters of the lane's 8 channels (fetched first: a late load is an
//                   exposed global-memory latency in a kernel with one workgroup per CU)
//   tail_residual   lane = (16-byte chunk, row mod 3): y = x + image, store y, write y back to the image, GroupNorm sums
//   tail_gn_stats   the GroupNorm statistics of the lane's group by shuffles
//   tail_y2         second pass over the image: y2 = act(y * scale + shift), 16-byte stores
// None of them needs a workgroup barrier.
//
// (The attention block's tail -- residual + LayerNorm over C + next GroupNorm -- was fused into the proj conv the same
//  way, in the accumulator layout with DPP row reductions: correct, but 374 us against 92 + 228 us for proj +
//  ew_board_kernel, because a row's LayerNorm statistics need cross-lane and cross-wave reductions and a per-element
//  gather of x; not kept.)
#pragma once
#include "conv_epilogue.h"

constexpr int TAIL_NCH = 20;         // 16-byte chunks per image row (160 channels)
constexpr int TAIL_NIT = 22;         // image rows per lane: ceil(64 / 3)

__device__ __forceinline__ void tail_gn_params(const GemmArgs& a, int c0, float (&gg)[8], float (&bb)[8]) {
    load8f(a.gn_gamma + c0, gg);
    load8f(a.gn_beta + c0, bb);
}

// y = x + image; lane = (chunk = lane % 20, rsub = lane / 20), rows rsub, rsub+3, ...; lanes 60..63 idle.  Row `row` of
// the lane is at img + lane_loff + row * 320 and at global offset lane_goff + row * ldo2 of yout (stored below rows_valid).
// The sum of two fp16 numbers rounded to fp16 is what the fp32 add + conversion gives, so y is computed with packed
// fp16 adds (4 instructions per 8 channels); the GroupNorm sums (this lane's 8 channels x its rows) use the
// 2-element fp16 dot product with fp32 accumulation, on the rounded y (the tensor that is actually stored).
__device__ __forceinline__ void tail_residual(char* img, uint32_t lane_loff, char* yout, uint32_t lane_goff, uint32_t ldo2,
                                              int rows_valid, const half8 (&xv)[TAIL_NIT], int lane, float& gs, float& gss) {
    const int rsub = lane / TAIL_NCH;
    const bool lane_on = rsub < 3;
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 ones = {(_Float16)1.f, (_Float16)1.f};
    gs = 0.f; gss = 0.f;
#pragma unroll
    for (int it = 0; it < TAIL_NIT; ++it) {
        const int row = rsub + 3 * it;
        if (lane_on && row < 64) {
            half8* ip = reinterpret_cast<half8*>(img + lane_loff + (uint32_t)(3 * it * TAIL_NCH) * 16u);
            const half8 yv = *ip + xv[it];
            static_for<0, 4>([&](auto i_) __attribute__((always_inline)) {
                constexpr int i = decltype(i_)::value;
                const h2 p = {yv[2 * i], yv[2 * i + 1]};
                gs = __builtin_amdgcn_fdot2(p, ones, gs, false);
                gss = __builtin_amdgcn_fdot2(p, p, gss, false);
            });
            *ip = yv;
            if (row < rows_valid) *reinterpret_cast<half8*>(yout + (lane_goff + (uint32_t)(3 * it) * ldo2)) = yv;
        }
    }
}

// GroupNorm statistics of y: over the 3 row classes (lanes chunk, chunk+20, chunk+40), then over the group's 16
// channels = this lane's 8 + the neighbour chunk's 8 (chunk ^ 1: the same group, a group is 2 chunks)
__device__ __forceinline__ void tail_gn_stats(float& gs, float& gss, int lane) {
    const int chunk = lane % TAIL_NCH;
    const float s1 = __shfl(gs, chunk + TAIL_NCH), s2 = __shfl(gs, chunk + 2 * TAIL_NCH);
    const float q1 = __shfl(gss, chunk + TAIL_NCH), q2 = __shfl(gss, chunk + 2 * TAIL_NCH);
    gs = __shfl(gs, chunk) + s1 + s2;                        // every lane: totals of its chunk (same order everywhere)
    gss = __shfl(gss, chunk) + q1 + q2;
    const float so = __shfl_xor(gs, 1), qo = __shfl_xor(gss, 1);      // partner chunk (chunk ^ 1 is lane ^ 1 for lanes < 60)
    const float lo_s = (chunk & 1) ? so : gs, hi_s = (chunk & 1) ? gs : so;
    const float lo_q = (chunk & 1) ? qo : gss, hi_q = (chunk & 1) ? gss : qo;
    gs = lo_s + hi_s; gss = lo_q + hi_q;
}

// y2 = act(GroupNorm(y)) from the image (same rows and offsets as tail_residual); gs / gss from tail_gn_stats
template <int ACT>
__device__ __forceinline__ void tail_y2(const char* img, uint32_t lane_loff, char* y2out, uint32_t lane_goff, uint32_t ldo2,
                                        int rows_valid, float gs, float gss, const float (&gg)[8], const float (&bb)[8], int lane) {
    const int rsub = lane / TAIL_NCH;
    const bool lane_on = rsub < 3;
    float mean, rstd;
    gn16_mean_rstd(gs, gss, mean, rstd);
    float scl[8], shl[8];
    static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
        constexpr int i = decltype(i_)::value;
        gn16_affine(mean, rstd, gg[i], bb[i], scl[i], shl[i]);
    });
#pragma unroll
    for (int it = 0; it < TAIL_NIT; ++it) {
        const int row = rsub + 3 * it;
        if (lane_on && row < 64 && row < rows_valid) {
            const half8 yv = *reinterpret_cast<const half8*>(img + lane_loff + (uint32_t)(3 * it * TAIL_NCH) * 16u);
            half8 ov;
            static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
                constexpr int i = decltype(i_)::value;
                ov[i] = (_Float16)act_fast<ACT>((float)yv[i] * scl[i] + shl[i]);
            });
            *reinterpret_cast<half8*>(y2out + (lane_goff + (uint32_t)(3 * it) * ldo2)) = ov;
        }
    }
}

// conv_big_kernel's layout (2 x 5 tiles of 32x32, conv_epilogue.h), PRE form: out = res + act(GroupNorm16(t)) (+ y2).
// C == 320 (one N block), 8 waves: wave = (board wm, channel half wn), NT == 5.
template <int ACT>
__device__ __forceinline__ void conv_tail_epilogue(float16v (&acc)[2][5], const GemmArgs& a, char* smem, int m0, int wm,
                                                   int wn, int wave, int lane) {
    constexpr int NT = 5;
    const int r31 = lane & 31;
    const int chunk = lane % TAIL_NCH, rsub = lane / TAIL_NCH;
    const bool lane_on = rsub < 3;
    float gg[8], bb[8];
    if (a.y2 != nullptr) tail_gn_params(a, wn * 160 + chunk * 8, gg, bb);
    // GroupNorm16 of t on the accumulators, as EPI_GN: per-column scale and shift
    float gv[NT], pv[NT];
    static_for<0, NT>([&](auto ni_) __attribute__((always_inline)) {
        constexpr int ni = decltype(ni_)::value;
        conv_gn_column<ni>(acc, a.pre_gamma, a.pre_beta, wn * 160 + ni * 32 + r31, gv[ni], pv[ni]);
    });

    // act(t * scale + shift) -> the wave's fp16 image; the loads of x are issued between the tile columns, into the
    // registers the staged accumulators free (x is 2-3 us away and nothing else runs on this CU)
    char* img = smem + wave * (NT * 64 * 64);
    char* wbase = conv_stage_base<NT>(img, lane);
    const uint32_t ldo2 = (uint32_t)a.ldo * 2u;
    const size_t tile_off = ((size_t)(m0 + wm * 64) * a.ldo + wn * 160) * 2;      // wave-uniform
    const char* xin = reinterpret_cast<const char*>(a.res) + tile_off;
    char* yout = reinterpret_cast<char*>(a.out) + tile_off;
    const int rows_valid = a.Mvalid - (m0 + wm * 64);
    const uint32_t lane_goff = (uint32_t)rsub * ldo2 + (uint32_t)chunk * 16u;
    const uint32_t lane_loff = (uint32_t)(rsub * TAIL_NCH + chunk) * 16u;
    half8 xv[TAIL_NIT];
    static_for<0, NT>([&](auto ni_) __attribute__((always_inline)) {
        constexpr int ni = decltype(ni_)::value;
        static_for<0, 2>([&](auto mi_) __attribute__((always_inline)) {
            constexpr int mi = decltype(mi_)::value;
            float v[16];
            static_for<0, 16>([&](auto r_) __attribute__((always_inline)) {
                constexpr int r = decltype(r_)::value;
                v[r] = act_fast<ACT>(acc[mi][ni][r] * gv[ni] + pv[ni]);
            });
            conv_stage_tile<NT, mi, ni>(v, wbase, lane);
        });
        __builtin_amdgcn_sched_barrier(0);
        static_for<ni * 5, (ni * 5 + 5 < TAIL_NIT ? ni * 5 + 5 : TAIL_NIT)>([&](auto it_) __attribute__((always_inline)) {
            constexpr int it = decltype(it_)::value;
            const int row = rsub + 3 * it;
            xv[it] = (lane_on && row < 64) ? *reinterpret_cast<const half8*>(xin + (lane_goff + (uint32_t)(3 * it) * ldo2))
                                           : half8{0, 0, 0, 0, 0, 0, 0, 0};
        });
        __builtin_amdgcn_sched_barrier(0);
    });

    float gs, gss;
    tail_residual(img, lane_loff, yout, lane_goff, ldo2, rows_valid, xv, lane, gs, gss);
    if (a.y2 == nullptr) return;
    tail_gn_stats(gs, gss, lane);
    tail_y2<ACT>(img, lane_loff, reinterpret_cast<char*>(a.y2) + tile_off, lane_goff, ldo2, rows_valid, gs, gss, gg, bb, lane);
}
