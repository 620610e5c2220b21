// attn_core_kernel: ChessAttention.forward lines 142-179 (scores, both softmaxes, PV) for one (board, head) per wave -- the
// attention of every trunk that is not 320 wide and of the split path (M0_FUSE_ATTN=0); the arithmetic is attn_math.h.
// qkv [B][64][3C] fp16, channel = (t*H + h)*D + d, D == 16.  o [B][64][C] fp16 with channel h*D+d.
#include "attn_math.h"

constexpr int ATT_BOARDS = 16;

__global__ __launch_bounds__(256) void attn_core_kernel(AttnArgs a) {
    // One wave per (board, head); the K and Q operands come straight from global memory.
    // The first version did PV on the VALU (1024 FMAs + 256 LDS reads per lane and job): 520 us per call, VALU-bound;
    // the second read rel_bias from global memory per job (32 KB per job, 2.7 GB per call through L2): 311 us.
    // Workgroup = 4 waves = 4 consecutive heads (they share the 128-byte lines of a qkv row), looping over
    // ATT_BOARDS boards (3 workgroups per CU at 154 VGPRs); the 4 heads' relative-position bias sits in LDS (fp16, pre-scaled) for all of them.
    constexpr int VROW = 68;                           // halfs per LDS row (64 keys + pad: 136 B, conflict-free b64 reads)
    __shared__ __attribute__((aligned(16))) _Float16 Vt[4][16][VROW];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[4][64][VROW];
    __shared__ __attribute__((aligned(16))) _Float16 Ms[64][VROW];       // visibility mask as 0/1 (same for every head and board)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, C = a.C;
    const int hgroups = (H + 3) >> 2;
    const int hg = blockIdx.x % hgroups, bgroup = blockIdx.x / hgroups;
    const int h = hg * 4 + wave;
    const bool hlive = h < H;
    const int r31 = lane & 31, half = lane >> 5;
    if (a.rel_bias != nullptr) {
        for (int i = tid; i < 4 * 64 * 16; i += 256) {             // 4 keys per item
            const int hh = i >> 10, q = (i >> 4) & 63, k4 = (i & 15) * 4;
            if (hg * 4 + hh < H) {
                const float4 v = *reinterpret_cast<const float4*>(a.rel_bias + ((size_t)(hg * 4 + hh) * 64 + q) * 64 + k4);
                *reinterpret_cast<half4v*>(&Bs[hh][q][k4]) = half4v{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
            }
        }
    }
    for (int i = tid; i < 64 * 16; i += 256) {                     // 4 keys per item
        const int q = i >> 4, k4 = (i & 15) * 4;
        const uint64_t m = a.mask[q] >> k4;
        *reinterpret_cast<half4v*>(&Ms[q][k4]) = half4v{(_Float16)(float)(m & 1), (_Float16)(float)((m >> 1) & 1),
                                                        (_Float16)(float)((m >> 2) & 1), (_Float16)(float)((m >> 3) & 1)};
    }
    __syncthreads();
    for (int it = 0; it < ATT_BOARDS; ++it) {
        const int b = bgroup * ATT_BOARDS + it;
        const bool live = hlive && b < a.B;
        if (!live) continue;                               // wave-uniform; no barriers below
        const _Float16* base = a.qkv + (size_t)b * 64 * 3 * C;
        {   // V row `lane` (key) -> Vt[d][key]
            const _Float16* vp = base + (size_t)lane * 3 * C + (2 * H + h) * 16;
            const half8 v0 = *reinterpret_cast<const half8*>(vp), v1 = *reinterpret_cast<const half8*>(vp + 8);
#pragma unroll
            for (int d = 0; d < 8; ++d) { Vt[wave][d][lane] = v0[d]; Vt[wave][8 + d][lane] = v1[d]; }
        }
        // MFMA operands: A = K (rows = keys), B = Q^T (cols = queries); lane holds 8 consecutive head dims
        half8 kf[2], qf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            kf[t] = *reinterpret_cast<const half8*>(base + (size_t)(t * 32 + r31) * 3 * C + (1 * H + h) * 16 + 8 * half);
            qf[t] = *reinterpret_cast<const half8*>(base + (size_t)(t * 32 + r31) * 3 * C + (0 * H + h) * 16 + 8 * half);
        }
        // Vt[wave] is private to this wave: its LDS writes and reads execute in program order, no barrier
        half8 vf[2][2];
        attn_v_frags(&Vt[wave][lane & 15][0], half, vf);
        float wm, wu;
        attn_branch_weights(a.mix, wm, wu);
        const float isd = a.inv_sqrt_d * kLog2e;
        const float clampv = 50.f * kLog2e;
        static_for<0, 2>([&](auto qt_) __attribute__((always_inline)) {
            constexpr int qt = decltype(qt_)::value;
            const int q = qt * 32 + r31;
            float16v st[2];
            attn_scores(kf[0], kf[1], qf[qt], st);
            const _Float16* rb = a.rel_bias ? &Bs[wave][q][0] : nullptr;
            const _Float16* vm = &Ms[q][0];
            auto bias = [&](auto kt_, auto g_) __attribute__((always_inline)) {
                half4v b4 = {0, 0, 0, 0};
                if (rb) b4 = *reinterpret_cast<const half4v*>(rb + decltype(kt_)::value * 32 + 8 * decltype(g_)::value + 4 * half);
                return b4;
            };
            auto vis = [&](auto kt_, auto g_) __attribute__((always_inline)) {
                return *reinterpret_cast<const half4v*>(vm + decltype(kt_)::value * 32 + 8 * decltype(g_)::value + 4 * half);
            };
            const float16v oacc = attn_softmax_pv(st, bias, vis, vf, isd, clampv, wm, wu);
            *reinterpret_cast<uint4v*>(a.o + ((size_t)b * 64 + q) * C + h * 16 + 8 * half) = attn_pack_o(oacc, half);
        });
    }
}

hipError_t launch_attn_core(const AttnArgs& a, hipStream_t st) {
    const int hgroups = (a.H + 3) / 4, bgroups = (a.B + ATT_BOARDS - 1) / ATT_BOARDS;
    hipLaunchKernelGGL(attn_core_kernel, dim3((unsigned)(hgroups * bgroups)), dim3(256), 0, st, a);
    return hipGetLastError();
}
