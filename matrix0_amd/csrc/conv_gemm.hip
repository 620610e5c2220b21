// conv_gemm_kernel: the small-tile implicit GEMM (any N % 32 == 0, Cin % 32 == 0) on v_mfma_f32_32x32x16_f16 -- the stem, the
// head convs and the FCs -- and launch_conv_gemm, which sends every conv / FC of the network to its kernel: here, or to
// conv_big_kernel (conv_big.hip) or conv_zs_kernel (conv_zs.hip) when N is a multiple of 320.  Data layout: net_kernels.h.
// WG = 4 WN waves, tile = 256 rows (4 boards) x 32 NT WN output channels; wave = (board wm, N part wn).  Operands go global ->
// registers -> LDS (rows padded by 8 halfs: conflict-free b128 reads), the weights double-buffered; a 3x3 conv reads its taps
// from a zero-bordered 10x10 image of each board.
#include "kernel_common.h"
#include "conv_epilogue.h"

// EPI_ELEMENT: bias / runtime activation / gate multiply / scale, fp16 or f32 stored per element, per-(board, channel) sums.
// EPI_GN: act<ACT>(GroupNorm16(conv)) [+ positional encoding] applied to the accumulators (a wave holds all 64 squares of its
//        board for its 32 NT channels = 2 NT whole groups), fp16 through the wave's LDS image in 16-byte stores -- the stem and
//        the head convs write no raw tensor + statistics for an ew_board pass to read back.
template <int TAPS, int WN, int NT, int KC, ConvEpi EPI = EPI_ELEMENT, int ACT = ACT_NONE>
__global__ __launch_bounds__(256 * WN) void conv_gemm_kernel(GemmArgs a) {
    constexpr int NB = WN * NT * 32;      // output channels per workgroup
    constexpr int NTHR = 256 * WN;
    constexpr int AST = KC + 8;           // LDS row stride in halfs (pad: conflict-free b128 reads)
    constexpr int APIX = (TAPS == 9) ? 100 : 64;
    constexpr int A_ELEMS = 4 * APIX * AST;
    constexpr int W_ELEMS = NB * AST;
    constexpr int A_PIECES = 4 * 64 * KC / 8;             // 16-byte pieces per A chunk
    constexpr int W_PIECES = NB * KC / 8;
    constexpr int A_PER = (A_PIECES + NTHR - 1) / NTHR;
    constexpr int W_PER = (W_PIECES + NTHR - 1) / NTHR;
    constexpr int K8 = KC / 8;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    _Float16* A_lds = reinterpret_cast<_Float16*>(smem);
    _Float16* W_lds = A_lds + A_ELEMS;                    // 2 buffers

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave % 4;              // board within the tile
    const int wn = wave / 4;              // N half
    const int m0 = blockIdx.x * 256;      // first row
    const int n0 = blockIdx.y * NB;
    const int Cin = a.Cin;
    const int nchunk = Cin / KC;
    const int Npad = a.Npad;

    // zero the halo image once (borders stay zero for the whole kernel)
    if (TAPS == 9) {
        for (int i = tid; i < A_ELEMS / 8; i += NTHR)
            reinterpret_cast<uint4*>(A_lds)[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();

    float16v acc[2][NT];
    static_for<0, 2>([&](auto mi) __attribute__((always_inline)) {
        static_for<0, NT>([&](auto ni) __attribute__((always_inline)) {
            acc[decltype(mi)::value][decltype(ni)::value] = float16v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
                                                                      0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        });
    });

    // per-lane LDS base of its two A rows (squares lane&31 and 32+(lane&31) of board wm)
    int apix[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        int px = mi * 32 + (lane & 31);
        if (TAPS == 9) apix[mi] = wm * 100 + ((px >> 3) + 1) * 10 + (px & 7) + 1;
        else apix[mi] = wm * 64 + px;
    }
    const int khalf = 8 * (lane >> 5);

    uint4 areg[A_PER];
    uint4 wreg[W_PER];

    auto load_A = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            int p = tid + i * NTHR;
            if (A_PIECES % NTHR == 0 || p < A_PIECES) {
                int row = p / K8, c8 = p % K8;
                areg[i] = *reinterpret_cast<const uint4*>(a.in + (size_t)(m0 + row) * Cin + chunk * KC + c8 * 8);
            }
        }
    };
    auto store_A = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            int p = tid + i * NTHR;
            if (A_PIECES % NTHR == 0 || p < A_PIECES) {
                int row = p / K8, c8 = p % K8;
                int b = row >> 6, px = row & 63;
                uint4 v = areg[i];
                int pix = (TAPS == 9) ? (b * 100 + ((px >> 3) + 1) * 10 + (px & 7) + 1) : row;
                *reinterpret_cast<uint4*>(A_lds + pix * AST + c8 * 8) = v;
            }
        }
    };
    auto load_W = [&](int step) {
        // step = chunk*TAPS + tap ; packed layout [tap][chunk][Npad][KC]
        int chunk = step / TAPS, tap = step % TAPS;
        const _Float16* src = a.w + ((size_t)(tap * nchunk + chunk) * Npad + n0) * KC;
#pragma unroll
        for (int i = 0; i < W_PER; ++i) {
            int p = tid + i * NTHR;
            if (W_PIECES % NTHR == 0 || p < W_PIECES)
                wreg[i] = *reinterpret_cast<const uint4*>(src + (size_t)p * 8);
        }
    };
    auto store_W = [&](int buf) {
#pragma unroll
        for (int i = 0; i < W_PER; ++i) {
            int p = tid + i * NTHR;
            if (W_PIECES % NTHR == 0 || p < W_PIECES) {
                int n = p / K8, k8 = p % K8;
                *reinterpret_cast<uint4*>(W_lds + buf * W_ELEMS + n * AST + k8 * 8) = wreg[i];
            }
        }
    };

    const int nsteps = nchunk * TAPS;
    load_A(0);
    load_W(0);
    for (int s = 0; s < nsteps; ++s) {
        const int chunk = s / TAPS, tap = s % TAPS;
        if (tap == 0) {
            if (s > 0) __syncthreads();   // previous chunk's reads of A_lds are done
            store_A(chunk);
        }
        store_W(s & 1);
        __syncthreads();
        if (s + 1 < nsteps) {
            load_W(s + 1);
            if ((s + 1) % TAPS == 0) load_A((s + 1) / TAPS);
        }
        const int tapoff = (TAPS == 9) ? ((tap / 3 - 1) * 10 + (tap % 3 - 1)) : 0;
        const _Float16* Wb = W_lds + (s & 1) * W_ELEMS + (wn * NT * 32 + (lane & 31)) * AST + khalf;
        static_for<0, KC / 16>([&](auto kk_) __attribute__((always_inline)) {
            constexpr int kk = decltype(kk_)::value;
            half8 af0 = *reinterpret_cast<const half8*>(A_lds + (apix[0] + tapoff) * AST + kk * 16 + khalf);
            half8 af1 = *reinterpret_cast<const half8*>(A_lds + (apix[1] + tapoff) * AST + kk * 16 + khalf);
            static_for<0, NT>([&](auto ni_) __attribute__((always_inline)) {
                constexpr int ni = decltype(ni_)::value;
                half8 bf = *reinterpret_cast<const half8*>(Wb + ni * 32 * AST + kk * 16);
                acc[0][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af0, bf, acc[0][ni], 0, 0, 0);
                acc[1][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af1, bf, acc[1][ni], 0, 0, 0);
            });
        });
    }

    // ---------------- epilogue (conv_epilogue.h) ----------------
    if constexpr (EPI == EPI_GN) {
        __syncthreads();                                  // every wave has left the operand tiles: the LDS becomes the staging images
        // destination of this wave's columns: columns from a.nsplit on are the second output's, from its column 0
        GemmArgs o = a;
        int out_col0 = 0;
        if (a.out2 != nullptr && n0 + wn * NT * 32 >= a.nsplit) { o.out = a.out2; o.ldo = a.ldo2; out_col0 = a.nsplit; }
        conv_tile_epilogue<EPI_GN, ACT, NT>(acc, o, smem + wave * (64 * 64 * NT), m0, n0, wm, wn, lane, out_col0);
    } else {
        conv_tile_epilogue<EPI_ELEMENT, ACT_NONE, NT>(acc, a, smem, m0, n0, wm, wn, lane);
    }
}

template <int TAPS, int WN, int NT, int KC>
static size_t conv_gemm_lds() {
    constexpr int NB = WN * NT * 32;
    constexpr int AST = KC + 8;
    constexpr int APIX = (TAPS == 9) ? 100 : 64;
    const size_t main_loop = (size_t)(4 * APIX * AST + 2 * NB * AST) * 2 + 64;
    const size_t staging = (size_t)WN * 4 * 64 * 64 * NT;          // EPI_GN: one [64 rows][32 NT] fp16 image per wave
    return main_loop > staging ? main_loop : staging;
}

template <int TAPS, int WN, int NT, int KC, ConvEpi EPI = EPI_ELEMENT, int ACT = ACT_NONE>
static hipError_t launch_conv_gemm_t(const GemmArgs& a, hipStream_t st) {
    constexpr int NB = WN * NT * 32;
    size_t lds = conv_gemm_lds<TAPS, WN, NT, KC>();
    static DeviceOnce once;
    hipError_t e = once.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_gemm_kernel<TAPS, WN, NT, KC, EPI, ACT>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    if (e != hipSuccess) return e;
    dim3 grid(a.Mrows / 256, a.Npad / NB);
    hipLaunchKernelGGL((conv_gemm_kernel<TAPS, WN, NT, KC, EPI, ACT>), grid, dim3(256 * WN), lds, st, a);
    return hipGetLastError();
}
// small tile with the fused GroupNorm epilogue: the stem (3x3, 64 channels per workgroup), one head conv (64 or 128 channels:
// the whole N in one workgroup, the input rows read once), or the policy-head and value-head convs together (64 + 128 channels,
// three wave groups, two outputs)
template <int ACT>
static hipError_t launch_conv_gemm_gn(const GemmArgs& a, int taps, hipStream_t st) {
    if (a.bias != nullptr || a.mul != nullptr || a.out_stats != nullptr || a.out_f32 || a.out_scale != 1.f || a.Npad != a.N)
        return hipErrorInvalidValue;
    // (stem: 64 channels per workgroup; a 160-channel tile -- two N blocks instead of five -- measured 1351 us against 711: 160
    // accumulator registers at one wave per SIMD)
    if (taps == 9) return a.Npad % 64 == 0 && a.out2 == nullptr ? launch_conv_gemm_t<9, 1, 2, 32, EPI_GN, ACT>(a, st) : hipErrorInvalidValue;
    if (a.posenc != nullptr) return hipErrorInvalidValue;
    if (a.out2 != nullptr) return a.Npad == 192 && a.nsplit == 64 ? launch_conv_gemm_t<1, 3, 2, 32, EPI_GN, ACT>(a, st) : hipErrorInvalidValue;
    if (a.Npad == 160) return launch_conv_gemm_t<1, 1, 5, 32, EPI_GN, ACT>(a, st);      // SSL head convs of the 320-wide trunk
    if (a.Npad == 128) return launch_conv_gemm_t<1, 2, 2, 32, EPI_GN, ACT>(a, st);
    if (a.Npad == 64) return launch_conv_gemm_t<1, 1, 2, 32, EPI_GN, ACT>(a, st);
    if (a.Npad == 32) return launch_conv_gemm_t<1, 1, 1, 32, EPI_GN, ACT>(a, st);
    return hipErrorInvalidValue;
}

hipError_t launch_conv_big(const GemmArgs& a, int taps, hipStream_t st);   // conv_big.hip
hipError_t launch_conv_zs(const GemmArgs& a, hipStream_t st);              // conv_zs.hip

int conv_gemm_tile_n(int Cin, int Npad) {
    return (Npad % 320 == 0 && Cin % 64 == 0) ? 320 : 32;
}
int conv_gemm_kc(int Cin, int Npad) {
    return (Npad % 320 == 0 && Cin % 64 == 0) ? 64 : 32;
}

hipError_t launch_conv_gemm(const GemmArgs& a, int taps, hipStream_t st) {
    if (a.Mrows % 256 != 0 || a.Cin % 32 != 0 || a.Npad % 32 != 0) return hipErrorInvalidValue;
    const bool big = conv_gemm_tile_n(a.Cin, a.Npad) == 320;
    if (a.gn_gamma != nullptr && !big) {                              // small tile with the fused GroupNorm epilogue
        if (a.epi_act == ACT_SILU) return launch_conv_gemm_gn<ACT_SILU>(a, taps, st);
        if (a.epi_act == ACT_RELU) return launch_conv_gemm_gn<ACT_RELU>(a, taps, st);
        return hipErrorInvalidValue;
    }
    if (taps == 9) {
        if (big) {
            if (!a.w_pp) return hipErrorInvalidValue;
            // conv_zs_kernel: the v_mfma_f32_16x16x32_f16 loop with the wave tile laid out so that the M-tiles that only see the
            // zero padding above / below the board are skipped (8.3 % of the MFMAs)
            return launch_conv_zs(a, st);
        }
        return launch_conv_gemm_t<9, 1, 1, 32>(a, st);
    } else if (taps == 1) {
        if (big) return a.w_pp ? hipErrorInvalidValue : launch_conv_big(a, 1, st);
        // Head convs over the whole trunk (M = 64 x boards, N = 64 / 128): a workgroup per 32 output channels re-reads its 256
        // trunk rows once per N block (168 MB x 2..4 at 4096 boards); 64 channels per workgroup halve that.
        // Same arithmetic per output element (bit-identical).  The FCs (M = boards) keep the narrow tile: they need the workgroups.
        // (64 channels per workgroup; 128 -- the whole value-head conv in one workgroup -- measured slower: 200 registers)
        if (a.Mrows / 256 >= 256 && a.Npad % 64 == 0) return launch_conv_gemm_t<1, 1, 2, 32>(a, st);
        return launch_conv_gemm_t<1, 1, 1, 32>(a, st);
    }
    return hipErrorInvalidValue;
}
