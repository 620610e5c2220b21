// conv_zs_kernel: the 3x3 320->320 implicit-GEMM conv of the tower with the zero padding SKIPPED.
//
// Workgroup: 8 waves, tile = 4 boards (256 rows) x 320 output channels, K walked as (64-channel chunk, tap) in half-tiles of 32 k.
// Wave (wp = wave >> 2, wn = wave & 3) owns the board PAIR wp x channels 80 wn .. 80 wn + 79: 8 x 5 accumulator tiles of
// v_mfma_f32_16x16x32_f16.  Why that shape: the main loop is POWER-bound, not issue-bound.  In-kernel stamps (tools/ubench,
// -DSW_STAMP, random operands, round 2, before the padding skip) showed this loop on 32x32x16 at 87.7 % of the MFMA issue rate but
// at 1.52-1.57 GHz; on 16x16x32 it spent more cycles (82 %) at 1.75-1.82 GHz and finished 5.6-7 % sooner: the chip holds a higher
// clock on this shape.
//
// M-tile mi = board row mi of both boards of the pair.  A 3x3 conv on an 8x8 board multiplies 92 of its 576 (square, tap)
// pairs by the zero padding; for the three taps with dy = -1 the operand of tile 0 is the padding row above both boards, for
// dy = +1 that of tile 7 the row below: those tiles' MFMAs and fragment reads are simply not issued -- 6 of the 72 (tap, tile)
// pairs, 8.3 % of the matrix work, results bit-identical (the skipped products are exact zeros).  Only the left / right padding
// column (one lane in eight) is still read from a zero region.  Per half-tile a wave reads 8 (7) activation fragments and 5 weight
// fragments and issues 40 (35) MFMAs.
//
// Fragments: lane l = (c15 = l & 15, q = l >> 4) holds k 8q .. 8q + 7 of the half-tile.  Activation fragment of tile mi: board
// c15 >> 3 of the pair, square 8 mi + (c15 & 7) shifted by the tap; weight fragment ni: output channel 80 wn + 16 ni + c15.
//
// LDS activation image: [256 rows = board * 64 + square][64 channels] fp16, 128-byte rows, 16-byte chunk index XOR
// key(row) = (column & 2) | (board parity << 2).  A ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31}, {32-35, 44-47, 52-59}, {36-43, 48-51, 60-63} (MI355X_MICROARCH.md, LDS): columns 0-3 of one board and 4-7 of the other with
// k-chunk q, the other halves with q ^ 1.  With this key the 16 lanes of every group touch 16 different bank quads for all
// three column shifts of a tap row (searched exhaustively; round 2's key ((column >> 1) & 3) was built for lanes 0-15 as one group
// and was 2-way conflicted for dx = -1 / +1: 31 % of the main loop's LDS cycles).  key does not change with the board row, so
// the 8 tiles of a tap are ONE base address plus immediate offsets mi * 1024.
// LDS weight half-tile: [320 channels][32 k] fp16, 64-byte rows, 16-byte chunk index XOR ((4 - (row >> 2)) & 3) (pack_gemm in
// net.hip): conflict-free for the weight fragment reads.
//
// DMA ring and barriers.  Half-tile y (NH = 18 Cin / 64 of them) lives in weight slot y & 3 of a four-slot ring; chunk c's
// activations in buffer c & 1.  Everything arrives by LDS-DMA (glds16) in 1-KiB pieces, wave-uniform addresses advanced
// incrementally.  In every half-tile every wave issues exactly THREE pieces of the half-tile three ahead: weight pieces wave and
// 8 + wave, then group 0 (waves 0-3) piece 16 + wave and group 1 (waves 4-7) one piece of the next chunk's activations (eight per
// wave and chunk) or, once those are out, a filler into the D region (past the last half-tile the weight pieces re-fetch it).
// The ring slot it fills held half-tile y - 1, which both groups have read.  Equal counts make one counted wait exact:
// `s_waitcnt vmcnt(3)` right after the issue leaves only those three pieces in flight, so the wave's pieces of half-tiles up to
// y + 2 have landed; a group reads half-tile y + 1 only after a barrier that the other group reaches after its own wait in
// half-tile y.  The prologue issues chunk 0 and half-tiles 0 .. 2 and waits with vmcnt(6).  Group 1 runs one barrier behind
// group 0 (an extra barrier after the prologue, matched by group 0 after the loop), so the two barriers of a half-tile (after
// the load section, after the MFMAs) alternate the groups: on every SIMD one wave issues its MFMAs while its partner (wave ^ 4)
// reads fragments and issues its DMA.  After the loop every wave drains its DMA (vmcnt(0)) and a last barrier frees the LDS for
// the epilogue's staging.
// (History: the 32x32x16 conv_pp_kernel of round 1 with the same ring is tools/ubench/conv_pp.hip.)
#include "kernel_common.h"
#include "conv_zs_epilogue.h"
#include "conv_zs_tail.h"

namespace {
constexpr int ZS_A_BYTES = 256 * 128;                 // 4 boards x 64 squares x 64 channels fp16
constexpr int ZS_WH_BYTES = 320 * 64;                 // 320 output channels x 32 k fp16, 64-byte rows
constexpr int ZS_OFF_W = 2 * ZS_A_BYTES;              // [4][WH_BYTES]  half-tile y in slot y & 3
constexpr int ZS_OFF_Z = ZS_OFF_W + 4 * ZS_WH_BYTES;  // zero region: 8 squares at 1-KiB stride (the tiles' immediate offsets)
constexpr int ZS_OFF_D = ZS_OFF_Z + 8192;             // [4][1024] sink of the filler DMA pieces
constexpr int ZS_LDS_MAIN = ZS_OFF_D + 4096;          // 159,744 B
}

#define ZS_FENCE() asm volatile("" ::: "memory")

#ifdef SW_STAMP
__device__ unsigned long long* g_zs_stamp;      // [blocks][4]: s_memtime / s_memrealtime at main-loop start and end
#endif

template <ConvEpi EPI, int ACT>
__global__ __launch_bounds__(512) void conv_zs_kernel(GemmArgs a) {
    constexpr int NG = 5, MT = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* A_lds = smem;                   // [2][A_BYTES]   chunk c in buffer c & 1
    char* W_lds = smem + ZS_OFF_W;
    char* Z_lds = smem + ZS_OFF_Z;
    char* D_lds = smem + ZS_OFF_D;

#ifdef SW_STAMP
    const unsigned long long st_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 3;              // channel quarter
    const int wp = wave >> 2;             // board pair of the tile = ping-pong group
    const int m0 = blockIdx.x * 256;
    const int n0 = blockIdx.y * 320;
    const int Cin = a.Cin;
    const int nchunk = Cin >> 6;
    const int NH = nchunk * 18;           // half-tiles
    const int c15 = lane & 15;
    const int q = lane >> 4;

    reinterpret_cast<uint4*>(Z_lds)[tid] = make_uint4(0, 0, 0, 0);          // 512 x 16 B = the whole zero region

    const char* in_bytes = reinterpret_cast<const char*>(a.in);
    const char* w_blk = reinterpret_cast<const char*>(a.w) + (size_t)blockIdx.y * (2 * ZS_WH_BYTES) + lane * 16;
    const size_t w_kt_stride = (size_t)gridDim.y * (2 * ZS_WH_BYTES);

    auto issue_A_piece = [&](int chunk, int qq) __attribute__((always_inline)) {
        const int p = 8 * qq + (lane >> 3);             // 1-KiB piece: rows 8qq..8qq+7 of the 256-row tile
        const int key = (p & 2) | (((p >> 6) & 1) << 2);
        const char* src = in_bytes + ((size_t)(m0 + p) * Cin + (size_t)chunk * 64) * 2 + 16 * ((lane & 7) ^ key);
        glds16(src, A_lds + (chunk & 1) * ZS_A_BYTES + qq * 1024);
    };
    auto issue_half = [&](int y) __attribute__((always_inline)) {      // prologue only
        const char* src = w_blk + (size_t)(y >> 1) * w_kt_stride + (size_t)(y & 1) * ZS_WH_BYTES;
        char* dst = W_lds + (y & 3) * ZS_WH_BYTES;
        glds16(src + wave * 1024, dst + wave * 1024);
        glds16(src + (8 + wave) * 1024, dst + (8 + wave) * 1024);
        if (wave < 4) glds16(src + (16 + wave) * 1024, dst + (16 + wave) * 1024);
        else glds16(w_blk, D_lds + (wave - 4) * 1024);   // filler: keeps 3 pieces per wave and half-tile (vmcnt)
    };

    float4v acc[MT][NG];
    static_for<0, MT>([&](auto mi) __attribute__((always_inline)) {
        static_for<0, NG>([&](auto ni) __attribute__((always_inline)) {
            acc[decltype(mi)::value][decltype(ni)::value] = float4v{0.f, 0.f, 0.f, 0.f};
        });
    });

    // per-lane constants of the fragment reads
    const int wfx = ((4 - ((c15 >> 2) & 3)) & 3) ^ q;                   // weight rows (64 B): chunk q ^ swizzle key
    const int wrow_off = (wn * 80 + c15) * 64;
    const int lx = c15 & 7;                                             // board column of this lane's A-operand rows
    const int lb = c15 >> 3;                                            // board of the pair
    const int arow0 = (2 * wp + lb) * 64 + lx;                          // tile row of (board, y = 0, x)

    // ---- prologue: chunk 0 activations, half-tiles 0..2 ----
#pragma unroll
    for (int i = 0; i < 4; ++i) issue_A_piece(0, wave * 4 + i);
    issue_half(0);
    issue_half(1);
    issue_half(2);
    // only the activations and half-tile 0 have to be there for the first load section; half-tiles 1 and 2 (6 pieces per wave)
    // stay in flight and are retired by the loop's own counted waits.  Raw barrier: __syncthreads() would drain the DMA queue.
    asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wp == 1) __builtin_amdgcn_s_barrier();          // group 1 runs one barrier behind group 0

    // ---- steady-state DMA (wave-uniform state, advanced incrementally; the ring is described in the header) ----
    const uint32_t w_lane = (uint32_t)lane * 16u;
    // activation piece qq = 4 xi + wave - 4 (xi = 0..7): rows 32 xi + 8 (wave - 4) + (lane >> 3); key = ((lane >> 3) & 2) | (xi & 2) << 1
    const uint32_t a_lane0 = (uint32_t)(lane >> 3) * (uint32_t)Cin * 2u + 16u * (uint32_t)((lane & 7) ^ ((lane >> 3) & 2));
    const uint32_t a_lane1 = (uint32_t)(lane >> 3) * (uint32_t)Cin * 2u + 16u * (uint32_t)((lane & 7) ^ (((lane >> 3) & 2) | 4));
    const char* w_base = reinterpret_cast<const char*>(a.w) + (size_t)blockIdx.y * (2 * ZS_WH_BYTES) + wave * 1024;  // uniform
    int t_next = 3;
    const char* w_ptr = w_base + (size_t)1 * w_kt_stride + ZS_WH_BYTES;     // half-tile 3 = K-tile 1, half 1
    int w_slot = 3 * ZS_WH_BYTES;
    const char* a_ptr = in_bytes;
    int a_dst = 0, a_left = 0;
    auto issue_next = [&](auto G_) __attribute__((always_inline)) {
        constexpr int G = decltype(G_)::value;
        char* dst = W_lds + w_slot + wave * 1024;
        glds16(w_ptr + w_lane, dst);
        glds16(w_ptr + 8192 + w_lane, dst + 8192);
        if constexpr (G == 0) {
            glds16(w_ptr + 16384 + w_lane, dst + 16384);
        } else {
            const bool have = a_left > 0;
            const uint32_t al = ((8 - a_left) & 2) ? a_lane1 : a_lane0;     // pieces 2, 3, 6, 7 of this wave: odd boards
            glds16((have ? a_ptr : in_bytes) + al, have ? A_lds + a_dst : D_lds + (wave - 4) * 1024);
            a_ptr += have ? (size_t)32 * Cin * 2 : 0;
            a_dst += have ? 4096 : 0;
            a_left -= have ? 1 : 0;
        }
        const bool more = t_next + 1 < NH;
        const size_t inc = (t_next & 1) ? (w_kt_stride - ZS_WH_BYTES) : (size_t)ZS_WH_BYTES;   // odd -> even: next K-tile
        w_ptr += more ? inc : 0;
        t_next += 1;
        w_slot = (t_next & 3) * ZS_WH_BYTES;
    };

    int y = 0;
#ifdef SW_STAMP
    const unsigned long long st_c0 = __builtin_amdgcn_s_memtime(), st_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    auto main_loop = [&](auto G_) __attribute__((always_inline)) {
    constexpr int G = decltype(G_)::value;
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        const char* Ab = A_lds + (c & 1) * ZS_A_BYTES;
        if constexpr (G == 1) {                          // this wave's 8 pieces of the next chunk's activations
            a_left = c + 1 < nchunk ? 8 : 0;
            a_ptr = in_bytes + ((size_t)(m0 + 8 * (wave - 4)) * Cin + (size_t)(c + 1) * 64) * 2;
            a_dst = ((c + 1) & 1) * ZS_A_BYTES + (wave - 4) * 1024;
        }
        static_for<0, 3>([&](auto t3_) __attribute__((always_inline)) {
            constexpr int t3 = decltype(t3_)::value;     // dy = t3 - 1
            constexpr int LO = t3 == 0 ? 1 : 0;          // first / one-past-last M-tile with an operand on the board
            constexpr int HI = t3 == 2 ? 7 : 8;
            // row of tile LO's operand for dx = -1:  dy = -1: tile 1 reads board row 0;  dy = 0: tile 0 row 0;  dy = +1: tile 0 row 1
            const int rbase = arow0 + (t3 == 2 ? 8 : 0) - 1;
#pragma unroll 1
            for (int dxi = 0; dxi < 3; ++dxi) {
                const int xx = lx + dxi - 1;
                const bool ok = (unsigned)xx < 8u;
                // a lane beside the board reads zeros at the bank slot the wrapped column (x + 8 / x - 8) would have used: the 16
                // lanes of a read group then touch 16 different slots for every tap
                const int key = (xx & 2) | (lb << 2);
                const char* rowp = ok ? Ab + (rbase + dxi) * 128 : Z_lds + (xx & 1) * 128;
                const char* ap0 = rowp + 16 * (key ^ q);
                const char* ap1 = rowp + 16 * (key ^ q ^ 4);
                static_for<0, 2>([&](auto h_) __attribute__((always_inline)) {
                    constexpr int h = decltype(h_)::value;
                    const int yh = y + h;
                    const char* ap = h ? ap1 : ap0;
                    half8 fa[MT], fb[NG];
                    const char* Wb = W_lds + (yh & 3) * ZS_WH_BYTES + wrow_off + 16 * wfx;
                    static_for<LO, HI>([&](auto mi_) __attribute__((always_inline)) {
                        constexpr int mi = decltype(mi_)::value;
                        fa[mi] = *reinterpret_cast<const half8*>(ap + (mi - LO) * 1024);
                    });
                    static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
                        constexpr int ni = decltype(ni_)::value;
                        fb[ni] = *reinterpret_cast<const half8*>(Wb + ni * 1024);
                    });
                    // This wave's share of the half-tile three ahead goes out HERE, in the load section (which has ~300 cycles of slack
                    // under the partner group's 40 MFMAs), not between this wave's own MFMAs: an LDS-DMA instruction takes 40-60
                    // cycles to issue, and in the compute section the SIMD's matrix pipe idles for them (three per half-tile: the
                    // main loop was 127.4 k cycles per tile with the DMA after the second channel tile's MFMAs, 113.4 k here; the
                    // chip gives part of it back as clock, 1.81 -> 1.71 GHz: -4 % wall).  The slot's previous tenant (the
                    // half-tile before this one) was read into registers by both wave groups at least a phase ago.
                    ZS_FENCE(); issue_next(G_); ZS_FENCE();
                    // all but this wave's three youngest pieces (the ones just issued) have landed
                    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                    ZS_FENCE();
                    __builtin_amdgcn_s_barrier();
                    ZS_FENCE();
                    __builtin_amdgcn_s_setprio(1);
                    static_for<0, NG>([&](auto ni_) __attribute__((always_inline)) {
                        constexpr int ni = decltype(ni_)::value;
                        static_for<LO, HI>([&](auto mi_) __attribute__((always_inline)) {
                            constexpr int mi = decltype(mi_)::value;
                            // operand order = accumulator layout (conv_zs_epilogue.h): weights as A for the plain / GroupNorm epilogues
                            // (a lane gets 4 consecutive channels of a square), activations as A for the fused tail
                            if constexpr (EPI == EPI_TAIL || EPI == EPI_TAIL_PRE)
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
                            else
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[ni], fa[mi], acc[mi][ni], 0, 0, 0);
                        });
                    });
                    __builtin_amdgcn_s_setprio(0);
                    ZS_FENCE();
                    __builtin_amdgcn_s_barrier();
                    ZS_FENCE();
                });
                y += 2;
            }
        });
    }
    };
    if (wp == 0) main_loop(std::integral_constant<int, 0>{});
    else main_loop(std::integral_constant<int, 1>{});
#ifdef SW_STAMP
    if (tid == 0) {
        unsigned long long* o = g_zs_stamp + (size_t)blockIdx.x * 4;
        o[0] = st_c0; o[1] = st_r0; o[2] = __builtin_amdgcn_s_memtime(); o[3] = __builtin_amdgcn_s_memrealtime();
    }
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's tail refetches / fillers have landed
    if (wp == 0) __builtin_amdgcn_s_barrier();          // matches group 1's extra barrier
    __builtin_amdgcn_s_barrier();                       // every wave's DMA has landed before anyone stages output (header)

    if constexpr (EPI == EPI_TAIL) zs_tail_epilogue<ACT, false>(acc, a, smem, m0, wp, wn, wave, lane);
    else if constexpr (EPI == EPI_TAIL_PRE) zs_tail_epilogue<ACT, true>(acc, a, smem, m0, wp, wn, wave, lane);
    else zs_tile_epilogue<EPI, ACT>(acc, a, smem + wave * 20480, m0, n0, wp, wn, lane);
#ifdef SW_STAMP     // timeline of the workgroup (10-ns ticks, wave 0) and where it ran: [blocks][4] behind the main-loop stamps
    if (tid == 0) {
        unsigned long long* o = g_zs_stamp + (size_t)gridDim.x * 4 + (size_t)blockIdx.x * 4;
        unsigned hw; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        unsigned xcc; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        o[0] = st_entry; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = hw; o[3] = xcc;
    }
#endif
}

template <ConvEpi EPI, int ACT>
static hipError_t launch_conv_zs_e(const GemmArgs& a, hipStream_t st) {
    const size_t lds = 160 * 1024;     // main loop 159,744 B; the epilogue stages the whole tile (8 x 20 KiB)
    static DeviceOnce once;             // the attribute is per device: a process may drive several GPUs (arena, tests)
    hipError_t e = once.run([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_zs_kernel<EPI, ACT>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    if (e != hipSuccess) return e;
    dim3 grid(a.Mrows / 256, a.Npad / 320);
    hipLaunchKernelGGL((conv_zs_kernel<EPI, ACT>), grid, dim3(512), lds, st, a);
    return hipGetLastError();
}

// 3x3 only; a.w must be in the half-tile layout (GemmArgs::w_pp).
hipError_t launch_conv_zs(const GemmArgs& a, hipStream_t st) {
    if (a.Cin % 64 != 0 || a.Npad % 320 != 0 || a.Mrows % 256 != 0) return hipErrorInvalidValue;
    if (a.mul != nullptr || a.out_f32 != 0) return hipErrorInvalidValue;      // 3x3 convs never use these
    if ((size_t)a.Mrows * a.ldo * 2 >= ((size_t)1 << 32)) return hipErrorInvalidValue;   // 32-bit store offsets
    if (a.res != nullptr) {                     // conv2 of a block with the block's tail fused (conv_zs_tail.h)
        if (a.N != 320 || a.Npad != 320 || a.ldo != 320 || a.bias != nullptr || a.out_stats != nullptr) return hipErrorInvalidValue;
        if (a.y2 != nullptr && a.gn_gamma == nullptr) return hipErrorInvalidValue;
        if (a.se_w1 != nullptr && (a.se_wf == nullptr || a.se_hidden < 1 || a.se_hidden > TAIL_SE_HMAX)) return hipErrorInvalidValue;
        if (a.pre_gamma != nullptr) {               // x += act(norm(conv(x))) (chess-feature conv) + next GroupNorm
            if (a.se_w1 != nullptr) return hipErrorInvalidValue;
            if (a.epi_act == ACT_SILU) return launch_conv_zs_e<EPI_TAIL_PRE, ACT_SILU>(a, st);
            if (a.epi_act == ACT_RELU) return launch_conv_zs_e<EPI_TAIL_PRE, ACT_RELU>(a, st);
            return hipErrorInvalidValue;
        }
        if (a.epi_act == ACT_SILU) return launch_conv_zs_e<EPI_TAIL, ACT_SILU>(a, st);
        if (a.epi_act == ACT_RELU) return launch_conv_zs_e<EPI_TAIL, ACT_RELU>(a, st);
        return hipErrorInvalidValue;
    }
    if (a.gn_gamma != nullptr) {                // conv1 of a block: GroupNorm + the network activation
        if (a.epi_act == ACT_SILU) return launch_conv_zs_e<EPI_GN, ACT_SILU>(a, st);
        if (a.epi_act == ACT_RELU) return launch_conv_zs_e<EPI_GN, ACT_RELU>(a, st);
        return hipErrorInvalidValue;
    }
    return a.epi_act == ACT_NONE ? launch_conv_zs_e<EPI_PLAIN, ACT_NONE>(a, st) : hipErrorInvalidValue;
}
