// attn_block_kernel: one whole ChessAttention block of the tower (resnet.py:133-181: qkv 1x1 -> per-head
// scores / softmax / PV -> proj 1x1 -> residual add -> LayerNorm) plus the pre-activation GroupNorm of the residual
// block that follows, in ONE kernel for the 320-channel trunk.
//
// Why: as four kernels (qkv GEMM, attn_core, proj GEMM, ew_board) the block moved 2.5 GB through HBM per launch at
// 4096 boards -- the [B][64][960] qkv tensor alone is written and read back (1 GB) -- and took 856 us against 310 us of
// traffic; here only the trunk is read (168 MB) and the outputs are written.
//
// Workgroup = 2 boards = 128 token rows, 8 waves.  The boards' trunk rows X [128][320] stay in LDS for the whole
// kernel (A operand of every qkv GEMM and the residual at the end).  The 20 heads are processed in 10 groups of 2:
//   1. qkv GEMM of the group  [128 x 320] x [320 x 96]   (96 = q,k,v of 2 heads; 5 weight pieces of K = 64)
//      -> Q, K as [head][token][16] and V transposed [unit][16][token] in LDS (fp16, as the split path's qkv tensor);
//   2. attention of the 4 (board, head) units, one per wave pair (a wave owns 32 queries): S^T = K Q^T and
//      O^T = V^T P^T on MFMA 32x32x16, the arithmetic of attn_math.h that attn_core_kernel runs too; the relative-position
//      bias of the wave's (head, query half) arrives in registers from a table pre-arranged in accumulator order; O overwrites Q;
//   3. proj GEMM accumulate  out[128 x 320] += O[128 x 32] x Wproj[32 x 320]  (2 weight pieces) into 80 accumulator
//      registers per lane that live across all groups (a wave owns 16 tokens x all 320 channels, so LayerNorm needs no
//      cross-wave reduction and GroupNorm group j is accumulator tile j).
// All GEMM tiles are MFMA 16x16x32 in the "swapped" orientation (A = weights, B = activations): the accumulator then
// holds 4 consecutive channels of one token per lane = one 8-byte LDS write.
// The weights of the whole block are one stream of 70 pieces of 12 KB (host-packed in LDS image order, net.hip)
// through a 4-slot ring filled by global_load_lds (two DMA instructions per wave and piece, so every wave's vmcnt
// bookkeeping is identical); one barrier per piece.  The proj pieces of a group are consumed together with the qkv pieces
// of the next one as one software-pipelined sequence: the fragments of the next half-piece are read from LDS (untracked
// inline-asm reads, counted lgkmcnt waits) while the MFMAs of the current one issue.
// A workgroup walks the board pairs b, b + grid, b + 2 grid, ... (grid = the CU count unless the caller caps it: LDS holds one
// workgroup per CU).  Only the first pair's rows arrive by LDS-DMA with nothing to overlap them; every later pair's rows are
// requested into registers as soon as the accumulators are dead (after the LayerNorm), travel under the rest of the epilogue
// and are written to the X image at the top of the next pass.
#include "attn_math.h"
#include "conv_epilogue.h"

typedef float float4v __attribute__((ext_vector_type(4)));

namespace {
constexpr int AB_PIECE = 12288;
constexpr int AB_PIECES_PER_GROUP = 7;
constexpr int AB_GROUPS = 10;
constexpr int AB_X = 0;                                   // [128][640 B], 16-byte chunk ^ (row>>1)&7 within 128 B
constexpr int AB_QK = 81920;                              // Q [2][128][16] | K [2][128][16]   (O overlays Q); a token's two 16-byte
                                                          // halves are stored at half ^ (token >> 3 & 1): conflict-free ds_read_b128 of
                                                          // 32 consecutive tokens, the staging's 8-byte writes 2-way instead of 4-way
constexpr int AB_VT = AB_QK + 16384;                      // [4 units][16][68]
constexpr int AB_VROW = 68;
constexpr int AB_RING = AB_VT + 4 * 16 * AB_VROW * 2;     // 107008
constexpr int AB_PAR = AB_RING + 4 * AB_PIECE;            // 156160: LayerNorm gamma, beta, next GroupNorm gamma, beta [4][320] f32
constexpr int AB_LDS = AB_PAR + 4 * 320 * 4;              // 161280

// What a lane knows about its place: built once, read by every phase.
struct AbLane {
    int tid, lane, w;                      // w = wave, wave-uniform
    int l15, lq, r31, half;                // lane & 15, lane >> 4, lane & 31, lane >> 5
    int wm, wn;                            // GEMM role: token rows 32 wm .. 32 wm + 31, column half wn
    uint32_t xa[2];                        // X rows 32 wm + l15 (and + 16 * 640: 32 wm + 16 + l15), k-step 0 / 1
    int wq0, wq1, wpo;                     // this lane's offset in a qkv piece (k-step 0 / 1) and in a proj piece
    uint32_t ring_a, of_a;                 // the ring; this wave's O rows (proj operand)
    const char* wsrc;                      // this lane's 16 bytes of piece 0 in global memory
    char* ring_w;                          // this wave's 1.5 KB of ring slot 0
    // attention role: unit au = (board, head-in-group), query aq of the board
    int au, aboard, ahl, aqt, aq;
};
// Registers that live across phases; every index into them is a compile-time constant (kernel_common.h).
struct AbRegs {
    float4v oc[20];                        // block output: 16 tokens x 320 channels per wave, across all groups
    float4v qa[2][3];                      // qkv of the current group
    half8 fs[2][5];                        // the two fragment sets of the pipelined sequence
    half8 of;                              // this wave's O rows, B operand of the proj tiles
    half8 bias8[4];                        // relative-position bias of (head, query half), accumulator order
    half2v visp[16];                       // visibility of key (kt, r) from query aq as a multiplicand, accumulator order: key =
                                           // kt*32 + 8(r>>2) + 4 half + (r&3)  (fp16 pairs: 16 registers; the products take them
                                           // as the fp16 operand of a mixed-precision FMA)
};
// The next pair on its way through registers: this lane's ten 16-byte chunks of the X image and (threads 0-319) its four
// values of the parameter table.  Alive from the LayerNorm of one pair to the top of the next, while AbRegs is dead.
struct AbNext {
    half8 x[10];
    float par[4];
};
}

// 64 bytes per lane from global memory that the compiler does not track (the caller waits: vmcnt)
__device__ __forceinline__ void ab_load64(half8& b0, half8& b1, half8& b2, half8& b3, const half8* p) {
    asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %4, off offset:16\n\t"
                 "global_load_dwordx4 %2, %4, off offset:32\n\tglobal_load_dwordx4 %3, %4, off offset:48"
                 : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3) : "v"(p) : "memory");
}
// 16 / 4 bytes per lane from `base` (wave-uniform) + `off`, untracked as well
__device__ __forceinline__ void ab_gload16(half8& d, int off, const void* base) {
    asm volatile("global_load_dwordx4 %0, %1, %2" : "+v"(d) : "v"(off), "s"(base) : "memory");
}
__device__ __forceinline__ void ab_gload4(float& d, int off, const void* base) {
    asm volatile("global_load_dword %0, %1, %2" : "+v"(d) : "v"(off), "s"(base) : "memory");
}
// LDS stores the compiler does not track (before an ordinary one hipcc drains every LDS-DMA in flight and reorders freely
// around s_barrier)
template <int OFF>
__device__ __forceinline__ void ab_lds_store16(uint32_t addr, const half8& v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(addr), "v"(v), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void ab_lds_store4(uint32_t addr, float v) {
    asm volatile("ds_write_b32 %0, %1 offset:%2" :: "v"(addr), "v"(v), "n"(OFF) : "memory");
}
// one 16-byte LDS read the compiler does not track (the caller waits: lgkmcnt)
template <int OFF>
__device__ __forceinline__ void ab_lds16(half8& d, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
// ... and the wait: at most N younger LDS reads outstanding; the operands tie their first use to this point
template <int N>
__device__ __forceinline__ void ab_lds_arrived(half8& f0, half8& f1, half8& f2, half8& f3, half8& f4, half8& f5) {
    static_assert(N == 0 || N == 5, "");
    if constexpr (N == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3), "+v"(f4), "+v"(f5) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(5)" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3), "+v"(f4), "+v"(f5) :: "memory");
}
template <int CTRL>
__device__ __forceinline__ float ab_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum over the 16 lanes of a DPP row (every lane gets the total; fixed order)
__device__ __forceinline__ float ab_row_sum(float v) {
    v += ab_dpp<0xB1>(v);      // quad_perm [1,0,3,2]
    v += ab_dpp<0x4E>(v);      // quad_perm [2,3,0,1]
    v += ab_dpp<0x141>(v);     // row_half_mirror
    v += ab_dpp<0x140>(v);     // row_mirror
    return v;
}

// AB_WAIT(4) = all but this wave's two youngest pieces have landed.  Only LDS-DMA operations may be outstanding at a
// counted wait: loads into registers and loads into LDS do not retire in one order (measured: a later DMA retired
// before an earlier register load and vmcnt(1) let a wave read its bias registers early), so a count over both kinds
// proves nothing about either.  The bias loads are therefore issued after a sequence's last counted wait and
// waited for with vmcnt(0).
#define AB_WAIT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define AB_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// The workgroup's LDS (map: AB_X .. AB_LDS).  Every phase names the array itself: handed down as a pointer in AbLane it reached
// the optimizer without its address space (seen: the parameter table's stores stayed in order with the global loads around them).
__device__ __forceinline__ char* ab_smem() {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    return smem;
}

__device__ __forceinline__ AbLane ab_lane(const AttnBlockArgs& a) {
    AbLane L;
    L.tid = threadIdx.x; L.lane = L.tid & 63;
    L.w = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    L.l15 = L.lane & 15; L.lq = L.lane >> 4; L.r31 = L.lane & 31; L.half = L.lane >> 5;
    L.wm = L.w >> 1; L.wn = L.w & 1;
    const int l15 = L.l15, lq = L.lq, w = L.w;
    const int xrow0 = 32 * L.wm + l15;
    const int xsw = (xrow0 >> 1) & 7;
    const int xe0 = ((lq ^ xsw) & 7) * 16, xe1 = (((4 + lq) ^ xsw) & 7) * 16;
    const uint32_t lds0 = (uint32_t)(uintptr_t)ab_smem();
    L.xa[0] = lds0 + AB_X + xrow0 * 640 + xe0; L.xa[1] = lds0 + AB_X + xrow0 * 640 + xe1;
    const int wsw = (l15 >> 1) & 7;
    L.wq0 = (3 * L.wn * 16 + l15) * 128 + ((lq ^ wsw) & 7) * 16;
    L.wq1 = (3 * L.wn * 16 + l15) * 128 + (((4 + lq) ^ wsw) & 7) * 16;
    // proj piece: 64-byte rows; a ds_read_b128 is served in lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (one row
    // quad of lq = 0 / 2 next to two of lq = 1 / 3): chunk ^ (4 - quad) & 3 gives the 16 lanes of a group 16 different bank quads
    L.wpo = l15 * 64 + ((lq ^ (4 - (l15 >> 2))) & 3) * 16;
    L.ring_a = lds0 + AB_RING;
    L.of_a = lds0 + AB_QK + (lq >> 1) * 4096 + (16 * w + l15) * 32 + ((lq & 1) ^ (l15 >> 3)) * 16;
    L.wsrc = reinterpret_cast<const char*>(a.wpack) + w * 1536 + L.lane * 16;
    L.ring_w = ab_smem() + AB_RING + w * 1536;
    L.au = w >> 1; L.aboard = L.au >> 1; L.ahl = L.au & 1; L.aqt = w & 1;
    L.aq = L.aqt * 32 + L.r31;
    return L;
}

// L is built once, but what the phases derive from it must not outlive a pass: with the pair loop around them hipcc forms every
// pair-independent per-lane value (the 64-bit source address of each weight piece with a constant index, the staging and
// attention addresses, the epilogue's) in front of the loop and holds it across all phases; there are no registers for that
// (seen: 31 to 161 spilled, the next pair's rows among them).  No instruction: the fields stay where they are, the optimizer
// just cannot see through them.
__device__ __forceinline__ void ab_per_pass(AbLane& L) {
    asm volatile("" : "+v"(L.lane), "+v"(L.l15), "+v"(L.lq), "+v"(L.r31), "+v"(L.half), "+v"(L.aq), "+v"(L.xa[0]), "+v"(L.xa[1]),
                      "+v"(L.wq0), "+v"(L.wq1), "+v"(L.wpo), "+v"(L.of_a), "+v"(L.wsrc));
}
// DMA weight piece t into its ring slot.
// A piece is 12 x 1 KB: every wave issues one full 16-byte DMA and one with its upper 32 lanes masked off (1.5 KB per
// wave), so the count of outstanding vector-memory operations is the same in all 8 waves.  (global_load_lds_dwordx3
// would give 16 x 768 B, but on gfx950 it places lane i's 12 bytes at base + 16 i.  Twelve full instructions -- waves 0-3
// two, waves 4-7 one, with per-wave wait counts -- measured the same or slower.)
// The lane test is opaque and each call has its own: given one condition under several calls in a row, hipcc joins their
// branches and moves the full DMAs between them into the two arms (seen at the top of the pair loop) -- lanes of one
// instruction then carry different pieces, while the LDS destination (M0) is one per wave, taken from the first lane.
__device__ __forceinline__ void ab_issue(const AbLane& L, int t) {
    const char* s = L.wsrc + (size_t)t * AB_PIECE;
    char* d = L.ring_w + (t & 3) * AB_PIECE;
    glds16(s, d);
    int lane = L.lane;
    asm volatile("" : "+v"(lane));
    if (lane < 32) glds16(s + 1024, d + 1024);
}

// The X image is filled in 16-byte chunks: lane l of wave w, piece n owns chunk q = (10 w + n) 64 + l at AB_X + 16 q.
// Byte offset in the pair's rows of the chunk that belongs there (the image's swizzle applied on the way in).
__device__ __forceinline__ int ab_x_source(const AbLane& L, int n) {
    const int q = (L.w * 10 + n) * 64 + L.lane;
    const int row = q / 40, pos = q - row * 40;
    const int src = (pos & ~7) | ((pos ^ (row >> 1)) & 7);
    return row * 640 + src * 16;
}
__device__ __forceinline__ const char* ab_pair_rows(const AttnBlockArgs& a, int pair) {
    return reinterpret_cast<const char*>(a.x) + (size_t)pair * (128 * 640);
}

// the first pair's rows, the first three weight pieces and the parameter table
__device__ __forceinline__ void ab_prologue(const AttnBlockArgs& a, const AbLane& L, int pair) {
    const char* xg = ab_pair_rows(a, pair);
#pragma unroll
    for (int n = 0; n < 10; ++n) glds16(xg + ab_x_source(L, n), ab_smem() + AB_X + (L.w * 10 + n) * 1024);
    ab_issue(L, 0); ab_issue(L, 1); ab_issue(L, 2);
    const int tid = L.tid;
    if (tid < 320) {
        float* par = reinterpret_cast<float*>(ab_smem() + AB_PAR);
        par[tid] = a.ln_g[tid]; par[320 + tid] = a.ln_b[tid];
        par[640 + tid] = a.y2 ? a.gn2_gamma[tid] : 0.f; par[960 + tid] = a.y2 ? a.gn2_beta[tid] : 0.f;
    }
}

// N's registers are given a definition on every path of a pass (no instruction): defined only where a next pair exists, they
// reach the loop's head as "maybe defined" and hipcc keeps all 44 alive around the whole loop (seen: every one spilled).
__device__ __forceinline__ void ab_define_next(AbNext& N) {
    asm volatile("" : "=v"(N.x[0]), "=v"(N.x[1]), "=v"(N.x[2]), "=v"(N.x[3]), "=v"(N.x[4]), "=v"(N.x[5]), "=v"(N.x[6]), "=v"(N.x[7]),
                      "=v"(N.x[8]), "=v"(N.x[9]), "=v"(N.par[0]), "=v"(N.par[1]), "=v"(N.par[2]), "=v"(N.par[3]));
}
// Request the next pair: ten 16-byte loads per lane and, where ab_second_output overwrites the parameter table (y2), the
// lane's four parameters.  Inline asm the compiler does not track: an ordinary load would be drained (vmcnt(0)) at whatever
// point hipcc places its first use.  Issued after the AB_WAIT(0) that ends a pair's sequences, retired by ab_next_arrived
// before the next pair's first DMA: no counted wait ever sees them (see AB_WAIT).
__device__ __forceinline__ void ab_request_next(const AttnBlockArgs& a, const AbLane& L, int pair, AbNext& N) {
    const char* xg = ab_pair_rows(a, pair);
    static_for<0, 10>([&](auto n_) __attribute__((always_inline)) {
        constexpr int n = decltype(n_)::value;
        ab_gload16(N.x[n], ab_x_source(L, n), xg);
    });
    if (a.y2 != nullptr && L.w < 5) {
        const int po = L.tid * 4;
        ab_gload4(N.par[0], po, a.ln_g); ab_gload4(N.par[1], po, a.ln_b);
        ab_gload4(N.par[2], po, a.gn2_gamma); ab_gload4(N.par[3], po, a.gn2_beta);
    }
}
// Top of every pass but the first.  All waves have left the X image, the parameter table and the GroupNorm scratch in the
// ring (barrier); the requested rows and this wave's flush stores have retired (vmcnt(0); the operands tie the registers
// to this point); the rows and parameters go to LDS; the first three weight pieces start.  ab_sequence's opening
// lgkmcnt(0) + barrier makes the image visible to all waves.
__device__ __forceinline__ void ab_next_arrived(const AttnBlockArgs& a, const AbLane& L, AbNext& N) {
    AB_LGKM0();
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(N.x[0]), "+v"(N.x[1]), "+v"(N.x[2]), "+v"(N.x[3]), "+v"(N.x[4]), "+v"(N.x[5]), "+v"(N.x[6]), "+v"(N.x[7]),
                   "+v"(N.x[8]), "+v"(N.x[9]), "+v"(N.par[0]), "+v"(N.par[1]), "+v"(N.par[2]), "+v"(N.par[3]) :: "memory");
    const uint32_t lds0 = (uint32_t)(uintptr_t)ab_smem();
    const uint32_t xd = lds0 + AB_X + L.w * 10240 + L.lane * 16;
    static_for<0, 10>([&](auto n_) __attribute__((always_inline)) {
        constexpr int n = decltype(n_)::value;
        ab_lds_store16<n * 1024>(xd, N.x[n]);
    });
    if (a.y2 != nullptr && L.w < 5) {
        const uint32_t pd = lds0 + AB_PAR + L.tid * 4;
        static_for<0, 4>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            ab_lds_store4<i * 1280>(pd, N.par[i]);
        });
    }
    ab_issue(L, 0); ab_issue(L, 1); ab_issue(L, 2);
}

__device__ __forceinline__ void ab_visibility(const AttnBlockArgs& a, const AbLane& L, half2v (&visp)[16]) {
    const uint64_t m = a.mask[L.aq];
    static_for<0, 32>([&](auto i_) __attribute__((always_inline)) {
        constexpr int i = decltype(i_)::value;
        constexpr int kt = i >> 4, r = i & 15;
        const int key = kt * 32 + 8 * (r >> 2) + 4 * L.half + (r & 3);
        visp[i >> 1][i & 1] = (_Float16)(float)((m >> key) & 1);
    });
}

__device__ __forceinline__ void ab_zero_qa(float4v (&qa)[2][3]) {
    const float4v zero4 = {0.f, 0.f, 0.f, 0.f};
    static_for<0, 2>([&](auto i_) __attribute__((always_inline)) {
        static_for<0, 3>([&](auto j_) __attribute__((always_inline)) { qa[decltype(i_)::value][decltype(j_)::value] = zero4; });
    });
}

// The pieces of a sequence are consumed in two halves each (one k-step of the qkv GEMM / 80 output channels of the proj);
// half U = piece T + (U >> 1), fragment set U & 1.  HP: the sequence starts with the two proj pieces of the previous group.
// (fragment reads are inline asm with counted lgkmcnt waits: after any inline asm hipcc's own waits are
// lgkmcnt(0), which would put every half's reads in front of the MFMAs of the half before it again)
template <bool HP, int U>
__device__ __forceinline__ void ab_load(const AbLane& L, AbRegs& R, const int T) {
    constexpr int S = U & 1, i = U >> 1, kk = U & 1;
    const uint32_t slot = L.ring_a + (uint32_t)(((T + i) & 3) * AB_PIECE);
    if constexpr (HP && i < 2) {
        if constexpr (U == 0) ab_lds16<0>(R.of, L.of_a);
        const uint32_t pa = slot + L.wpo;
        static_for<0, 5>([&](auto jj_) __attribute__((always_inline)) {
            constexpr int jj = decltype(jj_)::value;
            ab_lds16<(5 * kk + jj) * 1024>(R.fs[S][jj], pa);
        });
    } else {
        constexpr int p = i - (HP ? 2 : 0);
        ab_lds16<128 * p>(R.fs[S][3], L.xa[kk]);
        ab_lds16<128 * p + 16 * 640>(R.fs[S][4], L.xa[kk]);
        const uint32_t wa = slot + (kk ? L.wq1 : L.wq0);
        static_for<0, 3>([&](auto j_) __attribute__((always_inline)) {
            constexpr int j = decltype(j_)::value;
            ab_lds16<j * 2048>(R.fs[S][j], wa);
        });
    }
}
// the set of half U is in registers once at most N younger LDS reads are outstanding
template <int U, int N>
__device__ __forceinline__ void ab_arrived(AbRegs& R) {
    constexpr int S = U & 1;
    ab_lds_arrived<N>(R.fs[S][0], R.fs[S][1], R.fs[S][2], R.fs[S][3], R.fs[S][4], R.of);
}
template <bool HP, int U>
__device__ __forceinline__ void ab_mma(AbRegs& R) {
    constexpr int S = U & 1, i = U >> 1, kk = U & 1;
    if constexpr (HP && i < 2) {
        static_for<0, 5>([&](auto jj_) __attribute__((always_inline)) {
            constexpr int c = 10 * i + 5 * kk + decltype(jj_)::value;
            R.oc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(R.fs[S][decltype(jj_)::value], R.of, R.oc[c], 0, 0, 0);
        });
    } else {
        static_for<0, 3>([&](auto j_) __attribute__((always_inline)) {
            constexpr int j = decltype(j_)::value;
            R.qa[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(R.fs[S][j], R.fs[S][3], R.qa[0][j], 0, 0, 0);
            R.qa[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(R.fs[S][j], R.fs[S][4], R.qa[1][j], 0, 0, 0);
        });
    }
}

// The block's 70 weight pieces are consumed as one sequence per head group: [proj piece 0, 1 of the PREVIOUS group (HP),] qkv
// piece 0..4 of group g (HQ), starting at piece T of the stream.
// The fragments of half u+1 (weights from the ring, trunk rows / O from LDS) are read into the second register set before
// the MFMAs of half u are issued, so a half's LDS reads run under the matrix work of the half before it instead of in
// front of their own (both waves of a SIMD sit at the same barrier: nothing else would overlap them).  Per piece
// boundary: this wave's reads of piece i are complete (lgkmcnt) and its parts of piece i+1 have landed (vmcnt) ->
// barrier -> read the first half of piece i+1 -> DMA piece i+4 into the slot of piece i -> MFMAs of the last half of i.
template <bool HP, bool HQ>
__device__ __forceinline__ void ab_sequence(const AttnBlockArgs& a, const AbLane& L, AbRegs& R, const int T, const int g) {
    constexpr int NP = (HP ? 2 : 0) + (HQ ? 5 : 0), NU = 2 * NP;
    constexpr int BU = NU - 3;                            // the half under which the bias is requested: after the last counted wait
    AB_LGKM0();                                           // this wave's O rows of the previous group are in LDS
    AB_WAIT(4);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    ab_load<HP, 0>(L, R, T);
    ab_issue(L, T + 3);
    static_for<0, NU>([&](auto u_) __attribute__((always_inline)) {
        constexpr int u = decltype(u_)::value;
        if constexpr (u + 1 < NU) {
            if constexpr (u & 1) {
                ab_arrived<u, 0>(R);
                AB_WAIT(4);
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            }
            ab_load<HP, u + 1>(L, R, T);
            if constexpr (u & 1) ab_issue(L, T + (u >> 1) + 4);
            else ab_arrived<u, 5>(R);
        } else {
            ab_arrived<u, 0>(R);
        }
        if constexpr (HQ && u == BU) {
            // relative-position bias of (head, query half) in accumulator order: 64 B per lane, requested after the
            // sequence's last counted wait (see AB_WAIT) and waited for with vmcnt(0) before the scores
            // (inline asm: at the first use of an ordinary load's result hipcc waits vmcnt(0) wherever that use lands)
            const half8* bp = reinterpret_cast<const half8*>(a.bias) + ((size_t)((2 * g + L.ahl) * 2 + L.aqt) * 64 + L.lane) * 4;
            ab_load64(R.bias8[0], R.bias8[1], R.bias8[2], R.bias8[3], bp);
        }
        ab_mma<HP, u>(R);
        __builtin_amdgcn_sched_barrier(0);                // the next half's wait stays behind these MFMAs
    });
}

// stage q, k (token-major) and v (transposed) of the group as fp16
__device__ __forceinline__ void ab_stage_qkv(const AbLane& L, const float4v (&qa)[2][3]) {
    char* const smem = ab_smem();
    const int lane = L.lane, l15 = L.l15, lq = L.lq;
    static_for<0, 2>([&](auto i_) __attribute__((always_inline)) {
        static_for<0, 3>([&](auto j_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value, j = decltype(j_)::value;
            const int J = 3 * L.wn + j, type = J >> 1, hl = J & 1;          // wave-uniform
            const int token = 32 * L.wm + 16 * i + l15;
            const half4v h = {(_Float16)qa[i][j][0], (_Float16)qa[i][j][1], (_Float16)qa[i][j][2], (_Float16)qa[i][j][3]};
            if (type < 2) {
                *reinterpret_cast<half4v*>(smem + AB_QK + type * 8192 + hl * 4096 + token * 32 + (((lq >> 1) ^ (l15 >> 3)) & 1) * 16 + (lq & 1) * 8) = h;
            } else {
                // V transposed: [unit][dim][token].  Two-byte stores (one per dim and lane) cost ~60 cycles each with all
                // waves at it (sub-dword LDS writes); instead neighbouring lanes = neighbouring tokens exchange half of their
                // values (DPP), so that the even lane holds dims 4 lq, 4 lq + 1 and the odd lane dims 4 lq + 2, 4 lq + 3 of
                // BOTH tokens: two 4-byte stores per lane, the same bytes in the same places
                const int unit = (token >> 6) * 2 + hl, sq = token & 63;
                union { half2v h2; uint32_t u; } p01, p23;
                p01.h2 = half2v{h[0], h[1]}; p23.h2 = half2v{h[2], h[3]};
                const bool odd = (lane & 1) != 0;
                const uint32_t own = odd ? p23.u : p01.u;
                const uint32_t recv = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(odd ? p01.u : p23.u), 0xB1, 0xF, 0xF, true);   // lane ^ 1
                const uint32_t ta = odd ? recv : own, tb = odd ? own : recv;          // first / second token of the pair
                const uint32_t w0 = __builtin_amdgcn_perm(tb, ta, 0x05040100u);       // (dim r, token), (dim r, token + 1)
                const uint32_t w1 = __builtin_amdgcn_perm(tb, ta, 0x07060302u);       // dim r + 1
                uint32_t* vt = reinterpret_cast<uint32_t*>(reinterpret_cast<_Float16*>(smem + AB_VT) +
                                                           (unit * 16 + 4 * lq + (odd ? 2 : 0)) * AB_VROW + (sq & ~1));
                vt[0] = w0; vt[AB_VROW / 2] = w1;
            }
        });
    });
    AB_LGKM0();                                           // raw barrier: __syncthreads() would drain the weight DMA
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// attention of this wave's (board, head, query half); O overwrites the wave's Q rows
__device__ __forceinline__ void ab_attend(const AbLane& L, AbRegs& R, float isd, float clampv, float wm, float wu) {
    const int half = L.half, r31 = L.r31;
    const char* Kb = ab_smem() + AB_QK + 8192 + L.ahl * 4096 + L.aboard * 64 * 32;
    const int hsw = 16 * (half ^ ((r31 >> 3) & 1));                                     // this lane's half of its token's row
    const half8 kf0 = *reinterpret_cast<const half8*>(Kb + r31 * 32 + hsw);
    const half8 kf1 = *reinterpret_cast<const half8*>(Kb + (32 + r31) * 32 + hsw);
    char* Qp = ab_smem() + AB_QK + L.ahl * 4096 + (L.aboard * 64 + L.aq) * 32 + hsw;       // also where O goes
    const half8 qfr = *reinterpret_cast<const half8*>(Qp);
    half8 vf[2][2];
    attn_v_frags(reinterpret_cast<const _Float16*>(ab_smem() + AB_VT) + (L.au * 16 + L.l15) * AB_VROW, half, vf);
    float16v st[2];
    attn_scores(kf0, kf1, qfr, st);
    // the bias and every piece issued before it (those landed long ago); the operands tie the registers to this point
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(R.bias8[0]), "+v"(R.bias8[1]), "+v"(R.bias8[2]), "+v"(R.bias8[3]) :: "memory");
    auto bias = [&](auto kt_, auto g_) __attribute__((always_inline)) {
        constexpr int bi = decltype(kt_)::value * 16 + 4 * decltype(g_)::value;
        const half8 b = R.bias8[bi >> 3];
        return half4v{b[bi & 7], b[(bi & 7) + 1], b[(bi & 7) + 2], b[(bi & 7) + 3]};
    };
    auto vis = [&](auto kt_, auto g_) __attribute__((always_inline)) {
        constexpr int bi = decltype(kt_)::value * 16 + 4 * decltype(g_)::value;
        return half4v{R.visp[bi >> 1][0], R.visp[bi >> 1][1], R.visp[(bi >> 1) + 1][0], R.visp[(bi >> 1) + 1][1]};
    };
    const uint4v ov = attn_pack_o(attn_softmax_pv(st, bias, vis, vf, isd, clampv, wm, wu), half);
    // (inline asm: before an ordinary LDS store hipcc waits for every LDS-DMA in flight, vmcnt(0))
    asm volatile("ds_write_b128 %0, %1" :: "v"((uint32_t)(uintptr_t)Qp), "v"(ov) : "memory");
}

// this lane's four channels of accumulator tile j in its token's row of the X image (token 16 w + l15)
__device__ __forceinline__ half4v* ab_own4(const AbLane& L, int j) {
    const int token = 16 * L.w + L.l15;
    const int chunk = 2 * j + (L.lq >> 1);
    const int tsw = (token >> 1) & 7;
    const int pos = (chunk & ~7) | ((chunk ^ tsw) & 7);
    return reinterpret_cast<half4v*>(ab_smem() + AB_X + token * 640 + (L.lq & 1) * 8 + pos * 16);
}
// GroupNorm scratch over the drained ring: [8 waves][20][4] partial (sum, sum of squares), then [2 boards][20] (mean, rstd)
__device__ __forceinline__ float2* ab_gn_partials() { return reinterpret_cast<float2*>(ab_smem() + AB_RING); }
__device__ __forceinline__ float2* ab_gn_totals() { return ab_gn_partials() + 8 * 20 * 4; }

// residual + LayerNorm (per token: the wave holds all 320 channels of its 16 tokens); y replaces x in the X image, and the
// GroupNorm partial sums of y go to the scratch
__device__ __forceinline__ void ab_residual_layernorm(const AttnBlockArgs& a, const AbLane& L, float4v (&oc)[20]) {
    float s1 = 0.f, s2 = 0.f;
    static_for<0, 20>([&](auto j_) __attribute__((always_inline)) {
        constexpr int j = decltype(j_)::value;
        const half4v xv = *ab_own4(L, j);
        static_for<0, 4>([&](auto r_) __attribute__((always_inline)) {
            constexpr int r = decltype(r_)::value;
            const float v = oc[j][r] + (float)xv[r];
            oc[j][r] = v;
            s1 += v; s2 += v * v;
        });
    });
    s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
    s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
    const float cnt = (float)a.ln_count;
    const float mean = s1 / cnt;
    float var = s2 / cnt - mean * mean;
    var = var > 0.f ? var : 0.f;
    const float rstd = rsqrtf(var + 1e-5f);
    const float* par = reinterpret_cast<const float*>(ab_smem() + AB_PAR);
    float2* scr = ab_gn_partials();
    const float nmr = -mean * rstd;
    static_for<0, 20>([&](auto j_) __attribute__((always_inline)) {
        constexpr int j = decltype(j_)::value;
        const float4 gm = *reinterpret_cast<const float4*>(par + 16 * j + 4 * L.lq);
        const float4 bt = *reinterpret_cast<const float4*>(par + 320 + 16 * j + 4 * L.lq);
        const float gmv[4] = {gm.x, gm.y, gm.z, gm.w}, btv[4] = {bt.x, bt.y, bt.z, bt.w};
        float p1 = 0.f, p2 = 0.f;
        half4v h;
        static_for<0, 4>([&](auto r_) __attribute__((always_inline)) {
            constexpr int r = decltype(r_)::value;
            const float y = fmaf(fmaf(oc[j][r], rstd, nmr), gmv[r], btv[r]);      // (v - mean) rstd gamma + beta, two FMAs
            p1 += y; p2 += y * y;
            h[r] = (_Float16)y;
        });
        *ab_own4(L, j) = h;                                             // over this lane's own x values
        p1 = ab_row_sum(p1); p2 = ab_row_sum(p2);
        if (L.l15 == 0) scr[(L.w * 20 + j) * 4 + L.lq] = make_float2(p1, p2);
    });
}

// the wave's 16 rows are contiguous in the output: linear 16-byte reads of the LDS image, swizzle undone on the way
__device__ __forceinline__ void ab_flush(const AbLane& L, _Float16* outp, int pair) {
    char* og = reinterpret_cast<char*>(outp) + ((size_t)pair * 128 + 16 * L.w) * 640;
#pragma unroll
    for (int n = 0; n < 10; ++n) {
        const int q = n * 64 + L.lane;
        const int rl = q / 40, pos = q - rl * 40;
        const int grow = 16 * L.w + rl;
        const int src = (pos & ~7) | ((pos ^ (grow >> 1)) & 7);
        const uint4 v = *reinterpret_cast<const uint4*>(ab_smem() + AB_X + grow * 640 + pos * 16);
        *reinterpret_cast<uint4*>(og + rl * 640 + src * 16) = v;
    }
}

// second output: act(GroupNorm16(y)) for the next residual block (statistics per board and 16-channel group), in place
// in the X image
template <int ACT>
__device__ __forceinline__ void ab_second_output(const AbLane& L) {
    const int tid = L.tid;
    float2* scr = ab_gn_partials();
    float2* tot = ab_gn_totals();
    __syncthreads();
    if (tid < 40) {
        const int bd = tid / 20, j = tid - bd * 20;
        float s = 0.f, ss = 0.f;
        for (int ww = 0; ww < 4; ++ww)
            for (int q = 0; q < 4; ++q) { const float2 v = scr[((bd * 4 + ww) * 20 + j) * 4 + q]; s += v.x; ss += v.y; }
        float mu, rstd;
        gn16_mean_rstd(s, ss, mu, rstd);
        tot[tid] = make_float2(mu, rstd);
    }
    __syncthreads();
    // per (board, channel) scale and shift over the gamma / beta slots (the second GroupNorm's parameters are dead after this)
    float* par = reinterpret_cast<float*>(ab_smem() + AB_PAR);
    {
        float scv[2] = {0.f, 0.f}, shv[2] = {0.f, 0.f};
        if (tid < 320) {
            const float g2 = par[640 + tid], b2 = par[960 + tid];
#pragma unroll
            for (int bd = 0; bd < 2; ++bd) {
                const float2 mr = tot[bd * 20 + (tid >> 4)];
                scv[bd] = g2 * mr.y; shv[bd] = b2 - mr.x * scv[bd];
            }
        }
        __syncthreads();
        if (tid < 320) { par[tid] = scv[0]; par[320 + tid] = shv[0]; par[640 + tid] = scv[1]; par[960 + tid] = shv[1]; }
        __syncthreads();
    }
    static_for<0, 20>([&](auto j_) __attribute__((always_inline)) {
        constexpr int j = decltype(j_)::value;
        const float4 gm = *reinterpret_cast<const float4*>(par + (L.w >> 2) * 640 + 16 * j + 4 * L.lq);
        const float4 bt = *reinterpret_cast<const float4*>(par + (L.w >> 2) * 640 + 320 + 16 * j + 4 * L.lq);
        const float gmv[4] = {gm.x, gm.y, gm.z, gm.w}, btv[4] = {bt.x, bt.y, bt.z, bt.w};
        half4v h = *ab_own4(L, j);
        static_for<0, 4>([&](auto r_) __attribute__((always_inline)) {
            constexpr int r = decltype(r_)::value;
            h[r] = (_Float16)act_fast<ACT>((float)h[r] * gmv[r] + btv[r]);
        });
        *ab_own4(L, j) = h;
    });
}

template <int ACT>
__global__ __launch_bounds__(512) void attn_block_kernel(AttnBlockArgs a) {
    AbLane L = ab_lane(a);
    const int pairs = a.B >> 1, stride = (int)gridDim.x;
    int pair = (int)blockIdx.x;
    ab_prologue(a, L, pair);
    AbRegs R;
    ab_visibility(a, L, R.visp);
    float wm, wu;
    attn_branch_weights(a.mix, wm, wu);
    const float isd = a.inv_sqrt_d * kLog2e;
    const float clampv = 50.f * kLog2e;
    const float4v zero4 = {0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (;;) {
        ab_per_pass(L);
        static_for<0, 20>([&](auto j_) __attribute__((always_inline)) { R.oc[decltype(j_)::value] = zero4; });
        // qkv of group 0 | 9 x (attention of group g, then proj of g and qkv of g + 1 as one sequence) | attention and proj of group 9
        ab_zero_qa(R.qa);
        ab_sequence<false, true>(a, L, R, 0, 0);
#pragma unroll 1
        for (int g = 0; g < AB_GROUPS - 1; ++g) {
            ab_stage_qkv(L, R.qa);
            ab_attend(L, R, isd, clampv, wm, wu);
            ab_zero_qa(R.qa);
            ab_sequence<true, true>(a, L, R, 7 * g + 5, g + 1);
        }
        ab_stage_qkv(L, R.qa);
        ab_attend(L, R, isd, clampv, wm, wu);
        ab_sequence<true, false>(a, L, R, 7 * AB_GROUPS - 2, AB_GROUPS);
        // every wave's DMA (the three pad pieces included) has landed and every wave has left the ring before it is reused
        AB_WAIT(0);
        __syncthreads();

        ab_residual_layernorm(a, L, R.oc);
        // R is dead from here to the top of the next pass: that is where the next pair's rows travel
        const int next = pair + stride;
        const bool more = next < pairs;                   // workgroup-uniform: every wave runs the same barriers
        AbNext N;
        ab_define_next(N);
        if (more) ab_request_next(a, L, next, N);
        ab_flush(L, a.y, pair);
        if (a.y2 != nullptr) {
            ab_second_output<ACT>(L);
            ab_flush(L, a.y2, pair);
        }
        if (!more) break;
        ab_next_arrived(a, L, N);
        pair = next;
    }
}

// Workgroups of a launch: one per board pair up to the cap (0 = the device's CU count; LDS holds one workgroup per CU, so a
// larger grid only queues), each walking pairs b, b + grid, ...
hipError_t launch_attn_block(const AttnBlockArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.B % 2 != 0 || a.ln_count <= 0 || a.ln_count > 320 || a.grid_cap < 0) return hipErrorInvalidValue;
    if (a.y2 != nullptr && a.act != ACT_SILU && a.act != ACT_RELU) return hipErrorInvalidValue;
    static DeviceOnce once;
    static std::atomic<int> cu_count[32];                 // per device, written before DeviceOnce publishes the device
    int cus = 0;
    hipError_t e = once.run([&cus] {
        hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_block_kernel<ACT_SILU>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, AB_LDS);
        if (r != hipSuccess) return r;
        r = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_block_kernel<ACT_RELU>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, AB_LDS);
        if (r != hipSuccess) return r;
        int d = 0;
        if ((r = hipGetDevice(&d)) != hipSuccess) return r;
        if ((r = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d)) != hipSuccess) return r;
        if (cus <= 0) return hipErrorInvalidDevice;
        if ((unsigned)d < 32u) cu_count[d].store(cus, std::memory_order_relaxed);
        return hipSuccess;
    });
    if (e != hipSuccess) return e;
    if (cus == 0) {                                       // configured earlier
        int d = 0;
        if ((e = hipGetDevice(&d)) != hipSuccess) return e;
        cus = cu_count[d].load(std::memory_order_relaxed);
    }
    const int pairs = a.B / 2, cap = a.grid_cap > 0 ? a.grid_cap : cus;
    const dim3 grid((unsigned)(pairs < cap ? pairs : cap));
    if (a.act == ACT_RELU) hipLaunchKernelGGL(attn_block_kernel<ACT_RELU>, grid, dim3(512), AB_LDS, st, a);
    else hipLaunchKernelGGL(attn_block_kernel<ACT_SILU>, grid, dim3(512), AB_LDS, st, a);
    return hipGetLastError();
}

size_t attn_block_pack_bytes() { return (size_t)(AB_GROUPS * AB_PIECES_PER_GROUP + 3) * AB_PIECE; }
