// The per-board kernels around the convs of the network forward (data layout: net_kernels.h):
//   ew_board_kernel          per-board elementwise glue for the paths that are not fused into a conv or into
//       attn_block_kernel: GN+act, SE gate, residual add, positional encoding, LayerNorm over C, output statistics
//   se_gate_kernel           squeeze-excite gates from a conv epilogue's per-(board, channel) sums
//   planes_to_nhwc_kernel    f32 [B,19,8,8] -> fp16 [B,64,32]
//   nhwc_to_nchw_f32_kernel  SSL head outputs back to NCHW f32
#include "kernel_common.h"
#include "conv_epilogue.h"

// GroupNorm16 scale and shift of channel c from per-channel (sum, sumsq) over the board's 64 squares, st[C][2]: the totals of
// c's group of 16 channels, in channel order.  (gamma / beta by reference, as gn16_affine.)
__device__ __forceinline__ void ew_gn_channel(const float* st, int c, const float& gamma, const float& beta, float& scale,
                                              float& shift) {
    const int g0 = (c >> 4) << 4;
    float s = 0.f, ss = 0.f;
    for (int j = 0; j < 16; ++j) { s += st[2 * (g0 + j)]; ss += st[2 * (g0 + j) + 1]; }
    float mean, rstd;
    gn16_mean_rstd(s, ss, mean, rstd);
    gn16_affine(mean, rstd, gamma, beta, scale, shift);
}

// ---------------------------------------------------------------------------
// ew_board: one workgroup per board, tensor [64][C] fp16.
//   v = t
//   if gn_gamma: v = act(GroupNorm16(v))             (statistics from t_stats)
//   elif gate:   v *= gate[b][c]                     (squeeze-excite, se_gate_kernel)
//   if res:      v += res
//   if posenc:   v += posenc[n][c]
//   if ln_g:     v = LayerNorm_C(v)
//   y = v                                             (the raw residual stream)
//   out_stats = per-channel (sum, sumsq) of y over the 64 squares
//   if y2: y2 = act(GroupNorm16(y; gn2_gamma, gn2_beta))   -- the pre-activation input of the next block's conv1
//
// Memory-bound (4 x 40 KB per board at C = 320) and, per board, a chain of dependent steps (statistics -> gate MLP ->
// values -> statistics -> second output), so what decides the speed is how many bytes a CU keeps in flight:
// 2C threads, thread = (8-channel chunk, group of 4 squares); every thread issues ALL its tensor loads (4 squares x
// {t, res} x 16 B) before anything else, the gate / GroupNorm parameters are computed while they fly, the board's
// values stay packed in registers for the second output (no re-read), every lane is live, every reduction has a fixed
// order (bit-reproducible).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(768) void ew_board_kernel(EwArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = a.C, NC = C >> 3;
    float* sc = reinterpret_cast<float*>(smem);        // [C] scale (GN) or gate (SE); later GN2 scale
    float* sh = sc + C;                                // [C] shift / pooled mean
    float* tot = sh + C;                               // [C][2]
    float* rowbuf = tot + 2 * C;                       // [64][2] LayerNorm (mean, rstd) per square
    float* red = rowbuf + 128;                            // [16][C][2] stats partials; SE partials; LN partials [64][NC][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = blockDim.x, nw = nthr >> 6;       // 16 * NC threads
    const int chunk = tid % NC, sg = tid / NC;         // squares 4 sg .. 4 sg + 3
    const int c0 = chunk * 8;
    const int b = blockIdx.x;
    const _Float16* t = a.t + (size_t)b * 64 * C + (size_t)(sg * 4) * C + c0;
    const _Float16* res = a.res ? a.res + (size_t)b * 64 * C + (size_t)(sg * 4) * C + c0 : nullptr;
    const float* tst = a.t_stats ? a.t_stats + (size_t)b * C * 2 : nullptr;

    // 1. all tensor loads first
    const bool gn = a.gn_gamma != nullptr;
    const bool se = (!gn) && a.gate != nullptr;
    float gatev[8];
    if (se) load8f(a.gate + (size_t)b * C + c0, gatev);
    else static_for<0, 8>([&](auto i_) __attribute__((always_inline)) { gatev[decltype(i_)::value] = 1.f; });
    // (the second output's GroupNorm parameters too: a late load is one more exposed latency per board)
    float g2w = 0.f, g2b = 0.f;
    if (a.y2 != nullptr && tid < C) { g2w = a.gn2_gamma[tid]; g2b = a.gn2_beta[tid]; }
    half8 tv[4], rv[4];
    static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
        constexpr int k = decltype(k_)::value;
        tv[k] = *reinterpret_cast<const half8*>(t + k * C);
        rv[k] = res ? *reinterpret_cast<const half8*>(res + k * C) : half8{0, 0, 0, 0, 0, 0, 0, 0};
    });

    // 2. per-channel scale / shift
    if (gn) {
        for (int c = tid; c < C; c += nthr) ew_gn_channel(tst, c, a.gn_gamma[c], a.gn_beta[c], sc[c], sh[c]);
    }
    __syncthreads();

    // 3. values
    float scl[8], shl[8];
    static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
        constexpr int i = decltype(i_)::value;
        scl[i] = gn ? sc[c0 + i] : gatev[i];
        shl[i] = gn ? sh[c0 + i] : 0.f;
    });
    float x[4][8];
    float pe[4][8];                                      // positional encoding [64][C] f32 (stem only): two 16-byte loads per square
    if (a.posenc) {
        static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
            constexpr int k = decltype(k_)::value;
            load8f(a.posenc + (sg * 4 + k) * C + c0, pe[k]);
        });
    }
    static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
        constexpr int k = decltype(k_)::value;
        static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            float v = (float)tv[k][i];
            if (gn) v = act_apply(v * scl[i] + shl[i], a.act);
            else if (se) v *= scl[i];
            v += (float)rv[k][i];
            if (a.posenc) v += pe[k][i];
            x[k][i] = v;
        });
    });
    if (a.ln_g != nullptr) {
        // LayerNorm over C per square: partial sums per (square, chunk) -> 8 threads per square -> (mean, rstd)
        float2* part = reinterpret_cast<float2*>(red);          // [64][NC]
        static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
            constexpr int k = decltype(k_)::value;
            float rs = 0.f, rss = 0.f;
            static_for<0, 8>([&](auto i_) __attribute__((always_inline)) { const float v = x[k][decltype(i_)::value]; rs += v; rss += v * v; });
            part[(sg * 4 + k) * NC + chunk] = make_float2(rs, rss);
        });
        __syncthreads();
        float2* rowp = reinterpret_cast<float2*>(rowbuf);        // [64] (mean, rstd)
        for (int u = tid; u < 512; u += nthr) {                  // 8 consecutive lanes per square
            const int sq = u >> 3, p8 = u & 7;
            float rs = 0.f, rss = 0.f;
            for (int ch = p8; ch < NC; ch += 8) { const float2 v = part[sq * NC + ch]; rs += v.x; rss += v.y; }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) { rs += __shfl_xor(rs, o); rss += __shfl_xor(rss, o); }
            if (p8 == 0) {
                const float cnt = (float)(a.ln_count > 0 ? a.ln_count : C);
                const float mean = rs / cnt;
                float var = rss / cnt - mean * mean;
                var = var > 0.f ? var : 0.f;
                rowp[sq] = make_float2(mean, rsqrtf(var + 1e-5f));
            }
        }
        __syncthreads();
        float lg[8], lb[8];
        static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            lg[i] = a.ln_g[c0 + i]; lb[i] = a.ln_b[c0 + i];
        });
        static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
            constexpr int k = decltype(k_)::value;
            const float2 mr = rowp[sg * 4 + k];
            static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
                constexpr int i = decltype(i_)::value;
                x[k][i] = (x[k][i] - mr.x) * mr.y * lg[i] + lb[i];
            });
        });
        __syncthreads();                                         // part (red) is reused below
    }

    // 4. first output + per-channel statistics
    _Float16* y = a.y + (size_t)b * 64 * C + (size_t)(sg * 4) * C + c0;
    half8 yv[4];
    float csum[8], csq[8];
    static_for<0, 8>([&](auto i_) __attribute__((always_inline)) { csum[decltype(i_)::value] = 0.f; csq[decltype(i_)::value] = 0.f; });
    static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
        constexpr int k = decltype(k_)::value;
        static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            yv[k][i] = (_Float16)x[k][i];
            csum[i] += x[k][i]; csq[i] += x[k][i] * x[k][i];
        });
        *reinterpret_cast<half8*>(y + k * C) = yv[k];
    });
    if (a.out_stats == nullptr && a.y2 == nullptr) return;
    static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
        constexpr int i = decltype(i_)::value;
        reinterpret_cast<float2*>(red)[sg * C + c0 + i] = make_float2(csum[i], csq[i]);
    });
    __syncthreads();
    for (int c = tid; c < C; c += nthr) {
        float s = 0.f, ss = 0.f;
        for (int g = 0; g < 16; ++g) { const float2 v = reinterpret_cast<const float2*>(red)[g * C + c]; s += v.x; ss += v.y; }
        tot[2 * c] = s; tot[2 * c + 1] = ss;
        if (a.out_stats != nullptr) {
            a.out_stats[((size_t)b * C + c) * 2] = s;
            a.out_stats[((size_t)b * C + c) * 2 + 1] = ss;
        }
    }
    if (a.y2 == nullptr) return;
    __syncthreads();
    // 5. second output from the register copy of y
    if (tid < C) ew_gn_channel(tot, tid, g2w, g2b, sc[tid], sh[tid]);      // nthr == 2 C
    __syncthreads();
    _Float16* y2 = a.y2 + (size_t)b * 64 * C + (size_t)(sg * 4) * C + c0;
    static_for<0, 8>([&](auto i_) __attribute__((always_inline)) { constexpr int i = decltype(i_)::value; scl[i] = sc[c0 + i]; shl[i] = sh[c0 + i]; });
    static_for<0, 4>([&](auto k_) __attribute__((always_inline)) {
        constexpr int k = decltype(k_)::value;
        half8 ov;
        static_for<0, 8>([&](auto i_) __attribute__((always_inline)) {
            constexpr int i = decltype(i_)::value;
            ov[i] = (_Float16)act_apply((float)yv[k][i] * scl[i] + shl[i], a.act);
        });
        *reinterpret_cast<half8*>(y2 + k * C) = ov;
    });
}

hipError_t launch_ew_board(const EwArgs& a, int boards, hipStream_t st) {
    if (a.C > 384 || a.C % 32 != 0) return hipErrorInvalidValue;
    const int nthr = 2 * a.C;                           // (C/8 chunks) x 16 square groups
    const size_t lds = (size_t)(4 * a.C + 128 + 32 * a.C) * 4;
    hipLaunchKernelGGL(ew_board_kernel, dim3(boards), dim3(nthr), lds, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// se_gate: squeeze-excite gate of every board (resnet.py:59-68), gate = sigmoid(W2 act(W1 pool + b1) + b2) with
// pool = per-channel mean over the 64 squares, taken from the conv epilogue's sums.  One workgroup = 8 boards, C
// threads.  The gate is a chain of dependent global-memory latencies, so it runs here, once, with every weight
// fetched in batches of 16 independent loads and used for 8 boards, instead of inside each board's ew_board
// workgroup (measured there: +100 us per call).
// The multiply-adds are explicit fused operations.  Written as `s[q] += w * x` over the 8 boards of a thread, hipcc fused some
// of the eight and compiled the others as a packed multiply followed by a packed add (two roundings): the gate of a board then
// depended, in the last bit, on its position in the batch modulo 8 -- found in round 4 as root values that differed by 1e-6
// from run to run whenever two games raced for batch rows (tools/race_screen_small.py), and as a self-play test that failed
// once in a few dozen runs.  (The 320-wide path has its own squeeze-excite in conv_zs_tail.h and was never affected.)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(384) void se_gate_kernel(SeGateArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = a.C, Hd = a.hidden;
    float* pool = reinterpret_cast<float*>(smem);       // [8][C]
    float* part = pool + 8 * C;                         // [parts][8][Hd]
    float* hid = part + 8 * C;                          // [8][Hd]   (parts * Hd <= C)
    const int tid = threadIdx.x, nthr = blockDim.x;     // == C
    const int b0 = blockIdx.x * 8;
    const int nb = a.B - b0 < 8 ? a.B - b0 : 8;
    for (int q = 0; q < 8; ++q)
        pool[q * C + tid] = q < nb ? a.t_stats[((size_t)(b0 + q) * C + tid) * 2] * (1.f / 64.f) : 0.f;
    __syncthreads();
    const int parts = nthr / Hd;                        // >= 1 (launcher)
    {
        const int j = tid % Hd, p = tid / Hd;
        if (p < parts) {
            const int cpp = (C + parts - 1) / parts;
            const int cbeg = p * cpp, cend = cbeg + cpp < C ? cbeg + cpp : C;
            float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int cb = cbeg; cb < cend; cb += 16) {
                float w[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) w[u] = cb + u < cend ? a.w1[(size_t)(cb + u) * Hd + j] : 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int c = cb + u < cend ? cb + u : cbeg;      // w[u] == 0 past the end
#pragma unroll
                    for (int q = 0; q < 8; ++q) s[q] = __builtin_fmaf(w[u], pool[q * C + c], s[q]);   // explicit: see the header
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) part[(p * 8 + q) * Hd + j] = s[q];
        }
    }
    __syncthreads();
    for (int i = tid; i < 8 * Hd; i += nthr) {
        const int q = i / Hd, j = i - q * Hd;
        float s = a.b1[j];
        for (int p = 0; p < parts; ++p) s += part[(p * 8 + q) * Hd + j];
        hid[q * Hd + j] = act_apply(s, a.act);
    }
    __syncthreads();
    {
        const int c = tid;
        const float bias = a.b2[c];
        float s[8] = {bias, bias, bias, bias, bias, bias, bias, bias};
        for (int jb = 0; jb < Hd; jb += 16) {
            float w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = jb + u < Hd ? a.w2[(size_t)(jb + u) * C + c] : 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int j = jb + u < Hd ? jb + u : 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) s[q] = __builtin_fmaf(w[u], hid[q * Hd + j], s[q]);
            }
        }
        for (int q = 0; q < nb; ++q) a.gate[(size_t)(b0 + q) * C + c] = 1.f / (1.f + __expf(-s[q]));
    }
}

hipError_t launch_se_gate(const SeGateArgs& a, hipStream_t st) {
    if (a.C > 384 || a.C % 32 != 0 || a.hidden < 1 || a.hidden > a.C) return hipErrorInvalidValue;
    const size_t lds = (size_t)(8 * a.C + 8 * a.C + 8 * a.hidden) * 4;
    hipLaunchKernelGGL(se_gate_kernel, dim3((a.B + 7) / 8), dim3(a.C), lds, st, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// planes f32 [B][P][64] -> fp16 [B][64][32] (channels >= P zero)
// ---------------------------------------------------------------------------
__global__ void planes_to_nhwc_kernel(const float* __restrict__ x, _Float16* __restrict__ y, int B, int P) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)B * 64 * 32;
    if (i >= total) return;
    int c = (int)(i % 32);
    long bn = i / 32;
    int n = (int)(bn % 64);
    long b = bn / 64;
    float v = (c < P) ? x[(b * P + c) * 64 + n] : 0.f;
    y[i] = (_Float16)v;
}

hipError_t launch_planes_to_nhwc(const float* x, void* y, int B, int P, hipStream_t st) {
    long total = (long)B * 64 * 32;
    hipLaunchKernelGGL(planes_to_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x,
                       reinterpret_cast<_Float16*>(y), B, P);
    return hipGetLastError();
}

// fp16 [B][64][ld] (first n channels) -> f32 [B][ctot][64] at channel offset coff
// (SSL head outputs, NCHW for the boundary)
__global__ void nhwc_to_nchw_f32_kernel(const _Float16* __restrict__ x, float* __restrict__ y, int B, int ld, int n,
                                        int ctot, int coff) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)B * n * 64;
    if (i >= total) return;
    int sq = (int)(i % 64);
    long bc = i / 64;
    int c = (int)(bc % n);
    long b = bc / n;
    y[(b * ctot + coff + c) * 64 + sq] = (float)x[(b * 64 + sq) * ld + c];
}

hipError_t launch_nhwc_to_nchw_f32(const void* x, float* y, int B, int ld, int n, int ctot, int coff, hipStream_t st) {
    long total = (long)B * n * 64;
    hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const _Float16*>(x), y, B, ld, n, ctot, coff);
    return hipGetLastError();
}
