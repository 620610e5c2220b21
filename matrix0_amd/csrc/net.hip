// Host side of the network forward (see net.h): the workspace and the schedule of one forward.  Weight intake is net_pack.hip.
//
// The forward, step by step, with the kernel each step launches.  "fused" is what a 320-wide trunk runs by default; "unfused" is
// what a kernel-less width, M0_FUSE_TAIL=0 / M0_FUSE_ATTN=0 or a wide squeeze-excite falls back to: the raw conv with
// per-(board, channel) statistics, then ew_board_kernel.  Every "conv -> GroupNorm + act" step goes through conv_norm_act, which
// picks the form; Plan (net.h) holds the choices that do not depend on the step.
//
// Kernels: conv_gemm_kernel<taps> (conv_gemm.hip, small tile), conv_big_kernel (conv_big.hip, 1x1, N % 320 == 0), conv_zs_kernel
// (conv_zs.hip, 3x3, N % 320 == 0), attn_block_kernel / attn_core_kernel (attn_*.hip), the rest net_kernels.hip.  EPI_* is the
// conv's epilogue kind (ConvEpi, net_kernels.h); "conv" alone is the raw conv with statistics (EPI_PLAIN, small tile EPI_ELEMENT).
//
//   step                                   fused                                            unfused
//   input planes -> NHWC fp16              planes_to_nhwc (skipped when the engine encoded into X0_)
//   stem + positional encoding             conv_gemm_kernel<9> EPI_GN (trunk % 64 == 0)     conv_gemm_kernel<9> + ew_board
//   stem without chess features            --                                               conv_gemm_kernel<9> + ew_board (+ next bn1)
//   piece-square-table 1x1 + residual      conv_big_kernel EPI_TAIL_PRE (conv_tail.h)       conv + ew_board
//   interaction 3x3 + residual + next bn1  conv_zs_kernel EPI_TAIL_PRE (conv_zs_tail.h)     conv + ew_board
//   block conv1 + bn2                      conv_zs_kernel EPI_GN                            conv_gemm_kernel<9> + ew_board
//   block conv2 + SE + residual + next bn1 conv_zs_kernel EPI_TAIL (conv_zs_tail.h)         conv + se_gate + ew_board
//   attention block                        attn_block_kernel                                qkv GEMM + attn_core + proj GEMM + ew_board
//   policy_head.0 and value_head.0         one conv_gemm_kernel<1> EPI_GN, N = 64 + 128, two outputs  two convs, each + ew_board
//   policy FCs                             conv_gemm_kernel<1> EPI_ELEMENT (bias, ReLU; f32 logits * logit scale)
//   value_head.3                           conv_gemm_kernel<1> EPI_GN                       conv + ew_board
//   value_fc1                              conv_big_kernel split-K + splitk_reduce (widths 160, 320), else conv_gemm_kernel<1>
//   value_fc2, gate, fc3                   conv_gemm_kernel<1> EPI_ELEMENT
//   SSL head: conv + GN, conv, transpose   conv_gemm_kernel<1> EPI_GN (N in 32/64/128/160), conv, nhwc_to_nchw_f32
#include "net.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <stdlib.h>

const char* Net::check_supported(const m0_net_cfg& c) {
    if (!c.norm_group) return "HIP path supports norm='group' only (BatchNorm configs are not built)";
    if (!c.preact) return "HIP path supports preact=true only";
    if (c.channels % 32 != 0 || c.channels < 32 || c.channels > 384) return "channels must be a multiple of 32 in [32,384]";
    if (c.planes < 1 || c.planes > 32) return "planes must be in [1,32]";
    if (c.attention && (c.attention_heads <= 0 || c.channels % c.attention_heads != 0 ||
                        c.channels / c.attention_heads != 16))
        return "attention head_dim (channels/attention_heads) must be 16";
    if (c.activation != M0_ACT_SILU && c.activation != M0_ACT_RELU) return "activation must be silu or relu";
    if (c.blocks < 1) return "blocks must be >= 1";
    if (c.policy_factor_rank < 0) return "policy_factor_rank must be >= 0";
    if (c.self_supervised && c.ssl_tasks && (c.channels / 2) % 16 != 0) return "ssl heads need channels/2 % 16 == 0";
    return nullptr;
}

Net::Net(const m0_net_cfg& cfg, int device, hipStream_t stream) : cfg_(cfg), device_(device), stream_(stream) {
    // kernel-variant switches (A/B runs, and the tests' reference for the fused kernels): read ONCE, here, so that the layout
    // decisions of finalize() and forward() agree
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    sw_.fuse_tail = !off("M0_FUSE_TAIL");     // =0: conv2 + se_gate + ew_board as separate kernels
    sw_.fuse_attn = !off("M0_FUSE_ATTN");     // =0: qkv GEMM + attn_core + proj GEMM + ew_board as separate kernels
    if (const char* e = getenv("M0_ATTN_GRID")) sw_.attn_grid = std::max(0, atoi(e));   // most attn_block workgroups; 0 = CU count
    C_ = cfg.channels;
    Cp_ = (C_ > 256 && C_ < 320) ? 320 : C_;
    Cs_ = ceil_to(std::max(16, C_ / 2), 32);
    int k = cfg.attention_every_k;
    int stride = std::max(1, cfg.infer_attention_stride);
    int att_seen = 0;
    for (int i = 0; i < cfg.blocks; ++i) {
        tower_.push_back({0, (int)res_.size(), false});
        res_.emplace_back();
        if (cfg.attention && k > 0 && (i % k) == (k - 1)) {
            ++att_seen;
            bool skip = stride > 1 && (att_seen % stride) != 0;
            tower_.push_back({1, (int)att_.size(), skip});
            att_.emplace_back();
        }
    }
}

Net* Net::shared_view(hipStream_t stream) const {
    Net* v = new Net(*this);                 // member-wise copy: the packed-weight descriptors point at this network's buffers
    v->stream_ = stream;
    v->dev_allocs_.clear(); v->dev_sizes_.clear();          // not owned
    v->ws_allocs_.clear(); v->wsB_ = 0; v->wsM_ = 0;         // own workspace, allocated at its first forward
    v->tap_step_ = -1; v->TAPX_ = v->TAPA_ = nullptr;        // the tap buffers are not shared either
    v->sd_.clear();
    v->pev_.clear(); v->pflop_.clear(); v->ptail_.clear(); v->pev_used_ = 0; v->profile_ = false;
    v->prof_ms_ = v->prof_flop_ = v->prof_tail_ms_ = 0; v->prof_launches_ = v->prof_tail_launches_ = 0;
    return v;
}

Net::~Net() {
    for (hipEvent_t e : pev_) (void)hipEventDestroy(e);
    for (void* p : dev_allocs_) (void)hipFree(p);
    for (void* p : ws_allocs_) (void)hipFree(p);
}

void* Net::dalloc(size_t bytes, bool ws) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (!M0_HIP(*hip_, hipMalloc(&p, bytes))) return nullptr;
    (ws ? ws_allocs_ : dev_allocs_).push_back(p);
    if (!ws) dev_sizes_.push_back(bytes);
    // cleared ON THE STREAM THAT WILL USE IT (a NULL-stream hipMemset is not ordered with the non-blocking streams: round 2's
    // regrowth race).  Weight buffers are filled next by blocking NULL-stream copies, so their clear is waited for here.
    M0_HIP(*hip_, hipMemsetAsync(p, 0, bytes, stream_));
    if (!ws) M0_HIP(*hip_, hipStreamSynchronize(stream_));
    return hip_->ok() ? p : nullptr;
}

int Net::ssl_channels_total() const {
    int n = 0;
    for (auto& h : ssl_) n += h.out_ch;
    return n;
}

double Net::flops_per_position(bool with_ssl) const {
    // MAC count of the executed graph (SURVEY App. A.4 convention: 2 FLOP per MAC)
    const double C = C_;
    double mac = 64.0 * cfg_.planes * 9 * C;                                   // stem
    if (cfg_.chess_features) mac += 64.0 * C * C * (cfg_.piece_square_tables ? 1 : 0) + 64.0 * C * C * 9;
    for (auto& L : tower_) {
        if (L.kind == 0) {
            mac += 2 * 64.0 * C * C * 9;
            if (cfg_.se) mac += 2.0 * C * res_[L.index].se_hidden;
        } else if (!L.skip) {
            mac += 64.0 * C * 3 * C + 64.0 * C * C;                            // qkv + proj
            double nb = (cfg_.attention_unmasked_mix > 0.f && cfg_.attention_unmasked_mix < 1.f) ? 2.0 : 1.0;
            mac += 64.0 * 64.0 * C * (1.0 + nb);                               // QK^T + AV per branch
        }
    }
    mac += 64.0 * C * 64;
    if (cfg_.policy_factor_rank > 0) mac += 4096.0 * cfg_.policy_factor_rank + (double)cfg_.policy_factor_rank * M0_POLICY_SIZE;
    else mac += 4096.0 * M0_POLICY_SIZE;
    mac += 64.0 * C * 128 + 64.0 * 128 * 128 + 8192.0 * 2 * C + 2.0 * C * C + C * C + C;
    if (with_ssl) for (auto& h : ssl_) mac += 64.0 * C * (C / 2) + 64.0 * (C / 2) * h.out_ch;
    return 2.0 * mac;
}

int Net::ensure_workspace(int B, std::string& err) {
    const int Bp = std::max(ceil_to(B, 4), wsB_);             // a regrowth for the tap alone keeps the size
    const int Mfc = std::max(ceil_to(B, 256), wsM_);
    const bool want_tap = tap_step_ >= 0;
    if (Bp <= wsB_ && Mfc <= wsM_ && (!want_tap || TAPX_)) return M0_OK;
    M0_HIP(*hip_, hipSetDevice(device_));
    M0_HIP(*hip_, hipDeviceSynchronize());
    for (void* p : ws_allocs_) M0_HIP(*hip_, hipFree(p));
    if (!hip_->ok()) { err = "workspace: " + hip_->message(); return M0_ERR_HIP; }     // the list stays for the destructor
    ws_allocs_.clear();
    const size_t C = Cp_;
    const size_t nb = Bp, nh = std::max(Bp, Mfc);
    const size_t Cst = std::max<size_t>(C, 128);
    auto H = [&](size_t elems) { return (_Float16*)dalloc(elems * 2, true); };
    auto F = [&](size_t elems) { return (float*)dalloc(elems * 4, true); };
    X0_ = H(nb * 64 * 32);
    XA_ = H(nb * 64 * C); XB_ = H(nb * 64 * C); T1_ = H(nb * 64 * C); T2_ = H(nb * 64 * C); AA_ = H(nb * 64 * C);
    QKV_ = H(nb * 64 * 3 * C); O_ = H(nb * 64 * C);
    S1_ = F(nb * Cst * 2); S2_ = F(nb * Cst * 2); G_ = F(nb * Cst);
    PH_ = H(nh * 64 * 64); PH2_ = H(nh * 64 * 64);
    VH_ = H(nh * 64 * 128); VH2_ = H(nh * 64 * 128);
    const size_t rp = cfg_.policy_factor_rank > 0 ? ceil_to(cfg_.policy_factor_rank, 32) : 32;
    F1_ = H((size_t)Mfc * rp);
    F2_ = H((size_t)Mfc * ceil_to(2 * C_, 32)); F3_ = H((size_t)Mfc * ceil_to(C_, 32)); F4_ = H((size_t)Mfc * ceil_to(C_, 32));
    SH_ = H(nb * 64 * Cs_); SH2_ = H(nb * 64 * Cs_); SO_ = H(nb * 64 * 32);
    VAL_ = F((size_t)Mfc * 32);
    SPK_ = F((size_t)8 * Mfc * ceil_to(2 * C_, 32));
    TAPX_ = TAPA_ = nullptr;
    if (want_tap) { TAPX_ = H(nb * 64 * C); TAPA_ = H(nb * 64 * C); }
    // The clears were enqueued on stream_.  A forward may run on ANOTHER stream (the match engine runs network B on network
    // A's stream, selfplay.hip::one_step), so the (rare) regrowth ends by waiting for them: a late clear would zero
    // activations a kernel already wrote.  The wait also surfaces an asynchronous memset failure.
    // (tests/test_net_gpu.py::test_workspace_regrowth_keeps_results, tests/test_arena_gpu.py::test_step_right_after_create)
    M0_HIP(*hip_, hipStreamSynchronize(stream_));
    if (!M0_HIP(*hip_, hipGetLastError())) {     // an allocation (dalloc returned null), a clear or the wait has failed
        err = "workspace hipMalloc / clear failed: " + hip_->message(); wsB_ = wsM_ = 0; return M0_ERR_HIP;
    }
    wsB_ = Bp; wsM_ = Mfc;
    return M0_OK;
}

// The arguments every conv / FC launch starts from; a call site then sets what is special about it, by field name.
static GemmArgs gemm_args(const PackedGemm& g, const _Float16* in, void* out, int Mrows, int epi_act = ACT_NONE) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.w = g.w; a.out = out; a.bias = g.bias;
    a.Mrows = Mrows; a.Mvalid = Mrows; a.Cin = g.Cin; a.N = g.N; a.Npad = g.N; a.ldo = g.N;
    a.epi_act = epi_act; a.out_scale = 1.f; a.w_pp = g.pp ? 1 : 0;
    return a;
}

// The same for ew_board_kernel: y = t, then whatever the call site names.
static EwArgs ew_args(const _Float16* t, _Float16* y, int C, int act) {
    EwArgs e;
    memset(&e, 0, sizeof(e));
    e.t = t; e.y = y; e.C = C; e.act = act;
    return e;
}
static void ew_next_bn1(EwArgs& e, const NormParams* next_bn1, _Float16* y2) {
    if (next_bn1) { e.y2 = y2; e.gn2_gamma = next_bn1->gamma; e.gn2_beta = next_bn1->beta; }
}

static double conv3x3_flop(const PackedGemm& g, int rows) { return 2.0 * (double)rows * (double)g.N * (double)g.Cin * 9.0; }

template <class Launch>
hipError_t Net::profiled(bool on, hipStream_t st, double flop, bool tail, Launch&& launch) {
    if (!on) return launch();
    if (pev_used_ + 2 > pev_.size()) {
        for (int i = 0; i < 2; ++i) { hipEvent_t e; if (!M0_HIP(*hip_, hipEventCreate(&e))) return hip_->code(); pev_.push_back(e); }
    }
    M0_HIP(*hip_, hipEventRecord(pev_[pev_used_], st));
    hipError_t rc = hip_->ok() ? launch() : hip_->code();        // the caller records a failed launch under its own name
    if (rc == hipSuccess && !M0_HIP(*hip_, hipEventRecord(pev_[pev_used_ + 1], st))) rc = hip_->code();
    pev_used_ += 2;
    pflop_.push_back(flop);
    ptail_.push_back(tail ? 1 : 0);
    return rc;
}

hipError_t Net::run_gemm(const PackedGemm& g, GemmArgs a, hipStream_t st) {
    const bool big = conv_gemm_tile_n(g.Cin, g.N) == 320;
    // a long-K 1x1 GEMM (value_fc1: K = 8192; 32 tiles on 256 CUs at 4096 boards): split K eight ways into fp32 partial
    // tiles, then a fixed-order reduction with the bias and the activation.  Taken at EVERY batch size: the summation order of a
    // board's value must not depend on how many other boards share the launch (tests/test_net_gpu.py: bitwise batch invariance up
    // to the 24 832 boards of a self-play pass); at large batches the partial tiles cost ~0.1 % of the forward.
    const bool splitk = g.taps == 1 && big && g.Cin >= 4096 && (g.Cin >> 6) % 8 == 0 && !a.gn_gamma && !a.mul && !a.out_stats &&
                        !a.out_f32 && a.out_scale == 1.f && SPK_ != nullptr && (size_t)g.N <= (size_t)ceil_to(2 * C_, 32) &&
                        a.Mrows <= wsM_;
    // the roofline profile counts the 3x3 big-tile convs launched from here (and the fused block tails, forward())
    return profiled(profile_ && g.taps == 9 && big, st, conv3x3_flop(g, a.Mvalid), false, [&]() -> hipError_t {
        if (!splitk) return launch_conv_gemm(a, g.taps, st);
        _Float16* out = (_Float16*)a.out;
        const int act = a.epi_act;
        a.out = SPK_; a.bias = nullptr; a.epi_act = ACT_NONE; a.out_f32 = 1; a.ksplit = 8;
        hipError_t rc = launch_conv_gemm(a, g.taps, st);
        return rc != hipSuccess ? rc : launch_splitk_reduce(SPK_, 8, a.Mrows, g.N, g.bias, act, out, st);
    });
}

hipError_t Net::se_gate(const ResBlockW& r, const float* stats, int boards, hipStream_t st) {
    SeGateArgs g;
    g.t_stats = stats; g.w1 = r.se_w1; g.b1 = r.se_b1; g.w2 = r.se_w2; g.b2 = r.se_b2;
    g.gate = G_; g.B = boards; g.C = Cp_; g.hidden = r.se_hidden; g.act = plan_.act;
    return launch_se_gate(g, st);
}

hipError_t Net::conv_norm_act(const PackedGemm& g, const NormParams& n, const _Float16* in, _Float16* out, _Float16* scratch,
                              int Mrows, hipStream_t st, const ConvNormOpts& o) {
    const bool big = conv_gemm_tile_n(g.Cin, g.N) == 320;
    GemmArgs a = gemm_args(g, in, out, Mrows);
    if (big && o.res && plan_.fuse_tail) {
        // big tile, tail form: out = res + act(GroupNorm16(conv)), then the next block's GroupNorm + act into AA_.  Launched
        // outside the roofline bracket: the profile's "tail" launches are the residual blocks' conv2 only.
        a.epi_act = plan_.act; a.res = o.res; a.pre_gamma = n.gamma; a.pre_beta = n.beta;
        if (o.next_bn1) { a.y2 = AA_; a.gn_gamma = o.next_bn1->gamma; a.gn_beta = o.next_bn1->beta; }
        return launch_conv_gemm(a, g.taps, st);
    }
    // GroupNorm + act (+ posenc) epilogues, neither with a residual nor a second output: conv_zs_kernel's (3x3 big tile), and
    // conv_gemm_kernel's for a trunk that is a multiple of 64 wide: 3x3 over the stem's 32 input planes, 1x1 with all of
    // N = 32 / 64 / 128 / 160 in one workgroup
    const bool epilogue = big ? g.taps == 9
                              : plan_.gn_small && (g.taps == 9 ? g.Cin == 32 : g.N == 32 || g.N == 64 || g.N == 128 || g.N == 160);
    if (epilogue && !o.res && !o.next_bn1) {
        a.gn_gamma = n.gamma; a.gn_beta = n.beta; a.epi_act = plan_.act; a.posenc = o.posenc;
        return run_gemm(g, a, st);
    }
    // unfused: the raw conv with per-(board, channel) statistics, then ew_board_kernel
    a.out = scratch; a.out_stats = S1_;
    hipError_t rc = run_gemm(g, a, st);
    if (rc != hipSuccess) return rc;
    EwArgs e = ew_args(scratch, out, g.N, plan_.act);
    e.t_stats = S1_; e.gn_gamma = n.gamma; e.gn_beta = n.beta; e.res = o.res; e.posenc = o.posenc;
    ew_next_bn1(e, o.next_bn1, AA_);
    return launch_ew_board(e, Mrows / 64, st);
}

void Net::harvest_profile() {
    for (size_t i = 0; i + 1 < pev_used_; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pev_[i], pev_[i + 1]) == hipSuccess) {
            prof_ms_ += ms; prof_flop_ += pflop_[i / 2]; prof_launches_++;
            if (ptail_[i / 2]) { prof_tail_ms_ += ms; prof_tail_launches_++; }
        }
    }
    pev_used_ = 0;
    pflop_.clear();
    ptail_.clear();
}

// Every launch goes through M0_HIP on the network's status: after the first failure the rest of the schedule is skipped (the
// host arithmetic between the launches still runs) and the one test at the end reports it.
int Net::forward(const float* planes_dev, const _Float16* nhwc_dev, int B, float* logits_dev, float* value_dev,
                 float* ssl_dev, hipStream_t st, std::string& err) {
    if (!finalized_) { err = "weights not finalized"; return M0_ERR_STATE; }
    if (B <= 0) { err = "batch must be positive"; return M0_ERR_INVALID; }
    if (int rc = ensure_workspace(B, err)) return rc;
    HipStatus& hs = *hip_;
    const int Bp = ceil_to(B, 4);
    const int Mc = Bp * 64;
    const int Mfc = ceil_to(B, 256);
    const int act = plan_.act, vact = plan_.vact;
    const int C = Cp_;                 // in-memory trunk width

    const _Float16* x0 = nhwc_dev;
    if (!x0) {
        if (!planes_dev) { err = "no input"; return M0_ERR_INVALID; }
        M0_HIP(hs, launch_planes_to_nhwc(planes_dev, X0_, B, cfg_.planes, st));
        x0 = X0_;
    }
    // The residual stream alternates between xa (current) and xb; AA_ holds act(bn1(stream)) for the next residual block's
    // conv1, written by whichever step wrote the stream (next_bn1).
    _Float16* xa = XA_;
    _Float16* xb = XB_;
    const NormParams* first_bn1 = bn1(plan_.first_bn1);
    // trunk tap (net.h): after step `step`, whose stream is `stream` and which wrote AA_ when `second`
    auto tap = [&](int step, const _Float16* stream, bool second) {
        if (step != tap_step_) return;
        const size_t bytes = (size_t)Mc * C * sizeof(_Float16);
        M0_HIP(hs, hipMemcpyAsync(TAPX_, stream, bytes, hipMemcpyDeviceToDevice, st));
        if (second) M0_HIP(hs, hipMemcpyAsync(TAPA_, AA_, bytes, hipMemcpyDeviceToDevice, st));
        tap_second_ = second;
    };
    // stem (resnet.py:314-318) + chess features (229-244)
    ConvNormOpts so;
    if (cfg_.chess_features) so.posenc = posenc_; else so.next_bn1 = first_bn1;
    M0_HIP(hs, conv_norm_act(stem_, stem_n_, x0, xa, T1_, Mc, st, so));
    tap(0, xa, so.next_bn1 != nullptr);
    if (cfg_.chess_features) {
        if (cfg_.piece_square_tables) {
            ConvNormOpts po;
            po.res = xa;
            M0_HIP(hs, conv_norm_act(pst_, pst_n_, xa, xb, T1_, Mc, st, po));
            std::swap(xa, xb);
        }
        tap(1, xa, false);
        ConvNormOpts io;
        io.res = xa; io.next_bn1 = first_bn1;
        M0_HIP(hs, conv_norm_act(inter_, inter_n_, xa, xb, T1_, Mc, st, io));
        std::swap(xa, xb);
        tap(2, xa, first_bn1 != nullptr);
    } else {
        tap(1, xa, false);
        tap(2, xa, false);
    }
    // tower
    for (size_t li = 0; li < tower_.size(); ++li) {
        const TowerLayer& L = tower_[li];
        const NormParams* next_bn1 = bn1(L.next_bn1);
        if (L.kind == 0) {
            const ResBlockW& r = res_[L.index];
            // pre-activation block (resnet.py:45-51): conv1 reads AA_ = act(bn1(x)) and leaves T1_ = act(bn2(conv1)), so conv2
            // also reads a ready operand
            M0_HIP(hs, conv_norm_act(r.conv1, r.bn2, AA_, T1_, T2_, Mc, st));
            if (plan_.fuse_tail) {
                // conv2 + squeeze-excite + residual add + the next block's GroupNorm/activation in one kernel
                GemmArgs a = gemm_args(r.conv2, T1_, xb, Mc, act);
                a.res = xa;
                if (next_bn1) { a.y2 = AA_; a.gn_gamma = next_bn1->gamma; a.gn_beta = next_bn1->beta; }
                if (cfg_.se) { a.se_w1 = r.se_w1; a.se_b1 = r.se_b1; a.se_w2 = r.se_w2; a.se_b2 = r.se_b2; a.se_hidden = r.se_hidden;
                               a.se_wf = r.se_wf; }
                M0_HIP(hs, profiled(profile_, st, conv3x3_flop(r.conv2, Mc), true, [&] { return launch_conv_gemm(a, 9, st); }));
            } else {
                GemmArgs a = gemm_args(r.conv2, T1_, T2_, Mc);
                a.out_stats = S2_;
                M0_HIP(hs, run_gemm(r.conv2, a, st));
                EwArgs e = ew_args(T2_, xb, C, act);
                e.t_stats = S2_; e.res = xa;
                if (cfg_.se) { M0_HIP(hs, se_gate(r, S2_, Bp, st)); e.gate = G_; }
                ew_next_bn1(e, next_bn1, AA_);
                M0_HIP(hs, launch_ew_board(e, Bp, st));
            }
        } else {
            if (L.skip) { tap(3 + (int)li, xa, false); continue; }
            const AttnW& w = att_[L.index];
            const float inv_sqrt_d = 1.f / sqrtf((float)(C_ / cfg_.attention_heads));
            if (plan_.fuse_attn && w.blk_w != nullptr) {
                // the whole block (qkv, attention, proj, residual, LayerNorm, next block's GroupNorm/act) in one kernel
                AttnBlockArgs ab;
                memset(&ab, 0, sizeof(ab));
                ab.x = xa; ab.wpack = w.blk_w; ab.bias = w.blk_bias; ab.mask = mask_dev_;
                ab.ln_g = w.ln.gamma; ab.ln_b = w.ln.beta; ab.y = xb;
                if (next_bn1) { ab.y2 = AA_; ab.gn2_gamma = next_bn1->gamma; ab.gn2_beta = next_bn1->beta; }
                ab.B = Bp; ab.ln_count = C_; ab.act = act; ab.grid_cap = sw_.attn_grid; ab.mix = cfg_.attention_unmasked_mix; ab.inv_sqrt_d = inv_sqrt_d;
                M0_HIP(hs, launch_attn_block(ab, st));
            } else {
                M0_HIP(hs, run_gemm(w.qkv, gemm_args(w.qkv, xa, QKV_, Mc), st));
                AttnArgs aa;
                aa.qkv = QKV_; aa.rel_bias = w.rel_bias; aa.mask = mask_dev_; aa.o = O_;
                aa.B = Bp; aa.H = C / 16; aa.C = C; aa.mix = cfg_.attention_unmasked_mix;      // head_dim 16; padded heads are all-zero
                aa.inv_sqrt_d = inv_sqrt_d;
                M0_HIP(hs, launch_attn_core(aa, st));
                M0_HIP(hs, run_gemm(w.proj, gemm_args(w.proj, O_, T1_, Mc), st));
                EwArgs e = ew_args(T1_, xb, C, act);
                e.res = xa; e.ln_g = w.ln.gamma; e.ln_b = w.ln.beta; e.ln_count = C_;
                ew_next_bn1(e, next_bn1, AA_);
                M0_HIP(hs, launch_ew_board(e, Bp, st));
            }
        }
        std::swap(xa, xb);
        tap(3 + (int)li, xa, next_bn1 != nullptr);
    }
    // policy head (resnet.py:699-711).  Its first conv and the value head's read the same trunk: where the small-tile GroupNorm
    // epilogue is in use they are ONE launch over the joint weights hv_ (PH2_ <- policy columns, VH2_ <- value columns), the
    // fused form of the two conv_norm_act steps below.
    const bool joint = plan_.gn_small;
    if (joint) {
        GemmArgs a = gemm_args(hv_, xa, PH2_, Mc, act);
        a.gn_gamma = hv_n_.gamma; a.gn_beta = hv_n_.beta;
        a.ldo = 64; a.out2 = VH2_; a.ldo2 = 128; a.nsplit = 64;
        M0_HIP(hs, launch_conv_gemm(a, 1, st));
    } else {
        M0_HIP(hs, conv_norm_act(ph_conv_, ph_n_, xa, PH2_, PH_, Mc, st));
    }
    const bool factored = cfg_.policy_factor_rank > 0;
    if (factored) M0_HIP(hs, run_gemm(pfc1_, gemm_args(pfc1_, PH2_, F1_, Mfc, ACT_RELU), st));
    const PackedGemm& plast = factored ? pfc2_ : pfc1_;
    GemmArgs pl = gemm_args(plast, factored ? F1_ : PH2_, logits_dev, Mfc);
    pl.Mvalid = B; pl.out_f32 = 1; pl.out_scale = logit_scale_;
    M0_HIP(hs, run_gemm(plast, pl, st));
    // value head (resnet.py:721-734)
    if (!joint) M0_HIP(hs, conv_norm_act(vh0_, vh1_n_, xa, VH2_, VH_, Mc, st));
    // value_head.3 reads VH2_: its epilogue form writes VH_, the unfused form passes through VH_ and lands in VH2_ again
    _Float16* vflat = joint ? VH_ : VH2_;
    M0_HIP(hs, conv_norm_act(vh3_, vh4_n_, VH2_, vflat, VH_, Mc, st));
    M0_HIP(hs, run_gemm(vfc1_, gemm_args(vfc1_, vflat, F2_, Mfc, vact), st));
    M0_HIP(hs, run_gemm(vfc2_, gemm_args(vfc2_, F2_, F3_, Mfc, vact), st));
    GemmArgs vg = gemm_args(vgate_, F3_, F4_, Mfc, ACT_SIGMOID);
    vg.mul = F3_;
    M0_HIP(hs, run_gemm(vgate_, vg, st));
    GemmArgs v3 = gemm_args(vfc3_, F4_, VAL_, Mfc, ACT_TANH);
    v3.out_f32 = 1;
    M0_HIP(hs, run_gemm(vfc3_, v3, st));
    M0_HIP(hs, hipMemcpy2DAsync(value_dev, 4, VAL_, 32 * 4, 4, B, hipMemcpyDeviceToDevice, st));
    // ssl heads (resnet.py:738-745)
    if (ssl_dev && !ssl_.empty()) {
        const int ctot = ssl_channels_total();
        int coff = 0;
        for (auto& h : ssl_) {
            M0_HIP(hs, conv_norm_act(h.c0, h.n, xa, SH2_, SH_, Mc, st));
            M0_HIP(hs, run_gemm(h.c1, gemm_args(h.c1, SH2_, SO_, Mc), st));
            M0_HIP(hs, launch_nhwc_to_nchw_f32(SO_, ssl_dev, B, 32, h.out_ch, ctot, coff, st));
            coff += h.out_ch;
        }
    }
    if (!hs.ok()) { err = "kernel launch failed: " + hs.message(); return M0_ERR_HIP; }
    return M0_OK;
}
