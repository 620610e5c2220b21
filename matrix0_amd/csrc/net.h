// Host side of the network: state-dict intake and repacking into kernel layouts (net_pack.hip, over the host-only layout
// functions of net_pack.h), workspace management and the forward schedule (net.hip).
// Mirrors PolicyValueNet (azchess/model/resnet.py:285-582 ctor, 656-760 forward)
// for the inference configuration the self-play path uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "hip_check.h"
#include "net_kernels.h"

namespace net_pack { struct GemmShape; }

inline int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct PackedGemm {
    _Float16* w = nullptr;   // [taps][Cin/KC][N][KC]
    float* bias = nullptr;   // [N] or null
    int taps = 1, Cin = 0, N = 0;
    bool pp = false;         // 3x3 big tile in the half-tile layout of conv_zs_kernel [chunk*9+tap][N/320][k half][320][32]
};

struct NormParams {
    float* gamma = nullptr;
    float* beta = nullptr;
};

struct HostNorm { std::vector<float> gamma, beta; };   // a norm's padded parameters as they were uploaded

struct ResBlockW {
    PackedGemm conv1, conv2;
    NormParams bn1, bn2;
    float *se_w1 = nullptr, *se_b1 = nullptr, *se_w2 = nullptr, *se_b2 = nullptr;
    void* se_wf = nullptr;                           // fp16 MFMA fragment pieces for conv_zs_kernel's tail (conv_zs_tail.h)
    int se_hidden = 0;
};

struct AttnW {
    PackedGemm qkv, proj;
    NormParams ln;
    float* rel_bias = nullptr;
    void* blk_w = nullptr;         // attn_block_kernel: qkv + proj weight pieces (320-channel trunk only)
    _Float16* blk_bias = nullptr;  // rel_bias * log2(e) in accumulator order, fp16
};

struct TowerLayer {
    int kind;    // 0 = residual block, 1 = attention
    int index;   // into res / att vectors
    bool skip;   // inference attention stride (resnet.py:678-687)
    // res_ index of the residual block that consumes the stream right after this layer: its bn1 + activation is applied by
    // whatever writes the stream here.  -1: the next executed layer is attention, or the tower ends (finalize fills it in)
    int next_bn1 = -1;
};

struct SslHeadW {
    PackedGemm c0, c1;
    NormParams n;
    int out_ch = 0;
};

// Optional operands of Net::conv_norm_act, set by name at the call site.
struct ConvNormOpts {
    const float* posenc = nullptr;          // [64][N] added after the activation (stem)
    const _Float16* res = nullptr;          // residual added after the activation
    const NormParams* next_bn1 = nullptr;   // with it AA_ also receives act(GroupNorm16(out; next_bn1)), the next block's conv1 input
};

class Net {
public:
    // `stream`: the HIP stream every forward of this network runs on (allocations are cleared on it)
    explicit Net(const m0_net_cfg& cfg, int device, hipStream_t stream);
    ~Net();
    // A second instance over the SAME device weights (read-only after finalize) with its own stream and its own workspace: the
    // self-play engine evaluates the partial last round of a pass on it beside the main forward (selfplay.hip, tail split).  The
    // view owns no weights: it must not outlive the network it was made from.
    Net* shared_view(hipStream_t stream) const;
    static const char* check_supported(const m0_net_cfg& cfg);
    int load(const char* name, const void* data, int dtype, const int64_t* shape, int ndim, std::string& err);
    int finalize(std::string& err);
    bool ready() const { return finalized_; }
    // The first failed HIP call made for this network (hip_check.h); intake, workspace and forward issue nothing after it.  A
    // shared_view copies the pointer, not the status: it records into the network it was made from.
    HipStatus& hip() { return *hip_; }
    // every device buffer finalize() made (packed GEMM weights, norm parameters, bias / mask tables), in creation order: the same
    // list with the same sizes on every process that finalized a network of the same configuration
    const std::vector<void*>& device_buffers() const { return dev_allocs_; }
    const std::vector<size_t>& device_buffer_bytes() const { return dev_sizes_; }

    // planes: device f32 [B][planes][64] (planes_dev) or device fp16 NHWC [B][64][32] (nhwc_dev)
    // outputs (device): logits f32 [B][4672], value f32 [B]; ssl (optional) f32 concatenated
    int forward(const float* planes_dev, const _Float16* nhwc_dev, int B, float* logits_dev, float* value_dev,
                float* ssl_dev, hipStream_t st, std::string& err);
    int ensure_workspace(int B, std::string& err);
    int ssl_channels_total() const;
    const m0_net_cfg& cfg() const { return cfg_; }
    size_t param_count() const { return nparams_; }
    double flops_per_position(bool with_ssl) const;
    _Float16* input_nhwc() { return X0_; }   // engine-side encoders write here directly
    // Trunk tap (the per-layer parity tests): after step `step` of the next forwards the residual stream that step wrote, and AA_
    // when the step wrote it, are copied into buffers of this network, on the forward's stream.  Steps in execution order:
    // 0 = stem (+ positional encoding), 1 = piece-square conv, 2 = interaction conv, 3 + i = tower layer i.  A step the
    // configuration lacks, or a skipped attention layer, hands back the stream as the step before left it, without a second output.
    // -1 (the default) = off: the forward issues nothing for it.
    int tap_steps() const { return 3 + (int)tower_.size(); }
    int trunk_width() const { return Cp_; }
    void set_tap(int step) { tap_step_ = step; }
    const _Float16* tap_stream() const { return TAPX_; }      // [B][64][trunk_width()], valid after a tapped forward
    const _Float16* tap_second() const { return TAPA_; }
    bool tap_has_second() const { return tap_second_; }
    // Dominant-kernel timing (roofline): when enabled every 3x3 C->C conv launch is bracketed by HIP events on
    // the launch stream; harvest after the stream has been synchronised.
    void set_profile(bool on) { profile_ = on; }
    void harvest_profile();
    double prof_conv_ms() const { return prof_ms_; }
    double prof_conv_flop() const { return prof_flop_; }
    long prof_conv_launches() const { return prof_launches_; }
    void reset_profile() { prof_ms_ = 0; prof_flop_ = 0; prof_launches_ = 0; prof_tail_ms_ = 0; prof_tail_launches_ = 0; }
    double prof_tail_ms() const { return prof_tail_ms_; }          // the part of the above spent in launches with a fused tail
    long prof_tail_launches() const { return prof_tail_launches_; }

private:
    m0_net_cfg cfg_;
    int device_;
    hipStream_t stream_ = nullptr;
    HipStatus own_hip_, *hip_ = &own_hip_;
    struct Switches { bool fuse_tail = true, fuse_attn = true; int attn_grid = 0; } sw_;   // read once (constructor)
    // What forward() would otherwise derive again on every call: fixed by the configuration, the switches and the squeeze-excite
    // width, filled in at the end of finalize().  Layers are named by index into res_ (TowerLayer::next_bn1, first_bn1), not by
    // pointer: shared_view() copies the vectors, and an index stays valid in the copy.
    struct Plan {
        bool fuse_tail = false;   // conv2 + squeeze-excite + residual (+ next GroupNorm) and the chess-feature convs' tails in one kernel
        bool fuse_attn = false;   // attn_block_kernel
        bool gn_small = false;    // small-tile convs (stem, heads) take GroupNorm + activation in their epilogue: trunk % 64 == 0
        int act = 0, vact = 0;    // ACT_* of the network / of the value FCs
        int first_bn1 = -1;       // res_ index of the block that consumes the stem / chess-feature output, or -1
    } plan_;
    bool finalized_ = false;
    size_t nparams_ = 0;
    std::map<std::string, HostTensor> sd_;
    std::vector<void*> dev_allocs_;
    std::vector<size_t> dev_sizes_;          // bytes of dev_allocs_[i] (m0_net_broadcast_weights ships them in this order)
    std::vector<void*> ws_allocs_;

    int C_ = 0, Cs_ = 0 /*ssl hidden padded*/;
    int Cp_ = 0;   // trunk width in memory: C_, or 320 for 256 < C_ < 320 (zero-padded channels: the MFMA big-tile path)
    PackedGemm stem_;
    NormParams stem_n_;
    float* posenc_ = nullptr;
    PackedGemm pst_, inter_;
    NormParams pst_n_, inter_n_;
    std::vector<ResBlockW> res_;
    std::vector<AttnW> att_;
    std::vector<TowerLayer> tower_;
    PackedGemm ph_conv_, pfc1_, pfc2_;
    PackedGemm hv_;          // policy_head.0 and value_head.0 as ONE 1x1 GEMM over the trunk (N = 64 + 128)
    NormParams hv_n_;        // their GroupNorm parameters, concatenated
    NormParams ph_n_;
    float logit_scale_ = 1.f;
    PackedGemm vh0_, vh3_, vfc1_, vfc2_, vgate_, vfc3_;
    NormParams vh1_n_, vh4_n_;
    std::vector<SslHeadW> ssl_;
    uint64_t* mask_dev_ = nullptr;

    bool profile_ = false;
    std::vector<hipEvent_t> pev_;
    std::vector<double> pflop_;
    std::vector<char> ptail_;
    size_t pev_used_ = 0;
    double prof_ms_ = 0, prof_flop_ = 0, prof_tail_ms_ = 0;
    long prof_launches_ = 0, prof_tail_launches_ = 0;

    // workspace
    int wsB_ = 0, wsM_ = 0;
    _Float16 *X0_ = nullptr, *XA_ = nullptr, *XB_ = nullptr, *T1_ = nullptr, *T2_ = nullptr, *QKV_ = nullptr,
             *O_ = nullptr, *AA_ = nullptr;
    float *S1_ = nullptr, *S2_ = nullptr, *G_ = nullptr;   // G_: squeeze-excite gates [B][C]
    _Float16 *PH_ = nullptr, *PH2_ = nullptr, *VH_ = nullptr, *VH2_ = nullptr, *F1_ = nullptr, *F2_ = nullptr,
             *F3_ = nullptr, *F4_ = nullptr, *SH_ = nullptr, *SH2_ = nullptr, *SO_ = nullptr;
    float* VAL_ = nullptr;
    float* SPK_ = nullptr;      // split-K partial tiles [8][Mfc][2C] f32 (value_fc1)
    // trunk tap: sized like XA_, part of the workspace once a tap has been asked for (a shared_view starts without them)
    int tap_step_ = -1;
    bool tap_second_ = false;
    _Float16 *TAPX_ = nullptr, *TAPA_ = nullptr;

    // weight intake (net_pack.hip)
    const HostTensor* get(const std::string& k, std::string& err);
    const HostTensor* get(const std::string& k, size_t count, std::string& err);
    // the one place that allocates and fills a weight buffer: M0_ERR_HIP with `err` set when either fails, `dst` set otherwise
    int upload_bytes(void*& dst, const void* src, size_t bytes, std::string& err);
    template <class P, class T>
    int upload(P*& dst, const std::vector<T>& v, std::string& err);
    // `keep`: also hand back the packed host copy (the joint head is built from two of them)
    int pack_gemm(PackedGemm& g, const std::string& wkey, const std::string& bkey, const net_pack::GemmShape& s, std::string& err,
                  std::vector<_Float16>* keep = nullptr);
    int upload_norm(NormParams& n, const std::string& prefix, int C_real, int C_pad, std::string& err, HostNorm* keep = nullptr);
    int pack_chess_features(std::string& err);
    int pack_se(ResBlockW& r, const std::string& prefix, std::string& err);
    int pack_attn(AttnW& a, bool skip, const std::string& prefix, std::string& err);
    int pack_joint_head(const std::vector<_Float16>& ph_w, const std::vector<_Float16>& vh_w, const HostNorm& ph_n,
                        const HostNorm& vh_n, std::string& err);
    int pack_ssl_heads(std::string& err);
    void make_plan();
    void* dalloc(size_t bytes, bool ws);
    const NormParams* bn1(int res_index) const { return res_index < 0 ? nullptr : &res_[res_index].bn1; }
    // roofline bracket: `launch()` between two events on `st` when `on`, with its FLOP count and whether it carries a fused tail
    template <class Launch>
    hipError_t profiled(bool on, hipStream_t st, double flop, bool tail, Launch&& launch);
    // one conv / FC launch from filled-in arguments (gemm_args + named fields); splits K for value_fc1
    hipError_t run_gemm(const PackedGemm& g, GemmArgs a, hipStream_t st);
    // out = act(GroupNorm16(conv(in); n)) [+ posenc] [+ res], in the conv's epilogue where a kernel has one, else the raw conv
    // into `scratch` + ew_board_kernel
    hipError_t conv_norm_act(const PackedGemm& g, const NormParams& n, const _Float16* in, _Float16* out, _Float16* scratch,
                             int Mrows, hipStream_t st, const ConvNormOpts& o = ConvNormOpts());
    hipError_t se_gate(const ResBlockW& r, const float* stats, int boards, hipStream_t st);   // G_ <- the block's gates
};
