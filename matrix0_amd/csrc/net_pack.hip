// Weight intake of the network (see net.h): load() collects the state dict on the host, finalize() repacks it into the kernels'
// layouts and uploads it.  The layouts themselves are net_pack.h (host-only, tested on the CPU); every packer here does five
// things: fetch its keys, check their shapes, count the parameters, call the header, upload.  upload() is the one place that
// allocates and copies, and it reports: a failed hipMalloc or hipMemcpy ends finalize() with M0_ERR_HIP, so no forward ever
// sees a null or unwritten weight buffer.
#include "net.h"
#include "net_pack.h"
#include "attn_math.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace pk = net_pack;

static const char* kSslNames[5] = {"piece", "threat", "pin", "fork", "control"};
static const int kSslOut[5] = {13, 1, 1, 1, 3};

#define TRY(x) do { int rc_ = (x); if (rc_ != M0_OK) return rc_; } while (0)

int Net::load(const char* name, const void* data, int dtype, const int64_t* shape, int ndim, std::string& err) {
    if (finalized_) { err = "weights already finalized"; return M0_ERR_STATE; }
    if (!name || (!data && ndim >= 0)) { err = "null argument"; return M0_ERR_INVALID; }
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.resize(n);
    if (dtype == 0) memcpy(t.data.data(), data, n * 4);
    else if (dtype == 1) {
        const _Float16* h = (const _Float16*)data;
        for (size_t i = 0; i < n; ++i) t.data[i] = (float)h[i];
    } else { err = "dtype must be 0 (f32) or 1 (f16)"; return M0_ERR_INVALID; }
    std::string key(name);
    // resnet.py:1405-1416: legacy rename policy_fc.* -> policy_fc1.* only matters for factorised heads
    if (cfg_.policy_factor_rank > 0 && key.rfind("policy_fc.", 0) == 0) key = "policy_fc1." + key.substr(10);
    sd_[key] = std::move(t);
    return M0_OK;
}

const HostTensor* Net::get(const std::string& k, std::string& err) {
    auto it = sd_.find(k);
    if (it == sd_.end()) { err = "missing state-dict key: " + k; return nullptr; }
    return &it->second;
}

// ... with exactly `count` elements
const HostTensor* Net::get(const std::string& k, size_t count, std::string& err) {
    const HostTensor* t = get(k, err);
    if (t && t->data.size() != count) { err = "shape mismatch for " + k; return nullptr; }
    return t;
}

int Net::upload_bytes(void*& dst, const void* src, size_t bytes, std::string& err) {
    void* d = dalloc(bytes, false);
    if (d && bytes) M0_HIP(*hip_, hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    if (!hip_->ok()) { err = "weight upload failed: " + hip_->message(); return M0_ERR_HIP; }
    dst = d;
    return M0_OK;
}

template <class P, class T>
int Net::upload(P*& dst, const std::vector<T>& v, std::string& err) {
    void* d = nullptr;
    TRY(upload_bytes(d, v.data(), v.size() * sizeof(T), err));
    dst = (P*)d;
    return M0_OK;
}

int Net::pack_gemm(PackedGemm& g, const std::string& wkey, const std::string& bkey, const pk::GemmShape& s, std::string& err,
                   std::vector<_Float16>* keep) {
    const HostTensor* w = get(wkey, (size_t)s.N_real * s.Cin_real * s.taps, err);
    if (!w) return M0_ERR_INVALID;
    nparams_ += w->data.size();
    const bool big = conv_gemm_kc(s.Cin_pad, s.N_pad) == 64;
    const bool pp = big && s.taps == 9;       // 3x3 big tile: the half-tile layout of conv_zs_kernel
    const std::vector<_Float16> p =
        pk::gemm_weights<_Float16>(w->data.data(), pp ? pk::GEMM_BIG_3X3 : big ? pk::GEMM_BIG_1X1 : pk::GEMM_SMALL, s);
    TRY(upload(g.w, p, err));
    g.taps = s.taps; g.Cin = s.Cin_pad; g.N = s.N_pad; g.pp = pp;
    g.bias = nullptr;
    if (!bkey.empty()) {
        const HostTensor* b = get(bkey, s.N_real, err);
        if (!b) return M0_ERR_INVALID;
        nparams_ += s.N_real;
        TRY(upload(g.bias, pk::zero_padded<float>(b->data.data(), s.N_real, s.N_pad), err));
    }
    if (keep) *keep = p;
    return M0_OK;
}

// a 1x1 conv or FC [N_real][Cin_real], a 3x3 conv [N_real][Cin_real][9]
static pk::GemmShape fc(int Cin_real, int Cin_pad, int N_real, int N_pad) { return {1, Cin_real, Cin_pad, N_real, N_pad}; }
static pk::GemmShape conv3x3(int Cin_real, int Cin_pad, int N_real, int N_pad) { return {9, Cin_real, Cin_pad, N_real, N_pad}; }
// the FC behind a flatten of `ch` channels x 64 squares
static pk::GemmShape flattened(int ch, int N_real, int N_pad) {
    pk::GemmShape s = fc(ch * 64, ch * 64, N_real, N_pad);
    s.flatten_ch = ch;
    return s;
}

int Net::upload_norm(NormParams& n, const std::string& prefix, int C_real, int C_pad, std::string& err, HostNorm* keep) {
    const HostTensor* g = get(prefix + ".weight", C_real, err);
    if (!g) return M0_ERR_INVALID;
    const HostTensor* b = get(prefix + ".bias", C_real, err);
    if (!b) return M0_ERR_INVALID;
    nparams_ += 2 * (size_t)C_real;
    HostNorm h = {pk::zero_padded<float>(g->data.data(), C_real, C_pad), pk::zero_padded<float>(b->data.data(), C_real, C_pad)};
    TRY(upload(n.gamma, h.gamma, err));
    TRY(upload(n.beta, h.beta, err));
    if (keep) *keep = std::move(h);
    return M0_OK;
}

// positional encoding [64][P] and the two feature convs (resnet.py:229-244)
int Net::pack_chess_features(std::string& err) {
    const int C = C_, P = Cp_;
    const HostTensor* pe = get("chess_features.position_encoding", (size_t)C * 64, err);
    if (!pe) return M0_ERR_INVALID;
    nparams_ += pe->data.size();
    TRY(upload(posenc_, pk::transposed<float>(pe->data.data(), C, 64, 64, P), err));
    if (cfg_.piece_square_tables) {
        TRY(pack_gemm(pst_, "chess_features.pst_conv.weight", "", fc(C, P, C, P), err));
        TRY(upload_norm(pst_n_, "chess_features.pst_norm", C, P, err));
    }
    TRY(pack_gemm(inter_, "chess_features.interaction_conv.weight", "", conv3x3(C, P, C, P), err));
    return upload_norm(inter_n_, "chess_features.interaction_norm", C, P, err);
}

// squeeze-excite of one block: both FCs transposed for se_gate_kernel and, where the fused tail can take them, as fp16 MFMA
// fragment pieces for conv_zs_kernel
int Net::pack_se(ResBlockW& r, const std::string& p, std::string& err) {
    const int C = C_, P = Cp_;
    const int hd = std::max(8, (int)(C * cfg_.se_ratio));
    r.se_hidden = hd;
    const HostTensor* w1 = get(p + ".se_fc1.weight", (size_t)hd * C, err); if (!w1) return M0_ERR_INVALID;
    const HostTensor* b1 = get(p + ".se_fc1.bias", hd, err); if (!b1) return M0_ERR_INVALID;
    const HostTensor* w2 = get(p + ".se_fc2.weight", (size_t)hd * C, err); if (!w2) return M0_ERR_INVALID;
    const HostTensor* b2 = get(p + ".se_fc2.bias", C, err); if (!b2) return M0_ERR_INVALID;
    nparams_ += (size_t)2 * hd * C + hd + C;
    const std::vector<float> w1t = pk::transposed<float>(w1->data.data(), hd, C, P, hd);   // [P][hd] from [hd][C]
    const std::vector<float> w2t = pk::transposed<float>(w2->data.data(), C, hd, hd, P);   // [hd][P] from [C][hd]: coalesced across channels
    TRY(upload(r.se_w1, w1t, err));
    TRY(upload(r.se_b1, b1->data, err));
    TRY(upload(r.se_w2, w2t, err));
    if (P == 320 && hd <= TAIL_SE_HMAX) TRY(upload(r.se_wf, pk::se_fragments<_Float16>(w1t.data(), w2t.data(), hd), err));
    return upload(r.se_b2, pk::zero_padded<float>(b2->data.data(), C, P), err);
}

int Net::pack_attn(AttnW& a, bool skip, const std::string& p, std::string& err) {
    const int C = C_, P = Cp_, H = cfg_.attention_heads;
    if (skip) {   // never executed at inference; count parameters, keep nothing resident
        for (const char* k : {".qkv.weight", ".proj.weight", ".norm.weight", ".norm.bias", ".rel_bias"}) {
            auto it = sd_.find(p + k);
            if (it != sd_.end()) nparams_ += it->second.data.size();
        }
        return M0_OK;
    }
    pk::GemmShape qkv = fc(C, P, 3 * C, 3 * P);
    if (P != C) { qkv.qkv_heads = H; qkv.qkv_heads_pad = P / 16; }
    TRY(pack_gemm(a.qkv, p + ".qkv.weight", "", qkv, err));
    TRY(pack_gemm(a.proj, p + ".proj.weight", "", fc(C, P, C, P), err));
    TRY(upload_norm(a.ln, p + ".norm", C, P, err));
    std::vector<float> rbs;     // rel_bias * log2(e): the attention kernels exponentiate with exp2
    if (cfg_.attention_relbias) {
        const HostTensor* rb = get(p + ".rel_bias", (size_t)H * 4096, err); if (!rb) return M0_ERR_INVALID;
        nparams_ += rb->data.size();
        rbs.resize(rb->data.size());
        for (size_t i = 0; i < rbs.size(); ++i) rbs[i] = rb->data[i] * kLog2e;
    }
    if (P == 320) {
        // attn_block_kernel's operands, from the same tensors (counted above): the weight-piece stream and the bias table
        const HostTensor* wq = get(p + ".qkv.weight", (size_t)3 * C * C, err);
        const HostTensor* wp = get(p + ".proj.weight", (size_t)C * C, err);
        if (!wq || !wp) return M0_ERR_INVALID;
        if (C != H * 16 || pk::kAttnPackElems * 2 != attn_block_pack_bytes()) { err = "shape mismatch for " + p; return M0_ERR_INVALID; }
        TRY(upload(a.blk_w, pk::attn_block_weights<_Float16>(wq->data.data(), wp->data.data(), H), err));
        TRY(upload(a.blk_bias, pk::attn_block_bias<_Float16>(rbs.empty() ? nullptr : rbs.data(), H), err));
    }
    if (cfg_.attention_relbias)     // the split path's table: padded heads carry zero bias
        TRY(upload(a.rel_bias, pk::zero_padded<float>(rbs.data(), rbs.size(), (size_t)(P / 16) * 4096), err));
    return M0_OK;
}

// policy_head.0 (64 channels) and value_head.0 (128) read the same trunk: one GEMM with N = 192, columns [policy | value], both
// in the small-tile layout [Cin / 32][N][32]; GroupNorm parameters concatenated the same way.
int Net::pack_joint_head(const std::vector<_Float16>& ph_w, const std::vector<_Float16>& vh_w, const HostNorm& ph_n,
                         const HostNorm& vh_n, std::string& err) {
    TRY(upload(hv_.w, pk::joint_columns(ph_w, 64, vh_w, 128, Cp_), err));
    hv_.taps = 1; hv_.Cin = Cp_; hv_.N = 192; hv_.pp = false; hv_.bias = nullptr;
    TRY(upload(hv_n_.gamma, pk::joined(ph_n.gamma, vh_n.gamma), err));
    return upload(hv_n_.beta, pk::joined(ph_n.beta, vh_n.beta), err);
}

int Net::pack_ssl_heads(std::string& err) {
    for (int t = 0; t < 5; ++t) {
        if (!(cfg_.ssl_tasks & (1 << t))) continue;
        SslHeadW h;
        h.out_ch = kSslOut[t];
        std::string p = std::string("ssl_heads.") + kSslNames[t];
        TRY(pack_gemm(h.c0, p + ".0.weight", "", fc(C_, Cp_, C_ / 2, Cs_), err));
        TRY(upload_norm(h.n, p + ".1", C_ / 2, Cs_, err));
        TRY(pack_gemm(h.c1, p + ".3.weight", "", fc(C_ / 2, Cs_, h.out_ch, 32), err));
        ssl_.push_back(h);
    }
    return M0_OK;
}

// The schedule choices that do not depend on the batch (Plan, TowerLayer::next_bn1): see net.h.
void Net::make_plan() {
    const bool big = conv_gemm_tile_n(Cp_, Cp_) == 320;     // 320-wide trunk: conv_zs_kernel / conv_big_kernel with their epilogues
    // a squeeze-excite wider than the fused tail takes runs conv2 + se_gate + ew_board instead, as M0_FUSE_TAIL=0 does
    plan_.fuse_tail = big && sw_.fuse_tail &&
                      (!cfg_.se || (res_[0].se_hidden <= TAIL_SE_HMAX && res_[0].se_hidden % 4 == 0));
    plan_.fuse_attn = big && sw_.fuse_attn;
    plan_.gn_small = Cp_ % 64 == 0;
    plan_.act = cfg_.activation == M0_ACT_SILU ? ACT_SILU : ACT_RELU;
    plan_.vact = cfg_.value_activation == M0_ACT_SILU ? ACT_SILU : (cfg_.value_activation == M0_ACT_LEAKY ? ACT_LEAKY : ACT_RELU);
    int next = -1;                      // walking up from the end: the residual block that follows position i
    for (size_t i = tower_.size(); i-- > 0;) {
        TowerLayer& L = tower_[i];
        if (L.kind == 1 && L.skip) continue;
        L.next_bn1 = next;
        next = L.kind == 0 ? L.index : -1;
    }
    plan_.first_bn1 = next;
}

int Net::finalize(std::string& err) {
    if (finalized_) return M0_OK;
    if (!M0_HIP(*hip_, hipSetDevice(device_))) { err = hip_->message(); return M0_ERR_HIP; }
    const int C = C_, P = Cp_;          // real / in-memory trunk width (padded channels carry zeros everywhere)
    nparams_ = 0;
    TRY(pack_gemm(stem_, "stem.0.weight", "", conv3x3(cfg_.planes, 32, C, P), err));
    TRY(upload_norm(stem_n_, "stem.1", C, P, err));
    if (cfg_.chess_features) TRY(pack_chess_features(err));
    int ti = 0;
    for (auto& L : tower_) {
        std::string p = "tower." + std::to_string(ti++);
        if (L.kind == 0) {
            ResBlockW& r = res_[L.index];
            TRY(pack_gemm(r.conv1, p + ".conv1.weight", "", conv3x3(C, P, C, P), err));
            TRY(pack_gemm(r.conv2, p + ".conv2.weight", "", conv3x3(C, P, C, P), err));
            TRY(upload_norm(r.bn1, p + ".bn1", C, P, err));
            TRY(upload_norm(r.bn2, p + ".bn2", C, P, err));
            if (cfg_.se) TRY(pack_se(r, p, err));
        } else {
            TRY(pack_attn(att_[L.index], L.skip, p, err));
        }
    }
    TRY(upload(mask_dev_, pk::attn_mask(), err));
    // policy head; the first conv of each head is kept on the host for the joint GEMM (pack_joint_head)
    std::vector<_Float16> ph_w, vh_w;
    HostNorm ph_n, vh_n;
    TRY(pack_gemm(ph_conv_, "policy_head.0.weight", "", fc(C, P, 64, 64), err, &ph_w));
    TRY(upload_norm(ph_n_, "policy_head.1", 64, 64, err, &ph_n));
    if (cfg_.policy_factor_rank > 0) {
        const int r = cfg_.policy_factor_rank, rp = ceil_to(r, 32);
        TRY(pack_gemm(pfc1_, "policy_fc1.weight", "policy_fc1.bias", flattened(64, r, rp), err));
        TRY(pack_gemm(pfc2_, "policy_fc2.weight", "policy_fc2.bias", fc(r, rp, M0_POLICY_SIZE, M0_POLICY_SIZE), err));
    } else {
        TRY(pack_gemm(pfc1_, "policy_fc.weight", "policy_fc.bias", flattened(64, M0_POLICY_SIZE, M0_POLICY_SIZE), err));
    }
    {
        const HostTensor* ls = get("_policy_logit_scale_raw", err); if (!ls) return M0_ERR_INVALID;
        nparams_ += 1;
        double raw = ls->data.empty() ? 0.0 : ls->data[0];
        double sp = raw > 20.0 ? raw : log1p(exp(raw));
        logit_scale_ = (float)std::min(5.0, sp + 1e-3);
    }
    // value head
    TRY(pack_gemm(vh0_, "value_head.0.weight", "", fc(C, P, 128, 128), err, &vh_w));
    TRY(upload_norm(vh1_n_, "value_head.1", 128, 128, err, &vh_n));
    TRY(pack_gemm(vh3_, "value_head.3.weight", "", fc(128, 128, 128, 128), err));
    TRY(upload_norm(vh4_n_, "value_head.4", 128, 128, err));
    TRY(pack_joint_head(ph_w, vh_w, ph_n, vh_n, err));
    const int h1 = 2 * C, h1p = ceil_to(h1, 32), h2 = C, h2p = ceil_to(C, 32);
    TRY(pack_gemm(vfc1_, "value_fc1.weight", "value_fc1.bias", flattened(128, h1, h1p), err));
    TRY(pack_gemm(vfc2_, "value_fc2.weight", "value_fc2.bias", fc(h1, h1p, h2, h2p), err));
    TRY(pack_gemm(vgate_, "value_gate.0.weight", "value_gate.0.bias", fc(h2, h2p, h2, h2p), err));
    TRY(pack_gemm(vfc3_, "value_fc3.weight", "value_fc3.bias", fc(h2, h2p, 1, 32), err));
    if (cfg_.self_supervised) TRY(pack_ssl_heads(err));
    sd_.clear();
    // uploads (blocking NULL-stream copies) have landed before any non-blocking stream reads them
    if (!M0_HIP(*hip_, hipDeviceSynchronize())) { err = "weight upload failed: " + hip_->message(); return M0_ERR_HIP; }
    make_plan();
    finalized_ = true;
    return M0_OK;
}
