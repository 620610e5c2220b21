"""ORACLE (test infrastructure, not product): the network forward one step at a time, in float64, and a model of where the HIP
kernels round to fp16.

A "step" is what Net::forward (matrix0_amd/csrc/net.hip) runs between two states of the residual stream, in execution order:
0 = stem (+ positional encoding), 1 = piece-square conv, 2 = interaction conv, 3 + i = tower layer i (net_ref.tower_layout).
Every step maps the stream [B,C,8,8] (step 0: the input planes) to the next stream and, where a residual block consumes that
stream next, to the block's pre-activated input act(GroupNorm(stream; bn1)) -- the kernels' second output, AA_.

  step64 / heads64          the arithmetic of oracle/net_ref.py (its own functions, given float64 tensors)
  step_model / heads_model  the same arithmetic in float64 with a round-to-nearest fp16 wherever a kernel stores a tensor as
                            fp16 or multiplies fp16 operands; every such point cites the kernel code it was read off
  compare                   the per-tensor metric and the bound MARGIN x (model error) that tests/test_net_layers_gpu.py applies
                            to the GPU's steps, and tests/test_net_layers.py to mutated float64 steps (a test of the test)

  trained_like / regime_stats   the "trained" weight regime (sizes, signs and offsets of a checkpoint) and the conditions it meets
                            on the float64 chain (tests/test_net_regimes.py, tests/test_net_regimes_gpu.py); sharpen: the "sharp" one

Which kernel form a step takes (fused epilogue or conv + ew_board) decides where it rounds: kernel_plan restates the choices of
Net::make_plan (net_pack.hip) and Net::conv_norm_act (net.hip)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from . import net_ref

MARGIN = 3.0          # GPU error <= MARGIN x model error; tests/test_net_layers.py holds it below the weakest mutation
LOG2E = 1.44269504088896          # attn_math.h: kLog2e


def sd64(sd) -> Dict[str, torch.Tensor]:
    return {k: torch.as_tensor(v).double() for k, v in sd.items()}


_PEAKS: Optional[List[float]] = None          # regime_stats: the largest magnitude at every rounding point, before it rounds


def _h(t: torch.Tensor) -> torch.Tensor:
    """Round to nearest fp16 (a kernel's fp16 store or MFMA operand)."""
    if _PEAKS is not None:
        _PEAKS.append(float(t.abs().max()) if bool(torch.isfinite(t).all()) else math.inf)
    return t.to(torch.float16).to(torch.float64)


# ---- the schedule ---------------------------------------------------------------------------------------------------------
def schedule(cfg: dict) -> List[dict]:
    """One entry per step: kind ('stem' | 'pst' | 'inter' | 'res' | 'att'), prefix (state-dict prefix), run (False: the
    configuration lacks the step, or the inference stride skips the attention layer) and next_bn1 (prefix of the residual block
    whose bn1 + activation the step also applies, or None) -- TowerLayer::next_bn1 and Plan::first_bn1 of Net::make_plan."""
    cfg = net_ref.full_cfg(cfg)
    stride = max(1, int(cfg["infer_attention_stride"]))
    tower, att_seen = [], 0
    for kind, idx in net_ref.tower_layout(cfg):
        run = True
        if kind == "att":
            att_seen += 1
            run = not (stride > 1 and att_seen % stride != 0)
        tower.append(dict(kind=kind, prefix=f"tower.{idx}", run=run, next_bn1=None))
    nxt = None
    for st in reversed(tower):
        if not st["run"]:
            continue
        st["next_bn1"] = nxt
        nxt = st["prefix"] if st["kind"] == "res" else None
    cf = bool(cfg["chess_features"])
    return [dict(kind="stem", prefix="stem", run=True, next_bn1=None if cf else nxt),
            dict(kind="pst", prefix="chess_features.pst", run=cf and bool(cfg["piece_square_tables"]), next_bn1=None),
            dict(kind="inter", prefix="chess_features.interaction", run=cf, next_bn1=nxt if cf else None)] + tower


def kernel_plan(cfg: dict, fuse_tail: bool = True, fuse_attn: bool = True) -> dict:
    """The kernel forms Net::make_plan picks (net_pack.hip:208-216) and, per head conv, Net::conv_norm_act (net.hip:253-254);
    fuse_tail / fuse_attn False = M0_FUSE_TAIL=0 / M0_FUSE_ATTN=0.

      big          the trunk convs take the 320-column tile: conv_gemm_tile_n(Cp, Cp) == 320 (conv_gemm.hip:205-207), 320 alone
      gn_small     the small tile's GroupNorm epilogue is in use (trunk % 64 == 0): the stem (taps == 9, Cin == 32, net.hip:254),
                   the joint policy_head.0 / value_head.0 launch (N = 64 + 128, net.hip:397-402) and value_head.3 (N = 128)
      ssl_epilogue the SSL head conv has that epilogue too: gn_small AND its packed width Cs = ceil32(max(16, C / 2))
                   (net.hip:57) one of 32 / 64 / 128 / 160 (net.hip:254; conv_gemm.hip:195-198 has no other instance).  False at
                   192 (N = 96) and 384 (N = 192), where the conv is stored raw and ew_board normalises it.
    value_fc1 on the split-K path (widths 160 and 320, net.hip:218-228) sums its eight fp32 partial tiles in fp32 and rounds once,
    after bias and activation (splitk_reduce): no storage point of its own, so the plan has no entry for it.

    Before the widths other than 64 and 320 were run, heads_model applied gn_small to every head conv: wrong for the SSL
    heads at 192 and 384 (modelled as fused, run unfused).  The joint head launch, value_head.3 and value_fc1 were right at every
    width."""
    cfg = net_ref.full_cfg(cfg)
    C = int(cfg["channels"])
    Cp = 320 if 256 < C < 320 else C                           # net.hip: Cp_
    big = Cp % 320 == 0                                        # conv_gemm.hip: conv_gemm_tile_n(Cp, Cp) == 320
    hidden = max(8, int(C * float(cfg["se_ratio"])))
    gn_small = Cp % 64 == 0
    Cs = -(-max(16, C // 2) // 32) * 32                        # net.hip:57 Cs_
    return dict(big=big, gn_small=gn_small, ssl_epilogue=gn_small and Cs in (32, 64, 128, 160), fuse_attn=big and fuse_attn,
                fuse_tail=big and fuse_tail and (not cfg["se"] or (hidden <= 96 and hidden % 4 == 0)))


# ---- float64 --------------------------------------------------------------------------------------------------------------
def _second(out, sd, cfg, st):
    return None if st["next_bn1"] is None else net_ref._act(net_ref._norm(out, sd, st["next_bn1"] + ".bn1", cfg), cfg)


@torch.no_grad()
def step64(sd, cfg, step: int, x: torch.Tensor):
    """(stream after `step`, second output or None) in float64 from the step's input stream x (step 0: the planes).  `sd` from sd64."""
    cfg = net_ref.full_cfg(cfg)
    st = schedule(cfg)[step]
    x = x.double()
    if not st["run"]:
        return x, None
    k = st["kind"]
    if k == "stem":                                            # resnet.py:314-318, 229-232
        out = net_ref._act(net_ref._norm(F.conv2d(x, sd["stem.0.weight"], padding=1), sd, "stem.1", cfg), cfg)
        if cfg["chess_features"]:
            out = out + sd["chess_features.position_encoding"]
    elif k == "pst":                                           # resnet.py:233-238
        t = F.conv2d(x, sd["chess_features.pst_conv.weight"])
        out = x + net_ref._act(net_ref._norm(t, sd, "chess_features.pst_norm", cfg), cfg)
    elif k == "inter":                                         # resnet.py:239-244
        t = F.conv2d(x, sd["chess_features.interaction_conv.weight"], padding=1)
        out = x + net_ref._act(net_ref._norm(t, sd, "chess_features.interaction_norm", cfg), cfg)
    elif k == "res":
        out = net_ref._res_block(x, sd, st["prefix"], cfg)
    else:
        out = net_ref._attention(x, sd, st["prefix"], cfg, net_ref.attention_mask())
    return out, _second(out, sd, cfg, st)


@torch.no_grad()
def heads64(sd, cfg, feats: torch.Tensor):
    """(logits [B,4672], value [B], {task: ssl map}) in float64 from the last stream."""
    cfg = net_ref.full_cfg(cfg)
    return net_ref._heads(feats.double(), sd, cfg, True)


# ---- the storage model ----------------------------------------------------------------------------------------------------
def _gn_from(val, src, sd, prefix):
    """GroupNorm16 of `val` with the statistics of `src`: a kernel that normalises a tensor it has already rounded to fp16 still
    takes the sums from its fp32 values (conv_epilogue.h: EPI_PLAIN's out_stats; net_kernels.hip: ew_gn_channel)."""
    B, C = src.shape[:2]
    g = src.reshape(B, C // 16, -1)
    mean = g.mean(-1)
    rstd = torch.rsqrt(g.var(-1, unbiased=False) + 1e-5)
    mean = mean.repeat_interleave(16, 1)[:, :, None, None]
    rstd = rstd.repeat_interleave(16, 1)[:, :, None, None]
    return (val - mean) * rstd * sd[prefix + ".weight"][None, :, None, None] + sd[prefix + ".bias"][None, :, None, None]


def _model_second(y16, stats_src, sd, cfg, st):
    # every writer of AA_ normalises the fp16 stream it has just stored and rounds the result: conv_tail.h tail_y2 (sums of the
    # rounded y, tail_residual), net_kernels.hip ew_board step 5 and attn_block.hip ab_second_output (sums of the fp32 y)
    if st["next_bn1"] is None:
        return None
    return _h(net_ref._act(_gn_from(y16, stats_src, sd, st["next_bn1"] + ".bn1"), cfg))


def _model_conv_norm(x, sd, cfg, wkey, norm, pad, form, res=None, posenc=None):
    """Net::conv_norm_act (net.hip): out = act(GroupNorm(conv(x))) [+ posenc] [+ res] in one of its three forms."""
    t = F.conv2d(x, _h(sd[wkey]), padding=pad)                 # fp16 weights (net_pack.hip pack_gemm), fp16 operand x, fp32 sums
    if form == "tail":
        # conv_tail.h / conv_zs_tail.h, PRE: act(GroupNorm(t)) on the accumulators -> fp16 image; tail_residual: y = x + image as
        # a packed fp16 add
        return _h(res + _h(net_ref._act(_gn_from(t, t, sd, norm), cfg)))
    if form == "epilogue":
        # conv_epilogue.h EPI_GN / conv_zs_epilogue.h: GroupNorm + act (+ posenc) on the accumulators, one fp16 store
        y = net_ref._act(_gn_from(t, t, sd, norm), cfg)
        return _h(y if posenc is None else y + posenc)
    # unfused: the raw conv is stored as fp16 (conv_epilogue.h EPI_PLAIN / EPI_ELEMENT) with fp32 statistics, then
    # net_kernels.hip ew_board_kernel: act(GroupNorm(fp16 t)) + res + posenc in fp32, one fp16 store
    y = net_ref._act(_gn_from(_h(t), t, sd, norm), cfg)
    if res is not None:
        y = y + res
    if posenc is not None:
        y = y + posenc
    return _h(y)


def _model_res_block(x, sd, cfg, st, plan, block_in=None):
    p = st["prefix"]
    # conv1 reads AA_ = act(bn1(x)) as the previous step stored it (fp16; net.hip:345): `block_in` where the caller has that
    # tensor (the previous step's tapped second output), else recomputed here from the fp16 stream.  The recomputation takes the
    # statistics of the rounded stream where the writer took them of its fp32 values, which moves ~3 % of AA_ by one fp16 step
    # and, through the two convs, ~20 % of the block's output (measured at 256 wide); with AA_ itself 0.7 % remain.
    a = block_in.double() if block_in is not None else _h(net_ref._act(_gn_from(x, x, sd, p + ".bn1"), cfg))
    # conv1 + bn2 + act -> T1_: conv_zs_kernel EPI_GN on the 320-wide trunk, else conv + ew_board (net.hip conv_norm_act)
    t1 = _model_conv_norm(a, sd, cfg, p + ".conv1.weight", p + ".bn2", 1, "epilogue" if plan["big"] else "unfused")
    t = F.conv2d(t1, _h(sd[p + ".conv2.weight"]), padding=1)
    if plan["fuse_tail"]:
        gate = 1.0
        if cfg["se"]:
            # conv_zs_tail.h A-C: channel means and hidden units as fp16 hi + lo pairs (~fp32), W1 and W2 as fp16 fragments
            w = t.mean(dim=(2, 3))
            w = net_ref._act(F.linear(w, _h(sd[p + ".se_fc1.weight"]), sd[p + ".se_fc1.bias"]), cfg)
            gate = torch.sigmoid(F.linear(w, _h(sd[p + ".se_fc2.weight"]), sd[p + ".se_fc2.bias"]))[:, :, None, None]
        y = _h(x + _h(t * gate))                               # conv_zs_tail.h D: gate * t -> fp16 image; conv_tail.h tail_residual
        return y, _model_second(y, y, sd, cfg, st)
    t16 = _h(t)                                                # net.hip: conv2 -> T2_ (fp16) with fp32 sums in S2_
    gate = 1.0
    if cfg["se"]:
        w = t.mean(dim=(2, 3))                                 # net_kernels.hip se_gate_kernel: fp32 weights, pool from S2_
        w = net_ref._act(F.linear(w, sd[p + ".se_fc1.weight"], sd[p + ".se_fc1.bias"]), cfg)
        gate = torch.sigmoid(F.linear(w, sd[p + ".se_fc2.weight"], sd[p + ".se_fc2.bias"]))[:, :, None, None]
    yf = t16 * gate + x                                        # ew_board_kernel step 3
    y = _h(yf)
    return y, _model_second(y, yf, sd, cfg, st)


def _model_attention(x, sd, cfg, st, plan):
    p = st["prefix"]
    B, C = x.shape[:2]
    heads = int(cfg["attention_heads"])
    D = C // heads
    # qkv as fp16: QKV_ (net.hip, split path) / q, k, v in LDS (attn_block.hip ab_stage_qkv)
    qkv = _h(F.conv2d(x, _h(sd[p + ".qkv.weight"]))).reshape(B, 3, heads, D, 64).permute(1, 0, 2, 4, 3)
    q, k, v = qkv[0], qkv[1], qkv[2]
    # attn_math.h attn_softmax_pv: scores in log2 units, fp32; rel_bias * log2(e) as fp16 (net_pack.hip pack_attn:
    # attn_block_bias<_Float16>; attn_core.hip converts the same table into LDS)
    s = torch.matmul(q, k.transpose(-2, -1)) * (LOG2E / math.sqrt(D))
    if cfg["attention_relbias"]:
        s = s + _h(sd[p + ".rel_bias"] * LOG2E)
    e = torch.exp2(torch.clamp(s, -50.0 * LOG2E, 50.0 * LOG2E))          # no max subtraction: the clamp bounds the exponent
    vis = net_ref.attention_mask().double()[None, None]
    mix = float(cfg["attention_unmasked_mix"])
    if 0.0 < mix < 1.0:                                        # attn_math.h attn_branch_weights
        wm, wu = 1.0 - mix, 1.0 - (1.0 - mix)
    elif mix >= 1.0:
        wm, wu = 1.0, 0.0
    else:
        wm, wu = 0.0, 1.0
    cu = wu / e.sum(-1, keepdim=True)
    cm = wm / (e * vis).sum(-1, keepdim=True)
    pf = _h(e * (vis * cm + cu))                               # attn_math.h: pf[u] = (_Float16)(e * (vs * cm + cu)), MFMA operand
    o = _h(torch.matmul(pf, v))                                # attn_math.h attn_pack_o: O as fp16 (O_ / over Q in LDS)
    o = o.transpose(1, 2).reshape(B, 64, C).transpose(1, 2).reshape(B, C, 8, 8)
    t = F.conv2d(o, _h(sd[p + ".proj.weight"]))
    if not plan["fuse_attn"]:
        t = _h(t)                                              # net.hip split path: proj -> T1_ (fp16)
    # attn_block.hip ab_residual_layernorm / ew_board_kernel: residual and LayerNorm in fp32, one fp16 store
    yf = F.layer_norm((t + x).permute(0, 2, 3, 1), (C,), sd[p + ".norm.weight"], sd[p + ".norm.bias"], 1e-5).permute(0, 3, 1, 2)
    y = _h(yf)
    return y, _model_second(y, yf, sd, cfg, st)


@torch.no_grad()
def step_model(sd, cfg, step: int, x: torch.Tensor, plan: Optional[dict] = None, block_in: Optional[torch.Tensor] = None):
    """step64's results as the kernels' arithmetic gives them up to fp32 effects: float64 with fp16 rounding at the kernels'
    storage points.  x is the fp16-exact input (a GPU tap, or a rounded float64 stream); block_in, for a residual block, its
    second input AA_ as the step before wrote it (that step's second output), where the caller has it."""
    cfg = net_ref.full_cfg(cfg)
    plan = plan or kernel_plan(cfg)
    st = schedule(cfg)[step]
    x = x.double()
    if not st["run"]:
        return x, None
    k = st["kind"]
    if k == "stem":
        # planes_to_nhwc (net_kernels.hip) stores the planes as fp16; the stem runs conv_gemm_kernel<9> with the GroupNorm
        # epilogue where the trunk is a multiple of 64 wide and nothing else is asked of it (net.hip conv_norm_act)
        pe = sd["chess_features.position_encoding"] if cfg["chess_features"] else None
        form = "epilogue" if plan["gn_small"] and st["next_bn1"] is None else "unfused"
        y = _model_conv_norm(_h(x), sd, cfg, "stem.0.weight", "stem.1", 1, form, posenc=pe)
    elif k in ("pst", "inter"):
        form = "tail" if plan["fuse_tail"] else "unfused"      # conv_big_kernel / conv_zs_kernel EPI_TAIL_PRE, else conv + ew_board
        y = _model_conv_norm(x, sd, cfg, st["prefix"] + "_conv.weight", st["prefix"] + "_norm", 0 if k == "pst" else 1, form, res=x)
    elif k == "res":
        return _model_res_block(x, sd, cfg, st, plan, block_in)
    else:
        return _model_attention(x, sd, cfg, st, plan)
    # tail_y2 normalises the rounded y with its own sums; ew_board takes the sums of the fp32 y: the difference is far below
    # one fp16 rounding, and the rounded y stands for both here
    return y, _model_second(y, y, sd, cfg, st)


@torch.no_grad()
def heads_model(sd, cfg, feats: torch.Tensor, plan: Optional[dict] = None):
    """heads64 with the kernels' fp16 points (net.hip, after the tower): every head conv and FC has fp16 weights and an fp16
    output, except the logits and the value, which leave their GEMM as fp32."""
    cfg = net_ref.full_cfg(cfg)
    plan = plan or kernel_plan(cfg)
    x = feats.double()
    B = x.shape[0]
    # conv_gemm_kernel<1> EPI_GN: policy_head.0 and value_head.0 in the joint launch (net.hip:397-402), value_head.3 with N = 128
    # (net.hip:254, 416); without it (trunk % 64 != 0) each is conv + ew_board (net.hip:404, 413, 259-266)
    small = "epilogue" if plan["gn_small"] else "unfused"
    # the SSL head conv has N = C / 2: the epilogue exists for 32 / 64 / 128 / 160 alone (net.hip:254, 431)
    ssl_form = "epilogue" if plan["ssl_epilogue"] else "unfused"
    ph =_model_conv_norm(x, sd, cfg, "policy_head.0.weight", "policy_head.1", 0, small)       # PH2_ (joint launch hv_)
    pflat = ph.reshape(B, -1)
    if int(cfg["policy_factor_rank"]) > 0:
        f1 = _h(F.relu(F.linear(pflat, _h(sd["policy_fc1.weight"]), sd["policy_fc1.bias"])))   # F1_: EPI_ELEMENT, fp16
        p_ = F.linear(f1, _h(sd["policy_fc2.weight"]), sd["policy_fc2.bias"])
    else:
        p_ = F.linear(pflat, _h(sd["policy_fc.weight"]), sd["policy_fc.bias"])
    p_ = p_ * torch.clamp(F.softplus(sd["_policy_logit_scale_raw"]) + 1e-3, max=5.0)           # out_f32, out_scale
    v = _model_conv_norm(x, sd, cfg, "value_head.0.weight", "value_head.1", 0, small)          # VH2_
    v = _model_conv_norm(v, sd, cfg, "value_head.3.weight", "value_head.4", 0, small)          # VH_
    v = v.reshape(B, -1)
    v = _h(net_ref._value_act(F.linear(v, _h(sd["value_fc1.weight"]), sd["value_fc1.bias"]), cfg))     # F2_ (split-K sums in fp32)
    v = _h(net_ref._value_act(F.linear(v, _h(sd["value_fc2.weight"]), sd["value_fc2.bias"]), cfg))     # F3_
    v = _h(v * torch.sigmoid(F.linear(v, _h(sd["value_gate.0.weight"]), sd["value_gate.0.bias"])))     # F4_: GemmArgs::mul
    v = torch.tanh(F.linear(v, _h(sd["value_fc3.weight"]), sd["value_fc3.bias"])).squeeze(-1)          # VAL_ fp32
    ssl = {}
    if cfg["self_supervised"]:
        for task in cfg["ssl_tasks"]:
            if task in net_ref.SSL_OUT:
                h = f"ssl_heads.{task}"
                t = _model_conv_norm(x, sd, cfg, h + ".0.weight", h + ".1", 0, ssl_form)       # SH2_
                ssl[task] = _h(F.conv2d(t, _h(sd[h + ".3.weight"])))                           # SO_ fp16, widened by nhwc_to_nchw_f32
    return p_, v, ssl


# ---- inputs and weight regimes of the tests ------------------------------------------------------------------------------------
def random_planes(B: int, seed: int) -> torch.Tensor:
    """The input planes of tests/test_net_gpu.py: sparse piece planes, 0/1 flag planes, two counters in [0,1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, 19, 8, 8)
    x[:, :12] = (torch.rand(B, 12, 8, 8, generator=g) < 0.08).float()
    x[:, 12:17] = (torch.rand(B, 5, 1, 1, generator=g) < 0.5).float()
    x[:, 17:] = torch.rand(B, 2, 1, 1, generator=g)
    return x


def sharpen(sd, cfg) -> dict:
    """The "sharp" regime: in every attention layer the q and k rows of qkv.weight x4 and rel_bias x8 -- scores of a trained
    network's size, so that the +-50 clamp binds, exp2 works without a max subtraction near the ends of its range and the fp16
    bias table's quantisation matters."""
    C = int(net_ref.full_cfg(cfg)["channels"])
    out = dict(sd)
    for kind, idx in net_ref.tower_layout(cfg):
        if kind == "att":
            w = sd[f"tower.{idx}.qkv.weight"].clone()
            w[:2 * C] *= 4.0
            out[f"tower.{idx}.qkv.weight"] = w
            if f"tower.{idx}.rel_bias" in sd:
                out[f"tower.{idx}.rel_bias"] = sd[f"tower.{idx}.rel_bias"] * 8.0
    return out


@torch.no_grad()
def attention_stats(sd, cfg, step: int, x: torch.Tensor) -> dict:
    """Of an attention step on input x, in float64: the scores' std, the fraction outside the +-50 clamp and the mean largest
    probability of the unmasked softmax."""
    cfg = net_ref.full_cfg(cfg)
    p = schedule(cfg)[step]["prefix"]
    B, C = x.shape[:2]
    heads = int(cfg["attention_heads"])
    D = C // heads
    qkv = F.conv2d(x.double(), sd[p + ".qkv.weight"]).reshape(B, 3, heads, D, 64).permute(1, 0, 2, 4, 3)
    s = torch.matmul(qkv[0], qkv[1].transpose(-2, -1)) / math.sqrt(D)
    if cfg["attention_relbias"]:
        s = s + sd[p + ".rel_bias"]
    pr = F.softmax(torch.clamp(s, -50.0, 50.0), dim=-1)
    return {"std": float(s.std()), "clamped": float((s.abs() > 50.0).double().mean()), "maxprob": float(pr.max(-1).values.mean())}


def _attn_parts(sd, cfg, p, x):
    """q, k, v [B,H,64,D], the scores before the clamp and the mixed heads before proj [B,C,8,8] of attention layer p, float64."""
    B, C = x.shape[:2]
    heads = int(cfg["attention_heads"])
    D = C // heads
    qkv = F.conv2d(x.double(), sd[p + ".qkv.weight"]).reshape(B, 3, heads, D, 64).permute(1, 0, 2, 4, 3)
    q, k, v = qkv[0], qkv[1], qkv[2]
    s = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(D)
    if cfg["attention_relbias"]:
        s = s + sd[p + ".rel_bias"]
    c = torch.clamp(s, -50.0, 50.0)
    mix = float(cfg["attention_unmasked_mix"])
    pm = F.softmax(c.masked_fill(~net_ref.attention_mask()[None, None], -1e4), dim=-1)
    pu = F.softmax(c, dim=-1)
    pr = (1.0 - mix) * pm + mix * pu if 0.0 < mix < 1.0 else (pm if mix >= 1.0 else pu)
    o = torch.matmul(pr, v).transpose(1, 2).reshape(B, 64, C).transpose(1, 2).reshape(B, C, 8, 8)
    return q, k, v, s, o


def _res_parts(sd, cfg, p, x):
    """Of residual block p (preact) on the stream x, float64: bn2's output before the activation, and the squeeze-excite hidden
    units after theirs (None without squeeze-excite)."""
    a = net_ref._act(net_ref._norm(x.double(), sd, p + ".bn1", cfg), cfg)
    pre = net_ref._norm(F.conv2d(a, sd[p + ".conv1.weight"], padding=1), sd, p + ".bn2", cfg)
    if not cfg["se"]:
        return pre, None
    w = F.conv2d(net_ref._act(pre, cfg), sd[p + ".conv2.weight"], padding=1).mean(dim=(2, 3))
    return pre, net_ref._act(F.linear(w, sd[p + ".se_fc1.weight"], sd[p + ".se_fc1.bias"]), cfg)


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


@torch.no_grad()
def trained_like(sd, cfg, seed: int = 0, planes: Optional[torch.Tensor] = None) -> dict:
    """The "trained" regime: a random_state_dict of any supported width (group norm) given the sizes, signs and offsets of a
    trained checkpoint, everything at once, so that every place where a kernel could be wrong only off O(1) is exercised:

      GroupNorm gains    lognormal, median 2; one in ten negative; per layer one channel at +64 and one at -64 (a normalised value
                         stays within sqrt(1023) ~ 32 of zero, so the activation meets inputs beyond +-88.8, where fp32 exp
                         overflows); biases uniform in +-1.5
      position_encoding  x30 plus a level per 16-channel group: groups whose mean is many times their standard deviation
      residual blocks    conv2.weight x6; se_fc2.weight scaled to gate logits of rms 3 around biases uniform in +-3: a good part
                         of the gates saturated, the rest anywhere in between
      attention          norm.weight x12, one in ten negative; norm.bias a per-channel offset plus a per-group level; rel_bias x6;
                         the q and k rows of qkv.weight scaled to rms 3.5, the v rows to rms 4 and proj.weight so that the
                         attention branch has twice the rms of the stream it joins -- peaked softmaxes with |q|, |k|, |v| <= 64,
                         and an attention branch that the stream and the LayerNorm do not drown
      heads              value_gate x4; value_fc3 and its bias such that on `planes` one board's value is tanh(0.2) and the
                         farthest board's pre-activation is 0.2 +- 3 (|value| > 0.99); the policy logit scale at its 5.0 clamp

    The attention and value scales are set on the float64 chain over `planes` (default random_planes(6, seed)) as it is built,
    step by step, so the function is deterministic in (sd, cfg, seed, planes) and needs nothing but torch.  regime_stats reports
    the conditions the result meets."""
    full = net_ref.full_cfg(cfg)
    assert full["norm"] == "group"
    g = torch.Generator().manual_seed(7919 + seed)
    out = {k: torch.as_tensor(v).clone().float() for k, v in sd.items()}
    planes = random_planes(6, seed) if planes is None else planes

    def randn(*s):
        return torch.randn(*s, generator=g)

    def rand(*s):
        return torch.rand(*s, generator=g)

    def levels(n, scale):                                      # one level per 16-channel group: +-scale x [0.5, 1.5)
        m = max(1, n // 16)
        return (scale * torch.sign(randn(m)) * (0.5 + rand(m))).repeat_interleave(16)[:n]

    att_norms = {f"tower.{i}.norm" for kind, i in net_ref.tower_layout(full) if kind == "att"}
    for key in sorted(k for k in sd if k.endswith(".weight") and out[k].dim() == 1):
        prefix, n = key[:-len(".weight")], out[key].numel()
        if prefix in att_norms:
            w = 12.0 * out[key]
            out[key] = torch.where(rand(n) < 0.1, -w, w)
            out[prefix + ".bias"] = 4.0 * randn(n) + levels(n, 40.0)
            continue
        w = 2.0 * torch.exp(0.5 * randn(n))
        w = torch.where(rand(n) < 0.1, -w, w)
        i, j = torch.randperm(n, generator=g)[:2].tolist()
        w[i], w[j] = 64.0, -64.0
        out[key] = w
        out[prefix + ".bias"] = 3.0 * rand(n) - 1.5
    if full["chess_features"]:
        pe = out["chess_features.position_encoding"]
        out["chess_features.position_encoding"] = 30.0 * pe + levels(pe.shape[1], 25.0)[None, :, None, None]
    out["_policy_logit_scale_raw"] = torch.tensor(10.0)         # softplus(10) + 1e-3 > 5: the clamp binds
    out["value_gate.0.weight"] = 4.0 * out["value_gate.0.weight"]
    C = int(full["channels"])
    x = planes.double()
    for s, st in enumerate(schedule(full)):
        p = st["prefix"]
        if st["kind"] == "res":
            out[p + ".conv2.weight"] = 6.0 * out[p + ".conv2.weight"]
            if full["se"]:
                out[p + ".se_fc2.bias"] = 6.0 * rand(C) - 3.0
                if st["run"]:
                    hid = _res_parts(sd64(out), full, p, x)[1]
                    out[p + ".se_fc2.weight"] *= 3.0 / _rms(F.linear(hid, out[p + ".se_fc2.weight"].double()))
        elif st["kind"] == "att":
            if full["attention_relbias"]:
                out[p + ".rel_bias"] = 6.0 * out[p + ".rel_bias"]
            if st["run"]:
                q, k, v, _, _ = _attn_parts(sd64(out), full, p, x)
                w = out[p + ".qkv.weight"]
                w[:C] *= 3.5 / _rms(q)
                w[C:2 * C] *= 3.5 / _rms(k)
                w[2 * C:] *= 4.0 / _rms(v)
                o = _attn_parts(sd64(out), full, p, x)[4]
                out[p + ".proj.weight"] *= 2.0 * _rms(x) / _rms(F.conv2d(o, out[p + ".proj.weight"].double()))
        if st["run"]:
            x = step64(sd64(out), full, s, x)[0]
    # the value head: z = value_fc3.weight . (gated features) per board, then an affine map of z
    # (read through heads64 with the weight shrunk until tanh is the identity to float64)
    probe = sd64(out)
    probe["value_fc3.weight"], probe["value_fc3.bias"] = probe["value_fc3.weight"] * 1e-9, torch.zeros(1, dtype=torch.float64)
    z = heads64(probe, full, x)[1] * 1e9
    j = int(torch.argsort(z)[len(z) // 2])
    scale = 3.0 / float((z - z[j]).abs().max())
    out["value_fc3.weight"] = out["value_fc3.weight"] * scale
    out["value_fc3.bias"] = torch.tensor([0.2 - scale * float(z[j])])
    return out


@torch.no_grad()
def regime_stats(sd, cfg, planes: torch.Tensor, chain=None) -> dict:
    """What a weight regime does to the float64 chain over `planes` (sd from sd64), and how far the storage model stays from the
    fp16 range on those inputs:

      stream_max, first_block_in   max |stream| over all steps; at the input of the first residual block
      group_mean_over_std          largest |mean| / std of a (board, 16-channel group) of a stream that feeds a second output
      bn2_pre, second_pre          over residual blocks (over second outputs) the largest m such that one block's bn2 output (one
                                   second output's GroupNorm output) has a value <= -m and a value >= m
      se_outside                   largest fraction, over blocks, of squeeze-excite gates outside [0.02, 0.98]
      attention                    attention_stats of every attention step that runs;  qkv_max: max |q|, |k|, |v| over them
      neg_gains                    fraction of negative norm gains
      values, logit_scale          the value per board; the policy logit scale after its clamp
      finite, peak                 every tensor of step_model (both kernel plans) and heads_model is finite; the largest
                                   magnitude at any of their fp16 rounding points, before it rounds"""
    global _PEAKS
    full = net_ref.full_cfg(cfg)
    chain = chain if chain is not None else chain64(sd, full, planes)
    sched = schedule(full)
    out = dict(stream_max=max(float(y.abs().max()) for _, y, _ in chain), group_mean_over_std=0.0, bn2_pre=0.0, second_pre=0.0,
               se_outside=0.0, attention=[], qkv_max=0.0)
    first_res = [s for s, st in enumerate(sched) if st["kind"] == "res"][0]
    out["first_block_in"] = float(chain[first_res][0].abs().max())

    def both_sides(t):
        return min(float(t.max()), -float(t.min()))

    for s, st in enumerate(sched):
        if not st["run"]:
            continue
        x, y, _ = chain[s]
        if st["next_bn1"] is not None:
            grp = y.reshape(y.shape[0], y.shape[1] // 16, -1)
            out["group_mean_over_std"] = max(out["group_mean_over_std"], float((grp.mean(-1).abs() / grp.std(-1, unbiased=False)).max()))
            out["second_pre"] = max(out["second_pre"], both_sides(net_ref._norm(y, sd, st["next_bn1"] + ".bn1", full)))
        p = st["prefix"]
        if st["kind"] == "res":
            pre, hid = _res_parts(sd, full, p, x)
            out["bn2_pre"] = max(out["bn2_pre"], both_sides(pre))
            if full["se"]:
                gate = torch.sigmoid(F.linear(hid, sd[p + ".se_fc2.weight"], sd[p + ".se_fc2.bias"]))
                out["se_outside"] = max(out["se_outside"], float(((gate < 0.02) | (gate > 0.98)).double().mean()))
        elif st["kind"] == "att":
            out["attention"].append(attention_stats(sd, full, s, x))
            out["qkv_max"] = max(out["qkv_max"], *(float(t.abs().max()) for t in _attn_parts(sd, full, p, x)[:3]))
    gains = torch.cat([v.flatten() for k, v in sd.items() if k.endswith(".weight") and v.dim() == 1])
    out["neg_gains"] = float((gains < 0).double().mean())
    out["values"] = heads64(sd, full, chain[-1][1])[1].tolist()
    out["logit_scale"] = float(torch.clamp(F.softplus(sd["_policy_logit_scale_raw"]) + 1e-3, max=5.0))
    _PEAKS, finite = [], True
    try:
        for plan in (kernel_plan(full), kernel_plan(full, fuse_tail=False, fuse_attn=False)):
            for s in range(len(sched)):
                finite &= all(bool(torch.isfinite(t).all()) for t in step_model(sd, full, s, _h(chain[s][0]), plan) if t is not None)
            pm, vm, sslm = heads_model(sd, full, _h(chain[-1][1]), plan)
            finite &= all(bool(torch.isfinite(t).all()) for t in (pm, vm, *(sslm or {}).values()))
        out["peak"] = max(_PEAKS)
    finally:
        _PEAKS = None
    out["finite"] = finite and math.isfinite(out["peak"])
    return out


@torch.no_grad()
def chain64(sd, cfg, planes: torch.Tensor):
    """Every step in turn, float64 all the way: [(input, stream, second)] per step."""
    out, x = [], planes.double()
    for s in range(len(schedule(cfg))):
        y, y2 = step64(sd, cfg, s, x)
        out.append((x, y, y2))
        x = y
    return out


# ---- the comparator -------------------------------------------------------------------------------------------------------
def metric(got: torch.Tensor, ref: torch.Tensor, maps: bool = True) -> dict:
    """{'rel': max over (board, channel) of ||got - ref||_2 over the 64 squares / (||ref||_2 + 1e-3), 'abs': max |got - ref|};
    maps=False (logits, value): 'abs' alone."""
    got, ref = got.double(), ref.double()
    out = {"abs": float((got - ref).abs().max())}
    if maps:
        d = (got - ref).flatten(2).norm(dim=-1)
        out["rel"] = float((d / (ref.flatten(2).norm(dim=-1) + 1e-3)).max())
    return out


def compare(got: torch.Tensor, ref: torch.Tensor, model: torch.Tensor, maps: bool = True) -> dict:
    """Errors of `got` and of the storage model against the float64 `ref`, their ratios, and ok = every error within
    MARGIN x the model's."""
    e, m = metric(got, ref, maps), metric(model, ref, maps)
    ratio = {k: (e[k] / m[k] if m[k] > 0 else (0.0 if e[k] == 0 else math.inf)) for k in e}
    return {"err": e, "model": m, "ratio": ratio, "ok": all(e[k] <= MARGIN * m[k] for k in e)}


def worst(got: torch.Tensor, ref: torch.Tensor, n: int = 5):
    """The n worst (board, channel, square, got, ref) of a map: the pattern of an error names its cause."""
    d = (got.double() - ref.double()).abs().flatten(2)
    idx = torch.topk(d.flatten(), min(n, d.numel())).indices.tolist()
    C, S = d.shape[1], d.shape[2]
    return [(i // (C * S), (i // S) % C, i % S, float(got.flatten()[i]), float(ref.flatten()[i])) for i in idx]
