"""The networks, inputs and weight mutations that tests/test_net_layers.py (CPU) and tests/test_net_layers_gpu.py share."""
import torch

from oracle import net_layers as nl
from oracle import net_ref

B = 6            # a partial 4-board tile, three attention pairs, one 256-row FC tile
PLANES_SEED = 5
SSL5 = ["piece", "threat", "pin", "fork", "control"]


def r24_cfg(**kw):
    return dict(dict(planes=19, channels=320, blocks=24, attention_heads=20, policy_size=4672, norm="group", activation="silu",
                     preact=True, policy_factor_rank=128, self_supervised=True, ssl_tasks=SSL5), **kw)


def shipped_cfg(**kw):
    return dict(dict(planes=19, channels=288, blocks=22, attention=True, attention_heads=18, policy_size=4672, norm="group",
                     activation="silu", value_activation="leaky_relu", preact=True, policy_factor_rank=160,
                     infer_attention_stride=2, self_supervised=True, ssl_tasks=SSL5), **kw)


def planes():
    return nl.random_planes(B, PLANES_SEED)


# ---- one network per supported trunk width that is neither 64 nor 320 (tests/test_net_widths_gpu.py, tests/test_net_layers.py) ----
# Four blocks: res, res, res, att, res -- an attention block that writes the next block's second output, a last block that
# writes none.  C / 16 heads, group norm, preact and the five SSL tasks on every row; the remaining switches are spread so that
# each is met off 64 and 320 once (the "switch" column).
#
#   C    switch                               what the width is there for
#   32   --                                   one 32-column tile, ew_board in one wave, two dead attention waves, SE hidden 8,
#                                             SSL width 16 padded to 32
#   96   value_activation="leaky_relu"        no multiple of 64, H = 6, the LayerNorm loop ends mid-pass, SE hidden 24, SSL 48 -> 64
#   160  policy_factor_rank=0 (dense FC)      no multiple of 64, H = 10, value_fc1 on the big-tile split-K path, SSL width 80 -> 96
#   192  attention_relbias=False              GroupNorm epilogues with an unfused SSL conv (N = 96)
#   256  activation="relu", se=False          widest unpadded trunk under the padded band, SSL N = 128 in the two-wave-group epilogue
#   352  --                                   above 320 and no multiple of 64: 704 threads, H = 22, SE hidden 88
#   384  --                                   the upper bound: both launch bounds, the largest LDS, SSL N = 192 unfused
WIDE_B = 17      # five 4-board tiles (three padded boards), three se_gate groups (the last ragged), two attn_core board groups
LONG_B = 257     # two 256-row FC tiles, 17 attention board groups: on the 32 and 96 rows only


def width_cfg(C, **kw):
    return dict(dict(planes=19, channels=C, blocks=4, attention_heads=C // 16, policy_size=4672, norm="group", activation="silu",
                     preact=True, policy_factor_rank=32, self_supervised=True, ssl_tasks=SSL5), **kw)


WIDTHS = [
    (32, width_cfg(32)),
    (96, width_cfg(96, value_activation="leaky_relu")),
    (160, width_cfg(160, policy_factor_rank=0)),
    (192, width_cfg(192, attention_relbias=False)),
    (256, width_cfg(256, activation="relu", se=False)),
    (352, width_cfg(352)),
    (384, width_cfg(384)),
]
WIDTH_IDS = [str(c) for c, _ in WIDTHS]
LONG_WIDTHS = [w for w in WIDTHS if w[0] in (32, 96)]


def wide_planes(b=WIDE_B):
    return nl.random_planes(b, PLANES_SEED)


def weights(cfg, seed=0, sharp=False, trained=False, on=None):
    """trained: the regime of nl.trained_like, its attention and value scales set on the boards `on` (default planes())."""
    sd = net_ref.random_state_dict(cfg, seed)
    if trained:
        return nl.trained_like(sd, cfg, seed, planes() if on is None else on)
    return nl.sharpen(sd, cfg) if sharp else sd


# ---- one-layer mutations of R24-320: (name, step, function of the float64 state dict -> mutated copy) ------------------------
ATT3 = "tower.11"      # the 3rd attention block: step 3 + 11
RES10 = "tower.13"     # residual block 10 (from 0): step 3 + 13; tower.14 consumes its stream


def _mut(fn):
    def apply(sd):
        out = {k: v.clone() for k, v in sd.items()}
        fn(out)
        return out
    return apply


def _swap(sd, key, i, j):
    sd[key][[i, j]] = sd[key][[j, i]]


def _swap_norm(sd, prefix):
    _swap(sd, prefix + ".weight", 3, 4)
    _swap(sd, prefix + ".bias", 3, 4)


def _zero(key, index):
    def fn(sd):
        sd[key][index] = 0.0
    return fn


MUTATIONS = [
    ("rel_bias of head 19 dropped", 14, _mut(_zero(ATT3 + ".rel_bias", (0, 19)))),
    ("rel_bias row of query square 63 dropped", 14, _mut(_zero(ATT3 + ".rel_bias", (0, slice(None), 63)))),
    ("one LayerNorm beta dropped", 14, _mut(_zero(ATT3 + ".norm.bias", 0))),
    ("bn2 gamma/beta of channels 3 and 4 swapped", 16, _mut(lambda sd: _swap_norm(sd, RES10 + ".bn2"))),
    ("se_fc1 bias dropped", 16, _mut(_zero(RES10 + ".se_fc1.bias", slice(None)))),
    ("se_fc2 bias dropped", 16, _mut(_zero(RES10 + ".se_fc2.bias", slice(None)))),
    ("corner tap of conv2 zeroed on 16 channels", 16, _mut(_zero(RES10 + ".conv2.weight", (slice(0, 16), slice(None), 0, 0)))),
    # visible in the second output alone: the next block's bn1, applied by the step that writes the stream
    ("next block's bn1 gamma/beta of channels 3 and 4 swapped", 16, _mut(lambda sd: _swap_norm(sd, "tower.14.bn1"))),
]


# ---- one-layer mutations of a WIDTHS row: the same kinds, at the layers of the four-block tower -------------------------------
W_RES = "tower.1"      # step 4: a residual block that writes the next block's second output
W_ATT = "tower.3"      # step 6: the attention block
SE_FC1_ROW = 352       # the neighbour of the se=False row drops se_fc1.bias where the others drop se_fc2.bias


def _swap_across_groups(sd):
    """Channels 15 and 16: the last of GroupNorm group 0 and the first of group 1."""
    _swap(sd, W_RES + ".bn2.weight", 15, 16)
    _swap(sd, W_RES + ".bn2.bias", 15, 16)


def width_mutations(C, cfg):
    """[(name, step, mutate)] for one row of WIDTHS: three mutations, each of one parameter set of one layer."""
    full = net_ref.full_cfg(cfg)
    out = [("bn2 gamma/beta of channels 15 and 16 swapped", 4, _mut(_swap_across_groups))]
    if not full["se"]:
        out.append(("corner tap of conv2 zeroed on 16 channels", 4, _mut(_zero(W_RES + ".conv2.weight", (slice(0, 16), slice(None), 0, 0)))))
    elif C == SE_FC1_ROW:
        out.append(("se_fc1 bias dropped", 4, _mut(_zero(W_RES + ".se_fc1.bias", slice(None)))))
    else:
        out.append(("se_fc2 bias dropped", 4, _mut(_zero(W_RES + ".se_fc2.bias", slice(None)))))
    if full["attention_relbias"]:
        out.append((f"rel_bias of head {C // 16 - 1} dropped", 6, _mut(_zero(W_ATT + ".rel_bias", (0, C // 16 - 1)))))
    else:
        out.append((f"LayerNorm beta of channel {C - 1} dropped", 6, _mut(_zero(W_ATT + ".norm.bias", C - 1))))
    return out


WIDTH_MUTATIONS = [(C, cfg, *m) for C, cfg in WIDTHS for m in width_mutations(C, cfg)]
WIDTH_MUTATION_IDS = [f"{m[0]}:{m[2]}" for m in WIDTH_MUTATIONS]


# ---- the "trained" regime (nl.trained_like): its networks and its mutations of 320 x 6 ----------------------------------------
# 320 x 6 and every WIDTHS row have the same first five tower layers (res, res, res, att, res), so W_RES and W_ATT and the
# steps of width_mutations hold for 320 x 6 too.
REGIME_WIDTHS = (96, 192, 352)


def regime_networks():
    """name -> (cfg, boards): the networks tests/test_net_regimes_gpu.py runs, each with the boards its scales are set on."""
    nets = {"320x6": (r24_cfg(blocks=6), planes()),
            "288in320": (r24_cfg(channels=288, attention_heads=18, blocks=6, infer_attention_stride=2), planes())}
    for C in REGIME_WIDTHS:
        nets[f"width_{C}"] = (dict(WIDTHS)[C], wide_planes())
    return nets


def regime_weights(name):
    cfg, x = regime_networks()[name]
    return weights(cfg, trained=True, on=x)


def _flip_negative_gain(sd):
    """The first negative bn2 gain that is not the -64 one changes its sign."""
    w = sd[W_RES + ".bn2.weight"]
    i = int(((w < 0) & (w > -64)).nonzero()[0])
    w[i] = -w[i]


def _halve_largest_gain(sd):
    w = sd[W_RES + ".bn2.weight"]
    i = int(w.argmax())
    assert float(w[i]) == 64.0
    w[i] = 32.0


def regime_mutations(cfg):
    """[(name, step, mutate)] on 320 x 6 in the trained regime: the three of width_mutations, the remaining kinds of MUTATIONS at
    the same two layers, and two that mean something in this regime alone."""
    return width_mutations(320, cfg) + [
        ("rel_bias row of query square 63 dropped", 6, _mut(_zero(W_ATT + ".rel_bias", (0, slice(None), 63)))),
        ("one LayerNorm beta dropped", 6, _mut(_zero(W_ATT + ".norm.bias", 0))),
        ("corner tap of conv2 zeroed on 16 channels", 4, _mut(_zero(W_RES + ".conv2.weight", (slice(0, 16), slice(None), 0, 0)))),
        ("next block's bn1 gamma/beta of channels 3 and 4 swapped", 4, _mut(lambda sd: _swap_norm(sd, "tower.2.bn1"))),
        ("sign of one negative bn2 gain flipped", 4, _mut(_flip_negative_gain)),
        ("the +64 bn2 gain replaced by +32", 4, _mut(_halve_largest_gain)),
    ]
