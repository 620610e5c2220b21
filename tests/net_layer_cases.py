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


def weights(cfg, seed=0, sharp=False):
    sd = net_ref.random_state_dict(cfg, seed)
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
