"""GPU parity per layer: every step of the HIP forward (stem, chess-feature convs, residual and attention blocks), tapped at its
input and its output through m0_net_infer_tap, against the float64 step of oracle/net_layers.py computed from the GPU's OWN
input (exact fp16), and the heads against float64 heads over the GPU's last stream.

Metric per tensor: the largest per-(board, channel) relative L2 error over the 64 squares, ||got - ref|| / (||ref|| + 1e-3), and
the largest absolute difference (logits and value: the latter alone).  Bound: MARGIN = 3 times the same metric of the fp16
storage model (step_model / heads_model) on those very inputs.  The model rounds to nearest where a kernel stores fp16; the
kernels add fp32 summation order, exp2 / rsqrt / reciprocal approximations and the E[x^2] - mean^2 variance.  The weakest
one-layer mutation of tests/test_net_layers.py stands at 10 times the model.

Every comparison appends its errors and their ratio to the model to tests/_build/net_layer_parity.jsonl (kept out of git).
Largest ratio (error / model error) per variant over all steps and heads, measured on an MI355X (rel, abs):
    r24_320 1.115, 1.129    sharp_320x6:fused 1.040, 1.064    sharp_320x6:split 1.129, 1.137    split_320x6 1.080, 1.125
    padded_288x6_stride2 1.016, 1.099    64ch 1.076, 1.111    320_relu_plain 1.006, 1.000
i.e. the storage model is within 14 % of what the kernels do everywhere, and no step came near MARGIN."""
import numpy as np
import pytest

from oracle import net_layers as nl
from oracle import net_ref
from tests import net_layer_cases as cases
from tests.net_layer_checks import _check_network, _tap_all

pytestmark = pytest.mark.gpu


def _network(cfg, sd, monkeypatch=None, fuse_tail=True, fuse_attn=True):
    """(backend, taps, planes, plan); the kernel switches are read once, when a network is created."""
    from matrix0_amd.backend import M0Backend
    if not fuse_tail:
        monkeypatch.setenv("M0_FUSE_TAIL", "0")
    if not fuse_attn:
        monkeypatch.setenv("M0_FUSE_ATTN", "0")
    be = M0Backend.from_state_dict(cfg, sd)
    x = cases.planes()
    return be, _tap_all(be, x.numpy()), x, nl.kernel_plan(cfg, fuse_tail, fuse_attn)


@pytest.fixture(scope="module")
def r24():
    cfg = cases.r24_cfg()
    sd = cases.weights(cfg)
    be, taps, x, plan = _network(cfg, sd)
    yield cfg, sd, be, taps, x, plan
    be.close()


def test_r24_320_every_step(r24):
    """Network 1: R24-320, all 35 steps, default switches, init regime."""
    cfg, sd, _, taps, x, plan = r24
    assert len(taps) == 35
    _check_network("r24_320", cfg, sd, taps, x, plan)


@pytest.mark.parametrize("fuse_attn", [True, False], ids=["fused", "split"])
def test_sharp_regime_320x6(monkeypatch, fuse_attn):
    """Network 2: q, k x4 and rel_bias x8 in every attention layer: the +-50 clamp binds on ~6 % of the scores, the softmax is
    peaked (mean largest probability 0.75), exp2 runs without a max subtraction near both ends, the fp16 bias table is large."""
    cfg = cases.r24_cfg(blocks=6)
    sd = cases.weights(cfg, sharp=True)
    be, taps, x, plan = _network(cfg, sd, monkeypatch, fuse_attn=fuse_attn)
    be.close()
    _check_network(f"sharp_320x6:{'fused' if fuse_attn else 'split'}", cfg, sd, taps, x, plan)


def test_split_kernels_320x6(monkeypatch):
    """Network 3: M0_FUSE_TAIL=0 and M0_FUSE_ATTN=0: conv + se_gate + ew_board, and qkv + attn_core + proj + ew_board."""
    cfg = cases.r24_cfg(blocks=6)
    sd = cases.weights(cfg)
    be, taps, x, plan = _network(cfg, sd, monkeypatch, fuse_tail=False, fuse_attn=False)
    be.close()
    _check_network("split_320x6", cfg, sd, taps, x, plan)


def test_padded_288x6_with_attention_stride():
    """Network 4: 288 channels (18 heads) in a 320-wide trunk, infer_attention_stride=2: the real channels step by step, the 32
    padded channels exactly zero in both tapped tensors, the skipped attention layer's tap bit-identical to the step before."""
    cfg = cases.r24_cfg(channels=288, attention_heads=18, blocks=6, infer_attention_stride=2)
    sd = cases.weights(cfg)
    be, taps, x, plan = _network(cfg, sd)
    assert be.tap_info() == (11, 320) and taps[0][3].shape == (cases.B, 64, 320)
    be.close()
    assert [s for s, st in enumerate(nl.schedule(cfg)) if not st["run"]] == [6]
    _check_network("padded_288x6_stride2", cfg, sd, taps, x, plan)


@pytest.mark.parametrize("name", ["64ch", "320_relu_plain"])
def test_small_tile_path_and_plain_attention(name):
    """Network 5: 64 channels x 3 blocks, 4 heads (small-tile convs, se_gate, attn_core, ew_board); and 320 x 3 blocks with relu,
    no squeeze-excite, the masked branch alone and no relative bias, whose attention block is the last layer (no second output)."""
    if name == "64ch":
        cfg = dict(planes=19, channels=64, blocks=3, attention_heads=4, policy_size=4672, norm="group", activation="silu",
                   preact=True, policy_factor_rank=32, self_supervised=True, ssl_tasks=["piece", "control"])
    else:
        cfg = cases.r24_cfg(blocks=3, activation="relu", se=False, attention_unmasked_mix=1.0, attention_relbias=False)
    sd = cases.weights(cfg)
    be, taps, x, plan = _network(cfg, sd)
    be.close()
    assert taps[-1][4] is None
    _check_network(name, cfg, sd, taps, x, plan)


def test_tap_is_consistent_with_the_plain_forward(r24):
    """Network 1, bit for bit: a tapped forward computes what infer_np_ssl computes; a tap repeats; the step order, the step
    count and the trunk width are net_ref.tower_layout's; argument errors are M0_ERR_INVALID."""
    cfg, sd, be, taps, x, _ = r24
    layout = net_ref.tower_layout(cfg)
    assert be.tap_info() == (3 + len(layout), 320)
    sched = nl.schedule(cfg)
    assert [st["kind"] for st in sched[3:]] == [k for k, _ in layout]
    p, v, ssl = be.infer_np_ssl(x.numpy())
    for s in (0, 2, 6, 17, 34):
        assert np.array_equal(taps[s][0], p) and np.array_equal(taps[s][1], v), s
        for t in ssl:
            assert np.array_equal(taps[s][2][t], ssl[t]), (s, t)
    for s, st in enumerate(sched):
        assert (taps[s][4] is not None) == (st["next_bn1"] is not None), s
    for s in (2, 5, 6, 33):                                    # tail with and without a second output, attention, last res
        again = be.infer_tap(x.numpy(), s)
        assert np.array_equal(again[3], taps[s][3]), s
        assert (again[4] is None) == (taps[s][4] is None) and (again[4] is None or np.array_equal(again[4], taps[s][4])), s
    # the last tap is the stream the heads read; the plain forward after tapped ones is unchanged
    p2, v2 = be.infer_np(x.numpy())
    assert np.array_equal(p2, p) and np.array_equal(v2, v)
    for bad in (-1, 35):
        with pytest.raises(ValueError):
            be.infer_tap(x.numpy(), bad)
