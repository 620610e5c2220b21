"""GPU parity per layer in the "trained" weight regime (oracle/net_layers.trained_like): streams in the hundreds, GroupNorm groups
whose mean is ten times their standard deviation, negative gains and gains of +-64 that drive the activation beyond +-88.8,
saturated squeeze-excite gates, peaked softmaxes behind a strong attention branch, a value head that saturates tanh on some
boards and not on others, the policy logit scale at its 5.0 clamp.  tests/test_net_regimes.py asserts those conditions on the
float64 chain of each network here and holds one-layer mutations 2 x MARGIN above the storage model in this regime.

The networks: 320 x 6 with the default switches and with M0_FUSE_TAIL=0, M0_FUSE_ATTN=0 (raw conv2 and proj outputs stored as
fp16 at magnitude); 288 in a 320-wide trunk with infer_attention_stride=2 (the padding exactly zero under the offsets); the
rows 96, 192 and 352 of tests/net_layer_cases.WIDTHS at 17 boards.  The method, the metric and the bound MARGIN = 3 x the storage
model are those of tests/test_net_layers_gpu.py, through the same _check_network.  Besides: every output finite, the values of
the saturated boards right in sign and within the bound taken over those boards alone, and a board's taps bit-identical alone
and inside its batch.

Every comparison appends to tests/_build/net_layer_parity.jsonl.  Largest ratio (error / model error) per network over all steps
and heads, measured on an MI355X (rel, abs):
    trained_320x6 1.021, 1.017    trained_320x6:split 1.053, 1.122    trained_288in320_stride2 1.006, 1.209
    trained_width_96 1.002, 1.000    trained_width_192 1.011, 1.000    trained_width_352 1.005, 1.022
i.e. no step or head came near MARGIN, and neither a kernel nor the storage model had to change: at these magnitudes the model's
own error is 1e-2 rel and 0.2-0.3 abs on the residual steps (fp16 storage of values in the hundreds), and the kernels' fp32
statistics, exp and reciprocal stay a few per cent of that.  Two scratch changes to conv_epilogue.h, not kept, do fail here:
silu as v * exp(v) / (1 + exp(v)) (non-finite outputs on the four networks whose epilogues use act_fast) and
|gamma| for gamma in gn16_affine (all six networks, beyond MARGIN).
"""
import numpy as np
import pytest
import torch

from oracle import net_layers as nl
from tests import net_layer_cases as cases
from tests.net_layer_checks import _check_network, _nchw, _tap_all

pytestmark = pytest.mark.gpu


def _check_finite(tag, taps):
    for s, (p, v, ssl, stream, second) in enumerate(taps):
        outs = [p, v, stream] + list((ssl or {}).values()) + ([] if second is None else [second])
        assert all(np.isfinite(o).all() for o in outs), (tag, s)


def _check_saturated_values(tag, cfg, sd, taps, plan):
    """On the GPU's own last stream float64 saturates tanh on some boards (|value| > 0.99) and leaves one below 0.5; on the
    saturated boards the GPU's value has float64's sign and lies within MARGIN x the storage model's error over those boards."""
    s64 = nl.sd64(sd)
    feats = _nchw(taps[-1][3], int(cfg["channels"]))
    v64 = nl.heads64(s64, cfg, feats)[1]
    vm = nl.heads_model(s64, cfg, feats, plan)[1]
    got = torch.from_numpy(taps[-1][1]).double()
    sat = v64.abs() > 0.99
    assert bool(sat.any()) and float(v64.abs().min()) < 0.5, (tag, v64.tolist())
    bound = nl.MARGIN * float((vm - v64)[sat].abs().max())
    print("saturated values", tag, got[sat].tolist(), v64[sat].tolist(), "bound", bound)
    assert bool((torch.sign(got[sat]) == torch.sign(v64[sat])).all()), (tag, got.tolist())
    assert float((got - v64)[sat].abs().max()) <= bound, (tag, got[sat].tolist(), v64[sat].tolist(), bound)


def _run(name, tag, monkeypatch=None, fuse_tail=True, fuse_attn=True, feed_blocks=False, keep=False):
    """One regime network: created (the kernel switches are read then), tapped at every step, judged."""
    from matrix0_amd.backend import M0Backend
    cfg, x = cases.regime_networks()[name]
    sd = cases.regime_weights(name)
    if not fuse_tail:
        monkeypatch.setenv("M0_FUSE_TAIL", "0")
    if not fuse_attn:
        monkeypatch.setenv("M0_FUSE_ATTN", "0")
    be = M0Backend.from_state_dict(cfg, sd)
    try:
        taps = _tap_all(be, x.numpy())
        plan = nl.kernel_plan(cfg, fuse_tail, fuse_attn)
        assert len(taps) == len(nl.schedule(cfg)) and taps[0][3].shape[0] == x.shape[0]
        _check_finite(tag, taps)
        _check_network(tag, cfg, sd, taps, x, plan, feed_blocks=feed_blocks)
        _check_saturated_values(tag, cfg, sd, taps, plan)
    except BaseException:
        keep = False
        raise
    finally:
        if not keep:
            be.close()
    return be, taps, x


def _check_board_alone(be, taps, x, b, steps):
    """Board b alone (B = 1) against board b of the batch: streams, second outputs, logits, value and SSL maps, bit for bit."""
    for s in steps:
        p, v, ssl, stream, second = be.infer_tap(x[b:b + 1].numpy(), s)
        assert np.array_equal(stream[0], taps[s][3][b]), s
        assert (second is None) == (taps[s][4] is None) and (second is None or np.array_equal(second[0], taps[s][4][b])), s
        assert np.array_equal(p[0], taps[s][0][b]) and v[0] == taps[s][1][b], s
        for t in ssl:
            assert np.array_equal(ssl[t][0], taps[s][2][t][b]), (s, t)


def test_trained_regime_320x6():
    """All 11 steps and the heads with the default switches (conv_zs with its fused tail, the fused attention block); then
    board 3 of the 6 alone, at every step."""
    be, taps, x = _run("320x6", "trained_320x6", keep=True)
    try:
        _check_board_alone(be, taps, x, 3, range(len(taps)))
    finally:
        be.close()


def test_trained_regime_320x6_split_kernels(monkeypatch):
    """conv + se_gate + ew_board and qkv + attn_core + proj + ew_board: conv2's and proj's raw outputs pass through fp16."""
    _run("320x6", "trained_320x6:split", monkeypatch, fuse_tail=False, fuse_attn=False)


def test_trained_regime_padded_288_with_attention_stride():
    """288 channels in the 320-wide trunk, the first attention layer skipped: _check_network asserts the 32 padded channels of
    both tapped tensors exactly zero at every step, offsets and levels notwithstanding."""
    cfg, _ = cases.regime_networks()["288in320"]
    assert [s for s, st in enumerate(nl.schedule(cfg)) if not st["run"]] == [6]
    _, taps, _ = _run("288in320", "trained_288in320_stride2")
    assert taps[0][3].shape == (cases.B, 64, 320)


@pytest.mark.parametrize("C", cases.REGIME_WIDTHS)
def test_trained_regime_at_width(C):
    """17 boards: small-tile convs with the unfused GroupNorm (96, 352), the unfused SSL conv at N = 96 (192), the 704-thread
    kernels (352); at 96, board 16 -- the ragged tail of the last tile -- alone as well."""
    be, taps, x = _run(f"width_{C}", f"trained_width_{C}", feed_blocks=True, keep=C == 96)
    if C == 96:
        try:
            _check_board_alone(be, taps, x, 16, range(len(taps)))
        finally:
            be.close()
