"""What the per-layer GPU parity tests share: one tapped forward per step, the check of every step and of the heads of one
network against float64 within MARGIN x the storage model (oracle/net_layers.py), and the record of every comparison in
tests/_build/net_layer_parity.jsonl.  Used by tests/test_net_layers_gpu.py and tests/test_net_widths_gpu.py."""
import json
import os

import numpy as np
import torch

from oracle import net_layers as nl
from oracle import net_ref

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(obs):
    print("net layer parity", json.dumps(obs))
    try:
        os.makedirs(os.path.join(_ROOT, "tests", "_build"), exist_ok=True)
        with open(os.path.join(_ROOT, "tests", "_build", "net_layer_parity.jsonl"), "a") as f:
            f.write(json.dumps(obs) + "\n")
    except OSError:
        pass


def _nchw(t, C):
    """A tap f32 [B,64,Cp] as the oracle's [B,C,8,8] (the real channels)."""
    t = torch.from_numpy(t)
    return t.reshape(t.shape[0], 8, 8, t.shape[2]).permute(0, 3, 1, 2)[:, :C].double()


def _tap_all(be, x):
    """One tapped forward per step: [(policy, value, ssl, stream, second)]."""
    steps, _ = be.tap_info()
    return [be.infer_tap(x, s) for s in range(steps)]


def _check_network(tag, cfg, sd, taps, x, plan, feed_blocks=False):
    """Every step and the heads of one network against float64, within MARGIN x the storage model; all failures at once.
    feed_blocks: the model of a residual block reads the block's second input, AA_, as the GPU's step before wrote it (that
    step's tapped second output, judged there against float64) instead of recomputing it from the stream; the float64 reference
    is the same either way."""
    full = net_ref.full_cfg(cfg)
    C = int(full["channels"])
    s64 = nl.sd64(sd)
    sched = nl.schedule(cfg)
    assert len(taps) == len(sched)
    failures = []

    def judge(what, got, ref, model, maps=True):
        c = nl.compare(got, ref, model, maps)
        _record({"case": tag, "what": what, **{k: c[k] for k in ("err", "model", "ratio")}})
        if not c["ok"]:
            failures.append((what, c, nl.worst(got, ref) if maps else None))

    for s, st in enumerate(sched):
        stream, second = taps[s][3], taps[s][4]
        if stream.shape[2] > C:                                # zero-padded trunk: the padding stays exactly zero
            assert not stream[:, :, C:].any(), (tag, s)
            assert second is None or not second[:, :, C:].any(), (tag, s)
        if not st["run"]:                                      # a step that does not exist hands the bits on
            assert second is None and s > 0 and np.array_equal(stream, taps[s - 1][3]), (tag, s)
            continue
        xin = x.double() if s == 0 else _nchw(taps[s - 1][3], C)
        ref, ref2 = nl.step64(s64, cfg, s, xin)
        block_in = None
        if feed_blocks and st["kind"] == "res":                # the last step that ran wrote AA_ for this block
            prev = max(q for q in range(s) if sched[q]["run"])
            assert taps[prev][4] is not None, (tag, s)
            block_in = _nchw(taps[prev][4], C)
        mod, mod2 = nl.step_model(s64, cfg, s, xin, plan, block_in)
        judge(f"step{s}:{st['kind']}", _nchw(stream, C), ref, mod)
        assert (second is None) == (ref2 is None), (tag, s)
        if second is not None:
            judge(f"step{s}:{st['kind']}:second", _nchw(second, C), ref2, mod2)
    p, v, ssl = taps[-1][:3]
    feats = _nchw(taps[-1][3], C)
    p64, v64, ssl64 = nl.heads64(s64, cfg, feats)
    pm, vm, sslm = nl.heads_model(s64, cfg, feats, plan)
    judge("logits", torch.from_numpy(p), p64, pm, maps=False)
    judge("value", torch.from_numpy(v), v64, vm, maps=False)
    for t in (ssl or {}):
        judge(f"ssl:{t}", torch.from_numpy(ssl[t]), ssl64[t], sslm[t])
    assert not failures, (tag, failures)
