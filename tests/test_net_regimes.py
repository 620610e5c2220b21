"""The "trained" weight regime of oracle/net_layers.trained_like on the CPU: the conditions it must meet on the float64 chain of
every network tests/test_net_regimes_gpu.py runs, and the proof that the comparator keeps its power there -- with a stream in
the hundreds one fp16 step is 0.06-0.125 and the storage model's own error grows (rel up to 4e-2 on a residual step, against
5e-3 under init weights), so a one-layer mutation has to stay 2 x MARGIN above it or the regime drowns that layer."""
import pytest
import torch

from oracle import net_layers as nl
from oracle import net_ref
from tests import net_layer_cases as cases

NETS = list(cases.regime_networks())
_BUILT = {}


def _net(name):
    """(cfg, boards, float64 weights, float64 chain, regime_stats) of one regime network, computed once."""
    if name not in _BUILT:
        cfg, x = cases.regime_networks()[name]
        s64 = nl.sd64(cases.regime_weights(name))
        chain = nl.chain64(s64, cfg, x)
        _BUILT[name] = (cfg, x, s64, chain, nl.regime_stats(s64, cfg, x, chain))
    return _BUILT[name]


def test_regime_networks_are_those_of_the_gpu_test():
    assert NETS == ["320x6", "288in320", "width_96", "width_192", "width_352"]
    nets = cases.regime_networks()
    assert [len(nl.schedule(nets[n][0])) for n in NETS] == [11, 11, 8, 8, 8]
    assert [nets[n][1].shape[0] for n in NETS] == [cases.B, cases.B, cases.WIDE_B, cases.WIDE_B, cases.WIDE_B]


def test_regime_is_seeded_and_keeps_the_architecture():
    cfg, x = cases.regime_networks()["width_96"]
    base = net_ref.random_state_dict(cfg, 0)
    a, b = nl.trained_like(base, cfg, 0, x), nl.trained_like(base, cfg, 0, x)
    assert list(a) == list(base) and all(a[k].shape == base[k].shape and a[k].dtype == torch.float32 for k in base)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = nl.trained_like(base, cfg, 1, x)
    assert not torch.equal(a["tower.1.bn2.weight"], c["tower.1.bn2.weight"])
    assert all(torch.equal(base[k], net_ref.random_state_dict(cfg, 0)[k]) for k in base)          # the input is left alone


@pytest.mark.parametrize("name", NETS)
def test_regime_meets_its_conditions_on_the_reference(name):
    """Conditions, not measurements: each names something the init regime never does (see the opposite at the end)."""
    cfg, x, s64, chain, st = _net(name)
    print("trained regime", name, st)
    assert st["stream_max"] >= 100.0 and st["first_block_in"] >= 50.0, st
    assert st["group_mean_over_std"] >= 8.0, st
    assert st["bn2_pre"] >= 88.8 and st["second_pre"] >= 88.8, st                # a value <= -88.8 and one >= 88.8 in one tensor
    assert st["se_outside"] >= 0.10, st
    assert st["attention"] and all(a["std"] >= 4.0 and a["maxprob"] >= 0.3 for a in st["attention"]), st
    assert st["qkv_max"] <= 64.0, st
    assert 0.08 <= st["neg_gains"] <= 0.13, st
    assert max(abs(v) for v in st["values"]) > 0.99 and min(abs(v) for v in st["values"]) < 0.5, st
    assert st["logit_scale"] == 5.0, st
    assert st["finite"] and st["peak"] < 32752.0, st
    # per norm layer one gain of +64 and one of -64
    full = net_ref.full_cfg(cfg)
    att = {f"tower.{i}.norm.weight" for kind, i in net_ref.tower_layout(full) if kind == "att"}
    gains = [k for k, v in s64.items() if k.endswith(".weight") and v.dim() == 1 and k not in att]
    assert len(gains) >= 10 and all(float(s64[k].max()) == 64.0 and float(s64[k].min()) == -64.0 for k in gains)


def test_init_regime_meets_none_of_them():
    cfg, x = cases.regime_networks()["320x6"]
    s64 = nl.sd64(cases.weights(cfg))
    st = nl.regime_stats(s64, cfg, x)
    assert st["stream_max"] < 20.0 and st["group_mean_over_std"] < 2.0 and st["bn2_pre"] < 10.0 and st["second_pre"] < 10.0, st
    assert st["se_outside"] == 0.0 and st["neg_gains"] == 0.0 and max(abs(v) for v in st["values"]) < 0.9 and st["logit_scale"] < 1.0, st


def _ratios(cfg, s64, chain, step, mutate):
    """Error / model error, per tensor and metric, of a float64 step with mutated weights on the step's own fp16-rounded input."""
    x = nl._h(chain[step][0])
    ref = nl.step64(s64, cfg, step, x)
    model = nl.step_model(s64, cfg, step, x)
    got = nl.step64(mutate(s64), cfg, step, x)
    return [nl.compare(g, r, m)["ratio"] for g, r, m in zip(got, ref, model) if r is not None]


_M320 = cases.regime_mutations(cases.regime_networks()["320x6"][0])


def test_regime_mutation_list_is_the_one_asked_for():
    names = [m[0] for m in _M320]
    assert len(names) == 9 and names[:3] == [m[0] for m in cases.width_mutations(320, cases.regime_networks()["320x6"][0])]
    assert names[:3] == ["bn2 gamma/beta of channels 15 and 16 swapped", "se_fc2 bias dropped", "rel_bias of head 19 dropped"]


@pytest.mark.parametrize("name,step,mutate", _M320, ids=[m[0] for m in _M320])
def test_comparator_catches_a_one_layer_mutation_in_the_regime(name, step, mutate):
    cfg, _, s64, chain, _ = _net("320x6")
    res = _ratios(cfg, s64, chain, step, mutate)
    print("regime mutation", name, res)
    assert max(max(r.values()) for r in res) > 2 * nl.MARGIN, (name, res)


_MW = [(C, *m) for C in cases.REGIME_WIDTHS for m in cases.width_mutations(C, dict(cases.WIDTHS)[C])]


@pytest.mark.parametrize("C,name,step,mutate", _MW, ids=[f"{m[0]}:{m[1]}" for m in _MW])
def test_comparator_catches_a_one_layer_mutation_in_the_regime_at_width(C, name, step, mutate):
    cfg, _, s64, chain, _ = _net(f"width_{C}")
    res = _ratios(cfg, s64, chain, step, mutate)
    print("regime mutation", C, name, res)
    assert max(max(r.values()) for r in res) > 2 * nl.MARGIN, (C, name, res)


@pytest.mark.parametrize("name", NETS)
def test_comparator_passes_the_unmutated_model_in_the_regime(name):
    """Every step and head under both kernel plans; the model is a positive, fp16-sized distance from float64.  Absolute: the
    stored values stay below 512 (asserted), where one rounding moves a value by at most 0.125, and a step has a handful of
    them.  Relative to a channel's norm there is no such bound here: a channel that a gain of -64 pushes through silu to all but
    zero on a board has a norm of the size of one rounding of its input."""
    cfg, _, s64, chain, st = _net(name)
    sched = nl.schedule(cfg)
    assert st["peak"] < 512.0
    for plan in (nl.kernel_plan(cfg), nl.kernel_plan(cfg, fuse_tail=False, fuse_attn=False)):
        for step in range(len(chain)):
            x = nl._h(chain[step][0])
            ref = nl.step64(s64, cfg, step, x)
            model = nl.step_model(s64, cfg, step, x, plan)
            for r, m in zip(ref, model):
                assert (r is None) == (m is None)
                if r is not None and sched[step]["run"]:
                    c = nl.compare(m, r, m)
                    assert c["ok"] and 0 < c["model"]["rel"] and 0 < c["model"]["abs"] < 1.0, (name, step, c)
        feats = nl._h(chain[-1][1])
        p64, v64, ssl64 = nl.heads64(s64, cfg, feats)
        pm, vm, sslm = nl.heads_model(s64, cfg, feats, plan)
        assert nl.compare(pm, p64, pm, maps=False)["ok"] and nl.compare(vm, v64, vm, maps=False)["ok"]
        assert 0 < nl.metric(vm, v64, maps=False)["abs"] < 0.1
        for t in ssl64:
            assert 0 < nl.metric(sslm[t], ssl64[t])["abs"] < 1.0, (name, t)
