"""oracle/net_layers.py on the CPU: the float64 step chain against the fp32 oracle, the comparator of tests/test_net_layers_gpu.py
against one-layer weight mutations (the margin must stay below what a wrong kernel does), and the "sharp" weight regime."""
import pytest
import torch

from oracle import net_layers as nl
from oracle import net_ref
from tests import net_layer_cases as cases


@pytest.fixture(scope="module")
def r24():
    cfg = cases.r24_cfg()
    sd = cases.weights(cfg)
    s64 = nl.sd64(sd)
    return cfg, sd, s64, nl.chain64(s64, cfg, cases.planes())


def _chain_matches_oracle(cfg, sd, s64, chain):
    x = cases.planes()
    p, v, ssl, feats = net_ref.forward(sd, cfg, x, return_ssl=True, return_feats=True)
    p64, v64, ssl64 = nl.heads64(s64, cfg, chain[-1][1])
    assert len(chain) == 3 + len(net_ref.tower_layout(cfg))
    assert float((chain[-1][1] - feats).abs().max()) <= 1e-4
    assert float((p64 - p).abs().max()) <= 1e-4
    assert float((v64 - v).abs().max()) <= 1e-5
    assert list(ssl64) == list(ssl)
    for t in ssl:
        assert float((ssl64[t] - ssl[t]).abs().max()) <= 1e-4, t


def test_float64_chain_reproduces_the_oracle_r24_320(r24):
    _chain_matches_oracle(*r24)


def test_float64_chain_reproduces_the_oracle_shipped_288x22():
    cfg = cases.shipped_cfg()
    sd = cases.weights(cfg)
    s64 = nl.sd64(sd)
    chain = nl.chain64(s64, cfg, cases.planes())
    _chain_matches_oracle(cfg, sd, s64, chain)
    # every second attention layer is skipped: its step hands the stream on untouched and has no second output
    skipped = [s for s, st in enumerate(nl.schedule(cfg)) if not st["run"]]
    assert len(skipped) == 4
    for s in skipped:
        assert chain[s][1] is chain[s][0] and chain[s][2] is None


def test_schedule_names_the_step_that_feeds_each_residual_block():
    sch = nl.schedule(cases.r24_cfg())
    assert [st["kind"] for st in sch[:7]] == ["stem", "pst", "inter", "res", "res", "res", "att"]
    assert sch[0]["next_bn1"] is None and sch[1]["next_bn1"] is None and sch[2]["next_bn1"] == "tower.0"
    assert sch[3]["next_bn1"] == "tower.1" and sch[5]["next_bn1"] is None and sch[6]["next_bn1"] == "tower.4"
    assert sch[-1]["kind"] == "att" and sch[-1]["next_bn1"] is None
    # a skipped attention layer is looked through: the block before it feeds the block after it
    sch = nl.schedule(cases.shipped_cfg())
    assert not sch[6]["run"] and sch[5]["next_bn1"] == "tower.4" and sch[6]["next_bn1"] is None
    assert sch[10]["run"] and sch[9]["next_bn1"] is None


@pytest.mark.parametrize("name,step,mutate", cases.MUTATIONS, ids=[m[0] for m in cases.MUTATIONS])
def test_comparator_catches_a_one_layer_mutation(r24, name, step, mutate):
    """What the GPU test does with a kernel's output, done with a float64 step whose weights are wrong in one term: on the
    layer's own fp16-rounded input the mutated step must leave MARGIN x (the storage model's error) behind on the stream or on
    the second output.  Raising MARGIN until a wrong kernel passes fails here."""
    cfg, _, s64, chain = r24
    x = nl._h(chain[step][0])
    ref = nl.step64(s64, cfg, step, x)
    model = nl.step_model(s64, cfg, step, x)
    got = nl.step64(mutate(s64), cfg, step, x)
    res = [nl.compare(g, r, m) for g, r, m in zip(got, ref, model) if r is not None]
    print(name, [(r["err"], r["model"]) for r in res])
    assert any(not r["ok"] for r in res), (name, res)


def test_comparator_passes_the_unmutated_model_on_every_step(r24):
    cfg, _, s64, chain = r24
    for step in range(len(chain)):
        x = nl._h(chain[step][0])
        ref = nl.step64(s64, cfg, step, x)
        for plan in (nl.kernel_plan(cfg), nl.kernel_plan(cfg, fuse_tail=False, fuse_attn=False)):
            model = nl.step_model(s64, cfg, step, x, plan)
            for r, m in zip(ref, model):
                assert (r is None) == (m is None)
                if r is not None:
                    c = nl.compare(m, r, m)
                    assert c["ok"] and 0 < c["model"]["rel"] < 5e-3, (step, c)       # fp16: 2^-11 per rounding, a few of them
    feats = nl._h(chain[-1][1])
    for r, m in zip(nl.heads64(s64, cfg, feats)[:2], nl.heads_model(s64, cfg, feats)[:2]):
        assert nl.compare(m, r, m, maps=False)["ok"]


def test_sharp_regime_meets_its_conditions_on_the_reference():
    """320 x 6 blocks with q, k x4 and rel_bias x8: every feature finite, between 1 % and 20 % of the scores outside the +-50
    clamp and a mean largest probability above 0.5, in the first attention block -- on the float64 reference alone."""
    cfg = cases.r24_cfg(blocks=6)
    s64 = nl.sd64(cases.weights(cfg, sharp=True))
    chain = nl.chain64(s64, cfg, cases.planes())
    assert all(torch.isfinite(y).all() for _, y, _ in chain)
    first_att = [s for s, st in enumerate(nl.schedule(cfg)) if st["kind"] == "att"][0]
    st = nl.attention_stats(s64, cfg, first_att, chain[first_att][0])
    print("sharp regime:", st, "features within", max(float(y.abs().max()) for _, y, _ in chain))
    assert 0.01 <= st["clamped"] <= 0.20 and st["maxprob"] > 0.5, st
    # the init regime is the opposite: the clamp never binds
    plain = nl.sd64(cases.weights(cfg))
    st0 = nl.attention_stats(plain, cfg, first_att, nl.chain64(plain, cfg, cases.planes())[first_att][0])
    assert st0["clamped"] == 0.0 and st0["maxprob"] < 0.3, st0
    # and the storage model stays an fp16-sized distance from float64 there
    x = nl._h(chain[first_att][0])
    m = nl.metric(nl.step_model(s64, cfg, first_att, x)[0], nl.step64(s64, cfg, first_att, x)[0])
    assert m["rel"] < 1e-2, m
