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


# ---- the seven trunk widths of tests/test_net_widths_gpu.py ---------------------------------------------------------------------
_WIDTH_CHAINS = {}


def _width_chain(C, cfg):
    """(weights, float64 weights, float64 chain over the 17 boards) of one row of cases.WIDTHS, computed once."""
    if C not in _WIDTH_CHAINS:
        sd = cases.weights(cfg)
        s64 = nl.sd64(sd)
        _WIDTH_CHAINS[C] = (sd, s64, nl.chain64(s64, cfg, cases.wide_planes()))
    return _WIDTH_CHAINS[C]


def test_width_table_covers_the_switches():
    """Seven rows, every one a width check_supported takes with head dim 16 and no padding; each remaining switch on one row."""
    assert [C for C, _ in cases.WIDTHS] == [32, 96, 160, 192, 256, 352, 384]
    full = [net_ref.full_cfg(cfg) for _, cfg in cases.WIDTHS]
    for (C, _), f in zip(cases.WIDTHS, full):
        assert f["channels"] == C and f["attention_heads"] * 16 == C and f["blocks"] == 4 and f["norm"] == "group" and f["preact"]
        assert f["ssl_tasks"] == cases.SSL5 and [k for k, _ in net_ref.tower_layout(f)] == ["res", "res", "res", "att", "res"]
    assert sum(f["policy_factor_rank"] == 0 for f in full) == 1 and sum(f["policy_factor_rank"] == 32 for f in full) == 6
    assert sum(f["activation"] == "relu" and not f["se"] for f in full) == 1
    assert sum(not f["attention_relbias"] for f in full) == 1
    assert sum(f["value_activation"] == "leaky_relu" for f in full) == 1


def test_kernel_plan_follows_conv_norm_act_at_every_width():
    """The forms net.hip picks, width by width: the 320 tile at 320 alone, the GroupNorm epilogue where the trunk is a multiple
    of 64, and the SSL head conv unfused all the same at 192 (N = 96) and 384 (N = 192)."""
    got = {C: nl.kernel_plan(cases.width_cfg(C)) for C in range(32, 385, 32)}
    assert [C for C, p in got.items() if p["big"]] == [288, 320]                                # 288 runs padded to 320
    assert [C for C, p in got.items() if p["fuse_tail"] or p["fuse_attn"]] == [288, 320]
    assert [C for C, p in got.items() if p["gn_small"]] == [64, 128, 192, 256, 288, 320, 384]
    assert [C for C, p in got.items() if p["ssl_epilogue"]] == [64, 128, 256, 288, 320]
    assert not any(p["ssl_epilogue"] and not p["gn_small"] for p in got.values())


@pytest.mark.parametrize("C,cfg", cases.WIDTHS, ids=cases.WIDTH_IDS)
def test_float64_chain_reproduces_the_oracle_at_every_width(C, cfg):
    sd, s64, chain = _width_chain(C, cfg)
    x = cases.wide_planes()
    p, v, ssl, feats = net_ref.forward(sd, cfg, x, return_ssl=True, return_feats=True)
    p64, v64, ssl64 = nl.heads64(s64, cfg, chain[-1][1])
    assert len(chain) == 8 and chain[6][2] is not None and chain[7][2] is None
    assert float((chain[-1][1] - feats).abs().max()) <= 1e-4
    assert float((p64 - p).abs().max()) <= 1e-4
    assert float((v64 - v).abs().max()) <= 1e-5
    assert list(ssl64) == list(ssl) == cases.SSL5
    for t in ssl:
        assert float((ssl64[t] - ssl[t]).abs().max()) <= 1e-4, t


@pytest.mark.parametrize("C,cfg,name,step,mutate", cases.WIDTH_MUTATIONS, ids=cases.WIDTH_MUTATION_IDS)
def test_comparator_catches_a_one_layer_mutation_at_every_width(C, cfg, name, step, mutate):
    """test_comparator_catches_a_one_layer_mutation on the rows of cases.WIDTHS: the bound of tests/test_net_widths_gpu.py must lie
    below what one wrong parameter set of one layer does, at that width and on those 17 boards."""
    _, s64, chain = _width_chain(C, cfg)
    x = nl._h(chain[step][0])
    ref = nl.step64(s64, cfg, step, x)
    model = nl.step_model(s64, cfg, step, x)
    got = nl.step64(mutate(s64), cfg, step, x)
    res = [nl.compare(g, r, m) for g, r, m in zip(got, ref, model) if r is not None]
    print("width mutation", C, name, [{k: round(r["ratio"][k] / nl.MARGIN, 2) for k in r["ratio"]} for r in res])
    assert any(not r["ok"] for r in res), (C, name, res)


@pytest.mark.parametrize("C,cfg", cases.WIDTHS, ids=cases.WIDTH_IDS)
def test_comparator_passes_the_unmutated_model_at_every_width(C, cfg):
    """The storage model is an fp16-sized distance from float64 on every step and head of every row, and passes its own bound.
    (rel < 5e-3 on the silu rows, as on R24-320.  On the relu row a channel that relu leaves all but empty on a board has a norm
    of the size of one fp16 rounding of its input, so its relative error is not small -- 0.11 on the interaction step's second
    output -- while the absolute error, which the bound also holds, stays at 4e-3.)"""
    _, s64, chain = _width_chain(C, cfg)
    plan = nl.kernel_plan(cfg)
    rel_max = 5e-3 if net_ref.full_cfg(cfg)["activation"] == "silu" else 1.0
    for step in range(len(chain)):
        x = nl._h(chain[step][0])
        ref = nl.step64(s64, cfg, step, x)
        model = nl.step_model(s64, cfg, step, x, plan)
        for r, m in zip(ref, model):
            assert (r is None) == (m is None)
            if r is not None:
                c = nl.compare(m, r, m)
                assert c["ok"] and 0 < c["model"]["rel"] < rel_max and c["model"]["abs"] < 1e-2, (C, step, c)
    feats = nl._h(chain[-1][1])
    p64, v64, ssl64 = nl.heads64(s64, cfg, feats)
    pm, vm, sslm = nl.heads_model(s64, cfg, feats, plan)
    assert nl.compare(pm, p64, pm, maps=False)["ok"] and nl.compare(vm, v64, vm, maps=False)["ok"]
    for t in ssl64:
        assert 0 < nl.metric(sslm[t], ssl64[t])["rel"] < rel_max, (C, t)


def test_block_input_given_or_recomputed_is_the_same_model():
    """step_model of a residual block with its second input handed in: the previous step's modelled second output, computed from
    that step's unrounded stream as its kernel does, is the tensor the block recomputes from the rounded stream up to single
    fp16 steps -- on a few per cent of the elements -- and both models of the block keep the same distance from float64."""
    C, cfg = cases.WIDTHS[4]                                    # the relu row
    _, s64, chain = _width_chain(C, cfg)
    prev = nl.step_model(s64, cfg, 3, nl._h(chain[3][0]))      # its stream and second output feed step 4
    own = nl._h(net_ref._act(nl._gn_from(prev[0], prev[0], s64, "tower.1.bn1"), net_ref.full_cfg(cfg)))
    moved = (prev[1] != own)
    assert 0 < float(moved.double().mean()) < 0.1
    assert float((prev[1] - own).abs().max()) <= 2.0 ** -8     # one fp16 step below 8
    ref = nl.step64(s64, cfg, 4, prev[0])
    given = nl.step_model(s64, cfg, 4, prev[0], block_in=prev[1])
    recomputed = nl.step_model(s64, cfg, 4, prev[0])
    assert torch.equal(nl.step_model(s64, cfg, 4, prev[0], block_in=own)[0], recomputed[0])
    for g, r, ref_ in zip(given, recomputed, ref):
        mg, mr = nl.metric(g, ref_), nl.metric(r, ref_)
        assert 0.5 < mg["abs"] / mr["abs"] < 2.0, (mg, mr)


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
