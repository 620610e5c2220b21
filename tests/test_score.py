"""The training-loss score without a GPU: matrix0_amd/csrc/score_core.h under g++ (tests/score_shim, the kernel's lane split and
merge order) against the float64 reference on the case set; the power of the case set; and matrix0_amd/score.py (chunking,
float64 report, per-shard rule, per-sample file, command line) over a temporary store with a stand-in backend whose score is
the reference."""
import json

import numpy as np
import pytest

from matrix0_amd import _abi, score as sc
from matrix0_amd.backend import NonFiniteScore, resolve_mask_mode
from matrix0_amd.data_writer import ShardIndex, write_npz
from tests import score_cases as cases
from tests import score_ref as ref
from tests import score_shim as shim

GROUPS = {g["name"]: g for g in cases.groups()}
OPTS = {f"smooth{o['label_smoothing']}_{o['value_loss']}": o for o in cases.OPTION_SETS}


def _args(g):
    return g["logits"], g["value"], g["pi"], g["z"], g["mask"]


@pytest.fixture(scope="module")
def reference():
    return {(n, k): ref.score_rows(*_args(g), mask_mode=g["mask_mode"], **o) for n, g in GROUPS.items() for k, o in OPTS.items()}


# ---- (1) the row arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("group", GROUPS)
def test_core_matches_the_reference_on_the_case_set(reference, group, opts):
    g = GROUPS[group]
    got = shim.score_rows(*_args(g), mask_mode=g["mask_mode"], **OPTS[opts])
    worst = ref.compare(got, reference[group, opts])
    print(group, opts, "largest error / tolerance per column:", np.round(worst, 5).tolist())
    assert (worst <= 1.0).all(), dict(zip(_abi.SCORE_COLUMNS, worst.tolist()))


def test_the_case_set_holds_the_rows_it_promises(reference):
    legal, target, none = (reference[n, "smooth0.0_mse"] for n in ("legal", "target", "none"))
    names = GROUPS["legal"]["names"]
    row = lambda text: legal[next(i for i, n in enumerate(names) if n.startswith(text))]
    assert row("support of 1")[5] == 1 and row("support of 218")[5] == 218
    assert row("one-hot pi outside")[5] == 31 and row("one-hot pi outside")[7] == 0
    assert row("pi summing to 0")[7] == 4 and row("pi summing to 0")[5] == 31
    assert np.isclose(row("pi summing to 0")[1], np.log(31.0))
    assert row("empty support")[7] == 1 and not row("empty support")[:6].any()
    assert row("a NaN logit")[7] == 2 and row("an infinite value")[7] == 2 and not row("a NaN logit")[:5].any()
    assert row("an infinite value")[6] == 0.0
    assert row("+3e4 and -3e4 outside")[4] == 0.0 and row("+3e4 and -3e4 outside")[0] > 0
    assert row("best logit and target at column 0")[3] == 0 and row("best logit and target at column 4671")[3] == 0
    k = names.index("equal logits at the target")
    lg, m = GROUPS["legal"]["logits"][k], GROUPS["legal"]["mask"][k] != 0
    t = lg[int(np.argmax(GROUPS["legal"]["pi"][k]))]
    assert (lg[m] == t).sum() == 3 and legal[k][3] == (lg[m] > t).sum() >= 1
    assert row("equal pi maxima")[3] > 0
    assert (none[:, 5] == cases.N).all() and np.allclose(none[:, 4], 1.0) and (none[:, 1] == 0).all()
    assert set(GROUPS["legal"]["z"].tolist()) == {-1.0, 0.0, 1.0}
    d = np.abs(GROUPS["legal"]["value"][:10] - GROUPS["legal"]["z"][:10])
    assert (d < cases.HUBER_DELTA).any() and (d > cases.HUBER_DELTA).any() and cases.HUBER_DELTA != 1.0
    assert target[GROUPS["target"]["names"].index("empty support")][7] == 1
    assert resolve_mask_mode(GROUPS["none"]["pi"], None, None) == "none"
    assert resolve_mask_mode(GROUPS["target"]["pi"], None, None) == "target"
    assert resolve_mask_mode(GROUPS["legal"]["pi"], GROUPS["legal"]["mask"], None) == "legal"


def test_the_core_refuses_what_the_abi_refuses():
    g = GROUPS["legal"]
    for bad in (dict(label_smoothing=1.0), dict(label_smoothing=-0.01), dict(huber_delta=0.0), dict(huber_delta=-1.0)):
        with pytest.raises(ValueError):
            shim.score_rows(*_args(g), mask_mode="legal", **bad)
    with pytest.raises(ValueError):
        shim.score_rows(*_args(g)[:4], None, mask_mode="legal")


# ---- (2) the power of the case set ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_the_case_set_sees_each_mutation_of_the_reference(reference, mutation):
    """Some row of some set differs from the reference by at least 100 times the tolerance (a column that is no longer
    finite counts as differing without bound)."""
    worst = 0.0
    for (n, k), want in reference.items():
        g = GROUPS[n]
        got = ref.score_rows(*_args(g), mask_mode=g["mask_mode"], mutate=mutation, **OPTS[k])
        with np.errstate(invalid="ignore"):
            diff = np.where(np.isfinite(got), np.abs(got - want) / ref.tolerance(want), np.inf)
        worst = max(worst, float(diff.max()))
    assert worst >= 100.0, (mutation, worst)


# ---- (3) matrix0_amd/score.py over a temporary store ----------------------------------------------------------------------
class RefBackend:
    """score() is the float64 reference on logits and values made from the planes by a fixed seeded map; a row whose first plane
    cell is POISON gets a NaN logit, and the call then raises as M0Backend.score does."""
    POISON = 77.0

    def __init__(self):
        rng = np.random.default_rng(3)
        self.w = rng.standard_normal((16, cases.N)).astype(np.float32)
        self.calls = []

    def outputs(self, s):
        feat = np.asarray(s, np.float32).reshape(len(s), -1)[:, 64:80]
        logits = feat @ self.w
        logits[np.asarray(s)[:, 0, 0, 0] == self.POISON, 5] = np.nan
        return logits, np.tanh(feat.sum(axis=1))

    def score(self, s, pi, z, legal_mask=None, *, mask_mode=None, label_smoothing=0.0, value_loss="mse", huber_delta=1.0):
        self.calls.append((len(s), mask_mode))
        logits, value = self.outputs(s)
        rows = ref.score_rows(logits, value, pi, z, legal_mask, mask_mode=resolve_mask_mode(pi, legal_mask, mask_mode),
                              label_smoothing=label_smoothing, value_loss=value_loss, huber_delta=huber_delta).astype(np.float32)
        if (rows[:, 7].astype(int) & 2).any():
            raise NonFiniteScore("non-finite", rows)
        return rows

    def close(self):
        pass


def _shard(rng, n, kind):
    s = rng.standard_normal((n, 19, 8, 8)).astype(np.float32)
    pi = np.zeros((n, cases.N), np.float32)
    mask = np.zeros((n, cases.N), np.uint8)
    for b in range(n):
        cols = rng.choice(cases.N, size=12, replace=False)
        mask[b, cols] = 1
        if kind == "onehot":
            pi[b, cols[0]] = 1.0
        else:
            w = rng.dirichlet(np.ones(5)).astype(np.float32)
            pi[b, cols[:5]] = w
    z = np.array([(-1.0, 0.0, 1.0)[b % 3] for b in range(n)], np.float32)
    d = {"s": s, "pi": pi, "z": z}
    if kind == "masked":
        d["legal_mask"] = mask
    return d


@pytest.fixture()
def store(tmp_path):
    """three shards: 6 rows with masks (one row without legal moves or pi: empty; one poisoned), 7 rows of soft pi without masks,
    3 one-hot rows without masks under another source"""
    rng = np.random.default_rng(21)
    shards = [("a_masked.npz", "selfplay", _shard(rng, 6, "masked"), "legal"),
              ("b_soft.npz", "selfplay", _shard(rng, 7, "soft"), "target"),
              ("c_onehot.npz", "import", _shard(rng, 3, "onehot"), "none")]
    shards[0][2]["pi"][2] = 0
    shards[0][2]["legal_mask"][2] = 0
    shards[0][2]["s"][4, 0, 0, 0] = RefBackend.POISON
    index = ShardIndex(tmp_path)
    for name, source, data, _ in shards:
        write_npz(tmp_path / name, data)
        index.add(tmp_path / name, len(data["z"]), source)
    return tmp_path, shards


def _expected(shards, **opts):
    be = RefBackend()
    rows, zs = [], []
    for _, _, d, mode in shards:
        logits, value = be.outputs(d["s"])
        rows.append(ref.score_rows(logits, value, d["pi"], d["z"], d.get("legal_mask"), mask_mode=mode, **opts).astype(np.float32))
        zs.append(d["z"])
    return rows, zs


def _means(rows, z):
    r, z = np.concatenate(rows).astype(np.float64), np.concatenate(z).astype(np.float64)
    keep = (r[:, 7].astype(int) & 3) == 0
    r, z = r[keep], z[keep]
    signed = z != 0
    return {"scored": int(keep.sum()), "policy_loss": r[:, 0].mean(), "kl": (r[:, 0] - r[:, 1]).mean(), "value_loss": r[:, 2].mean(),
            "total": (r[:, 0] + r[:, 2]).mean(), "top1": (r[:, 3] < 1).mean(), "top3": (r[:, 3] < 3).mean(),
            "top5": (r[:, 3] < 5).mean(), "support_mass": r[:, 4].mean(),
            "value_sign_agreement": (np.sign(r[signed, 6]) == np.sign(z[signed])).mean()}


def test_score_arrays_chunks_with_a_partial_last_chunk(store):
    _, shards = store
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    want, _ = _expected(shards, **opts)
    for (_, _, d, mode), rows in zip(shards, want):
        be = RefBackend()
        got = sc.score_arrays(be, d["s"], d["pi"], d["z"], d.get("legal_mask"), batch=4, **opts)
        n = len(d["z"])
        assert [c[0] for c in be.calls] == [4] * (n // 4) + ([n % 4] if n % 4 else []) and {c[1] for c in be.calls} == {mode}
        assert got.dtype == np.float32 and np.array_equal(got, rows)
    # the rule is applied to the arrays given, not to a chunk: the first 4 rows of this shard alone would be one-hot
    d = shards[1][2]
    mixed = d["pi"].copy()
    mixed[:4] = shards[2][2]["pi"][[0, 1, 2, 0]]
    be = RefBackend()
    sc.score_arrays(be, d["s"], mixed, d["z"], None, batch=4)
    assert {c[1] for c in be.calls} == {"target"}
    with pytest.raises(ValueError):
        sc.score_arrays(be, d["s"], d["pi"], d["z"], None, batch=0)


def test_score_shards_report_is_the_float64_sum_over_the_rows(store, tmp_path):
    path, shards = store
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    want, zs = _expected(shards, **opts)
    be = RefBackend()
    per = tmp_path / "per_sample.npz"
    r = sc.score_shards(path, be, sources=("selfplay", "import"), batch=4, per_sample=str(per), **opts)
    assert [c[0] for c in be.calls] == [4, 2, 4, 3, 3] and [c[1] for c in be.calls] == ["legal"] * 2 + ["target"] * 2 + ["none"]
    assert r["rows"] == 16 and r["flags"] == {"empty": 1, "nonfinite": 1, "uniform": 0} and r["skipped"] == []
    for key, x in _means(want, zs).items():
        assert r[key] == pytest.approx(x, rel=1e-12, abs=0), key
    assert list(r["by_shard"]) == [s[0] for s in shards]
    for (name, source, _, mode), rows, z in zip(shards, want, zs):
        one = r["by_shard"][name]
        assert (one["rows"], one["source"], one["mask_mode"]) == (len(z), source, mode)
        for key, x in _means([rows], [z]).items():
            assert one[key] == pytest.approx(x, rel=1e-12, abs=0), (name, key)
    assert set(r["by_source"]) == {"selfplay", "import"} and r["by_source"]["selfplay"]["rows"] == 13
    for key, x in _means(want[:2], zs[:2]).items():
        assert r["by_source"]["selfplay"][key] == pytest.approx(x, rel=1e-12, abs=0), key
    with np.load(per) as f:
        assert np.array_equal(f["columns"], np.concatenate(want)) and f["columns"].dtype == np.float32
        assert f["shards"].tolist() == [s[0] for s in shards]
        assert f["shard_index"].tolist() == [0] * 6 + [1] * 7 + [2] * 3
        assert f["row"].tolist() == list(range(6)) + list(range(7)) + list(range(3))
    # the sources filter; a float32 sum would not reproduce the float64 means to 1e-12
    only = sc.score_shards(path, RefBackend(), sources=("import",), batch=4, **opts)
    assert only["rows"] == 3 and list(only["by_shard"]) == ["c_onehot.npz"] and only["flags"]["nonfinite"] == 0


def test_command_line_writes_the_report_and_answers_nonfinite_rows(store, tmp_path, monkeypatch, capsys):
    path, shards = store
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"model": {"planes": 19}, "training": {"policy_label_smoothing": 0.05, "value_loss": "huber",
                                                                     "huber_delta": 0.5}}))
    made = []
    monkeypatch.setattr(sc, "load_backend", lambda model_cfg, ckpt, device: made.append(ckpt) or RefBackend())
    out = tmp_path / "report.json"
    base = ["--config", str(cfg), "--data", str(path), "--batch", "4", "--json", str(out)]
    # the poisoned row is in a selfplay shard: exit status 1; two checkpoints give two lines
    assert sc.main(base + ["--checkpoint", "A.pt", "--checkpoint", "B.pt", "--sources", "selfplay", "import"]) == 1
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and lines[0].startswith("A.pt") and lines[1].startswith("B.pt") and made == ["A.pt", "B.pt"]
    rep = json.loads(out.read_text())
    assert rep["options"] == {"label_smoothing": 0.05, "value_loss": "huber", "huber_delta": 0.5}
    want, zs = _expected(shards, **rep["options"])
    assert set(rep["checkpoints"]) == {"A.pt", "B.pt"}
    for key, x in _means(want, zs).items():
        assert rep["checkpoints"]["A.pt"][key] == pytest.approx(x, rel=1e-12, abs=0), key
    # flags override the config's keys; without the poisoned shard the exit status is 0
    assert sc.main(base + ["--checkpoint", "A.pt", "--sources", "import", "--value-loss", "mse", "--label-smoothing", "0"]) == 0
    rep = json.loads(out.read_text())
    assert rep["options"] == {"label_smoothing": 0.0, "value_loss": "mse", "huber_delta": 0.5}
    want, zs = _expected(shards[2:], **rep["options"])
    assert rep["checkpoints"]["A.pt"]["policy_loss"] == pytest.approx(_means(want, zs)["policy_loss"], rel=1e-12, abs=0)
    assert sc.training_opts({}) == {"label_smoothing": 0.0, "value_loss": "mse", "huber_delta": 1.0}
