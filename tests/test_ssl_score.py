"""The SSL score without a GPU: matrix0_amd/csrc/ssl_targets_core.h and ssl_score_core.h under g++ (tests/ssl_score_shim, the
kernel's lane split and merge order) against the goldens of the reference's modules and the float64 reference on the case set;
the power of the case set; and matrix0_amd/score.py with ssl=... (packing, the per-shard choice, the float64 report, the
per-sample file, the command line) over a temporary store with a stand-in backend whose scores are the references."""
import json

import numpy as np
import pytest

from matrix0_amd import _abi, score as sc
from matrix0_amd.backend import NonFiniteScore
from matrix0_amd.data_writer import ShardIndex, write_npz
from oracle import chess_py as ch
from oracle import ssl_ref as oracle_ssl
from tests import ssl_score_cases as cases
from tests import ssl_score_ref as ref
from tests import ssl_score_shim as shim
from tests import test_score as ts
from tests.golden_ref import load_npz

GROUPS = {g["name"]: g for g in cases.groups()}
TASKS = ref.TASKS


@pytest.fixture(scope="module")
def reference():
    return {n: ref.score_rows(g["heads"], g["tasks"], g["planes"], g["targets"]) for n, g in GROUPS.items()}


@pytest.fixture(scope="module")
def gold():
    z = load_npz("ssl_loss.npz")
    g = {k: z[k] for k in z.files}
    g["cases"] = json.loads(str(g["cases_json"]))
    return g


def golden_targets(g):
    """the golden's target maps as [6,17,64]"""
    return np.concatenate([g["target_piece"].reshape(6, 13, 64)] + [g[f"target_{t}"].reshape(6, 1, 64) for t in TASKS[1:]],
                          axis=1).astype(np.float32)


# ---- (1) the core's own exp and log ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,x", [("exp", -np.concatenate([np.linspace(0, 87, 20001), np.geomspace(1e-9, 1, 2001)])),
                                     ("log", np.concatenate([np.linspace(1, 13, 20001), np.geomspace(1, 1e6, 2001)])),
                                     ("log1p", np.concatenate([np.geomspace(1e-38, 1, 20001), np.linspace(-0.29, 0.42, 2001)]))])
def test_the_cores_exp_and_log_are_good_to_a_few_ulp(which, x):
    """Within 4 * 2^-24 relative on the ranges the score uses: the truncated series are below 5e-9, each has about ten fmaf
    steps whose roundings weigh less and less, the range reduction is exact to 2^-24 |x| and one last product or sum rounds."""
    x = x.astype(np.float32)
    want = {"exp": np.exp, "log": np.log, "log1p": np.log1p}[which](x.astype(np.float64))
    err = np.abs(shim.math(x, which).astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    err[want == 0] = 0
    print(which, "largest relative error in units of 2^-24:", err.max() * 2 ** 24)
    assert err.max() <= 4 * 2.0 ** -24
    assert shim.math(np.array([-87.5, -1e30, -np.inf, np.nan], np.float32), "exp").tolist() == [0, 0, 0, 0]


# ---- (2) targets from stored planes -----------------------------------------------------------------------------------------
def test_targets_of_planes_equal_the_reference_goldens_and_the_oracle(gold):
    z = load_npz("ssl_targets.npz")
    planes = np.stack([ch.encode_board(ch.Board(str(f))) for f in z["fens"]]).astype(np.float32)
    want = np.concatenate([z["piece"].reshape(-1, 13, 64)] + [z[t].reshape(-1, 1, 64) for t in TASKS[1:]], axis=1)
    got, status = shim.targets_planes(planes)
    assert len(planes) == 121 and not status.any()
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got, np.stack([ref.pack(oracle_ssl.targets(p)) for p in planes]))
    got, status = shim.targets_planes(gold["x"])
    assert not status.any() and np.array_equal(got, golden_targets(gold))
    assert np.array_equal(got, ref.targets_planes(gold["x"])[0])


def test_unusable_rows_are_flagged_and_leave_their_targets_untouched():
    g = GROUPS["all:planes"]
    got, status = shim.targets_planes(g["planes"])
    bad = np.array([n.startswith("unusable") for n in g["names"]])
    assert bad.sum() == 4 and np.array_equal(status, bad.astype(np.int32))
    assert (got[bad] == shim.SENTINEL).all() and not (got[~bad] == shim.SENTINEL).any()
    assert np.array_equal(~bad, ref.targets_planes(g["planes"])[1])
    # -0 is 0, and castling, counters or an impossible position do not enter: only planes 0-12 are read
    p = g["planes"][:1].copy()
    p[0, :12][p[0, :12] == 0] = -0.0
    p[0, 13:] = 7.5
    p[0, 5] = 0
    p[0, 5, 0, :3] = np.where(p[0, :12, 0, :3].sum(axis=0) == 0, 1.0, 0.0)            # up to three white kings
    got, status = shim.targets_planes(p)
    assert status[0] == 0 and np.array_equal(got, ref.targets_planes(p)[0])


# ---- (3) the losses ---------------------------------------------------------------------------------------------------------
def test_loss_reproduces_every_case_of_the_reference_golden(gold):
    """float64 means over the 6 rows of columns 0-4 against tests/golden/ssl_loss.npz, the reference module's own numbers,
    within the bound tests/test_ssl_loss.py sets for the host function: 2e-6 * max(1, |want|)."""
    heads = np.concatenate([gold[f"head_{t}"].reshape(6, -1, 64) for t in TASKS], axis=1)
    stored = golden_targets(gold)
    for targets in (None, stored):
        rows = shim.score_rows(heads, 31, gold["x"], targets)
        assert not rows[:, 15].any()
    zero_threat = stored.copy()
    zero_threat[:, 13] = 0
    for c in gold["cases"]:
        rows = shim.score_rows(heads, 31, gold["x"], zero_threat if c.get("threat_zero") else stored)
        mean = dict(zip(TASKS, rows[:, :5].astype(np.float64).mean(axis=0)))
        term = {t: (1.0 if t == "piece" else c["weights"].get(t, 1.0)) * mean[t] for t in c["tasks"]}
        assert all(v > 0 for v in term.values())
        total = sum(term.values())
        print(c["tasks"], "total", total, "reference", c["total"])
        assert abs(total - c["total"]) <= 2e-6 * max(1.0, abs(c["total"])), (c["tasks"], total, c["total"])
        for t, want in c["single"].items():
            assert abs(term[t] - want) <= 2e-6 * max(1.0, abs(want)), (t, term[t], want)
    # a task subset reads its own channels: the same columns from the heads of {piece, control} alone
    sub = shim.score_rows(np.concatenate([heads[:, :13], heads[:, 16:]], axis=1), 17, gold["x"], stored)
    full = shim.score_rows(heads, 31, gold["x"], stored)
    assert np.array_equal(sub[:, [0, 4, 5, 6, 7, 14, 15]], full[:, [0, 4, 5, 6, 7, 14, 15]]) and not sub[:, [1, 2, 3, 8, 9, 10, 11, 12, 13]].any()


@pytest.mark.parametrize("group", GROUPS)
def test_core_matches_the_reference_on_the_case_set(reference, group):
    g = GROUPS[group]
    got = shim.score_rows(g["heads"], g["tasks"], g["planes"], g["targets"])
    worst = ref.compare(got, reference[group])
    print(group, "largest error / tolerance per column:", np.round(worst, 5).tolist())
    assert (worst <= 1.0).all(), dict(zip(_abi.SSL_SCORE_COLUMNS, worst.tolist()))


def test_the_case_set_holds_the_rows_it_promises(reference):
    planes, stored = reference["all:planes"], reference["all:stored"]
    names = GROUPS["all:planes"]["names"]
    row = lambda rows, text: rows[next(i for i, n in enumerate(names) if n.startswith(text))]
    for text in ("unusable: 0.5", "unusable: two pieces", "unusable: plane 12 not", "unusable: plane 12 is 2"):
        assert row(planes, text)[15] == 1 and not row(planes, text)[:15].any()
        assert int(row(stored, text)[15]) & 1 and row(stored, text)[0] > 0            # scored on the targets given
    assert row(planes, "a NaN head")[15] == 2 and row(planes, "an infinite head")[15] == 2 and not row(planes, "a NaN head")[:15].any()
    assert row(planes, "empty board")[7] == 0 and row(planes, "every square")[7] == 64
    assert row(planes, "logits of exactly")[:5].max() > 10
    eq = row(planes, "equal logits")
    assert np.isclose(eq[0], np.log(13)) and np.isclose(eq[1], np.log(2)) and np.isclose(eq[4], np.log(3)) and eq[9] == 0 == eq[12]
    k = names.index("equal logits: the arg-max is the lowest index")
    assert eq[5] == GROUPS["all:planes"]["planes"][k, 0].sum() > 0                  # class 0 is hit exactly on the white pawns
    flags = stored[:, 15].astype(int)
    kinds = np.arange(len(names)) % 6
    usable = (flags & 1) == 0
    assert ((flags & 4) != 0)[usable & np.isin(kinds, (1, 3, 5))].all() and not (flags & 4)[np.isin(kinds, (0, 2, 4))].any()
    assert not (flags & 4)[~usable].any()
    t = GROUPS["all:stored"]["targets"]
    assert t[:, 13:16].max() == 2.0 and t[:, 13:16].min() == -1.0 and (np.abs(t[:, 16]) == 0.5).any()
    assert (planes[:, [1, 2, 3]] >= 0).all() and planes[:, 2].max() > 0
    assert set(g["tasks"] for g in GROUPS.values()) == {31, 1, 17}
    for n in ("piece:planes", "piece_control:stored"):
        off = [c for c, t in zip((1, 2, 3, 4), TASKS[1:]) if not GROUPS[n]["tasks"] & _abi.SSL_BITS[t]]
        assert not reference[n][:, off].any() and not reference[n][:, 8:14].any()


def test_the_core_refuses_what_the_abi_refuses():
    g = GROUPS["all:planes"]
    for tasks in (0, 32, -1, 63):
        with pytest.raises(ValueError):
            shim.score_rows(g["heads"], tasks, g["planes"])
    with pytest.raises(ValueError):
        shim.score_rows(None, 31, g["planes"])


# ---- (4) the power of the case set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_the_case_set_sees_each_mutation_of_the_reference(reference, mutation):
    """Some row of some group differs from the reference by at least 100 times the tolerance, or in an exact column."""
    worst = 0.0
    for n, want in reference.items():
        g = GROUPS[n]
        got = ref.score_rows(g["heads"], g["tasks"], g["planes"], g["targets"], mutate=mutation)
        worst = max(worst, float((np.abs(got - want)[:, :5] / ref.tolerance(want[:, :5])).max()))
        if not np.array_equal(got[:, 5:], want[:, 5:]):
            worst = np.inf
    assert worst >= 100.0, (mutation, worst)


# ---- (5) matrix0_amd/score.py with ssl=... over a temporary store -----------------------------------------------------------
class SslRefBackend(ts.RefBackend):
    """score_ssl() is the two float64 references on outputs made from the planes by fixed seeded maps; the poisoned row of
    RefBackend also gets a NaN head output."""
    model_cfg = {"ssl_threat_weight": 2.0, "ssl_control_weight": 0.25}

    def __init__(self, tasks=TASKS):
        super().__init__()
        self.ssl_tasks = list(tasks)
        self.wh = np.random.default_rng(5).standard_normal((16, sum(ref.CHANNELS[t] for t in tasks) * 64)).astype(np.float32)
        self.ssl_calls = []

    def heads(self, s):
        board = np.asarray(s, np.float32).reshape(len(s), 19, 64)[:, :12]
        feat = board[:, :, :16].sum(axis=1) + 0.01 * board.sum(axis=(1, 2))[:, None]
        h = (feat @ self.wh).reshape(len(s), -1, 64)
        h[np.asarray(s)[:, 0, 0, 0] == self.POISON, 0, 0] = np.nan
        return h

    def score_ssl(self, s, pi, z, legal_mask=None, ssl_targets=None, **opts):
        self.ssl_calls.append((len(s), None if ssl_targets is None else ssl_targets.shape))
        try:
            rows = self.score(s, pi, z, legal_mask, **opts)
        except NonFiniteScore as e:
            rows = e.rows
        ssl_rows = ref.score_rows(self.heads(s), ref.bits(self.ssl_tasks), s, ssl_targets).astype(np.float32)
        if (rows[:, 7].astype(int) & 2).any() or (ssl_rows[:, 15].astype(int) & 2).any():
            raise NonFiniteScore("non-finite", rows, ssl_rows)
        return rows, ssl_rows


def _board_shard(rng, n, kind, with_ssl):
    d = ts._shard(rng, n, kind)
    d["s"] = np.stack([cases._board(rng, 0.4, b % 2 == 0) for b in range(n)])
    if with_ssl:
        t = ref.targets_planes(d["s"])[0].astype(np.float32)
        d.update(ssl_piece=t[:, :13].reshape(n, 13, 8, 8), **{f"ssl_{k}": t[:, 13 + i].reshape(n, 8, 8) for i, k in enumerate(TASKS[1:])})
    return d


@pytest.fixture()
def store(tmp_path):
    """three shards: 6 masked rows with stored targets (one poisoned, one with a target square altered), 7 rows without
    targets (one with unusable planes), 3 rows under another source with every key but ssl_fork"""
    rng = np.random.default_rng(31)
    a, b, c = _board_shard(rng, 6, "masked", True), _board_shard(rng, 7, "soft", False), _board_shard(rng, 3, "onehot", True)
    a["s"][4, 0, 0, 0] = SslRefBackend.POISON
    a["ssl_piece"][4, :, 0, 0] = 0
    a["ssl_piece"][4, 12, 0, 0] = 1                    # (the poison cell is not a piece: keep that row's targets in step)
    a["ssl_control"][2, 3, 3] = 1.0 if a["ssl_control"][2, 3, 3] != 1.0 else -1.0
    b["s"][5, 12, 0, 0] = 1.0 - b["s"][5, 12, 0, 0]
    del c["ssl_fork"]
    shards = [("a_stored.npz", "selfplay", a), ("b_plain.npz", "selfplay", b), ("c_partial.npz", "import", c)]
    index = ShardIndex(tmp_path)
    for name, source, d in shards:
        write_npz(tmp_path / name, d)
        index.add(tmp_path / name, len(d["z"]), source)
    return tmp_path, shards


def _ssl_block(ssl_rows, stored, base, tasks, weights, ssl_weight):
    """the report's "ssl" block from rows, written out independently of SslSums"""
    r = np.concatenate(ssl_rows).astype(np.float64)
    st = np.concatenate([np.full(len(x), s) for x, s in zip(ssl_rows, stored)])
    flags = r[:, 15].astype(int)
    keep = ((flags & 2) == 0) & (((flags & 1) == 0) | st)
    k = r[keep]
    loss = {t: k[:, TASKS.index(t)].mean() for t in tasks}
    total = sum((1.0 if t == "piece" else weights.get(t, 1.0)) * loss[t] for t in tasks if loss[t] > 0)
    return {"scored": int(keep.sum()), "loss": loss, "ssl_total": total,
            "total_with_ssl": base["policy_loss"] + base["value_loss"] + ssl_weight * total,
            "piece_accuracy": k[:, 5].sum() / (64 * len(k)), "piece_accuracy_occupied": k[:, 6].sum() / k[:, 7].sum(),
            "control_accuracy": k[:, 14].sum() / (64 * len(k)), "threat_precision": k[:, 8].sum() / k[:, 9].sum(),
            "threat_recall": k[:, 8].sum() / k[:, 10].sum(), "fork_precision": k[:, 11].sum() / k[:, 12].sum(),
            "fork_recall": k[:, 11].sum() / k[:, 13].sum()}


def _check_block(got, want):
    for key, x in want.items():
        if key == "loss":
            for t, v in x.items():
                assert got["loss"][t] == pytest.approx(v, rel=1e-12, abs=0), t
        else:
            assert got[key] == pytest.approx(x, rel=1e-12, abs=0), key


def test_score_shards_with_ssl_is_the_float64_sum_and_auto_picks_per_shard(store, tmp_path):
    path, shards = store
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    be = SslRefBackend()
    per = tmp_path / "per_sample.npz"
    r = sc.score_shards(path, be, sources=("selfplay", "import"), batch=4, per_sample=str(per), ssl="auto", ssl_weight=0.3, **opts)
    # the first shard has every key: stored; the second has none and the third lacks ssl_fork: planes
    assert [v["ssl"]["targets"] for v in r["by_shard"].values()] == ["stored", "planes", "planes"]
    assert [c[1] for c in be.ssl_calls] == [(4, 17, 64), (2, 17, 64)] + [None] * 3 and [c[0] for c in be.ssl_calls] == [4, 2, 4, 3, 3]
    plain = sc.score_shards(path, SslRefBackend(), sources=("selfplay", "import"), batch=4, **opts)
    strip = lambda d: {k: ({n: strip(x) for n, x in v.items()} if k in ("by_source", "by_shard") else v) for k, v in d.items() if k != "ssl"}
    assert strip(r) == plain and "ssl" not in plain and not any("ssl" in v for v in plain["by_shard"].values())
    want_rows = []
    for (_, _, d), stored in zip(shards, (True, False, False)):
        t = sc.pack_ssl_targets(d, len(d["z"]), TASKS) if stored else None
        want_rows.append(ref.score_rows(be.heads(d["s"]), 31, d["s"], t).astype(np.float32))
    weights = {"threat": 2.0, "control": 0.25}
    _check_block(r["ssl"], _ssl_block(want_rows, (True, False, False), r, TASKS, weights, 0.3))
    # (the poison cell, 77 in a piece plane, also makes that row's planes unusable: it is counted twice and scored never)
    assert r["ssl"]["rows"] == 16 and r["ssl"]["scored"] == 14 and r["ssl"]["flags"] == {"planes": 2, "nonfinite": 1, "mismatch": 1}
    assert r["ssl"]["tasks"] == list(TASKS) and r["ssl"]["dropped"] == [] and r["ssl"]["ssl_weight"] == 0.3
    _check_block(r["by_source"]["selfplay"]["ssl"], _ssl_block(want_rows[:2], (True, False), r["by_source"]["selfplay"], TASKS, weights, 0.3))
    for (name, _, _), rows, stored in zip(shards, want_rows, (True, False, False)):
        _check_block(r["by_shard"][name]["ssl"], _ssl_block([rows], (stored,), r["by_shard"][name], TASKS, weights, 0.3))
    with np.load(per) as f:
        assert np.array_equal(f["ssl_columns"], np.concatenate(want_rows)) and f["ssl_columns"].dtype == np.float32
        assert f["columns"].shape == (16, 8) and f["row"].tolist() == list(range(6)) + list(range(7)) + list(range(3))
    sc.score_shards(path, SslRefBackend(), batch=4, per_sample=str(tmp_path / "plain.npz"), **opts)
    with np.load(tmp_path / "plain.npz") as f:
        assert sorted(f.files) == ["columns", "row", "shard_index", "shards"]
    # planes ignores the stored targets: no audit, the altered square goes unseen
    r = sc.score_shards(path, SslRefBackend(), sources=("selfplay",), batch=4, ssl="planes", **opts)
    assert [v["ssl"]["targets"] for v in r["by_shard"].values()] == ["planes", "planes"] and r["ssl"]["flags"]["mismatch"] == 0
    assert r["ssl"]["ssl_weight"] == 0.1
    # explicit weights replace the model's
    r = sc.score_shards(path, SslRefBackend(), sources=("selfplay",), batch=4, ssl="planes", ssl_task_weights={"fork": 3.0}, **opts)
    x = r["ssl"]
    assert x["ssl_total"] == pytest.approx(sum((3.0 if t == "fork" else 1.0) * x["loss"][t] for t in TASKS if t not in x["dropped"]), rel=1e-12)


def test_stored_fails_on_a_missing_key_and_only_for_a_task_of_the_network(store):
    path, _ = store
    with pytest.raises(KeyError, match="b_plain.npz.*ssl_piece"):
        sc.score_shards(path, SslRefBackend(), batch=4, ssl="stored")
    with pytest.raises(KeyError, match="c_partial.npz.*ssl_fork"):
        sc.score_shards(path, SslRefBackend(), sources=("import",), batch=4, ssl="stored")
    r = sc.score_shards(path, SslRefBackend(("piece", "control")), sources=("import",), batch=4, ssl="stored")
    assert r["by_shard"]["c_partial.npz"]["ssl"]["targets"] == "stored" and set(r["ssl"]["loss"]) == {"piece", "control"}
    assert "threat_precision" not in r["ssl"] and r["ssl"]["control_accuracy"] is not None
    assert sc.score_shards(path, SslRefBackend(("piece", "control")), sources=("import",), batch=4, ssl="auto")["ssl"] == r["ssl"]
    for bad in (dict(ssl="yes"), dict(ssl="auto", ssl_target_weight=0.5)):
        with pytest.raises(ValueError):
            sc.score_shards(path, SslRefBackend(), batch=4, **bad)
    no_heads = SslRefBackend()
    no_heads.ssl_tasks = []
    with pytest.raises(ValueError):
        sc.score_shards(path, no_heads, batch=4, ssl="auto")


def test_a_task_whose_mean_loss_is_not_positive_is_dropped_from_the_total():
    sums = sc.SslSums()
    rows = np.zeros((2, 16), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 4] = 2.0, 0.0, 0.5
    sums.add(rows, stored=True)
    base = {"policy_loss": 1.0, "value_loss": 0.25}
    x = sums.report(base, ["piece", "threat", "control"], {"control": 0.5}, 0.1)
    assert x["dropped"] == ["threat"] and x["ssl_total"] == 2.25 and x["total_with_ssl"] == pytest.approx(1.25 + 0.225)
    assert sc.SslSums().report({"policy_loss": None, "value_loss": None}, ["piece"], {}, 0.1)["ssl_total"] is None


def test_command_line_prints_the_ssl_block_and_refuses_a_target_weight(store, tmp_path, monkeypatch, capsys):
    path, _ = store
    cfg = {"model": {"planes": 19, "ssl_threat_weight": 2.0}, "training": {"ssl_weight": 0.2}}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    monkeypatch.setattr(sc, "load_backend", lambda model_cfg, ckpt, device: SslRefBackend())
    out, per = tmp_path / "report.json", tmp_path / "rows.npz"
    base = ["--config", str(tmp_path / "config.json"), "--data", str(path), "--batch", "4", "--json", str(out), "--checkpoint", "A.pt"]
    assert sc.main(base + ["--sources", "import", "--ssl", "--per-sample", str(per), "--ssl-task-weight", "fork=3"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 2 and " ssl rows 3 scored 3 " in lines[1] and "total_with_ssl" in lines[1] and "ssl_weight 0.2" in lines[1]
    rep = json.loads(out.read_text())
    assert rep["ssl_options"] == {"ssl_weight": 0.2, "ssl_task_weights": {"threat": 2.0, "pin": 1.0, "fork": 3.0, "control": 1.0},
                                  "ssl_target_weight": 1.0, "ssl": "auto"}
    x = rep["checkpoints"]["A.pt"]["ssl"]
    assert x["total_with_ssl"] == pytest.approx(rep["checkpoints"]["A.pt"]["total"] + 0.2 * x["ssl_total"], rel=1e-12)
    assert np.load(per)["ssl_columns"].shape == (3, 16)
    # the poisoned row's heads: exit status 1; --ssl-weight overrides the config
    assert sc.main(base + ["--sources", "selfplay", "--ssl", "planes", "--ssl-weight", "0.5"]) == 1
    assert json.loads(out.read_text())["checkpoints"]["A.pt"]["ssl"]["ssl_weight"] == 0.5
    capsys.readouterr()
    # without --ssl: one line, no new keys
    assert sc.main(base + ["--sources", "import"]) == 0
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]) == 1
    rep = json.loads(out.read_text())
    assert sorted(rep) == ["checkpoints", "options", "sources"] and "ssl" not in rep["checkpoints"]["A.pt"]
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, training={"ssl_target_weight": 0.5})))
    with pytest.raises(ValueError, match="ssl_target_weight"):
        sc.main(base + ["--ssl"])
    with pytest.raises(ValueError):
        sc.ssl_opts(cfg, task_weights={"piece": 2.0})
