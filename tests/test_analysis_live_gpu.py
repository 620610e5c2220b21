"""Live searches on the analysis engine (include/m0_analysis_live.h: csrc/capi_analysis.hip, csrc/tree_reroot.hip) on the GPU,
with the external-evaluator engine and the evaluator of tests/test_search_gpu.py unless a test says otherwise: a peek does not
perturb, a stop equals the peek before it, a continued search equals the oracle's MCTS.run on the grafted subtree (visit
counts, moves, policy indices and PVs identical, priors and q within 1e-6, the tolerance of test_search_gpu._compare), the
fallback equals a plain submission bit for bit, final positions that need no search are answered at once, held slots are
counted apart, plain submissions do not notice a held neighbour, and the fused step equals the split step on the 320-wide
network."""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from oracle import net_ref
from tests.fake_net import FakeNet
from tests.test_analysis_gpu import MANY_MOVES, MULTIPV, PV_LEN, _oracle_lines
from tests.test_search_gpu import FENS, MCTS
from tests.test_timed_path_gpu import NET

pytestmark = pytest.mark.gpu

SIMS, LEAVES = 64, 8
REUSE_FENS = FENS[:5]           # the oracle's PV of each carries at least 7 visits on its second move at 64 simulations


def _cfg(sims=256, **mcts):
    return {"seed": 1234, "mcts": dict(MCTS, inference_batch_size=LEAVES, **mcts), "selfplay": {"num_simulations": sims}}


def _engine(slots, dirichlet=False, cfg=None):
    from matrix0_amd import engine as eng
    c = eng.selfplay_cfg_from_dict(cfg or _cfg(), concurrent_games=slots, record_games=False)
    return eng.AnalysisExtEngine(c, multipv=MULTIPV, pv_len=PV_LEN, dirichlet=dirichlet)


def _net():
    return FakeNet(seed=3, sharp=8.0)


def _poll_raw(e):
    """Every answered result as (id, bytes of the m0_analysis_result)."""
    from matrix0_amd import engine as eng
    out = []
    while True:
        r = eng.AnalysisResult()
        rc = e._L.m0_analysis_poll(e._h, C.byref(r))
        assert rc >= 0
        if rc == 0:
            return out
        out.append((int(r.id), bytes(r)))


def _as_dict(raw):
    from matrix0_amd import engine as eng
    return eng.analysis_result_to_dict(eng.AnalysisResult.from_buffer_copy(raw))


def _run(e, net, on_pass=None):
    """Step until nothing is pending; {id: bytes}."""
    got = dict(_poll_raw(e))
    for _ in range(10000):
        if e.pending() == 0:
            break
        e.step(net.infer_np, 1)
        if on_pass:
            on_pass()
        got.update(_poll_raw(e))
    assert e.pending() == 0
    return got


def test_peek_does_not_perturb():
    positions = list(FENS) + [MANY_MOVES]
    plain = _engine(3)
    for i, fen in enumerate(positions):
        plain.submit(fen, sims=SIMS, id=i, keep=False)
    want = _run(plain, _net())
    plain.close()
    e = _engine(3)
    for i, fen in enumerate(positions):
        e.submit(fen, sims=SIMS, id=i)
    seen, answered = [], set()

    def peek_all():
        for i in range(len(positions)):
            if i in answered:
                continue
            try:
                pk = e.peek(i)
            except ValueError:                     # answered by this pass, not polled yet
                answered.add(i)
                continue
            if pk is not None:
                seen.append(pk)
                assert e.peek(i) == pk             # and again: the same

    got = _run(e, _net(), on_pass=peek_all)
    e.close()
    assert sorted(got) == sorted(want) == list(range(len(positions)))
    for i in got:
        assert got[i] == want[i], positions[i]
    mid = [p for p in seen if 0 < p["sims"] < SIMS]
    assert mid and all(p["lines"] and p["root_n"] == p["sims"] for p in mid)
    assert any(p["sims"] == 0 and p["lines"] and p["lines"][0]["visits"] == 0 for p in seen)      # after the root's expansion
    assert any(p["nlegal"] == 218 and len(p["lines"]) == MULTIPV for p in mid)


def test_stop_equals_peek_and_the_slot_moves_on():
    e = _engine(2)
    net = _net()
    e.submit(FENS[0], sims=256, id=1, keep=True)
    e.submit(FENS[1], sims=256, id=2)
    e.submit(FENS[2], sims=SIMS, id=3)
    e.submit(FENS[3], sims=SIMS, id=5)
    for _ in range(3):
        e.step(net.infer_np, 1)
    assert e.peek(3) is None and e.pending() == 4
    # a queued search that is stopped: answered with zeros, no slot taken
    e.stop(5)
    (i5, raw5), = _poll_raw(e)
    z = _as_dict(raw5)
    assert i5 == 5 and (z["status"], z["sims"], z["root_n"], z["evals"], z["lines"]) == ("ok", 0, 0, 0, []) and z["nlegal"] > 0
    # a running one: the peek, then the stop
    pk = bytes(e.peek_raw(2))
    e.stop(2)
    (i2, raw2), = _poll_raw(e)
    assert i2 == 2 and raw2 == pk
    r2 = _as_dict(raw2)
    assert 0 < r2["sims"] < 256 and r2["sims"] == r2["root_n"] == 2 * LEAVES and r2["lines"][0]["visits"] > 0
    assert e.held() == 0 and e.pending() == 2
    with pytest.raises(ValueError):
        e.peek(2)
    with pytest.raises(ValueError):
        e.stop(2)
    e.step(net.infer_np, 1)                                 # the freed slot takes the next queued search
    assert e.peek(3) is not None
    # the kept one: stopped, held, continued on the same root
    pk = bytes(e.peek_raw(1))
    e.stop(1)
    (i1, raw1), = _poll_raw(e)
    assert i1 == 1 and raw1 == pk
    r1 = _as_dict(raw1)
    assert r1["sims"] == 3 * LEAVES < 256 and e.held() == 1
    reused = e.continue_search(1, [], sims=SIMS, id=4, keep=False)
    assert reused == r1["root_n"] == 3 * LEAVES and e.held() == 0
    before = e.peek(4)                                      # the kept tree, before any new simulation
    assert before["sims"] == 0 and before["root_n"] == reused
    assert [(ln["move"], ln["visits"]) for ln in before["lines"]] == [(ln["move"], ln["visits"]) for ln in r1["lines"]]
    got = _run(e, net)
    e.close()
    r4, r3 = _as_dict(got[4]), _as_dict(got[3])
    assert r4["sims"] == SIMS and r4["root_n"] == reused + SIMS and r3["root_n"] == SIMS


def _oracle_cfg(dirichlet):
    m = dict(MCTS, inference_batch_size=LEAVES)
    return ref.MCTSConfig.from_dict(dict(m, use_tt=False, virtual_loss_active=True, dirichlet_plies=(30 if dirichlet else 0),
                                         numerics="engine"))


def _oracle_first(fen, uid, dirichlet):
    o = ref.MCTS(_oracle_cfg(dirichlet), _net().infer_np, seed=1234, game=uid)
    b = ch.Board(fen)
    o.run(b, num_simulations=SIMS, ply=0)
    return o._last_root


def _oracle_continue(root, fen, ucis, uid, dirichlet):
    """MCTS.run with the streams of `uid` on the subtree behind `ucis` of a searched root (a copy of it): the oracle object
    finds the node as the child its last search's root has for the last move (tree-only reuse).  Returns (node before, run)."""
    root = copy.deepcopy(root)
    b = ch.Board(fen)
    parent, node = types.SimpleNamespace(children={"same": root}), root
    last = "same"
    for u in ucis:
        last = ch.Move.from_uci(u)
        parent, node = node, node.children[last]
        b.push(last)
    n_before = node.n
    o = ref.MCTS(_oracle_cfg(dirichlet), _net().infer_np, seed=1234, game=uid)
    o._last_root, o._last_move = parent, last
    _, _, rq = o.run(b, num_simulations=SIMS, ply=0)
    assert o._last_root is node
    return n_before, {"lines": _oracle_lines(node, MULTIPV, PV_LEN), "root_n": node.n, "root_q": rq, "evals": o.evals,
                      "nlegal": len(b.legal_moves)}


def _check(got, want, tag):
    assert got["status"] == "ok" and got["nlegal"] == want["nlegal"] and got["root_n"] == want["root_n"], tag
    assert got["evals"] == want["evals"] and got["sims"] == SIMS and not got["overflow"], tag
    for key in ("move", "policy_index", "visits", "pv"):
        assert [ln[key] for ln in got["lines"]] == [ln[key] for ln in want["lines"]], (tag, key)
    np.testing.assert_allclose([ln["prior"] for ln in got["lines"]], [ln["prior"] for ln in want["lines"]], rtol=0, atol=1e-6)
    np.testing.assert_allclose([ln["q"] for ln in got["lines"]], [ln["q"] for ln in want["lines"]], rtol=0, atol=1e-6)
    assert abs(got["root_q"] - want["root_q"]) < 1e-6, tag


@functools.lru_cache(maxsize=None)
def _continued(dirichlet):
    """Every position of REUSE_FENS searched with keep and continued by one ply, by two plies and by none, engine and oracle:
    ((uid, plies, reused_n, visits of the node before, engine result, oracle result), ...).  Computed once per setting."""
    n = len(REUSE_FENS)
    roots = [_oracle_first(fen, 600 + i, dirichlet) for i, fen in enumerate(REUSE_FENS)]
    pvs = [_oracle_lines(root, 1, 2)[0]["pv"] for root in roots]
    for root, pv in zip(roots, pvs):
        assert len(pv) == 2 and root.children[ch.Move.from_uci(pv[0])].children[ch.Move.from_uci(pv[1])].n >= 2
    e = _engine(n, dirichlet)
    net = _net()
    out = []
    for plies in (1, 2, 0):                                 # 0: the same root, searched further
        for i, fen in enumerate(REUSE_FENS):
            e.submit(fen, sims=SIMS, id=600 + i, keep=True)
        first = _run(e, net)
        assert e.held() == n and e.pending() == 0
        rows = []
        for i, fen in enumerate(REUSE_FENS):
            assert _as_dict(first[600 + i])["lines"][0]["pv"][:2] == pvs[i], fen
            uid = 700 + 10 * i + plies
            n_before, want = _oracle_continue(roots[i], fen, pvs[i][:plies], uid, dirichlet)
            reused = e.continue_search(600 + i, pvs[i][:plies], sims=SIMS, id=uid, keep=False)
            rows.append((uid, plies, reused, n_before, want))
        assert e.held() == 0 and e.pending() == n
        got = _run(e, net)
        out += [(uid, plies, reused, n_before, _as_dict(got[uid]), want) for uid, plies, reused, n_before, want in rows]
    e.close()
    return tuple(out)


@pytest.mark.parametrize("dirichlet", [False, True])
def test_continued_search_matches_the_oracle_on_the_grafted_subtree(dirichlet):
    """Visit counts, moves, policy indices and PVs identical; priors and q of every line within 1e-6."""
    runs = _continued(dirichlet)
    assert len(runs) == 3 * len(REUSE_FENS)
    for uid, plies, reused, n_before, got, want in runs:
        assert reused == n_before > 0, uid
        assert got["root_n"] == reused + SIMS, uid
        _check(got, want, uid)


def test_q_of_unvisited_lines_of_a_continued_search():
    """The lines WITHOUT a visit, on their own: such a child still reports the q it was created with, which the reference
    seeds with -parent.q when its node is expanded (mcts.py:221-222; oracle/mcts_ref.py, expand()) and expand_kernel seeds the
    same way (child_seed_q).  The children of a fresh root have no grandparent and report 0 on both sides; the root children
    of a continued search were created one or two plies down, and some of them carry a seed: the case must occur here."""
    unvisited, seeded = 0, 0
    for uid, plies, reused, n_before, got, want in _continued(False):
        for g, w in zip(got["lines"], want["lines"]):
            if w["visits"] == 0:
                unvisited += 1
                seeded += w["q"] != 0.0
                print(f"id {uid}: {w['move']} without visits: q {g['q']} (engine) {w['q']} (oracle)")
                assert g["visits"] == 0 and abs(g["q"] - w["q"]) <= 1e-6, (uid, w["move"], g["q"], w["q"])
    assert unvisited > 0 and seeded > 0


def _plain(cfg, fen, ucis, uid):
    e = _engine(1, cfg=cfg)
    e.submit(fen, ucis, sims=SIMS, id=uid)
    raw = _run(e, _net())[uid]
    e.close()
    return raw


def test_fallback_is_a_plain_submission_bit_for_bit():
    net = _net()
    # a move whose child was never visited, hence never expanded
    fen = FENS[0]
    e = _engine(1)
    e.submit(fen, sims=SIMS, id=40, keep=True)
    _run(e, net)
    root = _oracle_first(fen, 40, False)
    cold = next(c.move.uci() for c in root.children.values() if c.n == 0)
    assert e.continue_search(40, [cold], sims=SIMS, id=41) == 0
    got = _run(e, net)[41]
    assert got == _plain(None, fen, [cold], 41) and _as_dict(got)["root_n"] == SIMS
    # ... behind an expanded one: the walk fails at the second move, all moves are played all the same
    hot = _oracle_lines(root, 1, 1)[0]["move"]
    child = root.children[ch.Move.from_uci(hot)]
    cold2 = next(c.move.uci() for c in child.children.values() if c.n == 0)
    e.submit(fen, sims=SIMS, id=40, keep=True)
    _run(e, net)
    assert e.continue_search(40, [hot, cold2], sims=SIMS, id=42) == 0
    assert _run(e, net)[42] == _plain(None, fen, [hot, cold2], 42)
    with pytest.raises(ValueError):
        e.continue_search(40, [], sims=SIMS, id=43)          # no longer held
    e.close()
    # pruned roots: a legal move that is not among the children
    cfg = _cfg(max_children=4)
    e = _engine(1, cfg=cfg)
    e.submit(fen, sims=SIMS, id=50, keep=True)
    r = _as_dict(_run(e, net)[50])
    kept = [ln["move"] for ln in r["lines"]]
    assert len(kept) == 4 and r["nlegal"] == 20
    gone = next(m.uci() for m in ch.Board(fen).legal_moves if m.uci() not in kept)
    with pytest.raises(ValueError, match="Illegal move"):
        e.continue_search(50, ["e2e5"], sims=SIMS, id=51)    # nothing changed: still held
    assert e.held() == 1
    assert e.continue_search(50, [gone], sims=SIMS, id=51, keep=True) == 0
    got = _run(e, net)[51]
    assert e.held() == 1
    e.close()
    assert got == _plain(cfg, fen, [gone], 51)


@pytest.fixture(scope="module")
def tb3():
    from matrix0_amd.tablebase import Tablebase
    tb = Tablebase.build(3, 0)
    yield tb
    tb.close()


def test_final_positions_that_need_no_search_are_answered_at_once(tb3):
    net = _net()
    e = _engine(1)
    for fen, move, status in ((FENS[4], "d1d8", "checkmate"), (FENS[5], "f7g6", "stalemate")):
        e.submit(fen, sims=SIMS, id=1, keep=True)
        _run(e, net)
        assert e.held() == 1
        assert e.continue_search(1, [move], sims=SIMS, id=2, keep=True) == 0
        (i, raw), = _poll_raw(e)
        r = _as_dict(raw)
        assert i == 2 and (r["status"], r["lines"], r["evals"], r["nlegal"]) == (status, [], 0, 0)
        assert e.held() == 0 and e.pending() == 0
    e.close()
    # a root inside the attached tables: four men are searched, the capture leads into KQK
    fen = "8/8/8/4k3/8/8/1r6/K1Q5 w - - 0 1"
    e = _engine(1)
    e.set_search_tablebase(tb3, 3)
    e.submit(fen, sims=SIMS, id=1, keep=True)
    assert _as_dict(_run(e, net)[1])["status"] == "ok" and e.held() == 1
    assert e.continue_search(1, ["c1b2"], sims=SIMS, id=2, keep=True) == 0
    (i, raw), = _poll_raw(e)
    r = _as_dict(raw)
    assert i == 2 and r["status"] == "tablebase" and r["root_q"] == -1.0 and r["evals"] == 0 and r["lines"]
    assert e.held() == 0 and e.pending() == 0
    e.close()


def test_held_slots_are_counted_apart_and_call_order_holds():
    from matrix0_amd import _lib
    from matrix0_amd import engine as eng
    L = _lib.lib()
    net = _net()
    e = _engine(1)
    e.submit(FENS[0], sims=SIMS, id=1, keep=True)
    _run(e, net)
    assert e.pending() == 0 and e.held() == 1
    with pytest.raises(ValueError):
        e.release(2)
    e.submit(FENS[1], sims=SIMS, id=2)
    assert e.pending() == 1
    with pytest.raises(RuntimeError, match="held"):
        e.step(net.infer_np, 1)                             # M0_ERR_STATE, not a pass that does nothing
    assert e.pending() == 1 and e.held() == 1
    e.release(1)
    assert e.held() == 0
    # between select and expand every live call is refused
    cap = 1 * (LEAVES + 1)
    planes, rows = np.zeros((cap, 19, 8, 8), np.float32), C.c_int(0)
    assert L.m0_analysis_ext_select(e._h, C.byref(rows), planes.ctypes.data_as(C.c_void_p), cap) == _lib.M0_OK
    res, reused = eng.AnalysisResult(), C.c_int32(0)
    fen = FENS[0].encode()
    for rc in (L.m0_analysis_submit_keep(e._h, fen, None, 0, SIMS, 9), L.m0_analysis_peek(e._h, 2, C.byref(res)),
               L.m0_analysis_stop(e._h, 2), L.m0_analysis_continue(e._h, 1, None, 0, SIMS, 9, 0, C.byref(reused)),
               L.m0_analysis_release(e._h, 1), L.m0_analysis_held(e._h)):
        assert rc == _lib.M0_ERR_STATE
    lg, v = net.infer_np(planes[: rows.value])
    e._expand(L.m0_analysis_ext_expand, "m0_analysis_ext_expand", (lg, v))
    assert e.peek(2) is not None
    got = _run(e, net)
    e.close()
    assert _as_dict(got[2])["root_n"] == SIMS
    # and on an engine that is no analysis engine
    sp = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(_cfg(), concurrent_games=1))
    for rc in (L.m0_analysis_submit_keep(sp._h, fen, None, 0, SIMS, 9), L.m0_analysis_peek(sp._h, 2, C.byref(res)),
               L.m0_analysis_stop(sp._h, 2), L.m0_analysis_continue(sp._h, 1, None, 0, SIMS, 9, 0, C.byref(reused)),
               L.m0_analysis_release(sp._h, 1), L.m0_analysis_held(sp._h)):
        assert rc == _lib.M0_ERR_STATE
    sp.close()


def test_plain_submissions_do_not_notice_a_held_tree():
    positions = list(FENS) + [MANY_MOVES]
    net = _net()
    a = _engine(3)
    a.submit(FENS[1], sims=SIMS, id=99, keep=True)
    _run(a, net)
    assert a.held() == 1
    b = _engine(3)
    for e in (a, b):
        for i, fen in enumerate(positions):
            e.submit(fen, sims=SIMS, id=i)
    ga, gb = _run(a, net), _run(b, net)
    assert a.held() == 1 and b.held() == 0
    a.close()
    b.close()
    for i in range(len(positions)):
        assert ga[i] == gb[i], positions[i]


def test_fused_step_equals_split_step_on_the_real_network():
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(NET, net_ref.random_state_dict(NET, seed=7))
    c = eng.selfplay_cfg_from_dict(_cfg(), concurrent_games=2, record_games=False)
    kw = dict(multipv=MULTIPV, pv_len=PV_LEN, dirichlet=True)
    fused, split = eng.AnalysisEngine(be, c, **kw), eng.AnalysisExtEngine(c, **kw)

    def script(e, step):
        out = []
        e.submit(FENS[1], sims=128, id=1, keep=True)
        e.submit(FENS[3], sims=SIMS, id=2)
        for _ in range(4):
            step()
        out.append(bytes(e.peek_raw(1)))
        e.stop(1)
        out += _poll_raw(e)
        pv = _as_dict(out[0])["lines"][0]["pv"][:2]
        out.append(e.continue_search(1, pv, sims=SIMS, id=3, keep=True))
        out.append(bytes(e.peek_raw(3)))
        while e.pending():
            step()
        out += sorted(_poll_raw(e))
        out.append(e.held())
        return out

    f = script(fused, lambda: fused.step(1))
    s = script(split, lambda: split.step(be.infer_np, 1))
    fused.close()
    split.close()
    be.close()
    assert f == s
    # [peek of 1, (1, its stop), reused_n, peek of 3, (2, result), (3, result), held]
    assert len(f) == 7 and f[1] == (1, f[0]) and f[2] > 0 and f[-1] == 1 and _as_dict(f[0])["sims"] == 3 * LEAVES
    assert _as_dict(f[3])["root_n"] == f[2] and _as_dict(dict(f[4:6])[3])["root_n"] == f[2] + SIMS
