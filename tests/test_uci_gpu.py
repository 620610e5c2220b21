"""A scripted session on the real UciEngine (matrix0_amd/uci.py) over a one-slot external-evaluator analysis engine on the GPU,
against the same searches made through the engine's own calls: `go nodes N` is deterministic, so the best moves, the node counts
and the size of the reused tree must be the same."""
import pytest

from matrix0_amd import uci
from tests.fake_net import FakeNet
from tests.test_search_gpu import MCTS

pytestmark = pytest.mark.gpu

CFG = {"seed": 1234, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": 256}}
OPENING = ["e2e4", "e7e5"]


def _engine():
    from matrix0_amd import engine as eng
    c = eng.selfplay_cfg_from_dict(CFG, concurrent_games=1, record_games=False)
    return eng.AnalysisExtEngine(c, multipv=8, pv_len=16)


def _finish(e, net):
    while e.pending():
        e.step(net.infer_np, 1)
    r = e.poll()
    assert r is not None and e.poll() is None
    return r


def _last_info(lines):
    info = [ln for ln in lines if ln.startswith("info depth") and " multipv 1 " in ln][-1].split()
    return {"nodes": int(info[info.index("nodes") + 1]), "pv": info[info.index("pv") + 1:], "depth": int(info[info.index("depth") + 1])}


def test_scripted_session_equals_the_engine_calls():
    # the searches through the engine's own calls, ids 1, 2, 3 as the front end numbers them
    net = FakeNet(seed=3, sharp=8.0)
    e = _engine()
    e.submit(uci.START_FEN, OPENING, sims=128, id=1, keep=True)
    r1 = _finish(e, net)
    nxt = r1["lines"][0]["pv"][:2]
    assert len(nxt) == 2
    reused = e.continue_search(1, nxt, sims=128, id=2, keep=True)
    r2 = _finish(e, net)
    reused3 = e.continue_search(2, [], sims=256, id=3, keep=True)
    for _ in range(3):
        e.step(net.infer_np, 1)
    e.stop(3)
    r3 = e.poll()
    e.close()
    assert reused > 0 and r2["root_n"] == reused + 128 and reused3 == r2["root_n"] and r3["sims"] == 3 * 8

    # the session
    net = FakeNet(seed=3, sharp=8.0)
    e = _engine()
    out = []
    u = uci.UciEngine(e, CFG, out=out.append, step=lambda: e.step(net.infer_np, 1))
    u.command("uci")
    u.command("isready")
    assert out[-1] == "readyok" and "uciok" in out
    assert "option name MaxNodes type spin default 256 min 1 max 1000000" in out
    u.command("position startpos moves " + " ".join(OPENING))
    del out[:]
    u.command("go nodes 128")
    while u.pump():
        pass
    assert out[-1].split()[:2] == ["bestmove", r1["lines"][0]["move"]] and out[-1].split()[2:] == ["ponder", nxt[1]]
    li = _last_info(out)
    assert li["nodes"] == r1["root_n"] == 128 and li["pv"] == r1["lines"][0]["pv"] and li["depth"] == len(li["pv"])
    assert not any("reused" in ln for ln in out) and e.held() == 1

    u.command("position startpos moves " + " ".join(OPENING + nxt))
    del out[:]
    u.command("go nodes 128")
    assert out[0] == f"info string tree reused: {reused} nodes kept over 2 moves" and u.last_reused == reused > 0
    while u.pump():
        pass
    assert out[-1].split()[:2] == ["bestmove", r2["lines"][0]["move"]]
    li = _last_info(out)
    assert li["nodes"] == r2["root_n"] == reused + 128 and li["pv"] == r2["lines"][0]["pv"]

    del out[:]
    u.command("go infinite")
    assert out[0] == f"info string tree reused: {reused3} nodes kept over 0 moves"
    for _ in range(3):
        assert u.pump()
    u.command("isready")
    assert out[-1] == "readyok" and u.searching()
    u.command("stop")
    assert u.pump() is False
    assert out[-1].split()[:2] == ["bestmove", r3["lines"][0]["move"]]
    li = _last_info(out)
    assert li["nodes"] == r3["root_n"] == reused3 + 3 * 8 and li["pv"] == r3["lines"][0]["pv"]
    assert e.held() == 1
    u.command("ucinewgame")
    assert e.held() == 0
    e.close()
