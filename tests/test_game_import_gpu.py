"""Reading games back in, on the device: m0_replay_games (one wave per game, csrc/replay_kernels.hip) through
game_import.replay_games and import_pgn.  Every comparison is bit-exact: against the host shim of the same rule
(tests/host_shim/replay_shim.cpp), against encoding.encode_fens / engine.ssl_targets_fens on engine.fen_after positions, against the oracle, and
against the engine's own self-play records."""
import os

import numpy as np
import pytest

from matrix0_amd import arena
from matrix0_amd import encoding as enc
from matrix0_amd import engine as eng
from matrix0_amd import game_import as gi
from oracle import chess_py as ch
from oracle import net_ref
from tests import replay_util as ru

pytestmark = pytest.mark.gpu

PER_PLY = ("moves", "policy_idx", "nlegal", "turn", "planes", "mask", "ssl")


@pytest.fixture(scope="module")
def replayed():
    """All 125 fixture games in one call, with SSL maps."""
    return gi.replay_games([(None, toks) for toks, _ in ru.fixture_games()], ssl=True)


@pytest.fixture(scope="module")
def positions(replayed):
    """Per game the FEN before every ply, from engine.fen_after(start, moves[:k]); and one encode_fens call over all of them."""
    fens = []
    for r in replayed:
        ucis = [eng.move_to_uci(int(m)) for m in r["moves"]]
        fens.append([eng.fen_after(ch.START_FEN, ucis[:k]) for k in range(len(ucis))])
    flat = [f for g in fens for f in g]
    planes, mask, moves = enc.encode_fens(flat)
    return fens, flat, planes, mask, moves


def test_fixture_games_resolve_like_the_shim(replayed):
    games = ru.fixture_games()
    assert len(replayed) == 125
    for (toks, _), r in zip(games, replayed):
        want = ru.shim_replay(None, toks)
        assert r["status"] == "ok" and r["plies"] == len(toks) == len(r["moves"])
        assert r["end"] == want["end"]
        for k in ("moves", "policy_idx", "nlegal", "turn"):
            assert r[k].dtype == want[k].dtype and np.array_equal(r[k], want[k]), k
    assert sum(r["end"]["checkmate"] for r in replayed) == 96 and not any(r["end"]["stalemate"] for r in replayed)


def test_fixture_positions_equal_encode_fens(replayed, positions):
    _, flat, planes, mask, moves = positions
    assert len(flat) == 7875
    got = {k: np.concatenate([r[k] for r in replayed]) for k in ("planes", "mask", "policy_idx", "nlegal", "moves")}
    assert got["planes"].dtype == np.float32 and got["planes"].shape == (7875, 19, 8, 8) and np.array_equal(got["planes"], planes)
    assert got["mask"].dtype == np.uint8 and got["mask"].shape == (7875, 4672) and np.array_equal(got["mask"].astype(bool), mask)
    assert got["nlegal"].tolist() == [len(u) for u, _ in moves]
    assert got["policy_idx"].tolist() == [idx[u.index(eng.move_to_uci(int(m)))] for (u, idx), m in zip(moves, got["moves"])]
    assert got["mask"][np.arange(7875), got["policy_idx"]].all()


def test_ten_fixture_games_equal_the_oracle(replayed):
    for (toks, _), r in list(zip(ru.fixture_games(), replayed))[::13][:10]:
        b = ch.Board()
        for k in range(len(toks)):
            m = ch.Move.from_uci(eng.move_to_uci(int(r["moves"][k])))
            assert np.array_equal(r["planes"][k], ch.encode_board(b))
            assert np.array_equal(r["mask"][k].astype(bool), ch.get_legal_actions(b))
            assert r["policy_idx"][k] == ch.move_to_index(b, m) and r["turn"][k] == int(b.turn)
            b.push(m)
        assert r["end"]["checkmate"] == b.is_checkmate() and r["end"]["insufficient"] == b.is_insufficient_material()


def test_fixture_ssl_maps_equal_ssl_targets_fens(replayed, positions):
    _, flat, *_ = positions
    want = eng.ssl_targets_fens(flat)
    got = np.concatenate([r["ssl"] for r in replayed])
    assert got.dtype == np.float32 and got.shape == (7875, 17, 8, 8)
    assert np.array_equal(got[:, :13], want["piece"])
    for ch_, name in ((13, "threat"), (14, "pin"), (15, "fork"), (16, "control")):
        assert np.array_equal(got[:, ch_], want[name]), name


@pytest.mark.parametrize("name", sorted(ru.HAND_CASES))
def test_hand_made_cases(name):
    fen, toks, max_plies, status, plies, moves = ru.hand_case(name)
    (r,) = gi.replay_games([(fen, toks)], ssl=True, max_plies=max_plies)
    want = ru.shim_replay(fen, toks, max_plies=max_plies, planes=True)
    assert (r["status"], r["plies"]) == (status, plies) == (want["status"], want["plies"])
    assert r["end"] == want["end"]
    if moves is not None:
        assert [eng.move_to_uci(int(m)) for m in r["moves"][:plies]] == moves
    for k in ("moves", "policy_idx", "nlegal", "turn", "planes"):
        assert np.array_equal(r[k], want[k]), k
    for k in PER_PLY:
        assert len(r[k]) == len(toks) and not r[k][plies:].any(), k       # zero rows after the stop
    assert r["mask"][:plies].sum(axis=1).tolist() == r["nlegal"][:plies].tolist()


def test_hand_made_cases_in_one_call_and_a_bad_fen():
    names = [n for n in sorted(ru.HAND_CASES) if n != "too_long"]
    res = gi.replay_games([ru.hand_case(n)[:2] for n in names], planes=False, mask=False)
    for n, r in zip(names, res):
        _, _, _, status, plies, _ = ru.hand_case(n)
        assert (r["status"], r["plies"]) == (status, plies), n
        assert "planes" not in r and "mask" not in r and "ssl" not in r
    with pytest.raises(ValueError, match="index 2"):
        gi.replay_games([(None, ["e4"]), (None, ["d4"]), ("not a fen", ["e4"])])


def test_results_do_not_depend_on_launch_size_or_game_order():
    games = [(None, toks) for toks, _ in ru.fixture_games()[:20]]
    small = gi.replay_games(games, ssl=True, max_positions_per_launch=64)
    whole = gi.replay_games(games, ssl=True, max_positions_per_launch=0)
    back = gi.replay_games(games[::-1], ssl=True)[::-1]
    for a, b, c in zip(small, whole, back):
        assert a["status"] == b["status"] == c["status"] == "ok" and a["plies"] == b["plies"] == c["plies"]
        assert a["end"] == b["end"] == c["end"]
        for k in PER_PLY:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k


def test_engine_records_replay_to_their_own_samples():
    from matrix0_amd.backend import M0Backend
    net = dict(planes=19, channels=32, blocks=2, attention_heads=2, policy_size=4672, norm="group", activation="silu",
               preact=True, policy_factor_rank=16, self_supervised=False)
    cfg = {"seed": 7, "mcts": {"cpuct": 2.5, "legal_softmax": True, "inference_batch_size": 8},
           "selfplay": {"num_simulations": 8, "max_game_len": 24, "min_resign_plies": 50}}
    be = M0Backend.from_state_dict(net, net_ref.random_state_dict(net, seed=1))
    e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(cfg, concurrent_games=4, total_games=4, record_games=True))
    records = []
    for _ in range(2000):
        e.step(8)
        while (r := e.poll()) is not None:
            records.append(r)
        if not e.running():
            break
    e.close()
    be.close()
    assert len(records) == 4
    res = gi.replay_games([(r.get("start_fen"), [int(m) for m in r["played_raw"]]) for r in records])
    for rec, r in zip(records, res):
        T = rec["moves"]
        assert 1 <= T <= 24 and r["status"] == "ok" and r["plies"] == len(rec["played_raw"])
        n_open = len(rec["played_raw"]) - (T - (1 if rec["resigned"] else 0))      # plies played before the first recorded one
        assert n_open == 0
        n = r["plies"]
        assert np.array_equal(r["moves"], rec["played_raw"])
        assert np.array_equal(r["planes"], rec["s"][:n]) and np.array_equal(r["mask"], rec["legal_mask"][:n])
        assert (rec["pi"][np.arange(n), r["policy_idx"]] > 0).all()
        # the same game written as UCI strings
        (u,) = gi.replay_games([(rec.get("start_fen"), rec["played"])], notation="uci", planes=False, mask=False)
        assert u["status"] == "ok" and np.array_equal(u["moves"], r["moves"]) and np.array_equal(u["policy_idx"], r["policy_idx"])


def test_import_pgn_end_to_end(tmp_path):
    games = ru.fixture_games()
    pgn_dir = tmp_path / "pgn"
    paths = [arena.save_pgn(ru.shim_replay(None, toks)["moves"], result, {"Round": i + 1}, str(pgn_dir), i)
             for i, (toks, result) in enumerate(games)]
    pgn = tmp_path / "all.pgn"
    pgn.write_text("\n".join(open(p).read() for p in paths))
    turns = np.concatenate([ru.shim_replay(None, toks)["turn"] for toks, _ in games]).astype(np.float32) * 2 - 1
    header_z = np.concatenate([np.full(len(toks), {"1-0": 1.0, "0-1": -1.0, "1/2-1/2": 0.0}[res], np.float32) for toks, res in games])
    ends = [ru.shim_replay(None, toks)["end"] for toks, _ in games]

    def load(d):
        files = sorted(os.listdir(d))
        assert files == [f"import_{i:06d}.npz" for i in range(4)]
        shards = [np.load(os.path.join(d, f)) for f in files]
        assert [len(s["z"]) for s in shards] == [2048, 2048, 2048, 1731]
        for s in shards:
            n = len(s["z"])
            assert sorted(s.files) == ["legal_mask", "pi", "s", "z"]
            assert (s["s"].dtype, s["s"].shape) == (np.float32, (n, 19, 8, 8))
            assert (s["pi"].dtype, s["pi"].shape) == (np.float32, (n, 4672))
            assert (s["z"].dtype, s["z"].shape) == (np.float32, (n,))
            assert (s["legal_mask"].dtype, s["legal_mask"].shape) == (np.uint8, (n, 4672))
        return {k: np.concatenate([s[k] for s in shards]) for k in ("s", "pi", "z", "legal_mask")}

    summary = gi.import_pgn(str(pgn), str(tmp_path / "header"), shard_size=2048)
    assert summary == {"games_read": 125, "games_kept": 125, "games_filtered": 0, "games_truncated": 0, "games_dropped": 0,
                       "samples": 7875, "shards": 4, "result_mismatches": 83}
    d = load(tmp_path / "header")
    assert ((d["pi"] == 1.0).sum(axis=1) == 1).all() and (d["pi"].sum(axis=1) == 1.0).all()      # one-hot ...
    assert d["legal_mask"][np.arange(7875), d["pi"].argmax(axis=1)].all()                        # ... inside the mask
    assert np.array_equal(d["z"], header_z * turns)          # the header's result, sign flipped with the side to move
    assert np.array_equal(d["s"][:, 12, 0, 0] * 2 - 1, turns)

    summary = gi.import_pgn(str(pgn), str(tmp_path / "board"), shard_size=2048, result_source="board")
    assert summary["result_mismatches"] == 83 and summary["samples"] == 7875
    b = load(tmp_path / "board")
    assert np.array_equal(b["s"], d["s"]) and np.array_equal(b["pi"], d["pi"]) and np.array_equal(b["legal_mask"], d["legal_mask"])
    at = 0
    for (toks, res), end in zip(games, ends):
        z, t = b["z"][at: at + len(toks)], turns[at: at + len(toks)]
        if end["checkmate"]:                                 # the mated side is to move at the end: its samples carry -1
            mated = 1.0 if end["white_to_move"] else -1.0
            assert np.array_equal(z, np.where(t == mated, -1.0, 1.0).astype(np.float32))
        else:
            assert np.array_equal(z, header_z[at: at + len(toks)] * t)
        at += len(toks)
