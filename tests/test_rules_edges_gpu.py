"""The device's chess rules on the corpus of tests/rules_cases.py: the wave-per-position kernels behind encode_fens
(gen_legal_wave, encode_positions_kernel), replay_games (gen_legal_wave, the move matching, device make_move) and decode_planes
against the oracle, bit for bit, on positions chosen for the rules' corners and for move lists that need a second and a fourth
round of 64 lanes.  The replay test is perft with the moves written out: every legal sequence of two or three plies from seven
roots, each played on the device."""
import functools
import time

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import planes_cases as pc
from tests import rules_cases as rc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle_neighbourhood():
    """Per position of the two-ply neighbourhood: (ucis, policy indices), planes, mask, whether an en-passant capture is legal.
    Shared, never modified."""
    nb = rc.neighbourhood(2)
    planes = np.zeros((len(nb), 19, 8, 8), np.float32)
    mask = np.zeros((len(nb), 4672), bool)
    moves, ep = [], []
    for i, fen in enumerate(nb):
        b = ch.Board(fen)
        om, oi = ch.legal_moves_with_indices(b)
        moves.append(([m.uci() for m in om], oi))
        ep.append(ch.square_name(b.ep_square) if any(rc.is_en_passant(b, m) for m in om) else None)
        planes[i] = ch.encode_board(b)
        mask[i] = ch.get_legal_actions(b)
    planes.setflags(write=False); mask.setflags(write=False)
    return nb, moves, planes, mask, ep


def _first_difference(got, want):
    """Index of the first row in which two arrays differ bit for bit, or None."""
    a = np.ascontiguousarray(got).reshape(len(got), -1).view(np.uint8)
    b = np.ascontiguousarray(want).reshape(len(want), -1).view(np.uint8)
    assert a.shape == b.shape
    bad = np.flatnonzero((a != b).any(axis=1))
    return int(bad[0]) if bad.size else None


def test_encode_fens_over_the_whole_neighbourhood():
    from matrix0_amd import encoding as enc
    nb, want_moves, want_planes, want_mask, _ = _oracle_neighbourhood()
    t0 = time.time()
    planes, mask, moves = enc.encode_fens(list(nb))
    print(f"encode_fens: {len(nb)} positions in {time.time() - t0:.2f} s")
    assert planes.dtype == np.float32 and mask.dtype == bool
    for i, fen in enumerate(nb):
        assert moves[i][0] == want_moves[i][0], fen                     # the legal moves, in order (so nlegal as well)
        assert moves[i][1] == want_moves[i][1], fen
    bad = _first_difference(planes, want_planes)
    assert bad is None, nb[bad]
    bad = _first_difference(mask, want_mask)
    assert bad is None, nb[bad]
    assert mask.sum(axis=1).tolist() == [len(u) for u, _ in want_moves]
    assert max(len(u) for u, _ in moves) == 218 and sum(len(u) > 64 for u, _ in moves) > 300
    # the same positions in two calls of other sizes
    cut = 5001
    p1, m1, v1 = enc.encode_fens(list(nb[:cut]))
    p2, m2, v2 = enc.encode_fens(list(nb[cut:]))
    assert np.concatenate([p1, p2]).tobytes() == planes.tobytes() and np.concatenate([m1, m2]).tobytes() == mask.tobytes()
    assert v1 + v2 == moves


def _same_as_oracle(res, games, want):
    assert len(res) == len(games) == len(want)
    for r, (fen, ucis), (rows, end) in zip(res, games, want):
        assert r["status"] == "ok" and r["plies"] == len(ucis) == len(rows), (fen, ucis, r["status"], r["plies"])
        assert r["end"] == end, (fen, ucis)
        got = list(zip(r["nlegal"].tolist(), r["policy_idx"].tolist(), r["turn"].tolist(), r["moves"].tolist()))
        assert got == list(rows), (fen, ucis)


def test_perft_by_replay():
    """Every path of rules_cases.PERFT_PATHS as a game of UCI tokens: the device's legal count, policy index, side to move and
    move for every row and its end flags are the oracle's; the same in launches of another size; planes and masks of every 16th
    game."""
    from matrix0_amd import game_import as gi
    games, want = rc.replay_set()
    n_rows = sum(len(u) for _, u in games)
    assert len(games) > 40000 and n_rows > 160000
    t0 = time.time()
    res = gi.replay_games(games, notation="uci", planes=False, mask=False)
    print(f"replay_games: {len(games)} games, {n_rows} rows in {time.time() - t0:.2f} s")
    _same_as_oracle(res, games, want)
    again = gi.replay_games(games, notation="uci", planes=False, mask=False, max_positions_per_launch=4099)
    for a, b in zip(res, again):
        assert (a["status"], a["plies"], a["end"]) == (b["status"], b["plies"], b["end"])
        for k in ("moves", "policy_idx", "nlegal", "turn"):
            assert a[k].tobytes() == b[k].tobytes(), k
    some = games[::16]
    full = gi.replay_games(some, notation="uci", planes=True, mask=True)
    _same_as_oracle(full, some, want[::16])
    for r, (fen, ucis) in zip(full, some):
        b = ch.Board(fen)
        assert r["planes"].shape == (len(ucis), 19, 8, 8) and r["mask"].shape == (len(ucis), 4672)
        for k, u in enumerate(ucis):
            assert r["planes"][k].tobytes() == ch.encode_board(b).tobytes(), (fen, ucis, k)
            assert np.array_equal(r["mask"][k].astype(bool), ch.get_legal_actions(b)), (fen, ucis, k)
            b.push(ch.Move.from_uci(u))


def test_moves_that_are_not_legal_are_refused():
    """Per corpus root every from-to pair from a piece of the side to move that is no legal move, as a game of that one token:
    refused with nothing played; every legal move: played."""
    from matrix0_amd import game_import as gi
    games, legal = [], []
    for _, _, fen in rc.ROOTS:
        bad, good = rc.refusals(fen)
        games += [(fen, [u]) for u in bad]
        legal += [(fen, [u]) for u in good]
    assert len(games) > 20000 and len(legal) > 2000
    for r, (fen, toks) in zip(gi.replay_games(games, notation="uci", planes=False, mask=False), games):
        assert (r["status"], r["plies"]) == ("illegal", 0), (fen, toks)
        assert not r["moves"].any() and not r["nlegal"].any()
    for r, (fen, toks) in zip(gi.replay_games(legal, notation="uci", planes=False, mask=False), legal):
        assert (r["status"], r["plies"]) == ("ok", 1), (fen, toks)
        assert r["moves"].tolist() == [rc.raw_move(ch.Move.from_uci(toks[0]))]


def test_decode_planes_on_the_oracles_rows():
    """The way back, on rows the oracle wrote: every position of the neighbourhood is accepted, with the oracle's legal count, and
    the en-passant square comes back from the mask exactly where a capture is legal."""
    from matrix0_amd import encoding as enc
    nb, want_moves, planes, mask, ep = _oracle_neighbourhood()
    d = enc.decode_planes(planes, mask.astype(np.uint8))
    bad = np.flatnonzero(d["status"] != pc.OK)
    assert bad.size == 0, (nb[bad[0]], int(d["status"][bad[0]]))
    assert d["nlegal"].tolist() == [len(u) for u, _ in want_moves]
    assert sum(e is not None for e in ep) >= 5
    for fen, flags, got, e in zip(nb, d["flags"], d["fens"], ep):
        assert bool(flags & pc.EP_FROM_MASK) == (e is not None), fen
        assert got.split(" ")[3] == (e or "-"), (fen, got)
        assert not flags & ~pc.EP_FROM_MASK, fen
        assert got == ch.Board(fen).fen(), fen                          # the oracle's FEN names the square under the same rule
