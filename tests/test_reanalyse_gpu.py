"""Reanalyse on the GPU: decode_planes_kernel against the host build of the same decode (tests/host_shim/planes_shim.cpp), the round trip
planes -> position -> planes on replayed games, every root child's visits against the oracle tree of
tests/test_analysis_gpu.py, m0_analysis_submit_planes against m0_analysis_submit bit for bit, and the tool end to end on rows
of a short self-play run."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import planes_cases as pc
from tests.fake_net import FakeNet
from tests.golden_ref import load_npz
from tests.test_analysis_gpu import MANY_MOVES, SIMS, _cfg, _check, _ext, _oracle_run, _oracle_set, _positions

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _decode_rows():
    """About 1 500 rows with their masks: every seventh golden row, the hand-written en-passant positions, every malformed
    row.  Shared, never modified."""
    z = load_npz("ref_encoding.npz")
    sel = np.arange(0, len(z["fens"]), 7)
    n = len(sel)
    planes = np.zeros((n, 19, 8, 8), np.float32)
    planes[:, :17] = np.unpackbits(z["plane_bits"][sel], axis=2).reshape(n, 17, 8, 8)
    planes[:, 17] = z["counters"][sel, 0, None, None]
    planes[:, 18] = z["counters"][sel, 1, None, None]
    off = np.concatenate([[0], np.cumsum(z["nlegal"].astype(np.int64))])
    mask = np.zeros((n, 4672), np.uint8)
    for j, i in enumerate(sel):
        mask[j, z["idx"][off[i]: off[i + 1]]] = 1
    hand = [pc.encode(f) for f, _ in pc.EP_FENS]
    bad = pc.malformed_rows()
    planes = np.concatenate([planes, np.stack([h[0] for h in hand]), np.stack([b[2] for b in bad])])
    mask = np.concatenate([mask, np.stack([h[1] for h in hand]), np.stack([b[3] for b in bad])])
    planes.setflags(write=False); mask.setflags(write=False)
    return planes, mask, [b[1] for b in bad]


def _same(got, want, tag):
    for k in ("status", "flags", "nlegal"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (tag, k, int(bad[0]), int(got[k][bad[0]]), int(want[k][bad[0]]))
    assert got["fens"] == want["fens"], tag


def test_decode_kernel_equals_the_host_function():
    from matrix0_amd import encoding as enc
    planes, mask, bad_status = _decode_rows()
    n = len(planes)
    assert 1400 <= n <= 1600
    want = pc.host_decode(planes, mask)
    assert want["status"][-len(bad_status):].tolist() == bad_status and set(bad_status) == set(range(1, 12))
    assert (want["flags"] & pc.EP_FROM_MASK).sum() >= 7 and not want["status"][: n - len(bad_status)].any()
    _same(enc.decode_planes(planes, mask), want, "one launch")
    _same(enc.decode_planes(planes), pc.host_decode(planes), "one launch, no mask")
    # every row alone
    one = [enc.decode_planes(planes[i: i + 1], mask[i: i + 1]) for i in range(n)]
    _same({k: np.concatenate([o[k] for o in one]) for k in ("status", "flags", "nlegal")} | {"fens": [o["fens"][0] for o in one]},
          want, "n = 1")
    with pytest.raises(ValueError):
        enc.decode_planes(planes[:2], mask[:3])


def test_replayed_games_come_back_from_their_planes():
    """Ten of the reference's evaluation games: every position before a move, as the import writes it (planes + mask) ->
    position -> planes + mask again, bit for bit.  The ten are chosen for what arises in them by itself (counted on the CPU
    with the oracle): in eight an en-passant capture is legal once, in three a side loses its last castling right."""
    from matrix0_amd import encoding as enc
    from matrix0_amd import game_import
    from tests.replay_util import fixture_games
    games = [(None, fixture_games()[g][0]) for g in (3, 4, 7, 21, 32, 51, 53, 59, 60, 120)]
    res = game_import.replay_games(games)
    assert all(r["status"] == "ok" for r in res)
    planes = np.concatenate([r["planes"][: r["plies"]] for r in res])
    mask = np.concatenate([r["mask"][: r["plies"]] for r in res])
    nlegal = np.concatenate([r["nlegal"][: r["plies"]] for r in res])
    assert len(planes) == sum(len(toks) for _, toks in games) == 377
    d = enc.decode_planes(planes, mask)
    assert not d["status"].any() and np.array_equal(d["nlegal"], nlegal)
    assert not (d["flags"] & ~pc.EP_FROM_MASK).any()
    planes2, mask2, _ = enc.encode_fens(d["fens"], want_moves=False)
    assert planes2.tobytes() == planes.tobytes()
    assert np.array_equal(mask2, mask.astype(bool))
    rights = planes[:, 13:17, 0, 0].sum(axis=1)
    assert rights.max() == 4 and rights.min() == 0                     # from all four rights to none
    # the decoded en-passant squares are exactly the rows where such a capture is legal
    assert np.count_nonzero(d["flags"] & pc.EP_FROM_MASK) == 8
    for i in np.flatnonzero(d["flags"] & pc.EP_FROM_MASK):
        b = ch.Board(d["fens"][i])
        assert d["fens"][i].split()[3] != "-" and any(pc.is_en_passant(b, m) for m in b.legal_moves)
    assert all(f.split()[3] == "-" for f, fl in zip(d["fens"], d["flags"]) if not fl & pc.EP_FROM_MASK)


def _drain(an, visits):
    out = {}
    while True:
        r = an.engine.poll(visits=True) if visits else an.engine.poll()
        if r is None:
            return out
        out[r["id"]] = r


def _run_all(an, visits):
    got = _drain(an, visits)
    while an.engine.pending() > 0:
        an._step()
        got.update(_drain(an, visits))
    return got


def test_every_root_child_comes_back_and_equals_the_oracle():
    positions = _positions()
    want = _oracle_set(False)
    an = _ext(3)
    an.engine.keep_visits(True)
    for i, fen in enumerate(positions):
        an.engine.submit(fen, [], sims=SIMS, id=i)
    kept = _run_all(an, True)
    an.engine.keep_visits(False)
    for i, fen in enumerate(positions):
        an.engine.submit(fen, [], sims=SIMS, id=i)
    plain = _run_all(an, True)
    an.close()
    assert sorted(kept) == sorted(plain) == list(range(len(positions)))
    searched = 0
    for i, fen in enumerate(positions):
        g, w = kept[i], want[i]
        _check(g, w, (i, fen))
        if w["status"] != "ok":                                         # answered on the host
            assert g["visits"].size == 0 and g["policy_idx"].size == 0, fen
            continue
        searched += 1
        _, idxs = ch.legal_moves_with_indices(ch.Board(fen))
        assert g["policy_idx"].tolist() == idxs, fen                    # every child, in move-generation order
        assert g["visits"].tolist() == w["counts"], fen
        first_max = int(np.argmax(g["visits"]))                         # lines[0]: the first maximum
        assert (g["lines"][0]["policy_index"], g["lines"][0]["visits"]) == (idxs[first_max], w["counts"][first_max]), fen
        # keeping off: the same result without the children
        p = plain[i]
        assert p["visits"].size == 0 and p["policy_idx"].size == 0, fen
        assert {k: v for k, v in p.items() if k not in ("visits", "policy_idx")} == \
            {k: v for k, v in g.items() if k not in ("visits", "policy_idx")}, fen
    assert searched == len(positions) - 2 and kept[positions.index(MANY_MOVES)]["nlegal"] == 218   # four children on a lane
    import ctypes as C
    from matrix0_amd import _lib
    from matrix0_amd import engine as eng
    an = _ext(1)
    r, k, buf = eng.AnalysisResult(), C.c_int32(0), np.zeros(256, np.int32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert an.engine._L.m0_analysis_poll_visits(an.engine._h, C.byref(r), C.byref(k), ptr, ptr, 255) == _lib.M0_ERR_INVALID
    assert an.engine._L.m0_analysis_poll_visits(an.engine._h, C.byref(r), C.byref(k), ptr, ptr, 256) == 0
    an.close()


def test_submit_planes_equals_submit_fen_whatever_the_slots():
    from matrix0_amd import encoding as enc
    fens = _positions() + [f for f, _ in pc.EP_FENS]
    enc_rows = [pc.encode(f) for f in fens]
    bad = {name: (p, m) for name, _, p, m in pc.malformed_rows()}
    bad_rows = {4: "piece_value_nan", 17: "mask_missing_bit", len(fens) + 2: "board_of_queens"}
    planes, mask = [e[0] for e in enc_rows], [e[1] for e in enc_rows]
    for at in sorted(bad_rows):
        planes.insert(at, bad[bad_rows[at]][0]); mask.insert(at, bad[bad_rows[at]][1])
    planes, mask = np.stack(planes), np.stack(mask)
    n = len(planes)
    ids = np.arange(500, 500 + n)
    d = enc.decode_planes(planes, mask)
    good = [r for r in range(n) if r not in bad_rows]
    assert [int(d["status"][r]) for r in sorted(bad_rows)] == [pc.PIECE_VALUE, pc.MASK_MISMATCH, pc.TOO_MANY_MOVES]
    assert not d["status"][good].any()
    host_answered = sum(1 for r in good if d["nlegal"][r] == 0)
    assert host_answered == 2

    def by_planes(slots):
        an = _ext(slots, dirichlet=True)
        status, flags = an.engine.submit_planes(planes, mask, sims=SIMS, ids=ids)
        assert np.array_equal(status, d["status"]) and np.array_equal(flags, d["flags"])
        assert an.engine.pending() == len(good) - host_answered      # bad rows are reported, not queued
        got = _run_all(an, False)
        an.close()
        return got

    a, b = by_planes(3), by_planes(7)
    an = _ext(3, dirichlet=True)
    for r in good[::-1]:
        an.engine.submit(d["fens"][r], [], sims=SIMS, id=int(ids[r]))
    c = _run_all(an, False)
    an.close()
    assert sorted(a) == sorted(b) == sorted(c) == [int(ids[r]) for r in good]
    for r in good:
        i = int(ids[r])
        assert a[i] == b[i] == c[i], (r, d["fens"][r])                  # every field, floats included: bit for bit
    assert {a[int(ids[r])]["status"] for r in good} == {"ok", "checkmate", "stalemate"}
    assert any(fl & pc.EP_FROM_MASK for fl in d["flags"])


def test_reanalyse_rows_of_a_self_play_run():
    """64 rows of a short self-play run of a small network, searched again at 32 simulations: with the stand-in evaluator
    against the oracle search of the same rows (pi2 = visits / sum exactly), then on the network itself."""
    from matrix0_amd import analysis, encoding as enc, reanalyse
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    from oracle import net_ref
    net = dict(planes=19, channels=64, blocks=3, attention_heads=4, policy_size=4672, norm="group", activation="silu", preact=True,
               policy_factor_rank=32, self_supervised=True, ssl_tasks=["piece", "control"])
    be = M0Backend.from_state_dict(net, net_ref.random_state_dict(net, seed=11))
    cfg = _cfg(sims=32)
    sp = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(
        {"seed": 9, "mcts": cfg["mcts"], "selfplay": {"num_simulations": 16, "max_game_len": 20, "opening_random_plies": 4}},
        concurrent_games=4, total_games=4))
    recs = []
    for _ in range(400):
        if not sp.running():
            break
        sp.step(4)
    while True:
        r = sp.poll()
        if r is None:
            break
        recs.append(r)
    sp.close()
    recs.sort(key=lambda r: r["game_index"])
    s = np.concatenate([r["s"] for r in recs])[:64].copy()
    pi = np.concatenate([r["pi"] for r in recs])[:64].copy()
    z = np.concatenate([r["z"] for r in recs])[:64].copy()
    mask = np.concatenate([r["legal_mask"] for r in recs])[:64].copy()
    assert len(s) == 64
    corrupt = 21
    s[corrupt, 4, 3, 3] = 0.5
    ids = np.arange(300, 364)
    fens = enc.decode_planes(s, mask)["fens"]
    an = analysis.AnalyzerExt(FakeNet(seed=3, sharp=8.0).infer_np, cfg, slots=5)
    pi2, z2, rep = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=32, ids=ids, analyzer=an)
    an.close()
    assert rep["kept"] == {"decode:piece_value": 1} and rep["kept_ids"]["decode:piece_value"] == [300 + corrupt]
    assert rep["searched"] == 63 and rep["rows"] == 64 and rep["mask_mismatches"] == 0 and rep["mean_kl"] > 0
    assert np.array_equal(pi2[corrupt], pi[corrupt]) and fens[corrupt] == ""
    assert z2.tobytes() == z.tobytes()                                   # value_mix = 0
    for row in range(64):
        if row == corrupt:
            continue
        assert abs(float(pi2[row].sum(dtype=np.float64)) - 1.0) <= 1e-6, row
        assert not pi2[row][mask[row] == 0].any(), row
        o = _oracle_run(fens[row], [], int(ids[row]), False, 8.0, sims=32)
        _, idxs = ch.legal_moves_with_indices(ch.Board(fens[row]))
        want = np.zeros(4672, np.float32)
        counts = np.asarray(o["counts"], np.float64)
        want[idxs] = (counts / counts.sum()).astype(np.float32)
        assert np.array_equal(pi2[row], want), (row, fens[row])
    # the same rows on the network itself (the fused step): a blend of z and the root's q this time
    an = analysis.Analyzer(be, cfg, slots=16)
    pi3, z3, rep3 = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=32, ids=ids, analyzer=an, value_mix=0.5)
    st = an.stats()
    an.close()
    be.close()
    assert rep3["kept"] == {"decode:piece_value": 1} and rep3["searched"] == 63 and st["evals"] > 63
    ok = np.arange(64) != corrupt
    assert np.all(np.abs(pi3[ok].sum(axis=1, dtype=np.float64) - 1.0) <= 1e-6) and not pi3[mask == 0].any()
    assert np.array_equal(pi3[corrupt], pi[corrupt]) and z3[corrupt] == z[corrupt]
    assert np.all(np.abs(z3[ok] - 0.5 * z[ok]) <= 0.5 + 1e-6) and not np.array_equal(z3[ok], z[ok])
