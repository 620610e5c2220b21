"""The tablebases inside the search, the part that needs no GPU: m0_tb_root_lines (the analysis of a root inside the tables)
against a Python walk over the independent generator's tables with the oracle's rules (tests/tb_search_util.py), and the
configuration key."""
import ctypes as C

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import tb_search_util as su
from tests import tb_util as tu
from matrix0_amd import _lib, engine as eng, tablebase as tbm

MULTIPV, PV_LEN = 8, 16
REF = tu.ref_tables()


@pytest.fixture(scope="module")
def tb(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tbs") / "three.m0tb")
    ref = tu.ref_tables()
    tu.write_cache_file(path, {s: ref[s] for s in tu.THREE_MAN})
    t = tbm.Tablebase.load(path)
    yield t
    t.close()


def lib_root_lines(tb, fen, r):
    """m0_tb_root_lines into the caller's struct -> None (no hit) or the dict tests/tb_search_util.py::py_root_lines makes."""
    rc = tb._L.m0_tb_root_lines(tb.handle, fen.encode(), MULTIPV, PV_LEN, C.byref(r))
    assert rc in (0, 1), (fen, rc, _lib.last_error())
    if rc == 0:
        return None
    assert (r.status, r.evals, r.root_n, r.sims, r.nlines) == (3, 0, 0, 0, min(MULTIPV, r.nlegal)), fen
    lines = []
    for i in range(r.nlines):
        ln = r.lines[i]
        assert ln.visits == 0 and ln.prior == 0.0 and ln.pv[0] == ln.move, fen
        lines.append({"move": eng.move_to_uci(ln.move), "q": ln.q, "dtm": r.line_dtm[i],
                      "pv": [eng.move_to_uci(ln.pv[k]) for k in range(ln.pv_len)], "policy_index": ln.policy_index})
    return {"root_q": r.root_q, "dtm": r.tb_dtm, "nlegal": r.nlegal, "lines": lines}


def check_entry(tb, fen, r, best_reply, counts, with_index=True):
    want = su.py_root_lines(fen, REF, MULTIPV, PV_LEN, best_reply=best_reply)
    assert want is not None, fen
    if want["nlegal"] == 0:
        return False                                   # checkmate / stalemate: no lines to compare
    got = lib_root_lines(tb, fen, r)
    assert got is not None, fen
    board = ch.Board(fen) if with_index else None
    for ln in got["lines"]:                            # policy_index as usual; not part of the Python statement
        idx = ln.pop("policy_index")
        assert not with_index or idx == ch.move_to_index(board, ch.Move.from_uci(ln["move"])), (fen, ln)
    assert got == want, (fen, got, want)
    # along a decided PV the dtm falls by exactly one per ply, and the line ends in checkmate when it fits
    for ln in got["lines"]:
        if ln["q"] == 0.0:
            assert ln["pv"] == [ln["move"]] and ln["dtm"] == 0, (fen, ln)
            continue
        b, d = ch.Board(fen), ln["dtm"]
        for k, u in enumerate(ln["pv"]):
            b.push(ch.Move.from_uci(u))
            hit = su.py_probe(b, REF)
            assert hit is not None and hit[1] == d - k, (fen, ln, k)
        if d + 1 <= PV_LEN:
            assert len(ln["pv"]) == d + 1 and b.is_checkmate(), (fen, ln)
            counts["mates"] += 1
        else:
            assert len(ln["pv"]) == PV_LEN, (fen, ln)
    return True


@pytest.mark.parametrize("sig", ["KK", "KBK", "KNK"])
def test_root_lines_of_every_entry_of_the_drawn_tables(tb, sig):
    table = tu.ref_tables()[sig]
    r, n, counts = eng.AnalysisResult(), 0, {"mates": 0}
    for idx in np.nonzero(table != 255)[0].tolist():
        n += check_entry(tb, tu.index_to_fen(sig, idx), r, None, counts, with_index=idx % 61 == 0)   # policy_index: a sample
    print(f"{sig}: {n} entries with a legal move compared")
    assert n > 3000 and counts["mates"] == 0


@pytest.mark.parametrize("sig", ["KQK", "KRK", "KPK"])
def test_root_lines_of_sampled_entries_and_their_colour_flips(tb, sig):
    table = tu.ref_tables()[sig]
    valid = np.nonzero(table != 255)[0]
    rng = np.random.default_rng(20 + len(sig) + ord(sig[1]))
    r, n, best_reply, counts = eng.AnalysisResult(), 0, {}, {"mates": 0}
    for idx in rng.permutation(valid):
        fen = tu.index_to_fen(sig, int(idx))
        n += check_entry(tb, tu.flip_fen(fen) if n % 2 else fen, r, best_reply, counts)
        if n == 2000:
            break
    print(f"{sig}: {n} entries compared, {counts['mates']} lines end in checkmate")
    assert n == 2000 and counts["mates"] > 0


def test_no_hit_leaves_the_result_untouched(tb):
    r = eng.AnalysisResult()
    for fen in ("4k3/8/8/8/8/8/8/R3K3 w Q - 0 1",          # a castling right left
                "4k3/4p3/8/8/8/8/4P3/4K3 w - - 0 1",        # KPKP: not in scope
                "4k3/8/8/8/8/8/PPP5/4K3 w - - 0 1"):        # five men
        C.memset(C.byref(r), 0xAB, C.sizeof(r))
        assert tb._L.m0_tb_root_lines(tb.handle, fen.encode(), MULTIPV, PV_LEN, C.byref(r)) == 0, fen
        assert bytes(r) == b"\xab" * C.sizeof(r), fen
        assert tb.root_lines(fen, MULTIPV, PV_LEN) is None
    assert tb._L.m0_tb_root_lines(tb.handle, b"not a fen", MULTIPV, PV_LEN, C.byref(r)) == -1       # M0_ERR_INVALID
    for multipv, pv_len in ((0, 8), (9, 8), (1, 0), (1, 17)):
        assert tb._L.m0_tb_root_lines(tb.handle, b"8/8/8/4k3/8/8/4K3/R7 w - - 0 1", multipv, pv_len, C.byref(r)) == -1
    # the same rook ending without the right is a hit; Tablebase.root_lines is the dict an Analyzer returns for it
    d = tb.root_lines("4k3/8/8/8/8/8/8/R3K3 w - - 0 1", 2, 4)
    assert d["status"] == "tablebase" and d["root_q"] == 1.0 and d["dtm"] % 2 == 1 and d["evals"] == 0 and len(d["lines"]) == 2
    assert d["lines"][0]["dtm"] == d["dtm"] - 1 and d["lines"][0]["q"] == 1.0 and len(d["lines"][0]["pv"]) == 4


def test_in_search_configuration_key():
    base = {"max_pieces": 3, "cache": None}
    assert tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3}}}) == base          # existing configs: as before
    assert tbm.in_search({"engine": {"tablebase": {"max_pieces": 3}}}) is False and tbm.in_search({}) is False
    assert tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3, "in_search": True}}}) == dict(base, in_search=True)
    assert tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3, "in_search": False}}}) == dict(base, in_search=False)
    assert tbm.in_search({"engine": {"tablebase": {"max_pieces": 4, "in_search": True}}}) is True
    for bad in (1, 0, "true", None):
        with pytest.raises(ValueError, match="in_search"):
            tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3, "in_search": bad}}})
    with pytest.raises(ValueError, match="unknown"):
        tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3, "in_search": True, "on_gpu": True}}})
