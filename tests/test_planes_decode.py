"""Planes -> position on the CPU: csrc/planes_decode.h built for the host (tests/host_shim/planes_shim.cpp), the function that
decode_planes_kernel runs one wave per row.  All 10 016 rows of tests/golden/ref_encoding.npz (outputs of the reference's own
encode_board / move_to_index) decode to positions with the golden legal moves, indices, planes and FEN fields; hand-written
en-passant positions with and without their mask; one malformed row per status; and the same code under
-fsanitize=address,undefined as a stand-alone program over malformed rows."""
import os
import subprocess

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import planes_cases as pc
from tests.golden_ref import load_npz

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    z = load_npz("ref_encoding.npz")
    g = {k: z[k] for k in z.files}
    g["fens"] = [str(f) for f in g["fens"]]
    n = len(g["fens"])
    g["off"] = np.concatenate([[0], np.cumsum(g["nlegal"].astype(np.int64))])
    planes = np.zeros((n, 19, 8, 8), np.float32)
    planes[:, :17] = np.unpackbits(g["plane_bits"], axis=2).reshape(n, 17, 8, 8)
    planes[:, 17] = g["counters"][:, 0, None, None]
    planes[:, 18] = g["counters"][:, 1, None, None]
    mask = np.zeros((n, 4672), np.uint8)
    mask[np.repeat(np.arange(n), g["nlegal"].astype(np.int64)), g["idx"].astype(np.int64)] = 1
    g["planes"], g["mask"] = planes, mask
    # the file's promotion codes are python-chess piece types (N = 2 .. Q = 5), the engine's 1 .. 4
    g["moves_raw"] = np.where(g["moves"] >> 12, g["moves"] - (1 << 12), g["moves"]).astype(np.uint16)
    g["decoded"] = pc.host_decode(planes, mask)
    return g


def test_every_golden_row_decodes_to_the_golden_position(gold):
    fens, d = gold["fens"], gold["decoded"]
    n = len(fens)
    assert n == 10016
    assert not d["status"].any(), (int(np.flatnonzero(d["status"])[0]), fens[int(np.flatnonzero(d["status"])[0])])
    assert np.array_equal(d["nlegal"], gold["nlegal"].astype(np.int32))
    # the decoded position's planes, bit for bit
    assert np.array_equal(d["planes"].view(np.uint32), gold["planes"].view(np.uint32))
    n_ep = n_half = n_full = n_castle = 0
    for i in range(n):
        lo, hi = gold["off"][i], gold["off"][i + 1]
        k = hi - lo
        assert np.array_equal(d["moves"][i, :k], gold["moves_raw"][lo:hi]), fens[i]     # the legal list, in order
        assert np.array_equal(d["idx"][i, :k], gold["idx"][lo:hi].astype(np.int32)), fens[i]
        want, got = fens[i].split(), d["fens"][i].split()
        assert got[:4] == want[:4], (fens[i], d["fens"][i])           # placement, side, castling, en passant
        half, full = int(want[4]), int(want[5])
        assert got[4] == str(min(half, 99)) and got[5] == str(min(full, 199)), (fens[i], d["fens"][i])
        fl = int(d["flags"][i])
        assert bool(fl & pc.HALFMOVE_SATURATED) == (half >= 99) and bool(fl & pc.FULLMOVE_SATURATED) == (full >= 199), fens[i]
        assert bool(fl & pc.EP_FROM_MASK) == (want[3] != "-") and not fl & pc.NO_MASK, fens[i]
        if want[3] != "-":
            n_ep += 1
            b = ch.Board(fens[i])
            assert any(pc.is_en_passant(b, m) for m in b.legal_moves), fens[i]
        n_half += half >= 99
        n_full += full >= 199
        n_castle += want[2] != "-"
    # what the file holds of the rarer things (hence the hand-written positions below)
    assert (n_ep, n_half, n_full, n_castle) == (3, 1, 1, 1286)


def test_golden_rows_without_a_mask(gold):
    """No mask: the same positions but for en passant, which is unknown and set to none."""
    sel = np.arange(0, len(gold["fens"]), 5)
    ep_rows = [i for i, f in enumerate(gold["fens"]) if f.split()[3] != "-"]
    sel = np.unique(np.concatenate([sel, ep_rows]))
    d = pc.host_decode(gold["planes"][sel])
    assert not d["status"].any() and np.all(d["flags"] & pc.NO_MASK) and not np.any(d["flags"] & pc.EP_FROM_MASK)
    for j, i in enumerate(sel):
        want, got = gold["fens"][i].split(), d["fens"][j].split()
        assert got[:3] == want[:3] and got[3] == "-", gold["fens"][i]
        b = ch.Board(gold["fens"][i])
        assert d["nlegal"][j] == sum(1 for m in b.legal_moves if not pc.is_en_passant(b, m)), gold["fens"][i]


@pytest.mark.parametrize("fen,ep", pc.EP_FENS)
def test_en_passant_comes_from_the_mask(fen, ep):
    b = ch.Board(fen)
    planes, mask = pc.encode(fen)
    moves, idxs = ch.legal_moves_with_indices(b)
    n_ep = sum(1 for m in moves if pc.is_en_passant(b, m))
    assert (n_ep > 0) == (ep is not None), "the case is not what its comment says"
    d = pc.host_decode(planes[None], mask[None])
    assert d["status"][0] == pc.OK and d["nlegal"][0] == len(moves)
    assert d["fens"][0] == b.fen(), (d["fens"][0], b.fen())            # ep field only when the capture is legal
    assert d["fens"][0].split()[3] == (ep or "-")
    assert int(d["flags"][0]) == (pc.EP_FROM_MASK if ep else 0)
    assert d["idx"][0, : len(moves)].tolist() == idxs
    assert np.array_equal(d["planes"][0], planes)
    # without the mask: ep none, documented, not detected
    d = pc.host_decode(planes[None])
    assert d["status"][0] == pc.OK and int(d["flags"][0]) == pc.NO_MASK
    assert d["fens"][0].split()[3] == "-" and d["fens"][0].split()[:3] == fen.split()[:3]
    assert d["nlegal"][0] == len(moves) - n_ep
    assert np.array_equal(d["planes"][0], planes)


def test_every_status_has_its_row():
    rows = pc.malformed_rows()
    assert {want for _, want, _, _ in rows} == set(range(1, 12))
    planes, mask = np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows])
    d = pc.host_decode(planes, mask)
    for (name, want, _, _), st, nl, fen in zip(rows, d["status"], d["nlegal"], d["fens"]):
        assert st == want, (name, int(st))
        if want == pc.MASK_MISMATCH:                                   # the position and nlegal are still written
            assert fen == ch.START_FEN and nl == 20, name
        else:
            assert fen == "" and nl == 0, name
    # without masks: the same verdicts, except that nothing is there to mismatch
    d = pc.host_decode(planes)
    for (name, want, _, _), st in zip(rows, d["status"]):
        assert st == (pc.OK if want == pc.MASK_MISMATCH else want), (name, int(st))


def test_saturated_counters_decode_with_their_flag():
    for half, full, want in ((98, 198, 0), (99, 12, pc.HALFMOVE_SATURATED), (140, 199, pc.HALFMOVE_SATURATED | pc.FULLMOVE_SATURATED),
                             (3, 250, pc.FULLMOVE_SATURATED)):
        fen = f"4k3/8/8/8/8/8/4P3/4K3 w - - {half} {full}"
        planes, mask = pc.encode(fen)
        d = pc.host_decode(planes[None], mask[None])
        assert d["status"][0] == pc.OK and int(d["flags"][0]) == want, fen
        assert d["fens"][0].split()[4:] == [str(min(half, 99)), str(min(full, 199))], fen


def test_sanitizer_build_over_malformed_rows():
    """The decode as a stand-alone host program (its own main, never loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer over 20 000 malformed and well-formed rows with exactly-sized buffers."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_shim"), "../_build/planes_fuzz_san"])
    out = subprocess.run([os.path.join(HERE, "_build", "planes_fuzz_san")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    hist = dict(line.replace("status ", "").split(": ") for line in out.stdout.strip().split("\n"))
    assert sum(int(v) for v in hist.values()) == 20000 and int(hist["0"]) > 0 and int(hist["11"]) > 0, hist
