"""Games read back in: PGN files and move lists become training samples on the GPU.

The reference converts outside games with python-chess, one board at a time (azchess/tools/process_lichess.py:59-106:
`process_game` walks `game.mainline_moves()` and stores encode_board / a one-hot move_to_index / the header's result per ply), and
writes no legal masks, which its backfill_legal_masks.py adds later.  Here the host only tokenises: every written move becomes a
32-bit pattern (m0_san_pattern / m0_move_pattern, csrc/san_match.h) and m0_replay_games walks whole games on the device, one
wave per game, with the search's own move generator; planes, masks and SSL maps come from the kernels behind encoding.encode_fens
and engine.ssl_targets_fens.  There is no CPU implementation.

    replay_games(games)       [(start_fen or None, tokens)] -> per-game arrays
    read_pgn(path_or_text)    -> (headers, tokens) per game (pgn.py)
    import_pgn(path, out_dir) -> <prefix>_<index>.npz shards with s / pi / z (/ legal_mask / ssl_<task>) and a summary
    python -m matrix0_amd.game_import PGN OUT_DIR [--lichess ...]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._abi import MOVE_RAW, MOVE_UCI, REPLAY_END_BITS as END_BITS, REPLAY_STATUS as STATUS
from ._lib import ptr
from .data_writer import RowBuffer, write_npz
from .pgn import mainline_tokens, read_pgn  # noqa: F401  (the readers live in pgn.py; callers know them under this module too)

SSL_KEYS = _lib.SSL_ORDER
_RESULT_Z = {"1-0": 1.0, "0-1": -1.0, "1/2-1/2": 0.0}

_pattern_cache: Dict[Tuple[str, object], int] = {}


def move_pattern(token, notation: str = "san") -> int:
    """The 32-bit pattern of one written move (csrc/san_match.h), 0 for a token that is no move (it ends its game as
    "illegal", where python-chess ends the line).  A str is read as `notation` ("san" or "uci"); an integer is a raw move
    from | to<<6 | promo<<12, as in an engine record's `played_raw`."""
    raw = not isinstance(token, str)
    key = ("raw" if raw else notation, int(token) if raw else token)
    hit = _pattern_cache.get(key)
    if hit is not None:
        return hit
    L = _lib.lib()
    out = C.c_uint32(0)
    if raw:
        v = int(token)
        rc = L.m0_move_pattern(MOVE_RAW, None, v, C.byref(out)) if 0 <= v < 2 ** 32 else _lib.M0_ERR_INVALID
    elif notation == "san":
        rc = L.m0_san_pattern(token.encode("utf-8", "replace"), C.byref(out))
    elif notation == "uci":
        rc = L.m0_move_pattern(MOVE_UCI, token.encode("utf-8", "replace"), 0, C.byref(out))
    else:
        raise ValueError(f"notation must be 'san' or 'uci', not {notation!r}")
    pat = int(out.value) if rc == _lib.M0_OK else 0
    if len(_pattern_cache) < 1 << 20:
        _pattern_cache[key] = pat
    return pat


def end_flags_to_dict(flags: int) -> dict:
    return {k: bool(flags & b) for k, b in END_BITS.items()}


def replay_games(games: Sequence[Tuple[Optional[str], Sequence]], *, notation: str = "san", ssl: bool = False,
                 planes: bool = True, mask: bool = True, device_index: int = 0, max_plies: int = 1024,
                 max_positions_per_launch: int = 16384) -> List[dict]:
    """Replay `games` = [(start_fen or None, tokens)] on the device.  Tokens are SAN strings (or UCI strings with
    notation="uci") or raw integer moves; the kinds may differ from game to game but `notation` holds for every str.

    One dict per game, every array with len(tokens) rows of which the first `plies` are filled and the others zero (a game stops
    at its first token that does not resolve to exactly one legal move, or at max_plies).  Row k describes the position BEFORE
    move k: `moves` u16 (raw), `policy_idx` i32, `nlegal` i32, `turn` i8 (1 White), `planes` f32 [.,19,8,8], `mask` u8 [.,4672],
    `ssl` f32 [.,17,8,8] (piece 13, threat, pin, fork, control) when asked for.  `status` is "ok", "illegal", "ambiguous" or
    "too_long"; `end` holds checkmate / stalemate / insufficient / white_to_move of the position after the last resolved move.
    ValueError for a bad start FEN (the message names the game); RuntimeError without a HIP device."""
    L = _lib.lib()
    n = len(games)
    if n == 0:
        return []
    counts = [len(t) for _, t in games]
    offsets = np.zeros(n + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[n])
    pats = np.fromiter((move_pattern(t, notation) for _, toks in games for t in toks), np.uint32, total)
    fens = _lib.cstrings(f or None for f, _ in games)
    rows = max(total, 1)
    out = {
        "plies": np.zeros(n, np.int32), "status": np.zeros(n, np.int32), "end": np.zeros(n, np.int32),
        "moves": np.zeros(rows, np.uint16), "policy_idx": np.zeros(rows, np.int32), "nlegal": np.zeros(rows, np.int32),
        "turn": np.zeros(rows, np.int8),
        "planes": np.zeros((rows, 19, 8, 8), np.float32) if planes else None,
        "mask": np.zeros((rows, 4672), np.uint8) if mask else None,
        "ssl": np.zeros((rows, 17, 8, 8), np.float32) if ssl else None,
    }
    _lib.check(L.m0_replay_games(int(device_index), fens, ptr(pats if total else np.zeros(1, np.uint32)), ptr(offsets), n,
                                 int(max_plies), int(max_positions_per_launch or 0), ptr(out["plies"]), ptr(out["status"]),
                                 ptr(out["end"]), ptr(out["moves"]), ptr(out["policy_idx"]), ptr(out["nlegal"]),
                                 ptr(out["turn"]), ptr(out["planes"]), ptr(out["mask"]), ptr(out["ssl"])), "m0_replay_games")
    res = []
    for g in range(n):
        a, b = int(offsets[g]), int(offsets[g + 1])
        d = {"status": STATUS[int(out["status"][g])], "plies": int(out["plies"][g]), "end": end_flags_to_dict(int(out["end"][g]))}
        for k in ("moves", "policy_idx", "nlegal", "turn", "planes", "mask", "ssl"):
            if out[k] is not None:
                d[k] = out[k][a:b]
        res.append(d)
    return res


# ---- PGN -> shards ----

def _elo(headers: dict, key: str) -> Optional[int]:
    try:
        return int(headers.get(key, 0))
    except ValueError:
        return None


def _passes(headers: dict, min_elo: int, require_normal_termination: bool, skip_sites: Sequence[str], known_result: bool) -> bool:
    """The header filters of process_game (process_lichess.py:63-86)."""
    if require_normal_termination and headers.get("Termination") != "Normal":
        return False
    if any(s in headers.get("Site", "") for s in skip_sites):
        return False
    we, be = _elo(headers, "WhiteElo"), _elo(headers, "BlackElo")
    if we is None or be is None or we < min_elo or be < min_elo:       # a non-integer Elo drops the game, as int() raising does
        return False
    if known_result and headers.get("Result", "*") not in _RESULT_Z:
        return False
    return True


class _ShardWriter:
    """Collects sample arrays (data_writer.RowBuffer) and writes <prefix>_<index:06d>.npz with exactly shard_size samples each
    (the tail is shorter) through data_writer.write_npz; no row in the shard index."""

    def __init__(self, out_dir: str, prefix: str, shard_size: int, packed: bool = False, device_index: int = 0):
        self.out_dir, self.prefix, self.shard_size = out_dir, prefix, int(shard_size)
        self.packed, self.device_index = bool(packed), int(device_index)
        self.buf = RowBuffer()
        self.shards = 0
        self.seconds = 0.0
        os.makedirs(out_dir, exist_ok=True)

    def add(self, part: Dict[str, np.ndarray]) -> None:
        self.buf.add(part)
        while self.buf.rows >= self.shard_size:
            self._write(self.shard_size)

    def finish(self) -> None:
        if self.buf.rows:
            self._write(self.buf.rows)

    def _write(self, n: int) -> None:
        t0 = time.perf_counter()
        arrays = self.buf.take(n)
        if self.packed:                                     # (rowpack.py) the one-hot pi is never built
            from . import rowpack
            rows = rowpack.pack_rows_onehot(arrays.pop("s"), arrays.pop("_pi_idx"), arrays.pop("z"), arrays.pop("legal_mask", None),
                                            device=self.device_index)
            arrays = rowpack.packed_to_dict(rows, arrays)
        else:
            pi = np.zeros((n, 4672), np.float32)
            pi[np.arange(n), arrays.pop("_pi_idx")] = 1.0
            arrays["pi"] = pi
        write_npz(os.path.join(self.out_dir, f"{self.prefix}_{self.shards:06d}.npz"), arrays)
        self.shards += 1
        self.seconds += time.perf_counter() - t0


def import_pgn(path, out_dir: str, *, min_elo: int = 0, require_normal_termination: bool = False, skip_sites: Sequence[str] = (),
               max_games: Optional[int] = None, shard_size: int = 8192, legal_mask: bool = True, ssl_tasks: Sequence[str] = (),
               result_source: str = "header", on_error: str = "truncate", prefix: str = "import", lichess: bool = False,
               device_index: int = 0, max_plies: int = 1024, max_positions_per_launch: int = 16384,
               games_per_call: int = 1024, timings: Optional[dict] = None, packed: bool = False) -> dict:
    """PGN file (or text) -> NPZ shards of training samples, as the reference's process_game makes them: per ply `s` = the
    position before the move, `pi` one-hot at the move's index, `z` = the game's result from the side to move's point of view
    (what the engine's own records hold), plus `legal_mask` and `ssl_<task>` (the worker's channel split: piece [N,13,8,8], the
    others [N,8,8]) when asked for.

    lichess=True sets the reference tool's filters: Termination "Normal", no "FICSGames" site, both Elo values >= 2000 (or
    min_elo when that is higher) and a known result.  A game without a usable result is filtered in any case.
    on_error: "truncate" keeps the plies before the first token that does not resolve (python-chess ends the line there),
    "drop" leaves such a game out.  result_source: "header" trusts the Result tag as the reference does; "board" takes the result
    from the final position when it is checkmate or stalemate and the header otherwise.  max_games caps the games kept.
    packed=True writes packed shards (rowpack.py: bitboards and the one move per row; rowpack.load_shard and the readers of this
    package give the same dense arrays back, `python -m matrix0_amd.rowpack unpack` dense files for the reference's reader).
    Returns the summary: games_read, games_kept, games_filtered, games_truncated, games_dropped, samples, shards,
    result_mismatches (kept games whose final position is checkmate while the header names another result; "*" names none)."""
    if result_source not in ("header", "board"):
        raise ValueError("result_source must be 'header' or 'board'")
    if on_error not in ("truncate", "drop"):
        raise ValueError("on_error must be 'truncate' or 'drop'")
    if int(shard_size) <= 0:
        raise ValueError("shard_size must be positive")
    ssl_tasks = list(ssl_tasks)
    for t in ssl_tasks:
        if t not in SSL_KEYS:
            raise ValueError(f"unknown ssl task {t!r}")
    known_result = False
    if lichess:
        require_normal_termination, known_result = True, True
        skip_sites = tuple(skip_sites) + ("FICSGames",)
        min_elo = max(int(min_elo), 2000)
    summary = {"games_read": 0, "games_kept": 0, "games_filtered": 0, "games_truncated": 0, "games_dropped": 0, "samples": 0,
               "shards": 0, "result_mismatches": 0}
    tm = {"parse": 0.0, "device": 0.0, "compress": 0.0}
    writer = _ShardWriter(out_dir, prefix, shard_size, packed=packed, device_index=device_index)

    def flush(batch: List[Tuple[dict, List[str]]]) -> None:
        t0 = time.perf_counter()
        res = replay_games([(h.get("FEN") or None, toks) for h, toks in batch], ssl=bool(ssl_tasks), mask=bool(legal_mask),
                           device_index=device_index, max_plies=max_plies, max_positions_per_launch=max_positions_per_launch)
        tm["device"] += time.perf_counter() - t0
        for (headers, _), r in zip(batch, res):
            n, end = int(r["plies"]), r["end"]
            header = headers.get("Result", "*")
            board = None
            if end["checkmate"]:
                board = "0-1" if end["white_to_move"] else "1-0"
            elif end["stalemate"]:
                board = "1/2-1/2"
            result = board if (result_source == "board" and board is not None) else header
            if result not in _RESULT_Z:
                summary["games_filtered"] += 1
                continue
            if r["status"] != "ok" and (on_error == "drop" or n == 0):
                summary["games_dropped"] += 1
                continue
            if r["status"] != "ok":
                summary["games_truncated"] += 1
            if end["checkmate"] and header in _RESULT_Z and header != board:      # "*" claims nothing
                summary["result_mismatches"] += 1
            turn = r["turn"][:n].astype(np.float32)
            part = {"s": r["planes"][:n], "_pi_idx": r["policy_idx"][:n].astype(np.int64),
                    "z": (np.float32(_RESULT_Z[result]) * (2.0 * turn - 1.0)).astype(np.float32)}
            if legal_mask:
                part["legal_mask"] = r["mask"][:n]
            if ssl_tasks:
                maps = _lib.split_ssl(r["ssl"][:n])
                part.update({f"ssl_{t}": maps[t] for t in ssl_tasks})
            summary["games_kept"] += 1
            summary["samples"] += n
            writer.add(part)

    batch: List[Tuple[dict, List[str]]] = []
    t0 = time.perf_counter()
    for headers, tokens in read_pgn(path):
        if max_games is not None and summary["games_kept"] + len(batch) >= max_games:    # the batch may fill the cap: settle it
            tm["parse"] += time.perf_counter() - t0
            flush(batch)
            batch = []
            t0 = time.perf_counter()
            if summary["games_kept"] >= max_games:
                break
        summary["games_read"] += 1
        if not tokens or not _passes(headers, int(min_elo), require_normal_termination, skip_sites, known_result):
            summary["games_filtered"] += 1
            continue
        batch.append((headers, tokens))
        if len(batch) >= games_per_call:
            tm["parse"] += time.perf_counter() - t0
            flush(batch)
            batch = []
            t0 = time.perf_counter()
    tm["parse"] += time.perf_counter() - t0
    if batch:
        flush(batch)
    writer.finish()
    summary["shards"] = writer.shards
    tm["compress"] = writer.seconds
    if timings is not None:
        timings.update(tm)
    return summary


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.game_import",
                                 description="PGN (.pgn or .pgn.bz2) -> NPZ shards of training samples, replayed on the GPU")
    ap.add_argument("pgn")
    ap.add_argument("out_dir")
    ap.add_argument("--min-elo", type=int, default=0)
    ap.add_argument("--require-normal-termination", action="store_true")
    ap.add_argument("--skip-site", action="append", default=[], dest="skip_sites", help="drop games whose Site contains this (repeatable)")
    ap.add_argument("--max-games", type=int, default=None)
    ap.add_argument("--shard-size", type=int, default=8192)
    ap.add_argument("--no-legal-mask", action="store_false", dest="legal_mask")
    ap.add_argument("--ssl-task", action="append", default=[], dest="ssl_tasks", choices=SSL_KEYS)
    ap.add_argument("--result-source", choices=["header", "board"], default="header")
    ap.add_argument("--on-error", choices=["truncate", "drop"], default="truncate")
    ap.add_argument("--prefix", default="import")
    ap.add_argument("--lichess", action="store_true", help="the reference tool's filters: normal termination, no FICSGames, Elo >= 2000, known result")
    ap.add_argument("--device-index", type=int, default=0)
    ap.add_argument("--max-plies", type=int, default=1024)
    ap.add_argument("--max-positions-per-launch", type=int, default=16384)
    a = ap.parse_args(argv)
    summary = import_pgn(a.pgn, a.out_dir, min_elo=a.min_elo, require_normal_termination=a.require_normal_termination,
                         skip_sites=tuple(a.skip_sites), max_games=a.max_games, shard_size=a.shard_size, legal_mask=a.legal_mask,
                         ssl_tasks=tuple(a.ssl_tasks), result_source=a.result_source, on_error=a.on_error, prefix=a.prefix,
                         lichess=a.lichess, device_index=a.device_index, max_plies=a.max_plies,
                         max_positions_per_launch=a.max_positions_per_launch)
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
