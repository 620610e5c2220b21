#!/usr/bin/env python3
"""Positions per second of reading games back in, on one GPU: the device replay (matrix0_amd/game_import.py) against the host path
the package had before it, over the same games of one PGN file and in one process.

    python tools/bench_import.py PGN [GAMES] [--repeat 1] [--runs 3] [--device 0] [--shard-size 8192] [--out profiles/game_import.log]

--repeat takes the file's games that many times over (a small file at a size worth timing); --runs repeats the two timed device
calls and reports every run, so that the spread is on record.

host path    what pgn_book.mainline_fens does per ply, without its 20-ply cap: pgn_book.resolve_san (the SAN list of the position,
             m0_san_legal_fen, and a string match), m0_fen_after; then one encoding.encode_fens call over all positions (planes and masks).
device path  tokens -> patterns on the host, m0_replay_games (replay kernel, position encoder, copy back), then the shards.

For the device path the wall time is split: parse (PGN text -> headers and tokens, inside import_pgn), patterns (tokens -> 32-bit patterns), replay (the call
with only the per-ply scalars asked for: replay kernel and a small copy), planes + masks (the same call with planes and masks,
minus the replay: encoder kernel and the 9.5 KB per position coming back), shards (one-hot pi, np.savez_compressed).  No test
reads these numbers.  Appends to profiles/game_import.log.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_path(games, device):
    """[(headers, tokens)] -> positions resolved, seconds resolving, seconds encoding."""
    from matrix0_amd import encoding as enc
    from matrix0_amd import engine as eng
    from matrix0_amd.pgn import START_FEN
    from matrix0_amd.pgn_book import resolve_san
    t0 = time.perf_counter()
    fens = []
    for headers, tokens in games:
        fen = headers.get("FEN") or START_FEN
        for tok in tokens:
            hit = resolve_san(fen, tok)
            if hit is None:
                break
            fens.append(fen)
            fen = eng.fen_after(fen, [hit])
    t1 = time.perf_counter()
    for i in range(0, len(fens), 16384):
        enc.encode_fens(fens[i: i + 16384], device_index=device, want_moves=False)
    return len(fens), t1 - t0, time.perf_counter() - t1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pgn")
    ap.add_argument("games", nargs="?", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shard-size", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "game_import.log"))
    a = ap.parse_args()
    from matrix0_amd import game_import as gi
    from matrix0_amd import pgn

    games = []
    for headers, tokens in pgn.read_pgn(a.pgn):
        if tokens:
            games.append((headers, tokens))
        if len(games) >= a.games:
            break
    games = games * max(1, a.repeat)
    text_games = [(h.get("FEN") or None, toks) for h, toks in games]

    gi.replay_games(text_games[:1])                                     # library load, device context
    t0 = time.perf_counter()
    for _, toks in text_games:
        for t in toks:
            gi.move_pattern(t)
    t_pat = time.perf_counter() - t0                                    # fills the cache the calls below hit
    replay_runs, full_runs = [], []
    for _ in range(max(1, a.runs)):                                     # the calls end in blocking copies: host clock is enough
        t0 = time.perf_counter()
        res = gi.replay_games(text_games, planes=False, mask=False, device_index=a.device)
        replay_runs.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        gi.replay_games(text_games, device_index=a.device)
        full_runs.append(time.perf_counter() - t0)
    t_replay, t_full = min(replay_runs), min(full_runs)
    positions = sum(r["plies"] for r in res)

    timings = {}
    with tempfile.TemporaryDirectory() as tmp:
        pgn_games = "\n".join(f'[Result "{h.get("Result", "*")}"]\n' + (f'[FEN "{h["FEN"]}"]\n' if h.get("FEN") else "") + "\n" +
                              " ".join(toks) + " " + h.get("Result", "*") + "\n" for h, toks in games)
        t0 = time.perf_counter()
        summary = gi.import_pgn(pgn_games, tmp, shard_size=a.shard_size, device_index=a.device, timings=timings)
        t_import = time.perf_counter() - t0
        shard_bytes = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))

    n_host, t_resolve, t_encode = host_path(games, a.device)
    line = {
        "pgn": os.path.basename(a.pgn), "games": len(games), "repeat": a.repeat,
        "replay_runs_s": replay_runs, "replay_and_encode_runs_s": full_runs, "positions": positions, "host_positions": n_host,
        "device_path": {"positions_per_s_replay_and_encode": positions / max(t_pat + t_full, 1e-9),
                        "positions_per_s_import_pgn": summary["samples"] / max(t_import, 1e-9),
                        "split_s": {"parse": timings.get("parse", 0.0), "patterns": t_pat, "replay": t_replay,
                                    "planes_and_masks": max(t_full - t_replay, 0.0), "shards": timings.get("compress", 0.0)},
                        "import_pgn_s": t_import, "shard_bytes": shard_bytes, "summary": summary},
        "host_path": {"positions_per_s": n_host / max(t_resolve + t_encode, 1e-9), "resolve_s": t_resolve, "encode_fens_s": t_encode},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
