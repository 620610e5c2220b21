"""PGN text, read and written: the one reader behind the opening book (pgn_book.py) and the game import (game_import.py), and
the writer of the match module (arena.py).  The reference reads with python-chess (chess.pgn.read_game) and writes in `_save_pgn`
(azchess/arena.py:281-303); here the text is split into games and mainline move tokens on the host, and what a token means on
the board is the caller's business (pgn_book resolves it against the legal moves' SAN, game_import on the GPU)."""
from __future__ import annotations

import bz2
import os
import re
from typing import Dict, Iterator, List, Optional, Tuple

from . import engine as eng

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
RESULTS = {"1-0", "0-1", "1/2-1/2", "*"}
_TAG = re.compile(r'^\s*\[(\w+)\s+"((?:[^"\\]|\\.)*)"\]\s*$')
_TOKEN = re.compile(r'\{[^}]*\}|\(|\)|\$\d+|\d+\.(?:\.\.)?|\.\.\.|[^\s(){}]+')
_MOVE_NUMBER = re.compile(r"^\d+\.(?:\.\.)?")


def read_text(path_or_text) -> str:
    """The text of a PGN file (.bz2 through the standard library), or the argument itself when it is PGN text."""
    if isinstance(path_or_text, os.PathLike) or ("\n" not in path_or_text and os.path.exists(path_or_text)):
        p = os.fspath(path_or_text)
        opener = bz2.open if p.endswith(".bz2") else open
        with opener(p, "rt", errors="replace") as f:
            return f.read()
    return path_or_text


def games(text: str) -> Iterator[Tuple[dict, str]]:
    """Yield (headers, movetext) per game: a tag section, then movetext up to the next tag section."""
    headers, moves = {}, []
    for line in text.splitlines():
        if line.startswith("%"):                       # PGN escape line
            continue
        m = _TAG.match(line)
        if m:
            if "".join(moves).strip():                 # a tag pair after movetext starts the next game
                yield headers, "\n".join(moves)
                headers, moves = {}, []
            headers[m.group(1)] = m.group(2)
            continue
        moves.append(line.split(";", 1)[0])            # ';' comments run to the end of the line
    if headers or "".join(moves).strip():
        yield headers, "\n".join(moves)


def mainline_tokens(movetext: str) -> List[str]:
    """The mainline's move tokens: comments, NAGs, variations, move numbers (also glued: "1.e4", "12...Nf6") and the result token
    removed.  Annotations and check marks stay on the tokens; whoever resolves them drops them."""
    out: List[str] = []
    depth = 0
    for tok in _TOKEN.findall(movetext):
        if tok[0] in "{$":
            continue
        if tok == "(":
            depth += 1
            continue
        if tok == ")":
            depth = max(0, depth - 1)
            continue
        if depth > 0:
            continue
        if tok in RESULTS:
            break
        if tok == "..." or not tok.strip("!?"):                  # a stand-alone annotation is a NAG
            continue
        tok = _MOVE_NUMBER.sub("", tok)
        if tok:
            out.append(tok)
    return out


def read_pgn(path_or_text) -> Iterator[Tuple[dict, List[str]]]:
    """(headers, tokens) per game of a PGN file or text.  The start position is headers["FEN"] when there is one, as
    python-chess's Game.board() takes it."""
    for headers, movetext in games(read_text(path_or_text)):
        yield headers, mainline_tokens(movetext)


def save_pgn(moves_raw, result: str, headers: Dict[str, str], out_dir: str, idx: int, start_fen: Optional[str] = None) -> str:
    """game_{idx:04d}.pgn with the seven-tag roster + caller headers and SAN movetext (lines wrapped at 80 columns).  A game
    from an opening-book position (`start_fen`) also carries [SetUp "1"] and [FEN "..."], and its move numbers follow the FEN."""
    os.makedirs(out_dir, exist_ok=True)
    tags = {"Event": "?", "Site": "?", "Date": "????.??.??", "Round": "?", "White": "?", "Black": "?", "Result": result}
    tags.update({k: str(v) for k, v in headers.items()})
    tags["Result"] = result
    if start_fen:
        tags["SetUp"], tags["FEN"] = "1", start_fen
    words = (eng.san_game(moves_raw, start_fen).split() if len(moves_raw) else []) + [result]
    lines, cur = [], ""
    for w in words:
        if cur and len(cur) + 1 + len(w) > 80:
            lines.append(cur)
            cur = w
        else:
            cur = w if not cur else cur + " " + w
    if cur:
        lines.append(cur)
    path = os.path.join(out_dir, f"game_{idx:04d}.pgn")
    with open(path, "w") as f:
        for k, v in tags.items():
            f.write(f'[{k} "{v}"]\n')
        f.write("\n" + "\n".join(lines) + "\n")
    return path
