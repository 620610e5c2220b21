"""Batched position analysis on one MI355X: a list of arbitrary positions in, the best moves, the lines behind them and the
evaluation out -- what the reference answers one board at a time with `MCTS.run(board)` (its web UI, cli_play.py, its
benchmark and tactical tooling), and what a training run needs to see whether a checkpoint finds known best moves.

`Analyzer` owns an analysis engine (m0_analysis_create): the positions wait in a host queue, the engine's tree slots are
refilled from it as searches finish, select -> network -> expand run on the device as in self-play, and only the compact
results come back (per position: up to `multipv` root moves by visits, each with its principal variation, visits, prior and
q; the root's value and q).  A result depends on (seed, id) and the position alone -- not on the slot, the number of slots or
the other positions in flight.  `evaluate` is the mode without a tree: one network evaluation per position, the legal moves
ranked by legal-softmax prior.

    an = Analyzer(backend, cfg, slots=256, multipv=3)
    for r in an.analyse([fen, (fen2, ["e2e4", "e7e5"])], sims=800):
        print(r["lines"][0]["move"], r["lines"][0]["pv"], r["root_q"])

With `tablebase=` (a matrix0_amd.tablebase.Tablebase or the path of its cache file) the generated endgame tables take part: a
position inside them is answered from them alone (status "tablebase": exact root_q, `dtm` in plies, lines ranked shortest
win first with the `dtm` behind each move, no evaluation), and every other search takes the exact value of each leaf it finds
in them.

Command line: python -m matrix0_amd.analysis --config config.yaml --checkpoint CKPT --fens FILE [--sims N] [--multipv K]
[--tablebase PATH [--tb-men N]] prints one JSON object per position (FILE: one FEN per line, optionally followed by `moves` and
UCI moves)."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

from . import engine as eng

Position = Union[str, Tuple[str, Sequence[str]]]


def _split(p: Position) -> Tuple[str, List[str]]:
    if isinstance(p, str):
        return p, []
    fen, ucis = p
    return str(fen), [str(u) for u in ucis]


class Analyzer:
    """`backend`: an M0Backend (its weights and stream are used in place).  `cfg_dict`: config.yaml as a dict; its `mcts`
    section drives the search as in self-play.  `slots` trees are searched at a time; `max_sims` (default: the configured
    num_simulations) sizes their node arenas."""

    def __init__(self, backend, cfg_dict: dict, *, slots: int = 256, multipv: int = 1, pv_len: int = 8, dirichlet: bool = False,
                 leaves_per_step: Optional[int] = None, max_sims: Optional[int] = None, seed: Optional[int] = None,
                 tablebase=None, tb_men: int = 4, prove: bool = False):
        if not 1 <= int(multipv) <= eng.AN_MAX_LINES or not 1 <= int(pv_len) <= eng.AN_MAX_PV:
            raise ValueError(f"multipv must be in [1, {eng.AN_MAX_LINES}] and pv_len in [1, {eng.AN_MAX_PV}]")
        self.multipv = int(multipv)
        cfg = eng.selfplay_cfg_from_dict(cfg_dict, concurrent_games=int(slots), leaves_per_step=leaves_per_step, seed=seed,
                                         record_games=False)
        if max_sims:
            cfg.num_simulations = int(max_sims)
        self.cfg = cfg
        self.engine = self._make_engine(backend, cfg, multipv=self.multipv, pv_len=int(pv_len), dirichlet=bool(dirichlet))
        self._tb_owned = None
        if prove:                                   # the proof search: results carry `proof` / `proof_plies`, proven lines rank first
            self.engine.set_proof()
        if tablebase is not None:
            try:
                if isinstance(tablebase, (str, os.PathLike)):        # a cache file: loaded here, closed with the analyzer
                    from .tablebase import Tablebase
                    tablebase = self._tb_owned = Tablebase.load(tablebase)
                self.engine.set_search_tablebase(tablebase, int(tb_men))
            except Exception:
                self.close()
                raise

    def _make_engine(self, backend, cfg, **opts):
        return eng.AnalysisEngine(backend, cfg, **opts)

    def _step(self) -> None:
        self.engine.step(8)

    def _run(self, positions: Iterable[Position], sims: int, ids: Optional[Sequence[int]]) -> List[dict]:
        pos = [_split(p) for p in positions]
        ids = list(range(len(pos))) if ids is None else [int(i) for i in ids]
        if len(ids) != len(pos) or len(set(ids)) != len(ids):
            raise ValueError("ids must be distinct, one per position")
        for (fen, ucis), i in zip(pos, ids):
            self.engine.submit(fen, ucis, sims=sims, id=i)
        by_id: Dict[int, dict] = {}

        def drain():
            while True:
                r = self.engine.poll()
                if r is None:
                    return
                by_id[r["id"]] = r

        drain()
        while self.engine.pending() > 0:
            self._step()
            drain()
        out = []
        for (fen, ucis), i in zip(pos, ids):           # completion order -> submission order
            r = by_id[i]
            r["fen"], r["moves"] = fen, ucis
            out.append(r)
        return out

    def analyse(self, positions: Iterable[Position], sims: Optional[int] = None, ids: Optional[Sequence[int]] = None) -> List[dict]:
        """Search every position with `sims` simulations (default: the configured number).  `positions`: FENs or
        (fen, [uci, ...]) pairs -- the position after the moves, which count for repetitions.  `ids` (default 0, 1, ...)
        key the random streams.  Returns one dict per position, in submission order: status ("ok" | "checkmate" |
        "stalemate" | "tablebase"), nlegal, sims, root_n, root_q, value, evals, overflow and `lines`: [{move, pv, visits, prior, q,
        policy_index}], best first."""
        sims = int(self.cfg.num_simulations if sims is None else sims)
        if sims < 1:
            raise ValueError("sims must be positive (evaluate() is the mode without a search)")
        if sims > self.cfg.num_simulations:
            raise ValueError(f"sims = {sims} exceeds what the node arenas were sized for ({self.cfg.num_simulations}): pass max_sims")
        return self._run(positions, sims, ids)

    def evaluate(self, positions: Iterable[Position], topk: Optional[int] = None) -> List[dict]:
        """One network evaluation per position, no tree: `lines` are the `topk` (default and at most: multipv) legal moves by
        legal-softmax prior, `value` the network's value for the side to move."""
        topk = self.multipv if topk is None else int(topk)
        if not 1 <= topk <= self.multipv:
            raise ValueError(f"topk must be in [1, multipv = {self.multipv}]")
        out = self._run(positions, 0, None)
        for r in out:
            del r["lines"][topk:]
        return out

    def stats(self) -> Dict[str, float]:
        return self.engine.stats()

    def close(self) -> None:
        self.engine.close()                # the engine first: the tables outlive it
        if self._tb_owned is not None:
            self._tb_owned.close()
            self._tb_owned = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AnalyzerExt(Analyzer):
    """The same with the caller's evaluator behind the reference's infer_np seam (f32 [B,19,8,8] -> logits [B,4672], values
    [B]) instead of the HIP network (m0_analysis_create_ext): parity tests, foreign evaluators.  Search only."""

    def __init__(self, infer_np, cfg_dict: dict, **kw):
        self.infer_np = infer_np
        super().__init__(None, cfg_dict, **kw)

    def _make_engine(self, backend, cfg, **opts):
        return eng.AnalysisExtEngine(cfg, **opts)

    def _step(self) -> None:
        self.engine.step(self.infer_np, 8)

    def evaluate(self, positions, topk=None):
        raise RuntimeError("policy mode needs the engine's own network: use Analyzer")


def suite_accuracy(results: Sequence[dict], best_moves: Sequence[str], k: Sequence[int] = (1, 3)) -> Dict[str, float]:
    """Share of positions whose labelled best move is among the first kk lines, for every kk of `k`: {"n": positions,
    "top1": ..., "top3": ...}.  A position without lines (mate, stalemate) counts as missed."""
    if len(results) != len(best_moves):
        raise ValueError("one labelled move per result")
    n = len(results)
    out: Dict[str, float] = {"n": n}
    for kk in k:
        hit = sum(1 for r, b in zip(results, best_moves) if b in [ln["move"] for ln in r["lines"][: int(kk)]])
        out[f"top{int(kk)}"] = hit / n if n else 0.0
    return out


def read_positions(path: str) -> List[Position]:
    """One position per line: a FEN, optionally followed by `moves m1 m2 ...` (UCI); blank lines and #-comments are skipped."""
    out: List[Position] = []
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            fen, _, moves = line.partition(" moves ")
            out.append((fen.strip(), moves.split()) if moves.strip() else fen.strip())
    return out


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.analysis", description="Analyse positions with a checkpoint on one MI355X.")
    ap.add_argument("--config", required=True, help="config.yaml (or .json) of the run: model, mcts sections")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--fens", required=True, help="file with one FEN per line ('-' = standard input)")
    ap.add_argument("--sims", type=int, default=None, help="simulations per position (default: the configured number; 0 = policy only)")
    ap.add_argument("--multipv", type=int, default=1)
    ap.add_argument("--pv-len", type=int, default=8)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tablebase", default=None, metavar="PATH", help="cache file of generated endgame tables (matrix0_amd.tablebase)")
    ap.add_argument("--tb-men", type=int, default=4, help="probe positions with at most this many men (default 4)")
    ap.add_argument("--prove", action="store_true",
                    help="proof search: exact wins, losses and draws are backed up the tree, a proven root ends its search, and "
                         "the output carries proof / proof_plies for the root and every line")
    return ap


def load_config(path: str) -> dict:
    with open(path) as f:
        if path.endswith(".json"):
            return json.load(f)
        import yaml
        return yaml.safe_load(f) or {}


def result_line(r: dict) -> str:
    """The JSON object the command line prints for one position."""
    keys = ("fen", "moves", "status", "nlegal", "sims", "root_n", "root_q", "value", "evals", "lines", "proof", "proof_plies")
    return json.dumps({k: r[k] for k in keys if k in r})


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    cfg = load_config(args.config)
    positions = read_positions("/dev/stdin" if args.fens == "-" else args.fens)
    from .backend import M0Backend
    be = M0Backend.from_checkpoint(cfg.get("model", {}) or {}, args.checkpoint, args.device)
    kw = dict(slots=args.slots, multipv=args.multipv, pv_len=args.pv_len)
    if args.sims:
        kw["max_sims"] = args.sims
    if args.tablebase:
        kw.update(tablebase=args.tablebase, tb_men=args.tb_men)
    if args.prove:
        kw["prove"] = True
    with Analyzer(be, cfg, **kw) as an:
        results = an.evaluate(positions) if args.sims == 0 else an.analyse(positions, args.sims)
    for r in results:
        print(result_line(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
