"""The engine behind the UCI protocol: a GUI, cutechess-cli or a tournament manager plays a trained checkpoint against any
other UCI engine (the reference's side of this: azchess/engines/uci_bridge.py, cli_play.py).

    python -m matrix0_amd.uci --config config.yaml --checkpoint CKPT [--device N]

`UciEngine` is the protocol: `command(line)` takes one input line, `pump()` runs one pass of the search (select -> network ->
expand on the device) and prints whatever is due.  It drives an analysis engine with ONE tree slot through the live-search
calls (include/m0_analysis_live.h): the search is submitted with keep, read with `peek` for the periodic `info` lines, ended
with `stop` (`go infinite`, `go movetime`, the clock, the `stop` command), and its tree is held afterwards.  When the next
`position` extends the held one by 0..8 moves the next `go` continues in that tree (`continue_search`: the subtree behind the
moves is kept), anything else releases it and starts a fresh one.

Options: MultiPV 1..8 (lines printed), Move Overhead (ms taken off every time budget), MaxNodes (simulations of a search
that nothing ends earlier; it sizes the node arenas), Leaves 1..96 (leaves per pass, the search's inference_batch_size),
Tablebase (cache file of matrix0_amd.tablebase) and TablebaseMen.  MaxNodes, Leaves and the tablebase options rebuild the engine
before the next search.  Handled `go` arguments: nodes, movetime, wtime btime winc binc movestogo, infinite; depth, mate,
searchmoves and ponder are ignored with an `info string` each.  `go nodes N` is the only fully deterministic mode: every
other one ends on the clock.  `score mate` is printed for results from the endgame tables and, with the option ProveMates
(true / false, default false; `--prove` starts with it on; accepted by `setoption`, not listed by `uci`), for lines that the
proof search has proven (include/m0_proof.h): the search then ends as soon as its root is proven, and `go mate N` is honoured --
it ends once the root is a win in at most 2N-1 plies, or at its other limits -- instead of being ignored.

The command-line loop reads standard input on a thread into a queue and drains it between passes; every GPU call stays on the
main thread, so `isready` is answered during a search and `stop` / `quit` take effect between two passes."""
from __future__ import annotations

import argparse
import math
import queue
import sys
import threading
import time
from typing import Callable, List, Optional

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
ENGINE_NAME, ENGINE_AUTHOR = "matrix0-amd", "the matrix0_amd authors"

# Conventions, not measurements.
# q in [-1, 1] -> centipawns: lc0's mapping, cp = 90 tan(1.5637541897 q), clipped.
CP_SCALE, CP_ANGLE, CP_CLIP = 90.0, 1.5637541897, 12800
INFO_INTERVAL_MS = 500.0        # `info` lines at most this often while a search runs (and once before bestmove)
DEFAULT_MOVESTOGO = 30          # moves the remaining time is spread over when the GUI names none
INC_SHARE, MAX_SHARE = 0.75, 0.5    # of the increment added to / of the remaining time never exceeded by one move's budget
MAX_CONTINUE_MOVES = 8          # m0_analysis_continue follows at most this many moves
REUSE_TOTAL_FACTOR = 2          # a continued search stops growing a tree at this many times MaxNodes visits (the arenas'
                                # head-room: they are sized for MaxNodes simulations at ~125 nodes each, a search creates ~40)

OPTIONS = {        # name -> (type, default, min, max)
    "MultiPV": ("spin", 1, 1, 8),
    "Move Overhead": ("spin", 30, 0, 5000),
    "MaxNodes": ("spin", 800, 1, 1000000),
    "Leaves": ("spin", 32, 1, 96),
    "Tablebase": ("string", "", None, None),
    "TablebaseMen": ("spin", 4, 3, 4),
}
# ProveMates (check, default false): the proof search.  Proven lines print `score mate N` and `go mate N` is honoured.  It is
# accepted by setoption and is not in the list that `uci` prints (that list is pinned at six options): start the engine with
# --prove, or send `setoption name ProveMates value true`.
UNLISTED_OPTIONS = {"ProveMates": ("check", False, None, None)}
REBUILD_OPTIONS = ("MaxNodes", "Leaves", "Tablebase", "TablebaseMen", "ProveMates")
IGNORED_GO = ("depth", "mate", "searchmoves", "ponder")
GO_INT = ("nodes", "movetime", "wtime", "btime", "winc", "binc", "movestogo", "depth", "mate")
GO_WORDS = GO_INT + ("infinite", "ponder", "searchmoves")


def cp_from_q(q: float) -> int:
    q = max(-1.0, min(1.0, float(q)))
    cp = CP_SCALE * math.tan(CP_ANGLE * q)
    return int(max(-CP_CLIP, min(CP_CLIP, round(cp))))


def mate_score(dtm_plies: int, losing: bool) -> int:
    """Distance to mate in plies -> UCI's `score mate N` in moves: N = (dtm + 1) // 2, negative when the side to move loses."""
    n = (int(dtm_plies) + 1) // 2
    return -n if losing else n


def time_budget_ms(remaining: float, inc: float = 0.0, movestogo: Optional[int] = None, overhead: float = 0.0,
                   movetime: Optional[float] = None) -> float:
    """Milliseconds one move may take: movetime - overhead when movetime is given, else
    max(0, min(remaining / max(movestogo or 30, 1) + 0.75 inc, 0.5 remaining) - overhead)."""
    if movetime is not None:
        return max(0.0, float(movetime) - float(overhead))
    share = float(remaining) / max(int(movestogo or DEFAULT_MOVESTOGO), 1) + INC_SHARE * float(inc)
    return max(0.0, min(share, MAX_SHARE * float(remaining)) - float(overhead))


def parse_go(tokens: List[str]):
    """`go` arguments -> ({name: int | True | [moves]}, [names that were malformed])."""
    args, bad = {}, []
    i = 0
    while i < len(tokens):
        t = tokens[i]
        i += 1
        if t in GO_INT:
            try:
                args[t] = int(tokens[i])
                i += 1
            except (IndexError, ValueError):
                bad.append(t)
        elif t == "searchmoves":
            mv = []
            while i < len(tokens) and tokens[i] not in GO_WORDS:
                mv.append(tokens[i])
                i += 1
            args[t] = mv
        elif t in ("infinite", "ponder"):
            args[t] = True
        else:
            bad.append(t)
    return args, bad


def reuse_moves(held: Optional[dict], base: str, moves: List[str]) -> Optional[List[str]]:
    """The moves by which (base, moves) extends the held search's position, None when it does not (another base, another
    line, a shorter one, more than 8 moves further)."""
    if held is None or held["base"] != base:
        return None
    k = len(held["moves"])
    if len(moves) < k or moves[:k] != held["moves"] or len(moves) - k > MAX_CONTINUE_MOVES:
        return None
    return list(moves[k:])


class UciEngine:
    """`engine`: an AnalysisEngine / AnalysisExtEngine with one slot, created with multipv 8.  `cfg`: config.yaml as a dict (the
    defaults of MaxNodes and Leaves come from selfplay.num_simulations and mcts.inference_batch_size).  `out(line)` prints.
    `step()` runs one pass (default: engine.step(1)).  `rebuild(options) -> (engine, step)`, optional, makes a new engine when
    MaxNodes, Leaves or the tablebase options changed; `fen_after(fen, moves)` validates a position on the host (default:
    engine.fen_after of matrix0_amd.engine, m0_fen_after)."""

    def __init__(self, engine, cfg: Optional[dict] = None, *, out: Callable[[str], None], clock: Callable[[], float] = time.monotonic,
                 step: Optional[Callable[[], None]] = None, rebuild=None, fen_after=None):
        cfg = cfg or {}
        self.engine, self.out, self.clock, self.rebuild = engine, out, clock, rebuild
        self.step = step if step is not None else (lambda: self.engine.step(1))
        if fen_after is None:
            from . import engine as eng
            fen_after = eng.fen_after
        self.fen_after = fen_after
        self.options = {k: v[1] for k, v in OPTIONS.items()}
        self.unlisted = {k: v[1] for k, v in UNLISTED_OPTIONS.items()}      # beside `options`, which holds the listed ones
        sims = int((cfg.get("selfplay", {}) or {}).get("num_simulations", 0) or 0)
        leaves = int((cfg.get("mcts", {}) or {}).get("inference_batch_size", 0) or 0)
        if sims > 0:
            self.options["MaxNodes"] = min(sims, OPTIONS["MaxNodes"][3])
        if leaves > 0:
            self.options["Leaves"] = max(1, min(leaves, OPTIONS["Leaves"][3]))
        self.base, self.moves = START_FEN, []
        self.held: Optional[dict] = None        # {"id", "base", "moves"} of the search whose tree the engine holds
        self.search: Optional[dict] = None      # the running search
        self.next_id = 1
        self.quit = False
        self.dirty = False                      # an option changed that needs a new engine
        self.last_reused = 0

    # ---- input
    def command(self, line: str) -> None:
        tokens = line.split()
        if not tokens:
            return
        cmd, rest = tokens[0], tokens[1:]
        handler = {"uci": self._uci, "isready": self._isready, "setoption": self._setoption, "ucinewgame": self._newgame,
                   "position": self._position, "go": self._go, "stop": self._stop, "quit": self._quit}.get(cmd)
        if handler is None:
            self.out(f"info string unknown command: {cmd}")
        else:
            handler(rest)

    def _uci(self, rest):
        self.out(f"id name {ENGINE_NAME}")
        self.out(f"id author {ENGINE_AUTHOR}")
        for name, (kind, _, lo, hi) in OPTIONS.items():
            if kind == "spin":
                self.out(f"option name {name} type spin default {self.options[name]} min {lo} max {hi}")
            else:
                self.out(f"option name {name} type string default {self.options[name] or '<empty>'}")
        self.out("uciok")

    def _isready(self, rest):
        self.out("readyok")

    def _setoption(self, rest):
        if "name" not in rest:
            self.out("info string setoption needs a name")
            return
        i = rest.index("name")
        j = rest.index("value") if "value" in rest else len(rest)
        name = " ".join(rest[i + 1:j])
        value = " ".join(rest[j + 1:])
        every = {**OPTIONS, **UNLISTED_OPTIONS}
        key = {k.lower(): k for k in every}.get(name.lower())
        if key is None:
            self.out(f"info string unknown option: {name}")
            return
        kind, _, lo, hi = every[key]
        if kind == "check":
            if value.lower() not in ("true", "false"):
                self.out(f"info string option {key} needs true or false")
                return
            v = value.lower() == "true"
        elif kind == "spin":
            try:
                v = int(value)
            except ValueError:
                self.out(f"info string option {key} needs an integer")
                return
            if not lo <= v <= hi:
                self.out(f"info string option {key} must be in [{lo}, {hi}]")
                return
        else:
            v = "" if value == "<empty>" else value
        if self.search is not None and key in REBUILD_OPTIONS:
            self.out(f"info string option {key} cannot change during a search")
            return
        held_in = self.unlisted if key in UNLISTED_OPTIONS else self.options
        if held_in[key] != v and key in REBUILD_OPTIONS:
            self.dirty = True
        held_in[key] = v

    def _release(self):
        if self.held is not None:
            self.engine.release(self.held["id"])
            self.held = None

    def _newgame(self, rest):
        if self.search is not None:
            self.out("info string ucinewgame ignored during a search")
            return
        self._release()

    def _position(self, rest):
        if self.search is not None:
            self.out("info string position ignored during a search")
            return
        moves = []
        if "moves" in rest:
            k = rest.index("moves")
            rest, moves = rest[:k], rest[k + 1:]
        if rest[:1] == ["startpos"] and len(rest) == 1:
            base = START_FEN
        elif rest[:1] == ["fen"] and len(rest) > 1:
            base = " ".join(rest[1:])
        else:
            self.out("info string position needs startpos or fen")
            return
        try:
            self.fen_after(base, moves)
        except (ValueError, RuntimeError) as e:
            self.out(f"info string position refused: {e}")
            return
        self.base, self.moves = base, list(moves)

    def _go(self, rest):
        if self.search is not None:
            self.out("info string go ignored during a search")
            return
        args, bad = parse_go(rest)
        for name in bad:
            self.out(f"info string go: cannot read {name}")
        prove = bool(self.unlisted["ProveMates"])
        for name in IGNORED_GO:
            if name in args and not (name == "mate" and prove):
                self.out(f"info string go {name} is not supported and ignored")
        if self.dirty and self.rebuild is not None:
            self.held = None                                # the tree goes with its engine
            self.engine.close()
            self.engine, self.step = self.rebuild(dict(self.options, **self.unlisted))
        self.dirty = False
        max_nodes = int(self.options["MaxNodes"])
        sims = max(1, min(int(args["nodes"]), max_nodes)) if "nodes" in args else max_nodes
        budget = None
        overhead = float(self.options["Move Overhead"])
        white = self.fen_after(self.base, self.moves).split()[1] == "w"
        if "movetime" in args:
            budget = time_budget_ms(0, 0, None, overhead, movetime=args["movetime"])
        elif ("wtime" if white else "btime") in args and not args.get("infinite"):
            budget = time_budget_ms(args["wtime" if white else "btime"], args.get("winc" if white else "binc", 0),
                                    args.get("movestogo"), overhead)
        sid = self.next_id
        self.next_id += 1
        extra = reuse_moves(self.held, self.base, self.moves)
        self.last_reused = 0
        if extra is not None:
            held_id, self.held = self.held["id"], None
            self.last_reused = self.engine.continue_search(held_id, extra, sims, sid, keep=True)
            self.out(f"info string tree reused: {self.last_reused} nodes kept over {len(extra)} moves")
        else:
            self._release()
            self.engine.submit(self.base, self.moves, sims=sims, id=sid, keep=True)
        now = self.clock()
        self.search = {"id": sid, "t0": now, "budget": budget, "last_info": now, "longest": 0.0, "stopping": False,
                       "base": self.base, "moves": list(self.moves),
                       # go mate N with ProveMates: the search ends once the root is a win in at most 2N-1 plies (a search
                       # whose root is proven ends by itself, whatever the distance), or at its other limits
                       "mate": int(args["mate"]) if prove and "mate" in args else None,
                       # simulations a continued search may still add before its tree is REUSE_TOTAL_FACTOR x MaxNodes visits
                       "room": REUSE_TOTAL_FACTOR * max_nodes - self.last_reused if self.last_reused else None}
        self._collect()                                     # mate, stalemate, a root inside the tables: answered at once

    def _stop(self, rest):
        if self.search is not None:
            self.search["stopping"] = True

    def _quit(self, rest):
        self.quit = True
        if self.search is not None:                         # no bestmove after quit
            sid, self.search = self.search["id"], None
            try:
                self.engine.stop(sid)
                while self.engine.poll() is not None:
                    pass
            except (ValueError, RuntimeError):
                pass

    # ---- the search
    def searching(self) -> bool:
        return self.search is not None

    def _elapsed_ms(self) -> float:
        return (self.clock() - self.search["t0"]) * 1000.0

    def _collect(self) -> bool:
        """The search's answer, if it has come: info, bestmove, the tree held.  True when the search is over."""
        s = self.search
        while True:
            r = self.engine.poll()
            if r is None:
                return False
            if r["id"] == s["id"]:
                break
        self._info(r)
        if r["lines"]:
            pv = r["lines"][0]["pv"]
            self.out(f"bestmove {r['lines'][0]['move']}" + (f" ponder {pv[1]}" if len(pv) > 1 else ""))
        else:
            self.out("bestmove 0000")
        # a searched position keeps its tree; one answered on the host (mate, stalemate, tables) holds nothing
        self.held = {"id": s["id"], "base": s["base"], "moves": s["moves"]} if r["status"] == "ok" else None
        self.search = None
        return True

    def _info(self, r: dict) -> None:
        s = self.search
        ms = max(self._elapsed_ms(), 0.0)
        nps = int(r["sims"] * 1000.0 / ms) if ms > 0 else 0
        for k, ln in enumerate(r["lines"][: int(self.options["MultiPV"])]):
            if r["status"] == "tablebase" and ln["q"] != 0:
                score = f"mate {mate_score(ln['dtm'] + 1, ln['q'] < 0)}"     # ln["dtm"]: of the position after the move
            elif ln.get("proof") in ("win", "loss"):                         # ProveMates: a proven line
                score = f"mate {mate_score(ln['proof_plies'], ln['proof'] == 'loss')}"
            else:
                score = f"cp {cp_from_q(ln['q'])}"
            self.out(f"info depth {len(ln['pv'])} multipv {k + 1} score {score} nodes {r['root_n']} nps {nps} "
                     f"time {int(ms)} pv {' '.join(ln['pv'])}")
        s["last_info"] = self.clock()

    def _try_stop(self) -> bool:
        """End the search now if its best move has a visit; else one more pass.  True when the search is over."""
        s = self.search
        pk = self.engine.peek(s["id"])
        if pk is not None and pk["lines"] and pk["lines"][0]["visits"] > 0:
            self.engine.stop(s["id"])
            return self._collect()
        self._pass()
        return self._collect()

    def _pass(self) -> None:
        t = self.clock()
        self.step()
        s = self.search
        s["longest"] = max(s["longest"], (self.clock() - t) * 1000.0)
        if s["room"] is not None:                           # a pass adds at most Leaves simulations
            s["room"] -= int(self.options["Leaves"])
            if s["room"] <= 0:
                s["stopping"] = True

    def pump(self) -> bool:
        """One pass of the running search and whatever output is due.  False when nothing is being searched."""
        s = self.search
        if s is None:
            return False
        if self._collect():
            return False
        # a pass is started only if it fits: elapsed + the longest pass seen so far within the budget
        out_of_time = s["budget"] is not None and self._elapsed_ms() + s["longest"] > s["budget"]
        if s["stopping"] or out_of_time:
            self._try_stop()
            return self.search is not None
        self._pass()
        if self._collect():
            return False
        pk = None
        if s["mate"] is not None:                           # go mate N: found?
            pk = self.engine.peek(s["id"])
            if pk is not None and pk.get("proof") == "win" and pk["proof_plies"] <= 2 * s["mate"] - 1:
                s["stopping"] = True
        if (self.clock() - s["last_info"]) * 1000.0 >= INFO_INTERVAL_MS:
            pk = pk if pk is not None else self.engine.peek(s["id"])
            if pk is not None:
                self._info(pk)
        return True


# ---- command line
class _OwnedEngine:
    """The analysis engine of an Analyzer, closed together with the tables the Analyzer loaded for it."""

    def __init__(self, analyzer):
        self._an = analyzer

    def __getattr__(self, name):
        return getattr(self._an.engine, name)

    def close(self):
        self._an.close()


def make_engine(backend, cfg: dict, options: dict):
    """One-slot analysis engine on `backend` for the UCI options: (engine, step)."""
    from .analysis import Analyzer
    kw = dict(slots=1, multipv=8, pv_len=16, leaves_per_step=int(options["Leaves"]), max_sims=int(options["MaxNodes"]))
    if options.get("Tablebase"):
        kw.update(tablebase=options["Tablebase"], tb_men=int(options["TablebaseMen"]))
    if options.get("ProveMates"):
        kw["prove"] = True
    e = _OwnedEngine(Analyzer(backend, cfg, **kw))
    return e, (lambda: e.step(1))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.uci", description="UCI engine on one MI355X.")
    ap.add_argument("--config", required=True, help="config.yaml (or .json) of the run: model, mcts sections")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--prove", action="store_true", help="start with the option ProveMates on (the proof search)")
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    from .analysis import load_config
    from .backend import M0Backend
    cfg = load_config(args.config)
    be = M0Backend.from_checkpoint(cfg.get("model", {}) or {}, args.checkpoint, args.device)

    def out(line: str) -> None:
        sys.stdout.write(line + "\n")
        sys.stdout.flush()

    u = UciEngine(None, cfg, out=out, rebuild=lambda opts: make_engine(be, cfg, opts))
    u.unlisted["ProveMates"] = bool(args.prove)
    u.engine, u.step = make_engine(be, cfg, dict(u.options, **u.unlisted))
    lines: "queue.Queue[Optional[str]]" = queue.Queue()

    def reader():                          # standard input only; every GPU call stays on the main thread
        for line in sys.stdin:
            lines.put(line)
        lines.put(None)

    threading.Thread(target=reader, daemon=True).start()
    eof = False
    while not u.quit:
        try:
            line = lines.get(block=not u.searching()) if not eof else None
        except queue.Empty:
            line = ""
        if line is None:
            eof = True
            if not u.searching():
                break
        elif line:
            u.command(line)
            continue                       # drain the input before the next pass
        u.pump()
    u.engine.close()
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
