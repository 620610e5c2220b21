"""Generated 3- and 4-man endgame tablebases (the m0_tb_* part of the C-ABI, include/m0_engine.h).

The reference's worker ends a game as soon as the position after a move is found in a Syzygy table
(azchess/selfplay/internal.py:250-260, 559-581).  This engine computes the tables on the GPU instead of reading them
(distance to mate, no 50-move rule -- the reference looks at the sign of the WDL only), keeps them in host memory, and the
self-play engine probes them after every move (SelfplayEngine.set_tablebase).  With `in_search: true` they are also copied to
the GPU and probed inside the search (SelfplayEngine.set_search_tablebase): a leaf found in a table takes its exact value and
no network evaluation, in self-play, in matches (arena.play_match) and in analysis.

    engine: {tablebase: {max_pieces: 3 | 4, cache: <path or null>, in_search: false | true}}

in config.yaml makes the worker build (or load from `cache`) and attach them; `tablebases.enabled: true` of the reference's
own section is accepted only together with it.
"""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._abi import AnalysisResult
from .engine import analysis_result_to_dict

def tablebase_cfg(cfg_dict: dict) -> Optional[dict]:
    """`engine.tablebase` of config.yaml -> {"max_pieces": 3 | 4, "cache": path or None}; None when the key is absent.
    `in_search` (a bool, default false: the tables adjudicate only) appears in the result when the config names it."""
    tb = (cfg_dict.get("engine", {}) or {}).get("tablebase")
    if not tb:
        return None
    if not isinstance(tb, dict):
        raise ValueError("engine.tablebase must be a mapping {max_pieces: 3 | 4, cache: <path or null>, in_search: <bool>}")
    unknown = set(tb) - {"max_pieces", "cache", "in_search"}
    if unknown:
        raise ValueError(f"unknown engine.tablebase keys: {sorted(unknown)}")
    mp = tb.get("max_pieces", 4)
    if isinstance(mp, bool) or not isinstance(mp, int) or mp not in (3, 4):
        raise ValueError(f"engine.tablebase.max_pieces must be 3 or 4, not {mp!r}")
    cache = tb.get("cache")
    out = {"max_pieces": mp, "cache": str(cache) if cache else None}
    if "in_search" in tb:
        if not isinstance(tb["in_search"], bool):
            raise ValueError(f"engine.tablebase.in_search must be true or false, not {tb['in_search']!r}")
        out["in_search"] = tb["in_search"]
    return out


def in_search(cfg_dict: dict) -> bool:
    """`engine.tablebase.in_search`: the tables are probed inside the search, not only after a played move."""
    tb = tablebase_cfg(cfg_dict)
    return bool(tb and tb.get("in_search", False))


def probe_limit(cfg_dict: dict) -> int:
    """Men up to which the worker probes: min(tablebases.max_pieces, engine.tablebase.max_pieces).  `tablebases.max_pieces`
    defaults to 7 as in the reference (internal.py:562)."""
    tb = tablebase_cfg(cfg_dict)
    if tb is None:
        raise ValueError("engine.tablebase is not set")
    ref = (cfg_dict.get("tablebases", {}) or {}).get("max_pieces", 7)
    return min(int(ref), tb["max_pieces"])


class Tablebase:
    """A set of tables in host memory.  Immutable; may be attached to any number of engines, which it must outlive."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError(f"tablebase: {_lib.last_error()}")
        self._L = _lib.lib()
        self.handle = handle

    @classmethod
    def build(cls, max_men: int = 4, device: int = 0) -> "Tablebase":
        """Every signature in scope with at most `max_men` (3 or 4) men, built on GPU `device`."""
        return cls(_lib.lib().m0_tb_build(int(device), int(max_men)))

    @classmethod
    def build_signatures(cls, sigs: Sequence[str], device: int = 0) -> "Tablebase":
        """The given signatures ("KQKR", ...) and every table their captures and promotions lead into."""
        return cls(_lib.lib().m0_tb_build_signatures(int(device), _lib.cstrings(sigs), len(sigs)))

    @classmethod
    def load(cls, path: str) -> "Tablebase":
        """A cache file written by `save`; needs no GPU.  RuntimeError for a file that is damaged or of another format."""
        return cls(_lib.lib().m0_tb_load(os.fspath(path).encode()))

    @classmethod
    def cached(cls, path: Optional[str], max_men: int = 4, device: int = 0) -> "Tablebase":
        """Load `path` when it holds tables up to `max_men` men; otherwise build them and (with a path) save them there.
        Workers that share a cache path may all build and save at once: every save goes through a temporary file of its own,
        and a save that fails (a read-only directory, a full disk) is logged, not fatal -- the built tables are used."""
        if path and os.path.exists(path):
            tb = cls.load(path)
            if tb.max_men >= int(max_men):
                return tb
            tb.close()
        tb = cls.build(max_men, device)
        if path:
            try:
                tb.save(path)
            except (RuntimeError, ValueError) as e:
                logging.getLogger(__name__).warning("tablebase cache %s not written: %s", path, e)
        return tb

    def save(self, path: str) -> None:
        _lib.check(self._L.m0_tb_save(self.handle, os.fspath(path).encode()), "m0_tb_save")

    @property
    def max_men(self) -> int:
        return int(self._L.m0_tb_max_men(self.handle))

    def table(self, sig: str) -> np.ndarray:
        """The raw table of a signature (uint8, 2 * 64^n entries; a copy)."""
        p = C.POINTER(C.c_uint8)()
        n = C.c_size_t(0)
        _lib.check(self._L.m0_tb_table(self.handle, sig.encode(), C.byref(p), C.byref(n)), "m0_tb_table")
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    def info(self) -> List[Dict]:
        """Per table in build order: signature, largest d (-1: none decided), sweeps and milliseconds of its build."""
        out = []
        sig = C.create_string_buffer(8)
        maxd, sweeps, ms = C.c_int(0), C.c_int(0), C.c_double(0)
        i = 0
        while self._L.m0_tb_table_info(self.handle, i, sig, C.byref(maxd), C.byref(sweeps), C.byref(ms)) == 1:
            out.append({"sig": sig.value.decode(), "max_d": maxd.value, "sweeps": sweeps.value, "build_ms": ms.value})
            i += 1
        return out

    def probe(self, fens: Sequence[str]):
        """(hit bool[n], wdl int8[n] for the side to move, dtm int16[n] in plies)."""
        n = len(fens)
        hit = np.zeros(n, np.uint8); wdl = np.zeros(n, np.int8); dtm = np.zeros(n, np.int16)
        _lib.check(self._L.m0_tb_probe_fens(self.handle, _lib.cstrings(fens), n, _lib.ptr(hit), _lib.ptr(wdl), _lib.ptr(dtm)),
                   "m0_tb_probe_fens")
        return hit.astype(bool), wdl, dtm

    def root_lines(self, fen: str, multipv: int = 1, pv_len: int = 8) -> Optional[dict]:
        """The analysis of a position inside the tables, on the host: the dict an Analyzer returns for it (status "tablebase",
        root_q the wdl for the side to move, `dtm`, evals 0; lines best first -- shortest win, draws, longest loss -- each
        with q, `dtm` of the position after the move and the principal variation under the same rule).  None when `fen` is
        no hit."""
        r = AnalysisResult()
        rc = self._L.m0_tb_root_lines(self.handle, fen.encode(), int(multipv), int(pv_len), C.byref(r))
        return analysis_result_to_dict(r) if _lib.count(rc, "m0_tb_root_lines") == 1 else None

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._L.m0_tb_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
