"""ctypes view of the search / self-play part of the C-ABI (include/m0_engine.h)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np

from . import _lib

from ._abi import (AN_MAX_LINES, AN_MAX_PV, AnalysisLine, AnalysisOpts, AnalysisResult, BudgetCfg, GameRecord,  # noqa: F401
                   GumbelCfg, ProofLines, SelfplayCfg, SelfplayStats)
from ._lib import ptr

c_double, c_int = C.c_double, C.c_int


def selfplay_cfg_from_dict(cfg: dict, *, concurrent_games: int, total_games: int = 0, first_game_index: int = 0,
                           seed: Optional[int] = None, leaves_per_step: Optional[int] = None,
                           virtual_loss_active: bool = True, ssl_in_forward: bool = False,
                           record_games: bool = True, arena_nodes: int = 0, ssl_targets: bool = False,
                           compat: Optional[dict] = None, eval_cache: Optional[bool] = None,
                           tail_split=None) -> SelfplayCfg:
    """Merge config.yaml's `mcts`, `selfplay` and draw sections exactly as selfplay_worker does
    (azchess/selfplay/internal.py:192-199, 269-304) into the engine's C struct.  MCTSConfig
    defaults are the dataclass defaults of azchess/mcts.py:61-107."""
    m = dict(cfg.get("mcts", {}) or {})
    sp = dict(cfg.get("selfplay", {}) or {})
    draw = dict(cfg.get("draw", {}) or {})
    draw.update(sp.get("draw", {}) or {})
    c = SelfplayCfg()
    c.max_children = int(m.get("max_children", 0) or 0)                 # MCTS._prune_children (mcts.py:806-826)
    c.min_child_prior = float(m.get("min_child_prior", 0.0) or 0.0)
    if c.max_children < 0 or c.max_children > 256 or c.min_child_prior < 0.0:
        raise ValueError("mcts.max_children must be in [0, 256] and mcts.min_child_prior >= 0")
    c.num_simulations = int(sp.get("num_simulations", m.get("num_simulations", 800)))
    c.cpuct = float(sp.get("cpuct", m.get("cpuct", 2.5)))
    cs, ce, cp = m.get("cpuct_start"), m.get("cpuct_end"), int(m.get("cpuct_plies", 0) or 0)
    if cs is not None and ce is not None and cp > 0:
        c.cpuct_start, c.cpuct_end, c.cpuct_plies = float(cs), float(ce), cp
    else:
        c.cpuct_start = c.cpuct_end = c.cpuct
        c.cpuct_plies = 0
    cb, ci = m.get("cpuct_c_base"), m.get("cpuct_c_init")
    c.use_c_base = int(cb is not None and ci is not None)
    c.cpuct_c_base = float(cb or 1.0)
    c.cpuct_c_init = float(ci or 0.0)
    c.dirichlet_alpha = float(sp.get("dirichlet_alpha", m.get("dirichlet_alpha", 0.3)))
    c.dirichlet_frac = float(sp.get("dirichlet_frac", m.get("dirichlet_frac", 0.25)))
    dp = m.get("dirichlet_plies", 16)
    c.dirichlet_plies = -1 if dp is None else int(dp)
    c.selection_jitter = float(sp.get("selection_jitter", m.get("selection_jitter", 0.01)))
    c.fpu_reduction = float(m.get("fpu_reduction", 0.15))
    c.draw_penalty = float(m.get("draw_penalty", -0.1))
    c.virtual_loss = float(m.get("virtual_loss", 1.0))
    c.legal_softmax = int(bool(m.get("legal_softmax", False)))
    c.enable_entropy_noise = int(bool(m.get("enable_entropy_noise", True)))
    c.no_instant_backtrack = int(bool(m.get("no_instant_backtrack", True)))
    c.value_from_white = int(bool(m.get("value_from_white", False)))
    ibs = int(m.get("inference_batch_size", m.get("simulation_batch_size", 96)) or 96)
    c.inference_batch_size = int(leaves_per_step if leaves_per_step else ibs)
    c.playout_random_frac = float(m.get("playout_random_frac", 0.0))
    c.max_game_len = int(sp.get("max_game_len", 200))
    c.min_resign_plies = int(sp.get("min_resign_plies", 24))
    c.opening_random_plies = int(sp.get("opening_random_plies", (cfg.get("openings", {}) or {}).get("random_plies", 0)))
    c.resign_threshold = float(sp.get("resign_threshold", -0.98))
    c.resign_window = int(sp.get("resign_window", 4))
    c.resign_consecutive_bad = int(sp.get("resign_consecutive_bad", 5))
    c.resign_min_entropy = float(sp.get("resign_min_entropy", 0.3))
    c.resign_value_margin = float(sp.get("resign_value_margin", 0.05))
    c.temperature_start = float(sp.get("temperature_start", 1.0))
    c.temperature_end = float(sp.get("temperature_end", 0.1))
    c.temperature_moves = int(sp.get("temperature_moves", 20))
    c.low_visit_threshold = int(sp.get("low_visit_threshold", 0) or 0)
    c.draw_enabled = int(bool(draw.get("enabled", False)))
    c.draw_min_plies = int(draw.get("min_plies", 30))
    c.draw_window = int(draw.get("window", 12))
    c.draw_min_unique = int(draw.get("min_unique", 3))
    c.draw_halfmove_cap = int(draw.get("halfmove_cap", 50))
    c.draw_material_threshold = int(draw.get("material_draw_threshold", 10))
    c.draw_stalemate = int(bool(draw.get("stalemate_draw", True)))
    c.concurrent_games = int(concurrent_games)
    c.total_games = int(total_games)
    c.first_game_index = int(first_game_index)
    c.arena_nodes = int(arena_nodes)
    c.seed = int(cfg.get("seed", 1234) if seed is None else seed)
    c.virtual_loss_active = int(bool(virtual_loss_active))
    c.ssl_in_forward = int(bool(ssl_in_forward))
    c.ssl_targets = int(bool(ssl_targets))
    c.record_games = int(bool(record_games))
    # reference behaviours the engine deviates from by default: `engine.compat` in config.yaml, or the `compat` argument
    cp = dict(((cfg.get("engine", {}) or {}).get("compat", {}) or {}))
    cp.update(compat or {})
    unknown = set(cp) - {"fresh_tree_per_move", "tt_merge", "raw_legal_priors", "root_reinfer"}
    if unknown:
        raise ValueError(f"unknown engine.compat keys: {sorted(unknown)}")
    c.fresh_tree_per_move = int(bool(cp.get("fresh_tree_per_move", False)))
    c.tt_merge = int(bool(cp.get("tt_merge", False)))
    c.raw_legal_priors = int(bool(cp.get("raw_legal_priors", False)))
    c.root_reinfer = int(bool(cp.get("root_reinfer", False)))
    # evaluation cache: `engine.eval_cache` in config.yaml or the keyword; off unless asked for (parity tests count evaluations)
    ecfg = cfg.get("engine", {}) or {}
    c.eval_cache = int(bool(ecfg.get("eval_cache", False) if eval_cache is None else eval_cache))
    c.eval_cache_entries = int(ecfg.get("eval_cache_entries", 0) or 0)
    # `engine.tail_split` (default off): true / 1 = the partial last round of a big pass runs on a second instance
    # over the same weights beside the main forward (+0.4..0.5 % games/s measured); "halves" / 2 = the pass as two halves side by
    # side (+1.3 %; the halves' kernel timings overlap)
    ts = ecfg.get("tail_split", False) if tail_split is None else tail_split
    c.tail_split = 2 if ts in ("halves", "half", 2) and ts is not True else int(bool(ts))
    return c


GUMBEL_DEFAULTS = {"max_considered": 16, "c_visit": 50.0, "c_scale": 1.0}      # the paper's


def _number(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float))


def _integer(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, int)


def _finite_nonneg(x) -> bool:
    return _number(x) and 0.0 <= float(x) < float("inf")


def _check_mode_config(cfg: dict, asking: str) -> None:
    """The modes that `cfg` turns on, by their config keys, must go with `asking`, the one whose block is being read:
    ValueError for engine.compat.tt_merge beside it and, where the budget mix is asked for, for another mode beside it."""
    mcts, ecfg = cfg.get("mcts", {}) or {}, cfg.get("engine", {}) or {}
    on = [name for name, is_on in (
        ("engine.proof_search", bool(ecfg.get("proof_search", False))),
        *((f"mcts.{k}", isinstance(mcts.get(k), dict) and mcts[k].get("enabled") is True) for k in ("gumbel", "budget"))) if is_on]
    others = ["engine.compat.tt_merge"] if bool((ecfg.get("compat", {}) or {}).get("tt_merge", False)) else []
    if asking == "mcts.budget":
        others += [name for name in on if name != asking]
    if others:
        raise ValueError(f"{asking} does not go with {others[0]}")


def _mode_block(cfg: dict, key: str, defaults: dict, checks: dict) -> Optional[dict]:
    """`mcts.<key>` of config.yaml with `defaults` merged in; None without the block or with `enabled: false`.  A block that is
    present has to be right: ValueError for anything but a mapping with a boolean `enabled`, for an unknown key, for a value
    that fails its entry of `checks` (field: (predicate, what it must be)), and for a mode that does not go with the others."""
    b = (cfg.get("mcts", {}) or {}).get(key)
    if b is None:
        return None
    if not isinstance(b, dict):
        raise ValueError(f"mcts.{key} must be a mapping, not {b!r}")
    unknown = set(b) - {"enabled", *defaults}
    if unknown:
        raise ValueError(f"unknown mcts.{key} keys: {sorted(map(str, unknown))}")
    if not isinstance(b.get("enabled"), bool):
        raise ValueError(f"mcts.{key}.enabled must be true or false")
    v = dict(defaults, **{k: x for k, x in b.items() if k != "enabled"})
    for field, (ok, must_be) in checks.items():
        if not ok(v[field]):
            raise ValueError(f"mcts.{key}.{field} must be {must_be}, not {v[field]!r}")
    if not b["enabled"]:
        return None
    _check_mode_config(cfg, f"mcts.{key}")
    return v


def gumbel_cfg_from_dict(cfg: dict) -> Optional[GumbelCfg]:
    """`mcts.gumbel: {enabled, max_considered: 16, c_visit: 50.0, c_scale: 1.0}` of config.yaml as the library's struct (for
    SelfplayEngine.set_gumbel); None without the block or with `enabled: false`.  A block that is present has to be right
    (_mode_block): max_considered an integer in 1..256, the constants finite numbers >= 0, no engine.compat.tt_merge beside it."""
    v = _mode_block(cfg, "gumbel", GUMBEL_DEFAULTS, {
        "max_considered": (lambda m: _integer(m) and 1 <= m <= 256, "an integer in 1..256"),
        "c_visit": (_finite_nonneg, "a finite number >= 0"), "c_scale": (_finite_nonneg, "a finite number >= 0")})
    return None if v is None else GumbelCfg(int(v["max_considered"]), float(v["c_visit"]), float(v["c_scale"]))


BUDGET_DEFAULTS = {"full_prob": 0.25, "fast_simulations": 100, "forced_k": 2.0, "prune_targets": True}   # KataGo's forced_k
BUDGET_STATS = ("full_searches", "fast_searches", "forced_descents", "pruned_visits")


def budget_cfg_from_dict(cfg: dict) -> Optional[BudgetCfg]:
    """`mcts.budget: {enabled, full_prob: 0.25, fast_simulations: 100, forced_k: 2.0, prune_targets: true}` of config.yaml as the
    library's struct (for SelfplayEngine.set_budget); None without the block or with `enabled: false`.  A block that is present
    has to be right (_mode_block): full_prob a number in (0, 1], fast_simulations an integer >= 1, forced_k a finite number >= 0,
    prune_targets a boolean, and no mcts.gumbel, engine.proof_search or engine.compat.tt_merge beside it."""
    v = _mode_block(cfg, "budget", BUDGET_DEFAULTS, {
        "full_prob": (lambda p: _number(p) and 0.0 < float(p) <= 1.0, "a number in (0, 1]"),
        "fast_simulations": (lambda n: _integer(n) and n >= 1, "an integer >= 1"),
        "forced_k": (_finite_nonneg, "a finite number >= 0"),
        "prune_targets": (lambda x: isinstance(x, bool), "true or false")})
    return None if v is None else BudgetCfg(float(v["full_prob"]), int(v["fast_simulations"]), float(v["forced_k"]),
                                            int(v["prune_targets"]))


def move_to_uci(m: int) -> str:
    f, t, p = m & 63, (m >> 6) & 63, (m >> 12) & 7
    s = "abcdefgh"[f & 7] + str((f >> 3) + 1) + "abcdefgh"[t & 7] + str((t >> 3) + 1)
    return s + (" nbrq"[p] if p else "")


class SelfplayEngine:
    """Many concurrent games on one GPU.  `backend` is an M0Backend (its weights and stream are used
    in place); pass None for the split-step search API with an external evaluator."""

    def __init__(self, backend, cfg: SelfplayCfg):
        self._open(backend, cfg, "m0_selfplay_create", backend.handle if backend is not None else None, C.byref(cfg))

    def _open(self, backend, cfg: SelfplayCfg, create: str, *args) -> None:
        """What every engine class constructs: the handle from its own create call."""
        self._L = _lib.lib()
        self.backend = backend
        self.cfg = cfg
        self._h = getattr(self._L, create)(*args)
        if not self._h:
            raise RuntimeError(f"{create} failed: {_lib.last_error()}")

    def _select(self, fn, what: str, regions: int = 1) -> List[np.ndarray]:
        """A select call of the library, `fn(handle, rows..., planes..., max_rows)` with one rows counter and one planes buffer of
        concurrent_games * (inference_batch_size + 1) rows per region (network): the leaf planes f32 [rows,19,8,8] per region."""
        cap = self.cfg.concurrent_games * (self.cfg.inference_batch_size + 1)
        rows = [c_int(0) for _ in range(regions)]
        planes = [np.zeros((cap, 19, 8, 8), dtype=np.float32) for _ in range(regions)]
        _lib.check(fn(self._h, *[C.byref(r) for r in rows], *[ptr(p) for p in planes], cap), what)
        return [p[: r.value] for p, r in zip(planes, rows)]

    def _expand(self, fn, what: str, *answers) -> None:
        """An expand call of the library, `fn(handle, (logits, values, rows)...)`: one evaluator's answer (logits, values) per
        region, handed over as contiguous float32."""
        args = []
        for logits, values in answers:
            lg = np.ascontiguousarray(logits, dtype=np.float32)
            vv = np.ascontiguousarray(values, dtype=np.float32)
            args += [ptr(lg), ptr(vv), int(lg.shape[0])]         # the pointers keep their arrays alive
        _lib.check(fn(self._h, *args), what)

    def step(self, steps: int = 1) -> None:
        _lib.check(self._L.m0_selfplay_step(self._h, int(steps)), "m0_selfplay_step")

    def stats(self) -> Dict[str, float]:
        s = SelfplayStats()
        _lib.check(self._L.m0_selfplay_stats_get(self._h, C.byref(s)), "m0_selfplay_stats_get")
        return {k: getattr(s, k) for k, _ in SelfplayStats._fields_}

    def running(self) -> bool:
        return bool(self._L.m0_selfplay_running(self._h))

    def poll(self) -> Optional[dict]:
        """One finished game as the reference's NPZ dict (selfplay/internal.py:628-646) + queue metadata."""
        r = GameRecord()
        if _lib.count(self._L.m0_selfplay_poll(self._h, C.byref(r)), "m0_selfplay_poll") == 0:
            return None
        try:
            T = r.moves
            out = {
                "game_index": r.game_index, "moves": T, "resigned": bool(r.resigned),
                "resigner": {0: None, 1: "W", 2: "B"}[r.resigner], "draw": bool(r.draw), "result": float(r.result),
                "avg_policy_entropy": float(r.avg_policy_entropy), "avg_sims": float(r.avg_sims), "secs": float(r.secs),
                "played": ([move_to_uci(int(x)) for x in np.ctypeslib.as_array(r.played, shape=(r.total_plies,))]
                           if r.total_plies > 0 else []),
                "played_raw": (np.ctypeslib.as_array(r.played, shape=(r.total_plies,)).copy()
                               if r.total_plies > 0 else np.zeros(0, np.uint16)),
            }
            if r.start_fen:                                    # the game started from an opening-book position
                out["start_fen"] = r.start_fen.decode()
            if r.s and T > 0:                                  # arena records carry only the moves and the result
                out["s"] = np.ctypeslib.as_array(r.s, shape=(T, 19, 8, 8)).copy()
                out["pi"] = np.ctypeslib.as_array(r.pi, shape=(T, 4672)).copy()
                out["legal_mask"] = np.ctypeslib.as_array(r.legal_mask, shape=(T, 4672)).copy()
            if T > 0:
                out["z"] = np.ctypeslib.as_array(r.z, shape=(T,)).copy()
                out["search_values"] = np.ctypeslib.as_array(r.search_values, shape=(T,)).copy()
            if r.ssl:
                out["ssl"] = _lib.split_ssl(np.ctypeslib.as_array(r.ssl, shape=(T, 17, 8, 8)).copy())
            if getattr(self, "budget", None) is not None:      # budget mix: which plies were searched in full, and with how much
                full, sims = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int)()
                _lib.check(self._L.m0_game_record_budget(C.byref(r), C.byref(full), C.byref(sims)), "m0_game_record_budget")
                have = bool(full) and bool(sims) and T > 0
                out["full"] = np.ctypeslib.as_array(full, shape=(T,)).astype(bool) if have else np.zeros(0, bool)
                out["sims"] = np.ctypeslib.as_array(sims, shape=(T,)).astype(np.int32) if have else np.zeros(0, np.int32)
        finally:
            self._L.m0_game_record_free(C.byref(r))
        return out

    def set_openings(self, fens: List[str]) -> None:
        """Opening book positions (selfplay/internal.py:34-69); call before the first step."""
        _lib.check(self._L.m0_selfplay_set_openings(self._h, _lib.cstrings(fens), len(fens)), "m0_selfplay_set_openings")

    def set_tablebase(self, tb, max_pieces: int = 4) -> None:
        """Attach a matrix0_amd.tablebase.Tablebase (None detaches); call before the first step.  After every played move a
        position with at most `max_pieces` men is probed and a hit ends the game with the table's verdict
        (selfplay/internal.py:559-581).  The engine keeps a reference: the tables live as long as it does."""
        _lib.check(self._L.m0_selfplay_set_tablebase(self._h, tb.handle if tb is not None else None, int(max_pieces)),
                   "m0_selfplay_set_tablebase")
        self._tablebase = tb

    def tb_adjudications(self) -> int:
        """Games ended by a tablebase hit."""
        return int(self._L.m0_selfplay_tb_adjudications(self._h))

    def set_search_tablebase(self, tb, max_pieces: int = 4) -> None:
        """Attach a matrix0_amd.tablebase.Tablebase to the search itself (None detaches); every engine kind, before the first
        step.  The tables are copied to the engine's GPU once per handle and device; from then on a leaf with at most
        `max_pieces` men that is in the tables is a terminal leaf with the table's value and costs no evaluation.  A root inside
        the tables: self-play and match engines end the game there with the table's verdict (as `set_tablebase`), an analysis
        engine answers it from the tables (status "tablebase"), the split-step search searches it as given."""
        _lib.check(self._L.m0_selfplay_set_search_tablebase(self._h, tb.handle if tb is not None else None, int(max_pieces)),
                   "m0_selfplay_set_search_tablebase")
        self._tablebase = tb

    def tb_leaves(self) -> int:
        """Leaves the search took from the tables instead of the network (as of the last step)."""
        return int(self._L.m0_selfplay_tb_leaves(self._h))

    def ext_select(self) -> np.ndarray:
        """First half of a self-play step for an external evaluator: the leaf planes f32 [rows,19,8,8]."""
        return self._select(self._L.m0_selfplay_ext_select, "m0_selfplay_ext_select")[0]

    def ext_expand(self, logits: np.ndarray, values: np.ndarray) -> None:
        self._expand(self._L.m0_selfplay_ext_expand, "m0_selfplay_ext_expand", (logits, values))

    def last_batch_nhwc(self) -> np.ndarray:
        """The network batch the last select wrote on the device (what `step()` feeds the network): f16 [rows,64,32],
        row r = position r of the planes that select returned, channels 19..31 zero."""
        cap = self.cfg.concurrent_games * (self.cfg.inference_batch_size + 1) + 4
        out = np.zeros((cap, 64, 32), dtype=np.float16)
        rows = c_int(0)
        _lib.check(self._L.m0_selfplay_last_batch_nhwc(self._h, ptr(out), cap, C.byref(rows)),
                   "m0_selfplay_last_batch_nhwc")
        return out[: rows.value]

    # ---- split-step search ----
    def search_begin(self, g: int, fen: str, sims: int, dirichlet: bool, game_uid: int) -> None:
        _lib.check(self._L.m0_search_begin(self._h, g, fen.encode(), sims, int(dirichlet), game_uid), "m0_search_begin")

    def search_select(self) -> np.ndarray:
        return self._select(self._L.m0_search_select, "m0_search_select")[0]

    def search_expand(self, logits: np.ndarray, values: np.ndarray) -> None:
        self._expand(self._L.m0_search_expand, "m0_search_expand", (logits, values))

    def search_result(self, g: int) -> dict:
        n = c_int(0); rn = c_int(0); fin = c_int(0); rq = c_double(0)
        cn = np.zeros(256, np.int32); mv = np.zeros(256, np.uint16); idx = np.zeros(256, np.int32)
        pr = np.zeros(256, np.float64); q = np.zeros(256, np.float64)
        _lib.check(self._L.m0_search_result(self._h, g, C.byref(n), ptr(cn), ptr(mv), ptr(idx), ptr(pr), ptr(q),
                                            C.byref(rq), C.byref(rn), C.byref(fin)),
                   "m0_search_result")
        k = n.value
        return {"finished": bool(fin.value), "n": cn[:k].copy(), "moves": [move_to_uci(int(x)) for x in mv[:k]],
                "idx": idx[:k].copy(), "prior": pr[:k].copy(), "q": q[:k].copy(), "root_q": rq.value, "root_n": rn.value}

    def _mode_result(self, g: int, name: str, *out):
        """A search mode's result call `name` for slot g, beside search_result(g): `out` are its outputs in the call's order, a
        ctypes scalar or an array of 256 per root child.  Their values: a scalar's, an array's first k (the root's children)."""
        k = c_int(0)
        _lib.check(self._L.m0_search_result(self._h, g, C.byref(k), None, None, None, None, None, None, None, None),
                   "m0_search_result")
        _lib.check(getattr(self._L, name)(self._h, g, *[ptr(o) if isinstance(o, np.ndarray) else C.byref(o) for o in out]), name)
        return [o[: k.value].copy() if isinstance(o, np.ndarray) else o.value for o in out]

    # ---- Gumbel root search (include/m0_gumbel.h)
    def set_gumbel(self, gumbel: Optional[GumbelCfg] = None, *, max_considered: int = GUMBEL_DEFAULTS["max_considered"],
                   c_visit: float = GUMBEL_DEFAULTS["c_visit"], c_scale: float = GUMBEL_DEFAULTS["c_scale"]) -> None:
        """Turn the Gumbel root search on (a self-play engine, before the first step or search): `gumbel` as
        gumbel_cfg_from_dict returns it, or the three numbers."""
        g = gumbel if gumbel is not None else GumbelCfg(int(max_considered), float(c_visit), float(c_scale))
        _lib.check(self._L.m0_selfplay_set_gumbel(self._h, C.byref(g)), "m0_selfplay_set_gumbel")
        self.gumbel = g

    def search_gumbel_result(self, g: int) -> dict:
        """Beside search_result(g): `pick` (index into its children, -1 while the search runs), `v_mix`, `pi` and `gl` per root
        child, and `miss` (0 unless the schedule found no child with the visit count it asked for)."""
        pick, v_mix, pi, gl, miss = self._mode_result(g, "m0_search_gumbel_result", c_int(-1), c_double(0),
                                                      np.zeros(256, np.float64), np.zeros(256, np.float64), c_int(0))
        return {"pick": pick, "v_mix": v_mix, "pi": pi, "gl": gl, "miss": miss}

    # ---- self-play budget mix (include/m0_budget.h)
    def set_budget(self, budget: Optional[BudgetCfg] = None, *, full_prob: float = BUDGET_DEFAULTS["full_prob"],
                   fast_simulations: int = BUDGET_DEFAULTS["fast_simulations"], forced_k: float = BUDGET_DEFAULTS["forced_k"],
                   prune_targets: bool = BUDGET_DEFAULTS["prune_targets"]) -> None:
        """Turn the budget mix on (a self-play engine, before the first step or search): `budget` as budget_cfg_from_dict
        returns it, or the four values.  Most moves then get a fast search without noise, a random share of `full_prob` the full
        one with forced playouts at the root and a pruned policy target; `poll()` adds `full` and `sims` per ply."""
        b = budget if budget is not None else BudgetCfg(float(full_prob), int(fast_simulations), float(forced_k),
                                                        int(bool(prune_targets)))
        _lib.check(self._L.m0_selfplay_set_budget(self._h, C.byref(b)), "m0_selfplay_set_budget")
        self.budget = b

    def search_budget_result(self, g: int) -> dict:
        """Beside search_result(g): `pruned_n` and `pi` per root child (the plain visits and shares with forced_k = 0 or without
        prune_targets) and `forced_descents`, the descents the forcing rule has decided in the slot; zeros and -1 while the
        search runs."""
        pruned_n, pi, fd = self._mode_result(g, "m0_search_budget_result", np.zeros(256, np.int32), np.zeros(256, np.float64),
                                             c_int(-1))
        return {"pruned_n": pruned_n, "pi": pi, "forced_descents": fd}

    def budget_stats(self) -> Dict[str, int]:
        """Full searches, fast searches, descents decided by the forcing rule and visits pruned from targets so far."""
        out = np.zeros(4, np.uint64)
        _lib.check(self._L.m0_selfplay_budget_stats(self._h, ptr(out)), "m0_selfplay_budget_stats")
        return {k: int(x) for k, x in zip(BUDGET_STATS, out)}

    # ---- proof search (include/m0_proof.h)
    def set_proof(self, on: bool = True) -> None:
        """Turn the proof search on or off (before the first step or search): exact wins, losses and draws are backed up the
        tree, a search whose root is proven ends.  Not on a self-play engine that plays games with its own network."""
        _lib.check(self._L.m0_selfplay_set_proof(self._h, int(bool(on))), "m0_selfplay_set_proof")
        self.proof = bool(on)

    def search_proof_result(self, g: int) -> dict:
        """Beside search_result(g): the root's `state` (PROOF_STATES) and `plies`, `child_state` and `child_plies` per root child
        (from the view of the child's side to move) and `pick` (index into its children, -1 while the search runs)."""
        st, plies, cs, cp, pick = self._mode_result(g, "m0_search_proof_result", c_int(0), c_int(0), np.zeros(256, np.int32),
                                                    np.zeros(256, np.int32), c_int(-1))
        return {"state": PROOF_STATES[st], "plies": plies, "pick": pick,
                "child_state": [PROOF_STATES[int(x)] for x in cs], "child_plies": cp}

    def search_advance(self, g: int, slot: int, sims: int, dirichlet: bool) -> None:
        _lib.check(self._L.m0_search_advance(self._h, g, slot, sims, int(dirichlet)), "m0_search_advance")

    def close(self):
        if getattr(self, "_h", None):
            self._L.m0_selfplay_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SelfplayPool:
    """`streams` independent SelfplayEngines on ONE GPU behind the SelfplayEngine interface: every engine has its own
    network instance (weights, workspace, HIP stream) and an equal share of the concurrent games, and `step()` runs them
    concurrently, one host thread each (the C calls release the GIL).  Games never interact, so nothing else changes --
    a game's record depends only on (seed, game index), whichever engine plays it -- but the tree kernels, launch
    boundaries and epilogue HBM bursts of one share now overlap the network kernels of the other: +3..4 % evaluations/s
    at 2 x 128 games against 1 x 256 (bench.py --streams 2; 4 x 64 gives nothing more).  Costs one more copy of the
    weights in HBM.  Per-launch kernel timings taken in this mode include the other stream's kernels."""

    def __init__(self, backend_factory, cfg_dict: dict, *, streams: int, concurrent_games: int, total_games: int = 0,
                 first_game_index: int = 0, **cfg_kw):
        import threading
        self._threading = threading
        streams = max(1, min(int(streams), int(concurrent_games)))
        self.backends, self.engines = [], []
        per = [concurrent_games // streams + (1 if i < concurrent_games % streams else 0) for i in range(streams)]
        tot = [0] * streams if total_games <= 0 else \
              [total_games // streams + (1 if i < total_games % streams else 0) for i in range(streams)]
        first = first_game_index
        try:
            for i in range(streams):
                be = backend_factory()
                self.backends.append(be)
                cfg = selfplay_cfg_from_dict(cfg_dict, concurrent_games=(min(per[i], tot[i]) if total_games > 0 else per[i]) or 1,
                                             total_games=tot[i], first_game_index=first, **cfg_kw)
                self.engines.append(SelfplayEngine(be, cfg))
                # unbounded mode: each engine restarts games forever, so it gets a disjoint block of indices
                first += tot[i] if total_games > 0 else (1 << 20)
        except Exception:
            self.close()
            raise
        self._rr = 0

    def step(self, steps: int = 1) -> None:
        live = [e for e in self.engines if e.running()]
        if len(live) <= 1:
            for e in live:
                e.step(steps)
            return
        errs = []

        def run(e):
            try:
                e.step(steps)
            except Exception as ex:          # re-raised in the caller's thread
                errs.append(ex)

        th = [self._threading.Thread(target=run, args=(e,)) for e in live]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]

    def running(self) -> bool:
        return any(e.running() for e in self.engines)

    def poll(self) -> Optional[dict]:
        for k in range(len(self.engines)):
            e = self.engines[(self._rr + k) % len(self.engines)]
            rec = e.poll()
            if rec is not None:
                self._rr = (self._rr + k + 1) % len(self.engines)
                return rec
        return None

    def stats(self) -> Dict[str, float]:
        """Counters summed over the engines; the ms_* clocks are per-engine host clocks of concurrent work: averaged."""
        out: Dict[str, float] = {}
        sts = [e.stats() for e in self.engines]
        for k in sts[0]:
            v = sum(s[k] for s in sts)
            out[k] = v / len(sts) if k.startswith("ms_") or k == "steps" else v
        return out

    # ---- self-play budget mix: every engine of the pool, in slot order
    def set_budget(self, *args, **kw) -> None:
        for e in self.engines:
            e.set_budget(*args, **kw)

    def search_budget_result(self, g: int) -> dict:
        """Slot g counted over the engines in order (engine 0's slots first)."""
        for e in self.engines:
            if g < e.cfg.concurrent_games:
                return e.search_budget_result(g)
            g -= e.cfg.concurrent_games
        raise IndexError("slot out of range")

    def budget_stats(self) -> Dict[str, int]:
        sts = [e.budget_stats() for e in self.engines]
        return {k: sum(s[k] for s in sts) for k in sts[0]}

    def close(self):
        for e in getattr(self, "engines", []):
            e.close()
        for b in getattr(self, "backends", []):
            try:
                b.close()
            except Exception:
                pass
        self.engines, self.backends = [], []


# ---- host decision functions (no GPU needed) ----
def sample_move_index(visits, temperature: float, u: float) -> int:
    L = _lib.lib()
    v = np.ascontiguousarray(visits, dtype=np.int32)
    return int(L.m0_sample_move_index(ptr(v), int(v.shape[0]), float(temperature), float(u)))


def playout_cap(sims: int, frac: float, u: float) -> int:
    return int(_lib.lib().m0_playout_cap(int(sims), float(frac), float(u)))


def gumbel_schedule(m_eff: int, n: int):
    """(seq, phase_end), i32 [n] each: the visit count simulation s considers at the root and the first simulation after its
    phase, for m_eff considered children and n simulations (include/m0_gumbel.h)."""
    seq, end = np.zeros(int(n), np.int32), np.zeros(int(n), np.int32)
    _lib.check(_lib.lib().m0_gumbel_schedule(int(m_eff), int(n), ptr(seq), ptr(end)), "m0_gumbel_schedule")
    return seq, end


def gumbel_improve(prior, q, n, gl, root_v: float, c_visit: float = GUMBEL_DEFAULTS["c_visit"],
                   c_scale: float = GUMBEL_DEFAULTS["c_scale"]):
    """(pi f64 [k], v_mix, pick) of a root's children from their prior, q, visits and gl (include/m0_gumbel.h)."""
    pr, qq, gg = (np.ascontiguousarray(a, dtype=np.float64) for a in (prior, q, gl))
    nn = np.ascontiguousarray(n, dtype=np.int32)
    k = int(pr.shape[0])
    if not (qq.shape == nn.shape == gg.shape == (k,)):
        raise ValueError("prior, q, n and gl must have one entry per child")
    pi = np.zeros(k, np.float64)
    vm, pick = c_double(0), c_int(-1)
    g = GumbelCfg(GUMBEL_DEFAULTS["max_considered"], float(c_visit), float(c_scale))
    _lib.check(_lib.lib().m0_gumbel_improve(k, ptr(pr), ptr(qq), ptr(nn), ptr(gg), float(root_v), C.byref(g), ptr(pi),
                                            C.byref(vm), C.byref(pick)), "m0_gumbel_improve")
    return pi, vm.value, pick.value


def budget_is_full(seed: int, game_index: int, ply: int, full_prob: float) -> bool:
    """Whether searched ply `ply` of game `game_index` gets the full search (include/m0_budget.h)."""
    full = c_int(0)
    _lib.check(_lib.lib().m0_budget_is_full(int(seed), int(game_index), int(ply), float(full_prob), C.byref(full)),
               "m0_budget_is_full")
    return bool(full.value)


def budget_forced(forced_k: float, prior: float, n_sum: int) -> float:
    """sqrt(forced_k * prior * n_sum): the visits forced playouts bring a visited root child up to."""
    out = c_double(0)
    _lib.check(_lib.lib().m0_budget_forced(float(forced_k), float(prior), int(n_sum), C.byref(out)), "m0_budget_forced")
    return out.value


def budget_prune(prior, q, n, root_n: int, cpuct: float, forced_k: float = BUDGET_DEFAULTS["forced_k"]):
    """(pruned_n i32 [k], pi f64 [k], best) of a root's children from their prior, q and visits (include/m0_budget.h)."""
    pr, qq = (np.ascontiguousarray(a, dtype=np.float64) for a in (prior, q))
    nn = np.ascontiguousarray(n, dtype=np.int32)
    k = int(pr.shape[0])
    if not (qq.shape == nn.shape == (k,)):
        raise ValueError("prior, q and n must have one entry per child")
    pn, pi, best = np.zeros(k, np.int32), np.zeros(k, np.float64), c_int(-1)
    _lib.check(_lib.lib().m0_budget_prune(k, ptr(pr), ptr(qq), ptr(nn), int(root_n), float(cpuct), float(forced_k), ptr(pn),
                                          ptr(pi), C.byref(best)), "m0_budget_prune")
    return pn, pi, best.value


PROOF_STATES = ["none", "win", "loss", "draw"]                 # M0_PROOF_* of include/m0_proof.h, by value


def proof_combine(states, plies, complete: bool):
    """(state, plies) of a parent from its children's (names of PROOF_STATES, or their values) by the rule of the proof search
    (include/m0_proof.h); `complete`: the children are all of the parent's legal moves."""
    ss = np.ascontiguousarray([PROOF_STATES.index(s) if isinstance(s, str) else int(s) for s in states], dtype=np.int32)
    pp = np.ascontiguousarray(plies, dtype=np.int32)
    if ss.shape != pp.shape:
        raise ValueError("states and plies must have one entry per child")
    st, pl = c_int(0), c_int(0)
    _lib.check(_lib.lib().m0_proof_combine(int(ss.shape[0]), ptr(ss), ptr(pp), int(bool(complete)), C.byref(st), C.byref(pl)),
               "m0_proof_combine")
    return PROOF_STATES[st.value], pl.value


def temperature_for(fullmove: int, t_start: float, t_end: float, t_moves: int) -> float:
    return float(_lib.lib().m0_temperature_for(int(fullmove), float(t_start), float(t_end), int(t_moves)))


RULE_FLAGS = ["game_over", "game_over_claim", "adjudicate_draw", "checkmate", "stalemate", "insufficient",
              "can_claim_fifty", "repetition3", "can_claim_threefold", "fivefold", "seventyfive"]


def rules_probe(cfg: SelfplayCfg, fen: str, ucis: List[str]) -> dict:
    L = _lib.lib()
    flags = c_int(0); res = C.c_float(0)
    _lib.check(L.m0_rules_probe(C.byref(cfg), fen.encode(), _lib.cstrings(ucis), len(ucis), C.byref(flags), C.byref(res)),
               "m0_rules_probe")
    out = {name: bool(flags.value >> i & 1) for i, name in enumerate(RULE_FLAGS)}
    out["result"] = float(res.value)
    return out


def encode_fens_nhwc(fens, device_index: int = 0) -> np.ndarray:
    """encode_board (encoding.py:11-46) as the search's select kernel writes it for the network: f16 [n,64,32]."""
    L = _lib.lib()
    n = len(fens)
    out = np.empty((n, 64, 32), np.float16)
    _lib.check(L.m0_encode_fens_nhwc(int(device_index), _lib.cstrings(fens), n, ptr(out)), "m0_encode_fens_nhwc")
    return out


def planes_to_nhwc(planes: np.ndarray) -> np.ndarray:
    """f32 [n,19,8,8] -> the network's input layout f16 [n,64,32] (zero-padded channels)."""
    p = np.asarray(planes, np.float32)
    out = np.zeros((p.shape[0], 64, 32), np.float16)
    out[:, :, :19] = p.reshape(p.shape[0], 19, 64).transpose(0, 2, 1).astype(np.float16)
    return out


def ssl_targets_fens(fens, device_index: int = 0) -> dict:
    """create_enhanced_ssl_targets (ssl_algorithms.py:519-543) on the device for a list of FENs."""
    L = _lib.lib()
    n = len(fens)
    out = np.empty((n, 17, 8, 8), np.float32)
    _lib.check(L.m0_ssl_targets_fens(int(device_index), _lib.cstrings(fens), n, ptr(out)), "m0_ssl_targets_fens")
    return _lib.split_ssl(out)


def ssl_targets_planes(planes, device_index: int = 0) -> dict:
    """The same targets taken from stored planes f32 [n,19,8,8] (m0_ssl_targets_planes): the maps of ssl_targets_fens plus
    "status" i32 [n], 0 or 1 for a row whose planes 0-12 do not describe a board (its maps are zero)."""
    a = np.ascontiguousarray(planes, dtype=np.float32)
    if a.ndim != 4 or a.shape[1:] != (19, 8, 8):
        raise ValueError(f"expected planes [n,19,8,8], got {a.shape}")
    n = a.shape[0]
    out = np.zeros((n, 17, 8, 8), np.float32)
    status = np.zeros(n, np.int32)
    _lib.check(_lib.lib().m0_ssl_targets_planes(int(device_index), ptr(a), n, ptr(out), ptr(status)), "m0_ssl_targets_planes")
    return dict(_lib.split_ssl(out), status=status)


class ArenaEngine(SelfplayEngine):
    """Evaluation match engine (m0_arena_create): game i has `backend_a` as White when i is even; step / poll / stats as
    SelfplayEngine.  Records carry `played`, `result` (White's point of view) and `moves`, and `start_fen` when the game began
    from an opening-book position (`set_openings`; `cfg.arena_paired_openings` pairs games 2k and 2k+1 on one position).
    `cfg.arena_eval_cache` gives each network an evaluation cache per game (`cfg.eval_cache` is ignored here)."""

    def __init__(self, backend_a, backend_b, cfg: SelfplayCfg):
        self.backend_b = backend_b
        self._open(backend_a, cfg, "m0_arena_create", backend_a.handle, backend_b.handle, C.byref(cfg))


class ArenaExtEngine(SelfplayEngine):
    """Match engine without networks (m0_arena_create_ext): two external evaluators behind the infer_np seam."""

    def __init__(self, cfg: SelfplayCfg):
        self._open(None, cfg, "m0_arena_create_ext", C.byref(cfg))

    def arena_ext_select(self):
        pa, pb = self._select(self._L.m0_arena_ext_select, "m0_arena_ext_select", regions=2)
        return pa, pb

    def arena_ext_expand(self, lg_a, v_a, lg_b, v_b) -> None:
        self._expand(self._L.m0_arena_ext_expand, "m0_arena_ext_expand", (lg_a, v_a), (lg_b, v_b))


ANALYSIS_STATUS = {0: "ok", 1: "checkmate", 2: "stalemate", 3: "tablebase"}


def analysis_result_to_dict(r: AnalysisResult, proof: Optional[ProofLines] = None) -> dict:
    """One m0_analysis_result as plain Python: moves and principal variations as UCI strings.  A result from the endgame
    tablebases (status "tablebase") also carries `dtm`, the root's distance to mate in plies (0: a draw), and per line the
    `dtm` of the position after its move; its root_q is the exact wdl.  With `proof` (an engine in the proof search,
    m0_analysis_last_proof) it carries `proof` (a name of PROOF_STATES) and `proof_plies` of the root and, per line, of the
    root's side to move after that line's move."""
    from_tb = int(r.status) == 3
    lines = []
    for i in range(r.nlines):
        ln = r.lines[i]
        lines.append({"move": move_to_uci(int(ln.move)), "policy_index": int(ln.policy_index), "visits": int(ln.visits),
                      "prior": float(ln.prior), "q": float(ln.q),
                      "pv": [move_to_uci(int(ln.pv[k])) for k in range(ln.pv_len)]})
        if from_tb:
            lines[-1]["dtm"] = int(r.line_dtm[i])
    out = {"id": int(r.id), "status": ANALYSIS_STATUS.get(int(r.status), str(int(r.status))), "nlegal": int(r.nlegal),
           "overflow": bool(r.overflow), "sims": int(r.sims), "root_n": int(r.root_n), "evals": int(r.evals),
           "value": float(r.value), "root_q": float(r.root_q), "lines": lines}
    if from_tb:
        out["dtm"] = int(r.tb_dtm)
    if proof is not None:
        out["proof"], out["proof_plies"] = PROOF_STATES[int(proof.proof)], int(proof.proof_plies)
        for i, ln in enumerate(lines):
            ln["proof"], ln["proof_plies"] = PROOF_STATES[int(proof.line_proof[i])], int(proof.line_proof_plies[i])
    return out


class AnalysisEngine(SelfplayEngine):
    """Batched position analysis on the engine's own network (m0_analysis_create): `submit` positions, `step`, `poll` the
    results (completion order).  stats / close as SelfplayEngine; the game and split-search methods are refused by the library.
    matrix0_amd.analysis.Analyzer is the interface built on it."""

    def __init__(self, backend, cfg: SelfplayCfg, *, multipv: int = 1, pv_len: int = 8, dirichlet: bool = False):
        self.opts = AnalysisOpts(int(multipv), int(pv_len), int(bool(dirichlet)))
        if backend is not None:
            self._open(backend, cfg, "m0_analysis_create", backend.handle, C.byref(cfg), C.byref(self.opts))
        else:                                                  # AnalysisExtEngine
            self._open(None, cfg, "m0_analysis_create_ext", C.byref(cfg), C.byref(self.opts))

    def submit(self, fen: str, ucis=(), sims: int = 0, id: int = 0, keep: bool = False) -> None:
        """keep=True (sims > 0): the search's tree stays in its slot when it is answered, held under `id`, for
        `continue_search` / `release`."""
        ucis = list(ucis)
        if keep:
            _lib.check(self._L.m0_analysis_submit_keep(self._h, fen.encode(), _lib.cstrings(ucis), len(ucis), int(sims), int(id)),
                       "m0_analysis_submit_keep")
            return
        _lib.check(self._L.m0_analysis_submit(self._h, fen.encode(), _lib.cstrings(ucis), len(ucis), int(sims), int(id)),
                   "m0_analysis_submit")

    # ---- live searches (include/m0_analysis_live.h)
    def peek_raw(self, id: int) -> Optional[AnalysisResult]:
        r = AnalysisResult()
        rc = _lib.count(self._L.m0_analysis_peek(self._h, int(id), C.byref(r)), "m0_analysis_peek")
        return r if rc == 1 else None

    def _last_proof(self) -> Optional[ProofLines]:
        """The proofs of the result handed out last, on an engine in the proof search (set_proof); None otherwise."""
        if not getattr(self, "proof", False):
            return None
        p = ProofLines()
        _lib.check(self._L.m0_analysis_last_proof(self._h, C.byref(p)), "m0_analysis_last_proof")
        return p

    def peek(self, id: int) -> Optional[dict]:
        """The result of the running search `id` as it stands (`sims`: simulations done so far), None while it is queued.
        Reads only."""
        r = self.peek_raw(id)
        return None if r is None else analysis_result_to_dict(r, self._last_proof())

    def stop(self, id: int) -> None:
        """Answer the search `id` now (its result, equal to a peek, comes through `poll`); a queued one is answered with zeros."""
        _lib.check(self._L.m0_analysis_stop(self._h, int(id)), "m0_analysis_stop")

    def continue_search(self, held_id: int, ucis=(), sims: int = 1, id: int = 0, keep: bool = False) -> int:
        """Search the position of the held search `held_id` plus the moves `ucis` (at most 8) in its slot, under `id`: the
        subtree behind the moves is kept.  Returns the visits the kept root carries, 0 when a fresh tree had to be started
        (or the position was answered without a search)."""
        ucis = list(ucis)
        reused = C.c_int32(0)
        _lib.check(self._L.m0_analysis_continue(self._h, int(held_id), _lib.cstrings(ucis), len(ucis), int(sims), int(id),
                                                int(bool(keep)), C.byref(reused)), "m0_analysis_continue")
        return int(reused.value)

    def release(self, id: int) -> None:
        _lib.check(self._L.m0_analysis_release(self._h, int(id)), "m0_analysis_release")

    def held(self) -> int:
        return _lib.count(self._L.m0_analysis_held(self._h), "m0_analysis_held")

    def step(self, steps: int = 1) -> None:
        _lib.check(self._L.m0_analysis_step(self._h, int(steps)), "m0_analysis_step")

    def pending(self) -> int:
        return _lib.count(self._L.m0_analysis_pending(self._h), "m0_analysis_pending")

    def submit_planes(self, planes, mask=None, sims: int = 0, ids=None):
        """Stored rows straight into the queue: planes f32 [n,19,8,8] and, optionally, their legal masks [n,4672] are decoded on
        the engine's device (encoding.decode_planes says what is recovered) and every row of status 0 is queued under ids[i]
        (default i) as `submit(fen of the row)` would queue it -- same result, bit for bit; the planes hold no history.  Rows of
        another status are not queued and nothing is answered for them.  Returns (status i32 [n], flags i32 [n])."""
        pl = np.ascontiguousarray(planes, dtype=np.float32)
        if pl.ndim != 4 or pl.shape[1:] != (19, 8, 8):
            raise ValueError("planes must be [n,19,8,8]")
        n = int(pl.shape[0])
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask).reshape(n, -1), dtype=np.uint8)
            if mk.shape != (n, 4672):
                raise ValueError("mask must be [n,4672]")
        idv = None
        if ids is not None:
            idv = np.ascontiguousarray(ids, dtype=np.int64)
            if idv.shape != (n,):
                raise ValueError("one id per row")
        status, flags = np.zeros((n,), np.int32), np.zeros((n,), np.int32)
        if n:
            _lib.check(self._L.m0_analysis_submit_planes(self._h, ptr(pl), ptr(mk), n, int(sims), ptr(idv), ptr(status),
                                                         ptr(flags)),
                       "m0_analysis_submit_planes")
        return status, flags

    def keep_visits(self, on: bool = True) -> None:
        """With keeping on, every harvested search also brings every root child's (policy index, visits) to the host, for
        `poll(visits=True)`: what a policy target needs.  Off (the default) nothing extra is launched or copied."""
        _lib.check(self._L.m0_analysis_keep_visits(self._h, int(bool(on))), "m0_analysis_keep_visits")

    def poll(self, visits: bool = False) -> Optional[dict]:
        """One answered position, or None.  visits=True adds `policy_idx` and `visits` (i32 arrays, the root's children in
        move-generation order; empty for results answered on the host, policy-mode results and searches harvested while
        `keep_visits` was off)."""
        r = AnalysisResult()
        if not visits:
            rc = _lib.count(self._L.m0_analysis_poll(self._h, C.byref(r)), "m0_analysis_poll")
            return analysis_result_to_dict(r, self._last_proof()) if rc == 1 else None
        k = C.c_int32(0)
        idx, cn = np.zeros(256, np.int32), np.zeros(256, np.int32)
        rc = self._L.m0_analysis_poll_visits(self._h, C.byref(r), C.byref(k), ptr(idx), ptr(cn), 256)
        if _lib.count(rc, "m0_analysis_poll_visits") != 1:
            return None
        out = analysis_result_to_dict(r, self._last_proof())
        out["policy_idx"], out["visits"] = idx[: k.value].copy(), cn[: k.value].copy()
        return out


class AnalysisExtEngine(AnalysisEngine):
    """The same engine without a network (m0_analysis_create_ext): `step(infer_np)` runs select, the caller's evaluator on the
    leaf planes and expand.  Search only (no policy mode)."""

    def __init__(self, cfg: SelfplayCfg, **opts):
        super().__init__(None, cfg, **opts)

    def step(self, infer_np, steps: int = 1) -> None:
        for _ in range(int(steps)):
            if self.pending() == 0:
                break
            planes = self._select(self._L.m0_analysis_ext_select, "m0_analysis_ext_select")[0]
            answer = infer_np(planes) if len(planes) else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
            self._expand(self._L.m0_analysis_ext_expand, "m0_analysis_ext_expand", answer)


def arena_choose_move(visits, temp: float, ply: int, temp_plies: int, u: float) -> int:
    """arena.py:73-106 (host_rules.h::arena_choose_move)."""
    L = _lib.lib()
    v = np.ascontiguousarray(visits, dtype=np.int32)
    return int(L.m0_arena_choose_move(ptr(v), int(len(v)), float(temp), int(ply), int(temp_plies), float(u)))


def san_legal(fen: str):
    """[(uci, san)] of the legal moves of `fen` in legal_moves order (python-chess Board.san semantics)."""
    L = _lib.lib()
    mv = np.zeros(256, np.uint16)
    san = C.create_string_buffer(256 * 8)
    n = c_int(0)
    _lib.check(L.m0_san_legal_fen(fen.encode(), ptr(mv), san, C.byref(n)), "m0_san_legal_fen")
    raw = san.raw
    return [(move_to_uci(int(mv[i])), raw[8 * i: 8 * i + 8].split(b"\0", 1)[0].decode()) for i in range(n.value)]


def fen_after(fen: str, ucis) -> str:
    """Board.fen() after pushing the legal moves `ucis` on `fen` (python-chess semantics); ValueError for an illegal move."""
    L = _lib.lib()
    ucis = list(ucis)
    buf = C.create_string_buffer(128)
    rc = L.m0_fen_after(fen.encode(), _lib.cstrings(ucis), len(ucis), buf, len(buf))
    if rc == -1:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "m0_fen_after")
    return buf.value.decode()


def san_game(moves_raw, fen: Optional[str] = None) -> str:
    """Movetext '1. e4 e5 2. Nf3 ...' of a game (moves as in a record's `played_raw`) from the start position or from `fen`
    (a record's `start_fen`); the move numbers follow the FEN, '12... Nf6 13. e4' when Black moves first."""
    L = _lib.lib()
    mv = np.ascontiguousarray(moves_raw, dtype=np.uint16)
    buf = C.create_string_buffer(16 * (len(mv) + 4))
    if fen is None:
        rc = L.m0_san_game(ptr(mv), int(len(mv)), buf, len(buf))
    else:
        rc = L.m0_san_game_fen(fen.encode(), ptr(mv), int(len(mv)), buf, len(buf))
    _lib.count(rc, "m0_san_game")
    return buf.value.decode().strip()
