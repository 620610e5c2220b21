"""What libm0engine.so looks like from Python: the constants, structs and functions of include/m0_engine.h, written out once.

_lib.lib() applies FUNCTIONS to the library when it loads it; the other modules import their structs and constants from here.
Nothing is generated: tests/test_abi.py reads the header and compares it with this file, name by name and field by field."""
from __future__ import annotations

import ctypes as C
from ctypes import POINTER as P

# ---- constants (#define in the header) ----
M0_OK = 0
M0_ERR_INVALID = -1
M0_ERR_UNSUPPORTED = -2
M0_ERR_HIP = -3
M0_ERR_STATE = -4
M0_ERR_NONFINITE = -5
POLICY_SIZE = 4672
ACT = {"relu": 1, "silu": 2, "leaky_relu": 3}
SSL_BITS = {"piece": 1, "threat": 2, "pin": 4, "fork": 8, "control": 16}
AN_MAX_LINES, AN_MAX_PV = 8, 16
# m0_decode_planes: per row a status ...
DECODE_STATUS = {0: "ok", 1: "piece_value", 2: "square_clash", 3: "kings", 4: "pawn_rank", 5: "not_uniform", 6: "flag_value",
                 7: "castling", 8: "counter", 9: "opponent_in_check", 10: "too_many_moves", 11: "mask_mismatch"}
DECODE_OK, DECODE_MASK_MISMATCH = 0, 11
# ... and flag bits: information, not errors
HALFMOVE_SATURATED, FULLMOVE_SATURATED, EP_FROM_MASK, NO_MASK = 1, 2, 4, 8
# m0_replay_games: per game a status and the end flags of its last position; m0_move_pattern: the kinds of an exact move
REPLAY_STATUS = {0: "ok", 1: "illegal", 2: "ambiguous", 3: "too_long"}
REPLAY_END_BITS = {"checkmate": 1, "stalemate": 2, "insufficient": 4, "white_to_move": 8}
MOVE_UCI, MOVE_RAW = 0, 1
# include/m0_score.h: how a row's support is chosen, its columns and the flag bits of the last one
SCORE_MASK = {"legal": 0, "target": 1, "none": 2}
SCORE_COLS = 8
SCORE_COLUMNS = ("policy_loss", "entropy", "value_loss", "rank", "support_mass", "support_size", "value", "flags")
SCORE_FLAGS = {"empty": 1, "nonfinite": 2, "uniform": 4}
# include/m0_ssl_score.h: a row's columns and the flag bits of the last one
SSL_SCORE_COLS = 16
SSL_SCORE_COLUMNS = ("piece_loss", "threat_loss", "pin_loss", "fork_loss", "control_loss", "piece_hits", "piece_hits_occupied",
                     "occupied", "threat_true_positive", "threat_predicted", "threat_actual", "fork_true_positive",
                     "fork_predicted", "fork_actual", "control_hits", "flags")
SSL_SCORE_FLAGS = {"planes": 1, "nonfinite": 2, "mismatch": 4}
# include/m0_augment.h: the kinds of the trainer's augmentations
AUGMENT_KINDS = {"none": 0, "hflip": 1, "rot180": 2}
# include/m0_rowpack.h: the format's version, the kinds of a packed row and of its mask
ROWPACK_VERSION = 1
ROWPACK_ROW_KINDS = {"packed": 0, "raw": 1}
ROWPACK_MASK_KINDS = {"none": 0, "legal": 1, "list": 2}

# ---- structs ----
i32, i64, u8, u16, u32, u64, f32, f64 = (C.c_int, C.c_int64, C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_float,
                                         C.c_double)
vp, cstr, cstrs = C.c_void_p, C.c_char_p, P(C.c_char_p)


class NetCfg(C.Structure):
    _fields_ = [
        ("planes", i32), ("channels", i32), ("blocks", i32), ("attention", i32),
        ("attention_heads", i32), ("attention_every_k", i32), ("attention_relbias", i32),
        ("attention_unmasked_mix", f32), ("se", i32), ("se_ratio", f32),
        ("chess_features", i32), ("piece_square_tables", i32), ("policy_factor_rank", i32),
        ("norm_group", i32), ("activation", i32), ("value_activation", i32), ("preact", i32),
        ("self_supervised", i32), ("ssl_tasks", i32), ("infer_attention_stride", i32),
    ]


class SelfplayCfg(C.Structure):
    _fields_ = [
        ("num_simulations", i32), ("cpuct", f64), ("cpuct_start", f64), ("cpuct_end", f64),
        ("cpuct_plies", i32), ("use_c_base", i32), ("cpuct_c_base", f64), ("cpuct_c_init", f64),
        ("dirichlet_alpha", f64), ("dirichlet_frac", f64), ("dirichlet_plies", i32),
        ("selection_jitter", f64), ("fpu_reduction", f64), ("draw_penalty", f64), ("virtual_loss", f64),
        ("legal_softmax", i32), ("enable_entropy_noise", i32), ("no_instant_backtrack", i32), ("value_from_white", i32),
        ("inference_batch_size", i32), ("playout_random_frac", f64),
        ("max_game_len", i32), ("min_resign_plies", i32), ("opening_random_plies", i32),
        ("resign_threshold", f64), ("resign_window", i32), ("resign_consecutive_bad", i32),
        ("resign_min_entropy", f64), ("resign_value_margin", f64),
        ("temperature_start", f64), ("temperature_end", f64), ("temperature_moves", i32),
        ("low_visit_threshold", i32),
        ("draw_enabled", i32), ("draw_min_plies", i32), ("draw_window", i32), ("draw_min_unique", i32),
        ("draw_halfmove_cap", i32), ("draw_material_threshold", i32), ("draw_stalemate", i32),
        ("concurrent_games", i32), ("total_games", i32), ("first_game_index", i32), ("arena_nodes", i32),
        ("seed", u64), ("virtual_loss_active", i32), ("ssl_in_forward", i32), ("ssl_targets", i32), ("record_games", i32),
        ("arena_mode", i32), ("arena_temp", f64), ("arena_temp_plies", i32),
        ("fresh_tree_per_move", i32), ("tt_merge", i32), ("raw_legal_priors", i32), ("max_children", i32),
        ("min_child_prior", f64), ("root_reinfer", i32), ("eval_cache", i32), ("eval_cache_entries", i32),
        ("tail_split", i32), ("arena_eval_cache", i32), ("arena_paired_openings", i32),
    ]


class SelfplayStats(C.Structure):
    _fields_ = [("steps", u64), ("evals", u64), ("sims", u64), ("plies", u64), ("games_finished", u64),
                ("games_started", u64), ("ms_total", f64), ("ms_net", f64), ("ms_tree", f64),
                ("ms_host", f64), ("arena_overflows", u64), ("ssl_dropped", u64), ("evals_cached", u64), ("active_games", i32),
                ("rows_tail", u64)]


class GameRecord(C.Structure):
    _fields_ = [("game_index", i32), ("moves", i32), ("resigned", i32), ("resigner", i32), ("draw", i32),
                ("total_plies", i32), ("result", f32), ("avg_policy_entropy", f32), ("avg_sims", f32),
                ("secs", f64), ("s", P(f32)), ("pi", P(f32)), ("z", P(f32)),
                ("legal_mask", P(u8)), ("search_values", P(f32)),
                ("played", P(u16)), ("ssl", P(f32)), ("owner", vp),
                ("start_fen", cstr)]


class AnalysisOpts(C.Structure):
    _fields_ = [("multipv", i32), ("pv_len", i32), ("dirichlet", i32)]


class AnalysisLine(C.Structure):
    _fields_ = [("move", u16), ("policy_index", i32), ("visits", i32), ("prior", f32),
                ("q", f64), ("pv_len", i32), ("pv", u16 * AN_MAX_PV)]


class AnalysisResult(C.Structure):
    _fields_ = [("id", i64), ("status", i32), ("nlegal", i32), ("overflow", i32),
                ("sims", i32), ("root_n", i32), ("evals", u64), ("value", f32), ("root_q", f64),
                ("nlines", i32), ("lines", AnalysisLine * AN_MAX_LINES),
                ("tb_dtm", i32), ("line_dtm", i32 * AN_MAX_LINES)]


class ScoreOpts(C.Structure):
    _fields_ = [("mask_mode", i32), ("label_smoothing", f32), ("value_loss", i32), ("huber_delta", f32)]


class ProofLines(C.Structure):
    _fields_ = [("proof", i32), ("proof_plies", i32), ("line_proof", i32 * AN_MAX_LINES), ("line_proof_plies", i32 * AN_MAX_LINES)]


class RowpackPos(C.Structure):
    _fields_ = [("men", u64 * 12), ("turn", u8), ("castling", u8), ("ep", u8), ("halfmove", u8), ("fullmove", u8),
                ("row_kind", u8), ("mask_kind", u8), ("reserved", u8)]


class RowpackArrays(C.Structure):
    _fields_ = [("n", i64), ("pi_n", i64), ("mask_n", i64), ("raw_n", i64), ("pos", vp), ("z", vp), ("pi_off", vp),
                ("pi_idx", vp), ("pi_val", vp), ("mask_off", vp), ("mask_idx", vp), ("raw_planes", vp), ("raw_pi", vp),
                ("raw_mask", vp)]


class GumbelCfg(C.Structure):
    _fields_ = [("max_considered", i32), ("c_visit", f64), ("c_scale", f64)]


class BudgetCfg(C.Structure):
    _fields_ = [("full_prob", f64), ("fast_simulations", i32), ("forced_k", f64), ("prune_targets", i32)]


class WeightRule(C.Structure):
    _fields_ = [("policy", f32), ("kl", f32), ("value", f32), ("floor", f32), ("cap", f32)]


STRUCTS = {"m0_net_cfg": NetCfg, "m0_selfplay_cfg": SelfplayCfg, "m0_selfplay_stats": SelfplayStats,
           "m0_game_record": GameRecord, "m0_analysis_opts": AnalysisOpts, "m0_analysis_line": AnalysisLine,
           "m0_analysis_result": AnalysisResult}

# ---- functions: name -> (restype, [argtypes]), in the header's order.  Handles and numpy buffers travel as void pointers. ----
_cfg, _res, _pi32 = P(SelfplayCfg), P(AnalysisResult), P(i32)
_select = (i32, [vp, _pi32, vp, i32])              # (engine, rows out, planes out, max_rows)
_expand = (i32, [vp, vp, vp, i32])                 # (engine, logits, values, rows)
_attach = (i32, [vp, vp, i32])                     # (engine, tablebase, max_pieces)
FUNCTIONS = {
    "m0_last_error": (cstr, []),
    "m0_version": (cstr, []),
    "m0_device_count": (i32, []),
    # network
    "m0_net_create": (vp, [P(NetCfg), i32]),
    "m0_net_destroy": (None, [vp]),
    "m0_net_load_weight": (i32, [vp, cstr, vp, i32, P(i64), i32]),
    "m0_net_finalize": (i32, [vp]),
    "m0_net_infer": (i32, [vp, vp, i32, vp, vp, vp]),
    "m0_net_tap_info": (i32, [vp, _pi32, _pi32]),
    "m0_net_infer_tap": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, vp, _pi32]),
    "m0_net_ssl_channels": (i32, [vp]),
    "m0_net_param_count": (i64, [vp]),
    "m0_net_flops_per_position": (f64, [vp, i32]),
    "m0_net_bench_forward": (i32, [vp, i32, i32, i32, P(f32)]),
    "m0_net_profile_enable": (i32, [vp, i32]),
    "m0_net_profile_get": (i32, [vp, P(f64), P(f64), P(i64), i32]),
    "m0_net_profile_get_tail": (i32, [vp, P(f64), P(i64)]),
    # weight broadcast
    "m0_dist_unique_id": (i32, [vp]),
    "m0_dist_create": (vp, [i32, i32, cstr, i32]),
    "m0_dist_destroy": (None, [vp]),
    "m0_dist_rank": (i32, [vp]),
    "m0_dist_world": (i32, [vp]),
    "m0_net_broadcast_weights": (i32, [vp, vp, i32]),
    # position-wise encoding
    "m0_encode_fens": (i32, [i32, cstrs, i32, vp, vp, vp, vp, vp]),
    "m0_encode_fens_nhwc": (i32, [i32, cstrs, i32, vp]),
    "m0_decode_move_fen": (i32, [i32, cstr, i32, cstr]),
    "m0_ssl_targets_fens": (i32, [i32, cstrs, i32, vp]),
    "m0_move_to_index_fen": (i32, [i32, cstr, cstr, _pi32]),
    # self-play and match engines
    "m0_selfplay_create": (vp, [vp, _cfg]),
    "m0_selfplay_destroy": (None, [vp]),
    "m0_selfplay_step": (i32, [vp, i32]),
    "m0_selfplay_stats_get": (i32, [vp, P(SelfplayStats)]),
    "m0_selfplay_poll": (i32, [vp, P(GameRecord)]),
    "m0_game_record_free": (None, [P(GameRecord)]),
    "m0_selfplay_running": (i32, [vp]),
    "m0_selfplay_set_openings": (i32, [vp, cstrs, i32]),
    "m0_selfplay_ext_select": _select,
    "m0_selfplay_ext_expand": _expand,
    "m0_selfplay_last_batch_nhwc": (i32, [vp, vp, i32, _pi32]),
    "m0_arena_create": (vp, [vp, vp, _cfg]),
    "m0_arena_create_ext": (vp, [_cfg]),
    "m0_arena_ext_select": (i32, [vp, _pi32, _pi32, vp, vp, i32]),
    "m0_arena_ext_expand": (i32, [vp, vp, vp, i32, vp, vp, i32]),
    "m0_arena_choose_move": (i32, [vp, i32, f64, i32, i32, f64]),
    "m0_san_legal_fen": (i32, [cstr, vp, vp, _pi32]),
    "m0_san_game": (i32, [vp, i32, cstr, i32]),
    "m0_san_game_fen": (i32, [cstr, vp, i32, cstr, i32]),
    "m0_fen_after": (i32, [cstr, cstrs, i32, cstr, i32]),
    # split-step search
    "m0_search_begin": (i32, [vp, i32, cstr, i32, i32, i32]),
    "m0_search_select": _select,
    "m0_search_expand": _expand,
    "m0_search_result": (i32, [vp, i32, _pi32, vp, vp, vp, vp, vp, P(f64), _pi32, _pi32]),
    "m0_search_advance": (i32, [vp, i32, i32, i32, i32]),
    # analysis
    "m0_analysis_create": (vp, [vp, _cfg, P(AnalysisOpts)]),
    "m0_analysis_create_ext": (vp, [_cfg, P(AnalysisOpts)]),
    "m0_analysis_submit": (i32, [vp, cstr, cstrs, i32, i32, i64]),
    "m0_analysis_step": (i32, [vp, i32]),
    "m0_analysis_ext_select": _select,
    "m0_analysis_ext_expand": _expand,
    "m0_analysis_poll": (i32, [vp, _res]),
    "m0_analysis_pending": (i32, [vp]),
    "m0_analysis_result_size": (C.c_size_t, []),
    # stored rows back to positions
    "m0_decode_planes": (i32, [i32, vp, vp, i32, vp, vp, vp, cstr, i32]),
    "m0_analysis_submit_planes": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "m0_analysis_keep_visits": (i32, [vp, i32]),
    "m0_analysis_poll_visits": (i32, [vp, _res, _pi32, vp, vp, i32]),
    # endgame tablebases
    "m0_tb_build": (vp, [i32, i32]),
    "m0_tb_build_signatures": (vp, [i32, cstrs, i32]),
    "m0_tb_load": (vp, [cstr]),
    "m0_tb_save": (i32, [vp, cstr]),
    "m0_tb_destroy": (None, [vp]),
    "m0_tb_max_men": (i32, [vp]),
    "m0_tb_table": (i32, [vp, cstr, P(P(u8)), P(C.c_size_t)]),
    "m0_tb_table_info": (i32, [vp, i32, cstr, _pi32, _pi32, P(f64)]),
    "m0_tb_probe_fens": (i32, [vp, cstrs, i32, vp, vp, vp]),
    "m0_selfplay_set_tablebase": _attach,
    "m0_selfplay_tb_adjudications": (u64, [vp]),
    "m0_selfplay_set_search_tablebase": _attach,
    "m0_selfplay_tb_leaves": (u64, [vp]),
    "m0_tb_root_lines": (i32, [vp, cstr, i32, i32, _res]),
    # host decision functions
    "m0_sample_move_index": (i32, [vp, i32, f64, f64]),
    "m0_playout_cap": (i32, [i32, f64, f64]),
    "m0_temperature_for": (f64, [i32, f64, f64, i32]),
    "m0_rules_probe": (i32, [_cfg, cstr, cstrs, i32, _pi32, P(f32)]),
    # games read back in
    "m0_san_pattern": (i32, [cstr, P(u32)]),
    "m0_move_pattern": (i32, [i32, cstr, u32, P(u32)]),
    "m0_replay_games": (i32, [i32, cstrs, vp, vp, i32, i32, i32] + [vp] * 10),
}

# ---- include/m0_analysis_live.h (which m0_engine.h includes): live searches on an analysis engine, in that header's order;
# tests/test_abi_live.py compares the two as tests/test_abi.py compares the table above with m0_engine.h ----
LIVE_FUNCTIONS = {
    "m0_analysis_submit_keep": (i32, [vp, cstr, cstrs, i32, i32, i64]),
    "m0_analysis_peek": (i32, [vp, i64, _res]),
    "m0_analysis_stop": (i32, [vp, i64]),
    "m0_analysis_continue": (i32, [vp, i64, cstrs, i32, i32, i64, i32, _pi32]),
    "m0_analysis_release": (i32, [vp, i64]),
    "m0_analysis_held": (i32, [vp]),
}

# ---- include/m0_score.h (which m0_engine.h includes too): the training loss of stored rows, in that header's order;
# tests/test_abi_score.py compares the two ----
SCORE_STRUCTS = {"m0_score_opts": ScoreOpts}
SCORE_FUNCTIONS = {
    "m0_score_rows": (i32, [i32, vp, vp, vp, vp, vp, i32, P(ScoreOpts), vp]),
    "m0_net_score": (i32, [vp, vp, vp, vp, vp, i32, P(ScoreOpts), vp]),
    "m0_score_bench": (i32, [i32, i32, i32, P(f32), P(f64)]),
}

# ---- include/m0_ssl_score.h (which m0_engine.h includes too): the SSL heads' losses of stored rows, in that header's order;
# tests/test_abi_ssl_score.py compares the two ----
SSL_SCORE_FUNCTIONS = {
    "m0_ssl_score_rows": (i32, [i32, vp, i32, vp, vp, i32, vp]),
    "m0_net_score_ssl": (i32, [vp, vp, vp, vp, vp, vp, i32, P(ScoreOpts), vp, vp]),
    "m0_ssl_targets_planes": (i32, [i32, vp, i32, vp, vp]),
    "m0_ssl_score_bench": (i32, [i32, i32, i32, i32, i32, P(f32), P(f64)]),
}

# ---- include/m0_gumbel.h (which m0_engine.h includes too): the Gumbel root search, in that header's order;
# tests/test_abi_gumbel.py compares the two ----
GUMBEL_STRUCTS = {"m0_gumbel_cfg": GumbelCfg}
GUMBEL_FUNCTIONS = {
    "m0_selfplay_set_gumbel": (i32, [vp, P(GumbelCfg)]),
    "m0_search_gumbel_result": (i32, [vp, i32, _pi32, P(f64), vp, vp, _pi32]),
    "m0_gumbel_schedule": (i32, [i32, i32, vp, vp]),
    "m0_gumbel_improve": (i32, [i32, vp, vp, vp, vp, f64, P(GumbelCfg), vp, P(f64), _pi32]),
}

# ---- include/m0_augment.h (which m0_engine.h includes too): the trainer's flip and rotate augmentations of stored rows, in that
# header's order; tests/test_abi_augment.py compares the two ----
AUGMENT_FUNCTIONS = {
    "m0_augment_rows": (i32, [i32, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
    "m0_net_score_aug": (i32, [vp, vp, vp, vp, vp, vp, i32, P(ScoreOpts), vp]),
    "m0_augment_bench": (i32, [i32, i32, i32, P(f32), P(f64)]),
}

# ---- include/m0_proof.h (which m0_engine.h includes too): the proof search, in that header's order;
# tests/test_abi_proof.py compares the two ----
PROOF_STRUCTS = {"m0_proof_lines": ProofLines}
PROOF_FUNCTIONS = {
    "m0_selfplay_set_proof": (i32, [vp, i32]),
    "m0_search_proof_result": (i32, [vp, i32, _pi32, _pi32, vp, vp, _pi32]),
    "m0_analysis_last_proof": (i32, [vp, P(ProofLines)]),
    "m0_proof_combine": (i32, [i32, vp, vp, i32, _pi32, _pi32]),
}

# ---- include/m0_rowpack.h (which m0_engine.h includes too): packed training rows, in that header's order;
# tests/test_abi_rowpack.py compares the two ----
ROWPACK_STRUCTS = {"m0_rowpack_pos": RowpackPos, "m0_rowpack_arrays": RowpackArrays}
ROWPACK_FUNCTIONS = {
    "m0_rowpack_pack": (i32, [i32, vp, vp, vp, vp, i32, P(RowpackArrays), vp]),
    "m0_rowpack_unpack": (i32, [i32, P(RowpackArrays), vp, vp, vp, vp]),
    "m0_rowpack_pack_host": (i32, [vp, vp, vp, vp, i32, P(RowpackArrays), vp]),
    "m0_rowpack_unpack_host": (i32, [P(RowpackArrays), vp, vp, vp, vp]),
    "m0_net_score_packed": (i32, [vp, P(RowpackArrays), P(ScoreOpts), vp]),
    "m0_rowpack_bench": (i32, [i32, i32, i32, P(f32), P(f32), P(f64)]),
}

# ---- include/m0_batch.h (which m0_engine.h includes too): the resident store of packed rows and its batches, in that header's
# order; tests/test_abi_batch.py compares the two ----
ROWSTORE_HOST = -1
ROWSTORE_INFO = ("rows", "first_row", "next_row", "segments", "raw_rows", "bytes")
BATCH_FUNCTIONS = {
    "m0_rowstore_create": (vp, [i32, i32]),
    "m0_rowstore_destroy": (None, [vp]),
    "m0_rowstore_append": (i32, [vp, P(RowpackArrays), P(i64)]),
    "m0_rowstore_evict": (i32, [vp, i64]),
    "m0_rowstore_info": (i32, [vp, vp]),
    "m0_rowstore_batch": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]),
    "m0_rowstore_batch_host": (i32, [P(RowpackArrays), vp, vp, i32, vp, vp, vp, vp]),
    "m0_rowstore_bench": (i32, [i32, i32, i32, vp, vp, P(f64)]),
}

# ---- include/m0_batch_ssl.h (which m0_engine.h includes behind m0_batch.h): batches with the SSL target maps of their rows, in
# that header's order; tests/test_abi_batch_ssl.py compares the two ----
BATCH_SSL_CH = 17
BATCH_SSL_FUNCTIONS = {
    "m0_rowstore_batch_ssl": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp]),
    "m0_rowstore_batch_ssl_host": (i32, [P(RowpackArrays), vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "m0_rowstore_bench_ssl": (i32, [i32, i32, i32, vp, vp, P(f64)]),
}

# ---- include/m0_batch_weighted.h (which m0_engine.h includes behind m0_batch_ssl.h): a weight per resident row, draws in proportion
# to it and the batches of the drawn rows, in that header's order; tests/test_abi_batch_weighted.py compares the two ----
WEIGHT_MAX = 65536
WEIGHT_ONE_TICKS = 1 << 24
WEIGHT_ROWS_MAX = 1 << 23
WEIGHTS_INFO = ("total_ticks", "rows_with_ticks", "sanitised_or_skipped", "degenerate_draws")
BATCH_WEIGHTED_STRUCTS = {"m0_weight_rule": WeightRule}
BATCH_WEIGHTED_FUNCTIONS = {
    "m0_rowstore_set_weights": (i32, [vp, vp, vp, i64, i32, vp]),
    "m0_rowstore_fill_weights": (i32, [vp, i64, i64, f32]),
    "m0_rowstore_scale_weights": (i32, [vp, f32]),
    "m0_rowstore_get_weights": (i32, [vp, vp, i64, vp]),
    "m0_rowstore_weights_info": (i32, [vp, vp]),
    "m0_rowstore_sample": (i32, [vp, i32, u64, u64, i32, vp, vp, i32, vp]),
    "m0_rowstore_batch_sampled": (i32, [vp, i32, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "m0_net_score_resident": (i32, [vp, vp, vp, vp, i32, P(ScoreOpts), vp, P(WeightRule)]),
    "m0_weight_from_score": (i32, [vp, i32, P(WeightRule), vp]),
}

# ---- include/m0_budget.h (which m0_engine.h includes too): the self-play budget mix, in that header's order;
# tests/test_abi_budget.py compares the two ----
BUDGET_STRUCTS = {"m0_budget_cfg": BudgetCfg}
BUDGET_FUNCTIONS = {
    "m0_selfplay_set_budget": (i32, [vp, P(BudgetCfg)]),
    "m0_search_budget_result": (i32, [vp, i32, vp, vp, _pi32]),
    "m0_game_record_budget": (i32, [P(GameRecord), P(P(u8)), P(P(i32))]),
    "m0_selfplay_budget_stats": (i32, [vp, vp]),
    "m0_budget_is_full": (i32, [u64, i32, i32, f64, _pi32]),
    "m0_budget_forced": (i32, [f64, f64, i64, P(f64)]),
    "m0_budget_prune": (i32, [i32, vp, vp, vp, i32, f64, f64, vp, vp, _pi32]),
}


def bind(L) -> list:
    """Set restype and argtypes of every function of FUNCTIONS, LIVE_FUNCTIONS, SCORE_FUNCTIONS, SSL_SCORE_FUNCTIONS,
    GUMBEL_FUNCTIONS, AUGMENT_FUNCTIONS, PROOF_FUNCTIONS, ROWPACK_FUNCTIONS, BATCH_FUNCTIONS, BATCH_SSL_FUNCTIONS,
    BATCH_WEIGHTED_FUNCTIONS and BUDGET_FUNCTIONS on the loaded library; the names it does not export."""
    missing = []
    for name, (restype, argtypes) in (list(FUNCTIONS.items()) + list(LIVE_FUNCTIONS.items()) + list(SCORE_FUNCTIONS.items()) +
                                      list(SSL_SCORE_FUNCTIONS.items()) + list(GUMBEL_FUNCTIONS.items()) +
                                      list(AUGMENT_FUNCTIONS.items()) + list(PROOF_FUNCTIONS.items()) +
                                      list(ROWPACK_FUNCTIONS.items()) + list(BATCH_FUNCTIONS.items()) +
                                      list(BATCH_SSL_FUNCTIONS.items()) + list(BATCH_WEIGHTED_FUNCTIONS.items()) +
                                      list(BUDGET_FUNCTIONS.items())):
        fn = getattr(L, name, None)
        if fn is None:
            missing.append(name)
        else:
            fn.restype, fn.argtypes = restype, argtypes
    return missing
