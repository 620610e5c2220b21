"""The host builds of product headers that the CPU tests compare against: tests/host_shim/<name>_shim.cpp, compiled by g++ into
tests/_build/lib<name>_shim.so.  load(name) makes the library, opens it and types its functions from the table below."""
import ctypes as C
import functools
import os
import subprocess
from ctypes import POINTER as P

HERE = os.path.dirname(os.path.abspath(__file__))
i32, i64, u32, u64, vp, cstr = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p

# shim -> function -> (restype, [argtypes]); numpy buffers and ctypes arrays travel as void pointers
SHIMS = {
    "chess": {                                          # csrc/chess_core.h
        "hc_perft": (u64, [cstr, i32]),
        "hc_legal": (i32, [cstr, vp, vp]),
        "hc_legal_two_phase": (i32, [cstr, vp]),
        "hc_encode": (i32, [cstr, vp]),
        "hc_play": (i32, [cstr, P(cstr), i32, vp, vp, vp, vp]),
    },
    "planes": {                                         # csrc/planes_decode.h
        "pd_decode": (i32, [vp, vp, i32, vp, vp, vp, cstr, i32, vp, vp, vp]),
    },
    "replay": {                                         # csrc/san_match.h and a scalar replay over gen_legal
        "rs_san_pattern": (i32, [cstr, P(u32)]),
        "rs_uci_pattern": (i32, [cstr, P(u32)]),
        "rs_raw_pattern": (i32, [u32, P(u32)]),
        "rs_pattern_fields": (None, [u32, vp]),
        "rs_replay": (i32, [cstr, vp, i32, i32] + [vp] * 5 + [P(i32)] * 3),
    },
    "tb": {                                             # csrc/tb_core.h, csrc/tb.h
        "tbs_new": (vp, []),
        "tbs_free": (None, [vp]),
        "tbs_generate": (i32, [vp, cstr]),
        "tbs_table": (P(C.c_uint8), [vp, cstr, P(u64), P(i32), P(i32)]),
        "tbs_roundtrip": (i64, [cstr]),
        "tbs_locate": (i32, [cstr, P(i32), P(u32)]),
        "tbs_sig_code": (i32, [cstr]),
        "tbs_order": (i32, [cstr, cstr, i32]),
        "tbs_all_signatures": (i32, [i32, cstr, i32]),
    },
    "pack": {                                           # csrc/net_pack.h, int32 -> int32; (..., out, capacity) -> length
        "pk_gemm": (i64, [vp] + [i32] * 9 + [vp, i64]),
        "pk_attn_weights": (i64, [vp, vp, i32, vp, i64]),
        "pk_attn_bias": (i64, [vp, i32, vp, i64]),
        "pk_zero_padded": (i64, [vp, i64, i64, vp, i64]),
        "pk_transposed": (i64, [vp, i32, i32, i32, i32, vp, i64]),
        "pk_se_fragments": (i64, [vp, vp, i32, i32, vp, i64]),
        "pk_attn_mask": (None, [vp]),
        "pk_joint_columns": (i64, [vp, i32, vp, i32, i32, vp, i64]),
    },
    "check": {                                          # csrc/hip_check.h with injected hipError_t values; (..., msg, capacity)
        "hk_run": (i32, [vp, i32, vp, P(i32), vp, i32]),
        "hk_fresh": (i32, []),
        "hk_check_twice": (i32, [i32, i32, vp, i32]),
        "hk_adopt": (i32, [i32, i32, vp, i32]),
        "hk_convert": (i32, [i32, cstr, vp, i32]),
        "hk_error_string": (None, [i32, vp, i32]),
    },
}


@functools.lru_cache(maxsize=None)
def load(name):
    so = f"lib{name}_shim.so"
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_shim"), "../_build/" + so])
    lib = C.CDLL(os.path.join(HERE, "_build", so))
    for fn, (restype, argtypes) in SHIMS[name].items():
        f = getattr(lib, fn)
        f.restype, f.argtypes = restype, argtypes
    return lib
