"""ctypes loader for libm0engine.so (the C-ABI in include/m0_engine.h).

The product path fails loudly if the HIP library is missing: there is no CPU
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

from ._abi import (ACT, M0_ERR_HIP, M0_ERR_INVALID, M0_ERR_NONFINITE, M0_ERR_STATE,  # noqa: F401
                   M0_ERR_UNSUPPORTED, M0_OK, POLICY_SIZE, SSL_BITS, AnalysisResult, NetCfg, bind)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_build", "libm0engine.so")
SSL_ORDER = list(SSL_BITS)                         # task order of the SSL outputs and of a record's target maps
SSL_CH = {"piece": 13, "threat": 1, "pin": 1, "fork": 1, "control": 3}      # channels per task of the network's SSL heads

_lib = None


class EngineLibraryMissing(RuntimeError):
    pass


def lib():
    """Load libm0engine.so once; raise if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). matrix0_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 and libm0engine.so is linked against the
    # system one with the same SONAME.  If torch comes first the loader hands libm0engine the copy already resident;
    # the other way round the process ends up with two runtimes and the second to touch the device finds none
    # (observed: build() then smoke() in one interpreter).  torch is a dependency anyway (checkpoints, distributed).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    missing = bind(L)
    if missing:
        raise EngineLibraryMissing(f"{LIB_PATH} lacks {', '.join(missing)}: it was built from an older tree; rebuild it with "
                                   "`python -c 'import __graft_entry__ as g; g.build()'`")
    # the mirror against the library's own struct
    assert C.sizeof(AnalysisResult) == L.m0_analysis_result_size(), (C.sizeof(AnalysisResult), L.m0_analysis_result_size())
    _lib = L
    return L


def device_count() -> int:
    return int(lib().m0_device_count())


def last_error() -> str:
    return (lib().m0_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "m0 call"):
    """Non-zero return -> exception types the reference's callers catch
    (mcts.py:623: TimeoutError/RuntimeError; NaN/Inf -> ValueError, tests/test_error_handling.py)."""
    if rc == M0_OK:
        return
    msg = f"{what} failed ({rc}): {last_error()}"
    if rc == M0_ERR_NONFINITE:
        raise ValueError(msg)
    if rc == M0_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def ptr(a):
    """A numpy array (or None) as the void pointer the library takes."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cstrings(seq):
    """Strings as a `const char* const*` argument (never of length 0); a None entry stays a null pointer."""
    seq = list(seq)
    return (C.c_char_p * max(1, len(seq)))(*[s.encode() if s is not None else None for s in seq])


def count(rc: int, what: str) -> int:
    """The return of a call that answers a count, or a negative error code."""
    if rc < 0:
        check(rc, what)
    return rc


def split_ssl(a):
    """SSL target maps [n,17,8,8] as the NPZ fields of selfplay/internal.py:475-482: piece [n,13,8,8], the others [n,8,8]."""
    n = SSL_CH["piece"]
    return {"piece": a[:, :n], **{t: a[:, n + k] for k, t in enumerate(SSL_ORDER[1:])}}


def net_cfg_from_dict(d: dict) -> NetCfg:
    """NetConfig dict (config.yaml `model:` section, resnet.py:247-282 defaults) -> C struct."""
    g = d.get
    tasks = g("ssl_tasks", ["piece"]) if g("self_supervised", True) else []
    bits = 0
    for t in tasks:
        bits |= SSL_BITS.get(t, 0)
    c = NetCfg()
    c.planes = int(g("planes", 19)); c.channels = int(g("channels", 160)); c.blocks = int(g("blocks", 14))
    c.attention = int(bool(g("attention", True))); c.attention_heads = int(g("attention_heads", 8))
    c.attention_every_k = int(g("attention_every_k", 3)); c.attention_relbias = int(bool(g("attention_relbias", True)))
    c.attention_unmasked_mix = float(g("attention_unmasked_mix", 0.2))
    c.se = int(bool(g("se", True))); c.se_ratio = float(g("se_ratio", 0.25))
    c.chess_features = int(bool(g("chess_features", True))); c.piece_square_tables = int(bool(g("piece_square_tables", True)))
    c.policy_factor_rank = int(g("policy_factor_rank", 0))
    c.norm_group = 1 if g("norm", "batch") == "group" else 0
    c.activation = ACT.get(g("activation", "relu"), 1)
    c.value_activation = ACT.get(g("value_activation", "silu"), 1)
    c.preact = int(bool(g("preact", False)))
    c.self_supervised = int(bool(g("self_supervised", True))); c.ssl_tasks = bits
    c.infer_attention_stride = max(1, int(g("infer_attention_stride", 1)))
    if int(g("policy_size", 4672)) != 4672:
        raise ValueError("Unsupported policy_size; only the legacy 4672 mapping exists (resnet.py:302-306)")
    return c
