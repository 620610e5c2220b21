"""Inference-backend seam: a drop-in for the object the reference passes as
``MCTS(cfg, model, device, inference_backend=obj)`` (azchess/mcts.py:270-283), whose only
method is ``infer_np`` (azchess/mcts.py:618-621, 1021-1023; client side
azchess/selfplay/inference.py:585-645).

    backend = M0Backend.from_state_dict(model_cfg_dict, state_dict)      # weights: torch or numpy
    policy_logits, value = backend.infer_np(np.float32[B,19,8,8])       # -> f32 [B,4672], f32 [B]

All arithmetic runs in libm0engine.so on the MI355X; torch is used only to read
checkpoints (weight I/O).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, Optional, Tuple

import numpy as np

from . import _abi, _lib


def resolve_mask_mode(pi: np.ndarray, legal_mask, mask_mode: Optional[str]) -> str:
    """The support rule of a score call: "legal" with a mask; without one the reference's rule on the arrays given
    (train.py:454-460): every row one-hot -> "none" (imported games), otherwise "target" (soft search targets)."""
    if mask_mode is not None:
        if mask_mode not in _abi.SCORE_MASK:
            raise ValueError(f"mask_mode must be one of {sorted(_abi.SCORE_MASK)} or None, got {mask_mode!r}")
        return mask_mode
    if legal_mask is not None:
        return "legal"
    return "none" if bool(((np.asarray(pi) > 0).sum(axis=1) == 1).all()) else "target"


class NonFiniteScore(ValueError):
    """M0Backend.score met non-finite network outputs; `rows` holds the columns all the same (flag 2 marks the rows), and after
    score_ssl `ssl_rows` holds the SSL columns."""

    def __init__(self, msg: str, rows: np.ndarray, ssl_rows: Optional[np.ndarray] = None):
        super().__init__(msg)
        self.rows = rows
        self.ssl_rows = ssl_rows


def score_opts(mask_mode: str, label_smoothing: float, value_loss: str, huber_delta: float) -> "_abi.ScoreOpts":
    if value_loss not in ("mse", "huber"):
        raise ValueError(f"value_loss must be 'mse' or 'huber', got {value_loss!r}")
    return _abi.ScoreOpts(_abi.SCORE_MASK[mask_mode], float(label_smoothing), int(value_loss == "huber"), float(huber_delta))


class M0Backend:
    def __init__(self, model_cfg: dict, device_index: int = 0):
        self._L = _lib.lib()
        self.model_cfg = dict(model_cfg)
        self._cfg = _lib.net_cfg_from_dict(model_cfg)
        self._h = self._L.m0_net_create(C.byref(self._cfg), int(device_index))
        if not self._h:
            raise RuntimeError(f"m0_net_create failed: {_lib.last_error()}")
        self._finalized = False
        self.ssl_tasks = [t for t in _lib.SSL_ORDER if self._cfg.ssl_tasks & _lib.SSL_BITS[t]] \
            if self._cfg.self_supervised else []

    # ---- weight I/O -------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, "np.ndarray"]) -> None:
        """Feed every state-dict entry (reference key names) then repack.  Accepts torch tensors
        or numpy arrays.  Mirrors load_state_dict(strict=False): unknown keys are ignored by
        the engine; missing keys raise at finalize (the reference silently re-initialises them,
        resnet.py:1418-1440 -- a self-play run on half-random weights is not something to
        reproduce silently)."""
        for k, v in sd.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().float().numpy()
            a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
            shape = (C.c_int64 * max(1, a.ndim))(*a.shape)
            _lib.check(self._L.m0_net_load_weight(self._h, k.encode(), _lib.ptr(a), 0, shape, a.ndim),
                       f"m0_net_load_weight({k})")
        _lib.check(self._L.m0_net_finalize(self._h), "m0_net_finalize")
        self._finalized = True

    @classmethod
    def from_state_dict(cls, model_cfg: dict, sd, device_index: int = 0) -> "M0Backend":
        b = cls(model_cfg, device_index)
        b.load_state_dict(sd)
        return b

    @classmethod
    def from_checkpoint(cls, model_cfg: dict, ckpt_path: str, device_index: int = 0) -> "M0Backend":
        """Checkpoint dict layout of the reference: prefer model_ema, then model, then
        model_state_dict, then the raw dict (selfplay/internal.py:172-174, orchestrator.py:373-388)."""
        import torch  # weight I/O only
        state = torch.load(ckpt_path, map_location="cpu", weights_only=False)
        sd = state
        if isinstance(state, dict):
            for key in ("model_ema", "model", "model_state_dict"):
                if key in state and isinstance(state[key], dict):
                    sd = state[key]
                    break
        return cls.from_state_dict(model_cfg, sd, device_index)

    # ---- the seam ---------------------------------------------------------------------------
    def infer_np(self, arr: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        p, v, _ = self._infer(arr, False)
        return p, v

    def infer_np_ssl(self, arr: np.ndarray):
        """(policy, value, {task: f32 [B,ch,8,8]}) -- forward(return_ssl=True), resnet.py:738-745."""
        return self._infer(arr, True)

    def tap_info(self) -> Tuple[int, int]:
        """(steps of a forward the trunk tap can be armed at, trunk width in memory) -- m0_net_tap_info."""
        steps, width = C.c_int(0), C.c_int(0)
        _lib.check(self._L.m0_net_tap_info(self._h, C.byref(steps), C.byref(width)), "m0_net_tap_info")
        return steps.value, width.value

    def infer_tap(self, arr: np.ndarray, step: int):
        """infer_np_ssl with the trunk tap armed at `step` (m0_net_infer_tap): (policy, value, ssl, stream, second), the last
        two f32 [B,64,width]: the residual stream after that step and the next residual block's pre-activated input, or None
        where the step wrote none."""
        return self._infer(arr, True, int(step))

    def _infer(self, arr: np.ndarray, want_ssl: bool, tap_step: Optional[int] = None):
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        a = np.asarray(arr)
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[1:] != (self._cfg.planes, 8, 8):
            raise ValueError(f"expected input [B,{self._cfg.planes},8,8], got {a.shape}")  # mcts.py:1030-1040
        a = np.ascontiguousarray(a, dtype=np.float32)
        B = a.shape[0]
        pol = np.empty((B, _lib.POLICY_SIZE), dtype=np.float32)
        val = np.empty((B,), dtype=np.float32)
        sslc = self._L.m0_net_ssl_channels(self._h)
        ssl = np.empty((B, sslc, 8, 8), dtype=np.float32) if (want_ssl and sslc > 0) else None
        if tap_step is None:
            _lib.check(self._L.m0_net_infer(self._h, _lib.ptr(a), B, _lib.ptr(pol), _lib.ptr(val), _lib.ptr(ssl)), "m0_net_infer")
        else:
            width = self.tap_info()[1]
            stream = np.empty((B, 64, width), dtype=np.float32)
            second = np.empty((B, 64, width), dtype=np.float32)
            has_second = C.c_int(0)
            _lib.check(self._L.m0_net_infer_tap(self._h, _lib.ptr(a), B, tap_step, _lib.ptr(pol), _lib.ptr(val), _lib.ptr(ssl),
                                                _lib.ptr(stream), _lib.ptr(second), C.byref(has_second)), "m0_net_infer_tap")
        out = None
        if ssl is not None:
            out, off = {}, 0
            for t in self.ssl_tasks:
                n = _lib.SSL_CH[t]
                out[t] = ssl[:, off:off + n]
                off += n
        if tap_step is not None:
            return pol, val, out, stream, (second if has_second.value else None)
        return pol, val, out

    # ---- training loss of stored rows --------------------------------------------------------
    def _score_inputs(self, s, pi, z, legal_mask):
        """the rows of a score call as contiguous arrays of the types the library reads, their shapes checked"""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        a = np.ascontiguousarray(s, dtype=np.float32)
        if a.ndim != 4 or a.shape[1:] != (self._cfg.planes, 8, 8):
            raise ValueError(f"expected input [B,{self._cfg.planes},8,8], got {a.shape}")
        B = a.shape[0]
        pi = np.ascontiguousarray(pi, dtype=np.float32)
        z = np.ascontiguousarray(np.asarray(z).reshape(-1), dtype=np.float32)
        if pi.shape != (B, _lib.POLICY_SIZE) or z.shape != (B,):
            raise ValueError(f"expected pi [{B},{_lib.POLICY_SIZE}] and z [{B}], got {pi.shape} and {z.shape}")
        if legal_mask is not None:
            legal_mask = np.ascontiguousarray(np.asarray(legal_mask).reshape(B, -1), dtype=np.uint8)
            if legal_mask.shape != pi.shape:
                raise ValueError(f"expected legal_mask [{B},{_lib.POLICY_SIZE}], got {legal_mask.shape}")
        return a, pi, z, legal_mask

    def score(self, s: Optional[np.ndarray] = None, pi: Optional[np.ndarray] = None, z: Optional[np.ndarray] = None,
              legal_mask: Optional[np.ndarray] = None, *, mask_mode: Optional[str] = None, label_smoothing: float = 0.0,
              value_loss: str = "mse", huber_delta: float = 1.0, augment=None, packed=None) -> np.ndarray:
        """f32 [B, 8]: the columns of include/m0_score.h (_abi.SCORE_COLUMNS) for the rows (s, pi, z, legal_mask) under this
        network -- forward and loss on the device (m0_net_score), only the 8 columns come back.  mask_mode: "legal", "target",
        "none", or None for resolve_mask_mode.  A non-finite network output raises NonFiniteScore (a ValueError, as infer_np
        raises; it carries the rows).  augment: None for the rows as they are; "hflip", "rot180", "none" or a u8 [B] of
        _abi.AUGMENT_KINDS' values scores every row under that trainer augmentation, transformed on the device after the one
        upload (m0_net_score_aug, include/m0_augment.h); the mode is still resolved on the rows as given.  packed: a
        rowpack.PackedRows instead of s, pi, z and legal_mask -- the packed arrays are what is uploaded, the rows are unpacked
        on the device (m0_net_score_packed, include/m0_rowpack.h) and the columns are those of the dense rows bit for bit."""
        if packed is not None:
            return self._score_packed(packed, mask_mode, label_smoothing, value_loss, huber_delta, s, pi, z, legal_mask, augment)
        if s is None or pi is None or z is None:
            raise ValueError("score needs s, pi and z, or packed rows")
        dense = self._score_inputs(s, pi, z, legal_mask)
        mode = resolve_mask_mode(dense[1], dense[3], mask_mode)
        call = "m0_net_score" if augment is None else "m0_net_score_aug"
        return self._net_score(call, len(dense[0]), (mode, label_smoothing, value_loss, huber_delta), dense, augment=augment)[0]

    def score_resident(self, store, ids, kinds=None, rule=None, *, mask_mode: Optional[str] = None, label_smoothing: float = 0.0,
                       value_loss: str = "mse", huber_delta: float = 1.0) -> np.ndarray:
        """f32 [B, 8]: score()'s columns for rows that are resident in a device_replay.DeviceReplay on this network's device --
        the store's batch kernel fills the network's staging buffers from ids (and kinds: None, one kind or u8 [B], as
        store.batch takes them), nothing but the ids goes up and the columns come back (m0_net_score_resident,
        include/m0_batch_weighted.h).  The columns are those of score(packed=...) for the same rows bit for bit.  rule: a
        device_replay.weight_rule(...); every scored row then gets the rule's weight of its columns in the store, on the device.
        mask_mode None: "legal" for a store with masks, "target" for one without."""
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        ids, kinds = store._ids_kinds(ids, kinds)
        mode = resolve_mask_mode(None, None, mask_mode or ("legal" if store.with_mask else "target"))
        opts = score_opts(mode, label_smoothing, value_loss, huber_delta)
        rows = np.empty((len(ids), _abi.SCORE_COLS), dtype=np.float32)
        rc = self._L.m0_net_score_resident(self._h, store._h, _lib.ptr(ids), _lib.ptr(kinds), len(ids), C.byref(opts), _lib.ptr(rows),
                                           C.byref(rule) if rule is not None else None)
        if rc == _lib.M0_ERR_NONFINITE:
            raise NonFiniteScore(f"m0_net_score_resident failed ({rc}): {_lib.last_error()}", rows)
        _lib.check(rc, "m0_net_score_resident")
        return rows

    def _net_score(self, call: str, B: int, loss: tuple, dense=(), *, augment=None, packed=None, ssl_targets=None):
        """The one way into m0_net_score and its _aug, _packed and _ssl variants: the options (loss: score_opts' arguments), the
        output arrays [rows] or [rows, ssl_rows], the call, and NonFiniteScore with those arrays or _lib.check for its answer."""
        opts = score_opts(*loss)
        out = [np.empty((B, _abi.SCORE_COLS), dtype=np.float32)]
        if call == "m0_net_score_packed":
            arrays = packed.c_arrays()
            args = [C.byref(arrays)]
        else:
            args = [_lib.ptr(x) for x in dense]
            if call == "m0_net_score_aug":
                from .encoding import augment_kinds
                kinds = augment_kinds(augment, B)
                args.append(_lib.ptr(kinds))
            elif call == "m0_net_score_ssl":
                out.append(np.empty((B, _abi.SSL_SCORE_COLS), dtype=np.float32))
                args.append(_lib.ptr(ssl_targets))
            args.append(B)
        rc = getattr(self._L, call)(self._h, *args, C.byref(opts), *[_lib.ptr(x) for x in out])
        if rc == _lib.M0_ERR_NONFINITE:
            raise NonFiniteScore(f"{call} failed ({rc}): {_lib.last_error()}", *out)
        _lib.check(rc, call)
        return out

    def _score_packed(self, packed, mask_mode, label_smoothing, value_loss, huber_delta, *dense) -> np.ndarray:
        if not self._finalized:
            raise RuntimeError("weights not loaded")
        if any(d is not None for d in dense):
            raise ValueError("packed rows come instead of s, pi, z and legal_mask, and are not augmented")
        from .rowpack import mask_mode_of
        mode = resolve_mask_mode(None, None, mask_mode_of(packed, mask_mode))
        return self._net_score("m0_net_score_packed", packed.n, (mode, label_smoothing, value_loss, huber_delta), packed=packed)[0]

    def score_ssl(self, s: np.ndarray, pi: np.ndarray, z: np.ndarray, legal_mask: Optional[np.ndarray] = None,
                  ssl_targets: Optional[np.ndarray] = None, *, mask_mode: Optional[str] = None, label_smoothing: float = 0.0,
                  value_loss: str = "mse", huber_delta: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
        """(rows f32 [B, 8], ssl_rows f32 [B, 16]): `rows` as score gives them, `ssl_rows` the columns of include/m0_ssl_score.h
        (_abi.SSL_SCORE_COLUMNS) for this network's SSL tasks -- one forward with the heads, both losses on the device
        (m0_net_score_ssl).  ssl_targets f32 [B,17,8,8] (or [B,17,64]: piece one-hot, threat, pin, fork, control) as stored with
        the rows, or None to take the targets from the planes.  A network without SSL heads is a ValueError; non-finite
        outputs raise NonFiniteScore, which then carries `rows` and `ssl_rows`."""
        dense = self._score_inputs(s, pi, z, legal_mask)
        B = len(dense[0])
        if ssl_targets is not None:
            ssl_targets = np.ascontiguousarray(ssl_targets, dtype=np.float32)
            if ssl_targets.size != B * 17 * 64 or ssl_targets.shape[:2] != (B, 17):
                raise ValueError(f"expected ssl_targets [{B},17,8,8], got {ssl_targets.shape}")
        loss = (resolve_mask_mode(dense[1], dense[3], mask_mode), label_smoothing, value_loss, huber_delta)
        return tuple(self._net_score("m0_net_score_ssl", B, loss, dense, ssl_targets=ssl_targets))

    # ---- measurement helpers ----------------------------------------------------------------
    def param_count(self) -> int:
        return int(self._L.m0_net_param_count(self._h))

    def flops_per_position(self, with_ssl: bool = False) -> float:
        return float(self._L.m0_net_flops_per_position(self._h, int(with_ssl)))

    def bench_forward(self, batch: int, iters: int, with_ssl: bool = False) -> float:
        ms = C.c_float(0)
        _lib.check(self._L.m0_net_bench_forward(self._h, int(batch), int(iters), int(with_ssl), C.byref(ms)),
                   "m0_net_bench_forward")
        return float(ms.value)

    def profile_enable(self, on: bool = True) -> None:
        _lib.check(self._L.m0_net_profile_enable(self._h, int(on)), "m0_net_profile_enable")

    def profile_get(self, reset: bool = False):
        """(ms, algorithmic FLOP, launches) of the 3x3 conv kernel, HIP events on its launch stream."""
        ms, fl, n = C.c_double(0), C.c_double(0), C.c_int64(0)
        tms, tn = C.c_double(0), C.c_int64(0)
        _lib.check(self._L.m0_net_profile_get_tail(self._h, C.byref(tms), C.byref(tn)), "m0_net_profile_get_tail")
        self.last_tail_profile = (tms.value, tn.value)      # (ms, launches) of the convs with a fused block tail
        _lib.check(self._L.m0_net_profile_get(self._h, C.byref(ms), C.byref(fl), C.byref(n), int(reset)), "m0_net_profile_get")
        return ms.value, fl.value, n.value

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._L.m0_net_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
