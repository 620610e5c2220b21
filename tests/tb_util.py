"""Shared helpers of the tablebase tests: the independent generator (tests/tb_ref), the host shim
(tests/host_shim/tb_shim.cpp), a third, Python statement of the index contract (index -> FEN), the colour flip of a FEN, and
a writer of the cache-file format."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
THREE_MAN = ["KK", "KQK", "KRK", "KBK", "KNK", "KPK"]         # dependency order
GOLDEN = 0x9E3779B97F4A7C15


def ref_binary():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "tb_ref")])
    return os.path.join(BUILD, "tb_ref")


_ref_tables = None


def ref_tables():
    """{signature: uint8 array} of KK and the 3-man tables from the independent generator.  Generated once per checkout into
    tests/_build/tb_ref_tables (and again when the generator is newer than its output), read once per process."""
    global _ref_tables
    if _ref_tables is None:
        exe = ref_binary()
        out = os.path.join(BUILD, "tb_ref_tables")
        os.makedirs(out, exist_ok=True)
        paths = [os.path.join(out, s + ".bin") for s in THREE_MAN]
        if not all(os.path.exists(p) and os.path.getmtime(p) >= os.path.getmtime(exe) for p in paths):
            print(subprocess.check_output([exe, "gen", out] + THREE_MAN, text=True))
        _ref_tables = {s: np.fromfile(p, dtype=np.uint8) for s, p in zip(THREE_MAN, paths)}
        for s, t in _ref_tables.items():
            t.setflags(write=False)
            assert t.shape[0] == 2 * 64 ** len(s)
    return _ref_tables


def certificate(tables: dict, sig: str, seed: int, samples: int, workdir: str):
    """Run the reference's certificate check of tables[sig] (the other tables are what its moves lead into).
    Returns (exit code, {"checked", "sampled", "low_d", "violations", "skipped"}, output)."""
    for s, t in tables.items():
        np.ascontiguousarray(t, dtype=np.uint8).tofile(os.path.join(workdir, s + ".bin"))
    r = subprocess.run([ref_binary(), "cert", workdir, sig, str(seed), str(samples)], capture_output=True, text=True)
    words = r.stdout.split()
    res = {words[i]: int(words[i + 1]) for i in range(1, len(words) - 1, 2)} if r.stdout.startswith(sig + " ") else {}
    return r.returncode, res, r.stdout + r.stderr


def shim():
    return host_shim.load("tb")


def shim_table(l, h, sig):
    n, maxd, sweeps = C.c_uint64(0), C.c_int(0), C.c_int(0)
    p = l.tbs_table(h, sig.encode(), C.byref(n), C.byref(maxd), C.byref(sweeps))
    assert p, sig
    return np.ctypeslib.as_array(p, shape=(n.value,)).copy(), maxd.value, sweeps.value


# ---- the index contract once more, in Python ----
def sig_men(sig: str):
    """[(letter, is_white)] in index order: White king, White's men, Black king, Black's men."""
    k = sig.index("K", 1)
    return [(c, True) for c in sig[:k]] + [(c, False) for c in sig[k:]]


def index_to_fen(sig: str, idx: int) -> str:
    """FEN of entry idx (any entry whose men stand on distinct squares)."""
    men = sig_men(sig)
    board = [None] * 64
    for i, (c, white) in enumerate(men):
        sq = (idx >> (6 * i)) & 63
        assert board[sq] is None
        board[sq] = c if white else c.lower()
    stm = (idx >> (6 * len(men))) & 1
    rows = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for f in range(8):
            pc = board[r * 8 + f]
            if pc is None:
                gap += 1
            else:
                row += (str(gap) if gap else "") + pc
                gap = 0
        rows.append(row + (str(gap) if gap else ""))
    return "/".join(rows) + (" b" if stm else " w") + " - - 0 1"


def distinct_squares(sig: str, idx: int) -> bool:
    n = len(sig)
    return len({(idx >> (6 * i)) & 63 for i in range(n)}) == n


def flip_fen(fen: str) -> str:
    """Colours swapped, board mirrored top to bottom, side to move swapped (no castling rights, no en-passant square)."""
    parts = fen.split()
    rows = parts[0].split("/")[::-1]
    return "/".join(r.swapcase() for r in rows) + (" b " if parts[1] == "w" else " w ") + " ".join(parts[2:])


# ---- the cache file, written independently of the library ----
def _mix64(x):
    x = x.astype(np.uint64, copy=True)
    x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def checksum(table: np.ndarray) -> int:
    w = np.ascontiguousarray(table, dtype=np.uint8).view("<u8")
    with np.errstate(over="ignore"):
        k = np.arange(1, w.shape[0] + 1, dtype=np.uint64) * np.uint64(GOLDEN)
        return int(_mix64(w + k).sum(dtype=np.uint64))


def write_cache_file(path: str, tables: dict, maxd: dict = None, magic: bytes = b"M0TBASE\n", fmt: int = 1) -> None:
    """tables: {signature: uint8 array} in build order."""
    with open(path, "wb") as f:
        f.write(struct.pack("<8sII", magic, fmt, len(tables)))
        for s, t in tables.items():
            f.write(struct.pack("<8sQQii", s.encode(), t.shape[0], checksum(t), (maxd or {}).get(s, -1), 0))
        for t in tables.values():
            f.write(np.ascontiguousarray(t, dtype=np.uint8).tobytes())


def entry_wdl_dtm(v: int):
    """byte -> (wdl for the side to move, dtm in plies)"""
    if v == 0:
        return 0, 0
    d = v - 1
    return (1 if d % 2 else -1), d
