"""The weight layouts of csrc/net_pack.h on the CPU: the header built for the host with int32 elements
(tests/host_shim/pack_shim.cpp).  Every input tensor holds its elements' own flat index + 1, so a packed buffer is a map from
position to source element and 0 is padding.  For every layout: (a) every source element appears exactly once, (b) every other
position is 0, (c) the element the consuming kernel reads for (row, k, tap) is the right one -- the expected position is written
here from the kernels' addressing (DESIGN.md section 4 and the header comments of conv_gemm.hip, conv_big.hip, conv_zs.hip,
attn_block.hip and conv_zs_tail.h), as byte offsets into the kernel's LDS image, not taken from the header under test.  And the
same cases as a stand-alone program under -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from tests import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL, BIG_1X1, BIG_3X3 = 0, 1, 2


def ids(n, first=1):
    return np.arange(first, first + n, dtype=np.int32)


def call(fn, length, *args):
    """fn(*args, out, capacity) into an exactly-sized buffer; the function must report that length."""
    out = np.full(length, -1, np.int32)
    assert getattr(host_shim.load("pack"), fn)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args],
                                                out.ctypes.data, length) == length
    return out


def check_map(packed, pos, src):
    """packed[pos[i]] == src[i] for every source element (c), each exactly once (a), and 0 everywhere else (b)."""
    pos, src = np.asarray(pos).ravel(), np.asarray(src).ravel()
    assert pos.min() >= 0 and pos.max() < len(packed)
    assert np.array_equal(packed[pos], src)                                    # (c)
    assert np.array_equal(np.sort(packed[packed != 0]), np.sort(src))          # (a)
    assert np.count_nonzero(packed) == len(src) == len(np.unique(pos))         # (b)


# ---- the kernels' addressing, in bytes (fp16 operands: element = byte offset / 2)
def chunk16(k):
    return (k % 8) * 2          # byte of element k inside its 16-byte chunk


def small_tile_byte(n, k, tap, Cin, N):
    """conv_gemm_kernel: [tap][Cin/32][N][32], 64-byte rows, no swizzle."""
    return ((tap * (Cin // 32) + k // 32) * N + n) * 64 + (k % 32) * 2


def big_1x1_byte(n, k, tap, Cin, N):
    """conv_big_kernel: one [N][64 k] stage per (tap, 64-channel chunk); 128-byte rows, 16-byte chunk index XOR (row >> 1) & 7."""
    chunk = ((k % 64) // 8) ^ ((n >> 1) & 7)
    return ((tap * (Cin // 64) + k // 64) * N + n) * 128 + chunk * 16 + chunk16(k)


def big_3x3_byte(n, k, tap, Cin, N):
    """conv_zs_kernel: K walked as (64-channel chunk, tap) in half-tiles of 32 k; per N block of 320 a half-tile is [320 channels]
    [32 k], 64-byte rows, 16-byte chunk index XOR (4 - (row >> 2)) & 3."""
    row = n % 320
    chunk = ((k % 32) // 8) ^ ((4 - ((row >> 2) & 3)) & 3)
    half_tile = (((k // 64) * 9 + tap) * (N // 320) + n // 320) * 2 + (k % 64) // 32
    return (half_tile * 320 + row) * 64 + chunk * 16 + chunk16(k)


LAYOUT_BYTE = {SMALL: small_tile_byte, BIG_1X1: big_1x1_byte, BIG_3X3: big_3x3_byte}

GEMM_CASES = {
    # name: (layout, taps, Cin_real, Cin_pad, N_real, N_pad, flatten channels, heads, padded heads)
    "stem_small_3x3_19to32_x64": (SMALL, 9, 19, 32, 64, 64, 0, 0, 0),
    "small_1x1_96_x1to32": (SMALL, 1, 96, 96, 1, 32, 0, 0, 0),
    "big_1x1_320": (BIG_1X1, 1, 320, 320, 320, 320, 0, 0, 0),
    "big_1x1_qkv_288to320_heads18to20": (BIG_1X1, 1, 288, 320, 864, 960, 0, 18, 20),
    "big_3x3_320": (BIG_3X3, 9, 320, 320, 320, 320, 0, 0, 0),
    "big_3x3_288to320": (BIG_3X3, 9, 288, 320, 288, 320, 0, 0, 0),
    "flatten64_small_4096_x40to64": (SMALL, 1, 4096, 4096, 40, 64, 64, 0, 0),
    "flatten128_big_8192_x640": (BIG_1X1, 1, 8192, 8192, 640, 640, 128, 0, 0),
}


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_layout(name):
    layout, taps, cin, cin_pad, n_real, n_pad, flat, heads, heads_pad = GEMM_CASES[name]
    w = ids(n_real * cin * taps)
    packed = call("pk_gemm", taps * cin_pad * n_pad, w, layout, taps, cin, cin_pad, n_real, n_pad, flat, heads, heads_pad)
    row, k, tap = np.meshgrid(np.arange(n_real), np.arange(cin), np.arange(taps), indexing="ij")
    if heads:           # qkv rows (type, head, dim 16): the kernels address head h of type t at ((t * padded heads) + h) * 16
        row = ((row // 16 // heads) * heads_pad + (row // 16) % heads) * 16 + row % 16
    if flat:            # the reference flattens NCHW (k = c * 64 + square); the activations here are NHWC: square * channels + c
        k = (k % 64) * flat + k // 64
    check_map(packed, LAYOUT_BYTE[layout](row, k, tap, cin_pad, n_pad) // 2, w)


@pytest.mark.parametrize("heads", [20, 18])
def test_attn_block_weight_pieces(heads):
    """attn_block_kernel: 10 groups of two heads, 7 pieces of 12 KB each -- five qkv pieces [96 cols = (q, k, v) x 2 heads x 16]
    [64 k] (128-byte rows, chunk ^ (col >> 1) & 7), two proj pieces [160 output channels][32 k = 2 heads x 16] (64-byte rows,
    chunk ^ (4 - (ch >> 2)) & 3) -- then three zero pieces."""
    C, piece = heads * 16, 12288
    wq, wp = ids(3 * C * C), ids(C * C, 1 + 3 * C * C)
    packed = call("pk_attn_weights", 73 * piece // 2, wq, wp, heads)
    t, h, d, k = np.meshgrid(np.arange(3), np.arange(heads), np.arange(16), np.arange(C), indexing="ij")      # wq [t][h][d][k]
    col, kk = t * 32 + (h % 2) * 16 + d, k % 64
    q_byte = ((h // 2) * 7 + k // 64) * piece + col * 128 + ((kk // 8) ^ ((col >> 1) & 7)) * 16 + chunk16(kk)
    oc, h, d = np.meshgrid(np.arange(C), np.arange(heads), np.arange(16), indexing="ij")                      # wp [oc][h][d]
    ch, kk = oc % 160, (h % 2) * 16 + d
    p_byte = ((h // 2) * 7 + 5 + oc // 160) * piece + ch * 64 + ((kk // 8) ^ ((4 - ((ch >> 2) & 3)) & 3)) * 16 + chunk16(kk)
    check_map(packed, np.concatenate([q_byte.ravel(), p_byte.ravel()]) // 2, np.concatenate([wq, wp]))
    assert not packed[70 * piece // 2:].any()                                  # the three pad pieces
    assert not packed[(heads // 2) * 7 * piece // 2:70 * piece // 2].any()     # groups of padded heads


@pytest.mark.parametrize("heads", [20, 18])
def test_attn_block_bias_table(heads):
    """[20 heads][2 query halves][64 lanes][32] in MFMA 32x32 accumulator order: lane = query % 32 + 32 half, element
    e = 16 kt + r holds key 32 kt + 8 (r >> 2) + 4 half + (r & 3) (AbRegs::visp, attn_block.hip)."""
    rb = ids(heads * 4096)
    packed = call("pk_attn_bias", 20 * 2 * 64 * 32, rb, heads)
    h, q, key = np.meshgrid(np.arange(heads), np.arange(64), np.arange(64), indexing="ij")
    within = key % 32
    lane = q % 32 + 32 * ((within % 8) // 4)
    e = 16 * (key // 32) + 4 * (within // 8) + within % 4
    check_map(packed, ((h * 2 + q // 32) * 64 + lane) * 32 + e, rb)
    assert not packed[heads * 2 * 64 * 32:].any()                              # padded heads
    # the split path's table: the same array, padded heads zero
    padded = call("pk_zero_padded", 20 * 4096, rb, len(rb), 20 * 4096)
    assert np.array_equal(padded[:len(rb)], rb) and not padded[len(rb):].any()


@pytest.mark.parametrize("C", [320, 288])
@pytest.mark.parametrize("hd", [8, 20, 80, 96])
def test_se_fragments(hd, C):
    """conv_zs_kernel's tail (conv_zs_tail.h): 1-KiB B-fragment pieces of v_mfma_f32_16x16x32_f16, lane (c15 = lane & 15,
    q = lane >> 4) holds column c15, k = 8 q .. 8 q + 7 of its tile: 10 x ceil(hd/16) pieces of W1 (column = hidden unit,
    k = channel), then 20 x ceil(hd/32) of W2 (column = channel, k = hidden unit)."""
    nt1, ks2 = (hd + 15) // 16, (hd + 31) // 32
    w1, w2 = ids(hd * C), ids(C * hd, 1 + hd * C)
    packed = call("pk_se_fragments", (10 * nt1 + 20 * ks2) * 512, w1, w2, hd, C)

    def frag(piece, column, k):
        return (piece * 64 + ((k % 32) // 8) * 16 + column % 16) * 8 + k % 8

    j, c = np.meshgrid(np.arange(hd), np.arange(C), indexing="ij")             # w1 [hd][C]
    pos1 = frag((j // 16) * 10 + c // 32, j, c)
    c, j = np.meshgrid(np.arange(C), np.arange(hd), indexing="ij")             # w2 [C][hd]
    pos2 = frag(10 * nt1 + (c // 16) * ks2 + j // 32, c, j)
    check_map(packed, np.concatenate([pos1.ravel(), pos2.ravel()]), np.concatenate([w1, w2]))


def test_se_transposes_and_positional_encoding():
    """se_gate_kernel reads W1 as [P][hd] and W2 as [hd][P]; the stem's epilogue reads the positional encoding as [64][P]."""
    for rows, cols, out_rows, out_cols in ((20, 288, 320, 20), (288, 20, 20, 320), (288, 64, 64, 320), (64, 64, 64, 64)):
        src = ids(rows * cols)
        t = call("pk_transposed", out_rows * out_cols, src, rows, cols, out_rows, out_cols)
        r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        check_map(t, c * out_cols + r, src)


def test_zero_padded():
    v = ids(288)
    p = call("pk_zero_padded", 320, v, 288, 320)
    assert np.array_equal(p[:288], v) and not p[288:].any()
    assert np.array_equal(call("pk_zero_padded", 64, v[:64].copy(), 64, 64), v[:64])


def test_attn_mask():
    """resnet.py:104-130: same row, same column, same diagonal, a knight's move, or adjacent."""
    got = np.zeros(64, np.uint64)
    host_shim.load("pack").pk_attn_mask(got.ctypes.data)
    rows, cols = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)
    dr, dc = rows[:, None] - rows[None, :], cols[:, None] - cols[None, :]
    knight = ((np.abs(dr) == 2) & (np.abs(dc) == 1)) | ((np.abs(dr) == 1) & (np.abs(dc) == 2))
    vis = (dr == 0) | (dc == 0) | (np.abs(dr) == np.abs(dc)) | knight | ((np.abs(dr) <= 1) & (np.abs(dc) <= 1))
    want = (vis.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    assert np.array_equal(got, want)
    assert vis.sum() == 1856 and np.array_equal(vis, vis.T)


@pytest.mark.parametrize("cin,cin_pad", [(320, 320), (288, 320), (64, 64)])
def test_joint_head(cin, cin_pad):
    """policy_head.0 (64 columns) and value_head.0 (128) as one small-tile GEMM with N = 192: chunk by chunk the two separately
    packed halves side by side, which is also the packing of the stacked weight matrix [policy rows | value rows]."""
    wa, wb = ids(64 * cin), ids(128 * cin, 1 + 64 * cin)
    a = call("pk_gemm", cin_pad * 64, wa, SMALL, 1, cin, cin_pad, 64, 64, 0, 0, 0)
    b = call("pk_gemm", cin_pad * 128, wb, SMALL, 1, cin, cin_pad, 128, 128, 0, 0, 0)
    joint = call("pk_joint_columns", cin_pad * 192, a, 64, b, 128, cin_pad)
    j = joint.reshape(cin_pad // 32, 192, 32)
    assert np.array_equal(j[:, :64], a.reshape(-1, 64, 32)) and np.array_equal(j[:, 64:], b.reshape(-1, 128, 32))
    stacked = call("pk_gemm", cin_pad * 192, np.concatenate([wa, wb]), SMALL, 1, cin, cin_pad, 192, 192, 0, 0, 0)
    assert np.array_equal(joint, stacked)


def test_sanitizer_build_over_the_same_cases():
    """The header as a stand-alone host program (its own main, never loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer: the cases above over exactly-sized buffers."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_shim"), "../_build/pack_shim_san"])
    out = subprocess.run([os.path.join(HERE, "_build", "pack_shim_san")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
    assert out.stdout.strip().endswith("\n0 failures") and out.stdout.count(" ok\n") == 25, out.stdout
