"""attn_block_kernel's pair loop: a workgroup walks the board pairs b, b + grid, ... and every pair but its first reaches
LDS through registers, requested under the epilogue of the pair before.  Which workgroup handles a pair, and in which
pass, must not show in the result: every loop shape below gives the same bits as one workgroup per pair (no pass but the
first, the schedule without the loop).  M0_ATTN_GRID caps the grid; like every kernel switch it is read when a network is
created, so each shape gets a backend of its own."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import net_ref
from tests.test_net_gpu import _r24_cfg

pytestmark = pytest.mark.gpu

DEFAULT = dict(blocks=6)
LAST_IN_TOWER = dict(blocks=3)                     # the attention block ends the tower: no second output, table not rebuilt
RELU_NO_BIAS = dict(blocks=6, attention_unmasked_mix=1.0, attention_relbias=False, activation="relu")
TRUNK_288 = dict(blocks=6, channels=288, attention_heads=18)


def _boards(B):
    g = torch.Generator().manual_seed(12)
    x = torch.zeros(B, 19, 8, 8)
    x[:, :12] = (torch.rand(B, 12, 8, 8, generator=g) < 0.08).float()
    x[:, 12:17] = (torch.rand(B, 5, 1, 1, generator=g) < 0.5).float()
    x[:, 17:] = torch.rand(B, 2, 1, 1, generator=g)
    return x.numpy()


def _backend(extra, grid):
    from matrix0_amd.backend import M0Backend
    cfg = dict(_r24_cfg(), **extra)
    sd = net_ref.random_state_dict(cfg, seed=5)
    old = os.environ.get("M0_ATTN_GRID")
    try:
        if grid is None:
            os.environ.pop("M0_ATTN_GRID", None)
        else:
            os.environ["M0_ATTN_GRID"] = str(grid)
        return M0Backend.from_state_dict(cfg, sd)
    finally:
        if old is None:
            os.environ.pop("M0_ATTN_GRID", None)
        else:
            os.environ["M0_ATTN_GRID"] = old


def _outputs(be, B):
    p, v, ssl = be.infer_np_ssl(_boards(B))
    return [p, v] + [ssl[t] for t in be.ssl_tasks]


@functools.lru_cache(maxsize=None)
def _run(extra_items, B, grid):
    """Logits, values and SSL maps of the variant at B boards with the grid capped at `grid` (None: the CU count).
    Computed once per shape and shared; nobody writes to it."""
    be = _backend(dict(extra_items), grid)
    try:
        out = _outputs(be, B)
    finally:
        be.close()
    for a in out:
        a.setflags(write=False)
    return out


def _same(extra, B, grid, ref_grid):
    got, want = _run(tuple(sorted(extra.items())), B, grid), _run(tuple(sorted(extra.items())), B, ref_grid)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (extra, B, grid, i, float(np.abs(g - w).max()))


@pytest.mark.parametrize("grid", [1, 3, 19])
def test_loop_shapes_are_bit_identical(grid):
    """37 boards = 20 pairs after padding.  Grid 20 is one pair per workgroup; grid 1 is 20 passes in one workgroup; grid 3 is
    7 / 7 / 6 passes (workgroups stop requesting a next pair at different times); grid 19 is one workgroup with two passes
    next to eighteen with one."""
    _same(DEFAULT, 37, grid, 20)


def test_single_pair():
    """Two boards: one pair, nothing to request, under a cap of 1 and under the default grid."""
    _same(DEFAULT, 2, 1, None)


@pytest.mark.parametrize("grid", [1, 3])
def test_no_second_output(grid):
    """The attention block as the last tower layer: a pass ends after the first flush and the parameter table survives it."""
    _same(LAST_IN_TOWER, 37, grid, 20)


@pytest.mark.parametrize("extra", [RELU_NO_BIAS, TRUNK_288], ids=["relu_no_bias", "trunk_288"])
def test_other_variants(extra):
    _same(extra, 37, 3, 20)


def test_repeats_are_bit_identical():
    """Race screen for the wait in front of the register-to-LDS copy: three more runs of the grid-3 shape, each bit for bit
    the shared one."""
    want = _run(tuple(sorted(DEFAULT.items())), 37, 3)
    be = _backend(DEFAULT, 3)
    try:
        for rep in range(3):
            for i, (g, w) in enumerate(zip(_outputs(be, 37), want)):
                assert np.array_equal(g, w), (rep, i)
    finally:
        be.close()
