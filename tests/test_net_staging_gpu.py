"""The staging arrays of one network handle over its life (csrc/capi_net.hip): the four groups -- forward I/O, score, SSL score
and augmentation -- grow on their own, only past their capacity (64 rows at least), and a growth frees a group's arrays before it
allocates the new ones.  A handle that has grown, shrunk back to a small batch, grown another group and grown again must answer
every call with the bits a fresh handle gives for that call alone: nothing of an earlier batch is left in an array, no call
reads an array of a group it did not reserve, and no growth of one group disturbs another."""
import numpy as np
import pytest

from oracle import net_layers as nl
from tests import net_layer_cases as net_cases
from tests.test_score_gpu import SMALL, _targets

pytestmark = pytest.mark.gpu

OPTS = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)


def _rows(B):
    """(s, pi, z, mask) at B rows, drawn as tests/test_augment_gpu.py::stored draws them"""
    pi, z, mask = _targets(9, B)
    return nl.random_planes(B, 5).numpy().astype(np.float32), pi, z, mask


def _same_as_fresh_handles(make, calls):
    """every call of the sequence on one handle gives the bits of the same call on a handle that has made no other"""
    be = make()
    try:
        for k, call in enumerate(calls):
            got = call(be)
            fresh = make()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), f"call {k} of the sequence"
    finally:
        be.close()


def test_a_handles_answers_do_not_depend_on_the_calls_before_them():
    from matrix0_amd import rowpack as rp
    from matrix0_amd.backend import M0Backend
    sd = net_cases.weights(SMALL, sharp=True)
    rows = {B: _rows(B) for B in (3, 5, 65, 70, 130)}
    packed = rp.pack_rows(*rows[65], device=0)
    score = lambda B, **kw: lambda be: (be.score(*rows[B], **OPTS, **kw),)
    _same_as_fresh_handles(lambda: M0Backend.from_state_dict(SMALL, sd), [
        score(5),
        score(65),                                      # past the 64-row floor: the I/O and the score group regrow
        score(5),
        score(3, augment="hflip"),
        score(70, augment="hflip"),                     # three groups regrow
        lambda be: (be.score(packed=packed, **OPTS),),
        lambda be: be.infer_np(rows[130][0]),           # the I/O group alone regrows
        score(65),
    ])


def test_the_ssl_score_staging_grows_with_the_others():
    from matrix0_amd.backend import M0Backend
    from tests.golden_ref import load_npz
    from tests.golden_util import load_net_golden
    cfg, sd = load_net_golden("gn_silu_preact")[:2]
    x = load_npz("ssl_loss.npz")["x"].astype(np.float32)
    rows = {B: (x[np.arange(B) % len(x)],) + _targets(9, B) for B in (5, 66)}
    ssl = lambda B: lambda be: be.score_ssl(*rows[B], **OPTS)
    _same_as_fresh_handles(lambda: M0Backend.from_state_dict(cfg, sd), [
        ssl(5),
        lambda be: (be.score(*rows[5], **OPTS),),
        ssl(66),                                        # every group but the augmentation's regrows
        ssl(5),
        lambda be: (be.score(*rows[66], **OPTS),),
    ])
