"""Endgame tablebases without a GPU: the core the build kernels are made of (matrix0_amd/csrc/tb_core.h, compiled for the host
by tests/host_shim/tb_shim.cpp, init pass and sweeps in a plain loop) against the independent generator (tests/tb_ref: the oracle's mailbox
rules, another loop), the cache file through the library's host-only loader and prober, and the worker's configuration."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import tb_util as tu
from matrix0_amd import selfplay, tablebase as tbm

# Largest d per table (plies).  Folklore: mate in at most 10 moves with the queen, 16 with the rook, 28 with the pawn; the
# loser's count is twice the moves.  KK, KBK and KNK hold no decided entry.
LARGEST_D = {"KK": -1, "KQK": 20, "KRK": 32, "KBK": -1, "KNK": -1, "KPK": 56}


@pytest.fixture(scope="module")
def shim():
    return tu.shim()


@pytest.fixture(scope="module")
def shim_tables(shim):
    h = shim.tbs_new()
    out = {}
    for s in tu.THREE_MAN:
        assert shim.tbs_generate(h, s.encode()) == 0, s
        out[s] = tu.shim_table(shim, h, s)
    shim.tbs_free(h)
    return out


def test_signatures_in_scope_and_build_order(shim):
    buf = C.create_string_buffer(1024)
    assert shim.tbs_all_signatures(3, buf, len(buf)) == 6 and set(buf.value.decode().split()) == set(tu.THREE_MAN)
    assert shim.tbs_all_signatures(4, buf, len(buf)) == 35
    sigs = buf.value.decode().split()
    assert len(set(sigs)) == 35 and "KPKP" not in sigs and sum(len(s) == 4 for s in sigs) == 29
    for s in sigs:
        assert shim.tbs_sig_code(s.encode()) >= 0, s
    for bad in ("KPKP", "KKQ", "KRKQ", "KPQK", "KQRBK", "QK", "KXK", ""):      # out of scope or not canonical
        assert shim.tbs_sig_code(bad.encode()) == -1, bad
    # KRPK promotes into KQRK, KRRK, KRBK and KRNK; captures lead down to the 3-man tables and KK; dependencies come first
    assert shim.tbs_order(b"KRPK", buf, len(buf)) == 11
    order = buf.value.decode().split()
    assert set(order) == {"KK", "KQK", "KRK", "KBK", "KNK", "KPK", "KQRK", "KRRK", "KRBK", "KRNK", "KRPK"}
    assert order[0] == "KK" and order[-1] == "KRPK" and order.index("KPK") < order.index("KQRK")
    assert shim.tbs_order(b"KQKR", buf, len(buf)) == 4 and buf.value.decode().split() == ["KK", "KQK", "KRK", "KQKR"]


@pytest.mark.parametrize("sig", ["KQK", "KPK"])
def test_index_and_decode_round_trip_over_every_valid_entry(shim, sig):
    valid = shim.tbs_roundtrip(sig.encode())
    assert valid == int((tu.ref_tables()[sig] != 255).sum())      # ... and the reference agrees on which entries are valid


def test_shim_tables_equal_the_reference_generator_byte_for_byte(shim_tables):
    ref = tu.ref_tables()
    for s in tu.THREE_MAN:
        got, maxd, sweeps = shim_tables[s]
        decided = ref[s][(ref[s] != 0) & (ref[s] != 255)]
        ref_maxd = int(decided.max()) - 1 if decided.size else -1
        print(f"{s}: largest d {maxd} (reference {ref_maxd}), {sweeps} sweeps, {decided.size} decided entries")
        assert np.array_equal(got, ref[s]), f"{s}: {int((got != ref[s]).sum())} entries differ"
        assert maxd == ref_maxd == LARGEST_D[s]
    for s in ("KK", "KBK", "KNK"):
        assert set(np.unique(ref[s]).tolist()) <= {0, 255}


@pytest.fixture(scope="module")
def cache_file(shim_tables, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tb") / "three.m0tb")
    tu.write_cache_file(path, {s: shim_tables[s][0] for s in tu.THREE_MAN}, {s: shim_tables[s][1] for s in tu.THREE_MAN})
    return path


def test_cache_file_loads_and_probes_agree_with_the_tables(cache_file, shim_tables):
    tb = tbm.Tablebase.load(cache_file)
    assert tb.max_men == 3
    assert [i["sig"] for i in tb.info()] == tu.THREE_MAN and {i["sig"]: i["max_d"] for i in tb.info()} == LARGEST_D
    rng = np.random.default_rng(7)
    for s in tu.THREE_MAN:
        table = shim_tables[s][0]
        assert np.array_equal(tb.table(s), table)
        idx = [int(i) for i in rng.integers(0, table.shape[0], size=3000) if tu.distinct_squares(s, int(i))]
        idx += [int(i) for i in np.nonzero(table == 1)[0][:50]] + [int(i) for i in np.nonzero(table == table[table != 255].max())[0][:50]]
        fens = [tu.index_to_fen(s, i) for i in idx]
        hit, wdl, dtm = tb.probe(fens)
        fhit, fwdl, fdtm = tb.probe([tu.flip_fen(f) for f in fens])      # a position and its colour flip probe alike
        assert np.array_equal(hit, fhit) and np.array_equal(wdl, fwdl) and np.array_equal(dtm, fdtm)
        for k, i in enumerate(idx):
            v = int(table[i])
            if v == 255:
                assert not hit[k], (s, i)
            else:
                assert hit[k] and (int(wdl[k]), int(dtm[k])) == tu.entry_wdl_dtm(v), (s, i, fens[k])
    # known positions: mate, mate in one, the flip with the sign for the side to move, castling rights, more men than the tables
    hit, wdl, dtm = tb.probe(["7k/5Q2/6K1/8/8/8/8/8 b - - 0 1",         # stalemate
                              "7k/6Q1/6K1/8/8/8/8/8 b - - 0 1",         # checkmate
                              "7k/8/6K1/8/8/8/8/5Q2 w - - 0 1",         # mate in one (Qf8)
                              "8/8/8/8/8/6k1/6q1/7K w - - 0 1",         # White is checkmated: Black is the greater side
                              "4k3/8/8/8/8/8/8/4K2R w K - 0 1",         # a castling right left
                              "4k3/8/8/8/8/8/8/4K2R w - - 0 1",
                              "4k3/8/8/8/8/8/PP6/4K3 w - - 0 1"])       # 4 men, the handle holds 3
    assert hit.tolist() == [True, True, True, True, False, True, False]
    assert (int(wdl[1]), int(dtm[1])) == (-1, 0) and (int(wdl[2]), int(dtm[2])) == (1, 1) and (int(wdl[3]), int(dtm[3])) == (-1, 0)
    assert int(wdl[0]) == 0 and int(wdl[5]) == 1
    tb.close()


def test_damaged_cache_files_are_refused(cache_file, tmp_path):
    raw = open(cache_file, "rb").read()
    cases = {"truncated": raw[:len(raw) - 1000], "wrong magic": b"X" + raw[1:],
             "flipped table byte": raw[:len(raw) - 12345] + bytes([raw[len(raw) - 12345] ^ 1]) + raw[len(raw) - 12344:],
             "trailing bytes": raw + b"\0", "other version": raw[:8] + (2).to_bytes(4, "little") + raw[12:]}
    want = {"truncated": "truncated", "wrong magic": "magic", "flipped table byte": "checksum", "trailing bytes": "trailing",
            "other version": "version"}
    for name, data in cases.items():
        p = tmp_path / "bad.m0tb"
        p.write_bytes(data)
        with pytest.raises(RuntimeError, match=want[name]):
            tbm.Tablebase.load(str(p))
    with pytest.raises(RuntimeError, match="cannot open"):
        tbm.Tablebase.load(str(tmp_path / "missing.m0tb"))
    # the library's own writer round-trips (temporary file + rename: nothing else is left behind)
    tb = tbm.Tablebase.load(cache_file)
    out = tmp_path / "copy.m0tb"
    tb.save(str(out))
    assert out.read_bytes() == raw and sorted(os.listdir(tmp_path)) == ["bad.m0tb", "copy.m0tb"]
    assert (os.stat(out).st_mode & 0o777) == 0o644
    tb.close()


def test_cached_loads_an_existing_file_and_survives_a_failed_save(cache_file, tmp_path, monkeypatch, caplog):
    tb = tbm.Tablebase.cached(cache_file, 3)             # no GPU needed: the file holds what is asked for
    assert tb.max_men == 3 and len(tb.info()) == 6
    tb.close()
    # more men than the file holds, or no file: the tables are built (stubbed here: the build needs a GPU) and saved
    built = []
    monkeypatch.setattr(tbm.Tablebase, "build", classmethod(lambda cls, max_men=4, device=0: built.append(max_men) or cls.load(cache_file)))
    fresh = tmp_path / "fresh.m0tb"
    tb = tbm.Tablebase.cached(str(fresh), 3)
    assert built == [3] and fresh.read_bytes() == open(cache_file, "rb").read()
    tb.close()
    tb = tbm.Tablebase.cached(cache_file, 4)
    assert built == [3, 4]
    tb.close()
    # a cache that cannot be written is a warning, not the end of the worker
    with caplog.at_level("WARNING"):
        tb = tbm.Tablebase.cached(str(tmp_path / "no_such_dir" / "tb.m0tb"), 3)
    assert tb.max_men == 3 and "not written" in caplog.text
    tb.close()
    assert tbm.Tablebase.cached(None, 3).max_men == 3


def test_savers_of_one_path_do_not_disturb_each_other(cache_file, tmp_path):
    """Workers that share `engine.tablebase.cache` all build and save at the same time: every save must succeed, the file must
    be whole at every moment a reader looks, and no temporary file stays behind."""
    import threading
    raw = open(cache_file, "rb").read()
    target = str(tmp_path / "shared.m0tb")
    handles = [tbm.Tablebase.load(cache_file) for _ in range(4)]
    errors = []

    def saver(tb):
        try:
            for _ in range(5):
                tb.save(target)                            # ctypes releases the GIL: the saves overlap
                tbm.Tablebase.load(target).close()         # a reader between two renames sees a complete, valid file
        except Exception as e:                             # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=saver, args=(h,)) for h in handles]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    assert open(target, "rb").read() == raw and os.listdir(tmp_path) == ["shared.m0tb"]
    for h in handles:
        h.close()


def test_engine_tablebase_configuration():
    assert tbm.tablebase_cfg({}) is None and tbm.tablebase_cfg({"engine": {"tablebase": None}}) is None
    assert tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 3}}}) == {"max_pieces": 3, "cache": None}
    assert tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 4, "cache": "tb.bin"}}}) == {"max_pieces": 4, "cache": "tb.bin"}
    for bad in (2, 5, 7, "4", True, 3.0):
        with pytest.raises(ValueError, match="max_pieces"):
            tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": bad}}})
    with pytest.raises(ValueError, match="unknown"):
        tbm.tablebase_cfg({"engine": {"tablebase": {"max_pieces": 4, "path": "syzygy"}}})
    # tablebases.enabled is accepted only together with engine.tablebase; the probe limit is the smaller of the two
    with pytest.raises(NotImplementedError, match="tablebases"):
        selfplay.check_unsupported_sections({"tablebases": {"enabled": True, "path": "tb", "max_pieces": 7}})
    with pytest.raises(NotImplementedError, match="engine.tablebase"):
        selfplay.check_unsupported_sections({"tablebases": {"enabled": True}, "engine": {"concurrent_games": 4}})
    cfg = {"tablebases": {"enabled": True, "path": "tb", "max_pieces": 7}, "engine": {"tablebase": {"max_pieces": 4}}}
    selfplay.check_unsupported_sections(cfg)
    assert tbm.probe_limit(cfg) == 4
    assert tbm.probe_limit({"tablebases": {"enabled": True, "max_pieces": 3}, "engine": {"tablebase": {"max_pieces": 4}}}) == 3
    assert tbm.probe_limit({"engine": {"tablebase": {"max_pieces": 3}}}) == 3
    selfplay.check_unsupported_sections({"engine": {"tablebase": {"max_pieces": 3}}})
    with pytest.raises(ValueError, match="max_pieces"):
        selfplay.check_unsupported_sections({"tablebases": {"enabled": True}, "engine": {"tablebase": {"max_pieces": 6}}})


def test_tablebase_needs_a_gpu_to_build_and_says_so():
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):
            tbm.Tablebase.build(3)
    with pytest.raises(RuntimeError, match="max_men"):
        tbm.Tablebase.build(5)
