"""matrix0_amd/_abi.py against include/m0_engine.h (no GPU; only the last tests need the built library): the header is read with
its comments stripped and every function, struct and constant of it is compared with the Python side, name by name, so that a
field moved, a parameter dropped or a constant changed on one side alone fails here and says where."""
import ctypes as C
import os
import re

import pytest

from matrix0_amd import _abi, _lib, encoding, engine as eng, game_import

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m0_engine.h")
SCALARS = {"int": "i4", "int32_t": "i4", "uint32_t": "u4", "int16_t": "i2", "uint16_t": "u2", "int8_t": "i1", "uint8_t": "u1",
           "int64_t": "i8", "uint64_t": "u8", "size_t": "u8", "float": "f4", "double": "f8", "char": "i1"}


def kind_of_c(decl, defines):
    """(kind, name) of a C declaration `const float* s`, `uint16_t pv[M0_AN_MAX_PV]`, `int n`, `void`: kind is "ptr", a scalar as
    "i4" / "u8" / "f8", "void", ("array", element kind, length) or ("struct", name)."""
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    m = re.fullmatch(r"(.*?)(\w+)\s*\[\s*(\w+)\s*\]", decl)
    if m:
        n = m.group(3)
        return ("array", kind_of_c(m.group(1) + " x", defines)[0], int(n) if n.isdigit() else defines[n]), m.group(2)
    words = re.findall(r"\w+|\*", decl)
    name = words.pop() if len(words) > 1 and words[-1] != "*" and words[-1] not in SCALARS else None
    if "*" in words:
        return "ptr", name
    assert len(words) == 1, decl
    base = words[0]
    return ("void" if base == "void" else SCALARS[base] if base in SCALARS else ("struct", base)), name


def kind_of_ctype(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if issubclass(t, C.Array):
        return ("array", kind_of_ctype(t._type_), t._length_)
    if issubclass(t, C.Structure):
        return ("struct", {v: k for k, v in _abi.STRUCTS.items()}[t])
    if t in (C.c_float, C.c_double):
        return "f%d" % C.sizeof(t)
    assert issubclass(t, C._SimpleCData), t
    return ("i" if t._type_ in "bhilq" else "u") + str(C.sizeof(t))


def parse_header(path=HEADER):
    """{"defines": {name: int}, "structs": {name: [(field, kind)]}, "functions": {name: (return kind, [parameter kinds])}}"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(M0_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(m0_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            kind, fname = kind_of_c(first, defines)
            base = first[: first.rindex(fname)].rstrip("* ")          # `double cpuct, cpuct_start`: the others share the base type
            fields += [(fname, kind)] + [kind_of_c(base + " " + d, defines)[::-1] for d in more]
        structs[name] = fields
    text = re.sub(r"typedef\s+struct\s+\w+\s*(\{.*?\})?\s*\w+\s*;", " ", text, flags=re.S)
    functions = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(m0_\w+)\s*\(([^)]*)\)\s*;", text):
        assert name not in functions, name
        params = [] if params.strip() == "void" else [kind_of_c(p, defines)[0] for p in params.split(",")]
        functions[name] = (kind_of_c(ret + " x", defines)[0], params)
    return {"defines": defines, "structs": structs, "functions": functions}


@pytest.fixture(scope="module")
def hdr():
    return parse_header()


def check_functions(h):
    only_header = sorted(set(h["functions"]) - set(_abi.FUNCTIONS))
    only_table = sorted(set(_abi.FUNCTIONS) - set(h["functions"]))
    assert not only_header and not only_table, f"in the header alone: {only_header}; in the table alone: {only_table}"
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.FUNCTIONS[name]
        assert len(argtypes) == len(params), f"{name}: the header has {len(params)} parameters, the table {len(argtypes)}"
        assert kind_of_ctype(restype) == ret, f"{name}: returns {ret} in the header, {restype} in the table"
        for k, (a, p) in enumerate(zip(argtypes, params)):
            assert kind_of_ctype(a) == p, f"{name}: parameter {k} is {p} in the header, {a} in the table"


def check_structs(h):
    assert set(h["structs"]) == set(_abi.STRUCTS)
    for name, fields in h["structs"].items():
        mirror = _abi.STRUCTS[name]
        assert [f for f, _ in fields] == [f[0] for f in mirror._fields_], \
            f"{name}: " + str([(a, b[0]) for (a, _), b in zip(fields, mirror._fields_) if a != b[0]] or "a field more or less")
        for (fname, kind), (_, t) in zip(fields, mirror._fields_):
            assert kind_of_ctype(t) == kind, f"{name}.{fname}: {kind} in the header, {kind_of_ctype(t)} in the mirror"


def check_constants(h):
    d = h["defines"]

    def group(prefix, but=()):
        return {k[len(prefix):].lower(): v for k, v in d.items() if k.startswith(prefix) and k not in but}

    assert d["M0_OK"] == _lib.M0_OK == 0
    errs = group("M0_ERR_")
    assert errs == {k[len("M0_ERR_"):].lower(): getattr(_lib, k) for k in dir(_lib) if k.startswith("M0_ERR_")} and len(errs) == 5
    assert d["M0_POLICY_SIZE"] == _lib.POLICY_SIZE == encoding.LEGACY_POLICY_SIZE
    assert {"relu": "relu", "silu": "silu", "leaky": "leaky_relu"}.keys() == group("M0_ACT_").keys()
    assert {("leaky_relu" if k == "leaky" else k): v for k, v in group("M0_ACT_").items()} == _lib.ACT
    assert group("M0_SSL_") == _lib.SSL_BITS and list(group("M0_SSL_")) == _lib.SSL_ORDER == game_import.SSL_KEYS
    assert (d["M0_AN_MAX_LINES"], d["M0_AN_MAX_PV"]) == (eng.AN_MAX_LINES, eng.AN_MAX_PV) == (8, 16)
    flags = {"halfmove_saturated": encoding.HALFMOVE_SATURATED, "fullmove_saturated": encoding.FULLMOVE_SATURATED,
             "ep_from_mask": encoding.EP_FROM_MASK, "no_mask": encoding.NO_MASK}
    status = group("M0_DECODE_", but=["M0_DECODE_" + k.upper() for k in flags])
    assert len(status) == 12 and {v: k for k, v in status.items()} == encoding.DECODE_STATUS, \
        sorted(set(status.items()) ^ {(k, v) for v, k in encoding.DECODE_STATUS.items()})
    assert encoding.DECODE_OK == d["M0_DECODE_OK"], "DECODE_OK"
    assert encoding.DECODE_MASK_MISMATCH == d["M0_DECODE_MASK_MISMATCH"], \
        f"DECODE_MASK_MISMATCH is {encoding.DECODE_MASK_MISMATCH}, the header says {d['M0_DECODE_MASK_MISMATCH']}"
    assert {k: d["M0_DECODE_" + k.upper()] for k in flags} == flags
    ends = group("M0_REPLAY_END_")
    assert ends == game_import.END_BITS and len(ends) == 4
    replay = group("M0_REPLAY_", but=["M0_REPLAY_END_" + k.upper() for k in ends])
    assert {v: k for k, v in replay.items()} == game_import.STATUS and len(replay) == 4
    assert group("M0_MOVE_") == {"uci": game_import.MOVE_UCI, "raw": game_import.MOVE_RAW}


def test_every_declared_function_is_in_the_table_with_its_types(hdr):
    check_functions(hdr)
    assert len(hdr["functions"]) == 87
    # no function with another return than int left on the ctypes default (the table has no defaults: every entry says its own)
    for name, (ret, _) in hdr["functions"].items():
        assert ret == "i4" or _abi.FUNCTIONS[name][0] is not C.c_int, name


def test_every_struct_has_a_mirror_field_by_field(hdr):
    assert len(hdr["structs"]) == 7 and len(hdr["structs"]["m0_selfplay_cfg"]) == 63
    check_structs(hdr)
    # what the earlier tests of the analysis structs pinned
    assert C.sizeof(eng.AnalysisLine) * eng.AN_MAX_LINES < C.sizeof(eng.AnalysisResult)
    names = [f[0] for f in eng.AnalysisResult._fields_]
    assert names[-2:] == ["tb_dtm", "line_dtm"] and names.index("lines") == len(names) - 3
    assert eng.AnalysisResult.tb_dtm.offset == eng.AnalysisResult.lines.offset + C.sizeof(eng.AnalysisLine) * eng.AN_MAX_LINES
    assert eng.ANALYSIS_STATUS[3] == "tablebase"


def test_every_mirrored_constant_equals_the_header(hdr):
    text = open(HEADER).read()
    assert "#define M0_AN_MAX_LINES 8" in text and "#define M0_AN_MAX_PV    16" in text
    check_constants(hdr)


def test_public_names_stay_where_callers_find_them():
    for name in ("SelfplayCfg", "SelfplayStats", "GameRecord", "AnalysisOpts", "AnalysisLine", "AnalysisResult"):
        assert getattr(eng, name) is getattr(_abi, name), name
    assert _lib.NetCfg is _abi.NetCfg


def test_split_ssl_is_the_channel_split_of_a_record():
    import numpy as np
    a = np.arange(3 * 17 * 64, dtype=np.float32).reshape(3, 17, 8, 8)
    got = _lib.split_ssl(a)
    want = {"piece": a[:, :13], "threat": a[:, 13], "pin": a[:, 14], "fork": a[:, 15], "control": a[:, 16]}
    assert list(got) == list(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def test_the_built_library_exports_the_table_and_has_the_mirror_size():
    L = _lib.lib()
    for name in _abi.FUNCTIONS:
        assert hasattr(L, name), name
    assert C.sizeof(eng.AnalysisResult) == L.m0_analysis_result_size()
    assert L.m0_dist_destroy.restype is None and L.m0_version.argtypes == []
