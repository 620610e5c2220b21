"""csrc/hip_check.h on the CPU: HipStatus, M0_HIP and m0_hip_error built for the host (tests/host_shim/check_shim.cpp) and
driven with injected hipError_t values.  No HIP runtime call is made but hipGetErrorString, which needs no device.  The
properties: a fresh status is ok and hipSuccess keeps it ok; the FIRST failure stays, code and message, whatever follows; the
message is the text of the failing call expression plus HIP's own string for the code; after a failure M0_HIP does not evaluate
its call expression (counted inside the expression); m0_hip_error returns M0_ERR_HIP and sets the error string with the caller's
context in front.  And the same as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
M0_ERR_HIP = -3                                         # include/m0_engine.h
# hipError_t values (hip_runtime_api.h): stable numbers of the HIP ABI
SUCCESS, INVALID_VALUE, OUT_OF_MEMORY, ILLEGAL_ADDRESS, LAUNCH_FAILURE = 0, 1, 2, 700, 719
CALL_TEXT = "inject(codes[i])"                          # the expression check_shim.cpp hands to M0_HIP in hk_run


def shim():
    # One HIP runtime per process (matrix0_amd/_lib.py): PyTorch-ROCm ships its own libamdhip64 under the system one's SONAME.
    # With torch resident first the loader hands the shim that copy, and a later test's engine library finds its device.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    return host_shim.load("check")


def text(fn, *args):
    buf = C.create_string_buffer(512)
    rc = fn(*args, buf, len(buf))
    return rc, buf.value.decode()


def hip_string(code):
    return text(shim().hk_error_string, code)[1]


def run(codes):
    """M0_HIP over the codes on one fresh status -> (calls evaluated, what each M0_HIP yielded, code kept, message kept)."""
    arr = np.asarray(codes, np.int32)
    oks = np.full(len(arr), -1, np.int32)
    code = C.c_int(-1)
    buf = C.create_string_buffer(512)
    evaluated = shim().hk_run(arr.ctypes.data, len(arr), oks.ctypes.data, C.byref(code), buf, len(buf))
    return evaluated, oks.tolist(), code.value, buf.value.decode()


def test_hip_strings_differ():
    """The expectations below lean on HIP's own texts being distinct and non-empty for the injected codes."""
    texts = [hip_string(c) for c in (INVALID_VALUE, OUT_OF_MEMORY, ILLEGAL_ADDRESS, LAUNCH_FAILURE)]
    assert all(texts) and len(set(texts)) == len(texts)


def test_fresh_status_is_ok_and_success_keeps_it_ok():
    assert shim().hk_fresh() == 1
    evaluated, oks, code, msg = run([SUCCESS] * 4)
    assert evaluated == 4 and oks == [1, 1, 1, 1] and code == SUCCESS and msg == ""


@pytest.mark.parametrize("codes,first", [
    ([OUT_OF_MEMORY], 0),
    ([SUCCESS, SUCCESS, ILLEGAL_ADDRESS, INVALID_VALUE, SUCCESS, LAUNCH_FAILURE], 2),
    ([INVALID_VALUE, OUT_OF_MEMORY], 0),
    ([SUCCESS, LAUNCH_FAILURE, SUCCESS, SUCCESS], 1),
])
def test_first_failure_is_kept_and_nothing_is_evaluated_after_it(codes, first):
    evaluated, oks, code, msg = run(codes)
    assert evaluated == first + 1                        # the calls up to and including the failing one, none after it
    assert oks == [1] * first + [0] * (len(codes) - first)
    assert code == codes[first]
    assert msg == f"{CALL_TEXT}: {hip_string(codes[first])}"
    for later in set(codes[first + 1:]) - {SUCCESS, codes[first]}:
        assert hip_string(later) not in msg


def test_check_keeps_the_first_of_two_different_failures():
    code, msg = text(shim().hk_check_twice, INVALID_VALUE, OUT_OF_MEMORY)
    assert code == INVALID_VALUE and msg == f"first call: {hip_string(INVALID_VALUE)}"
    code, msg = text(shim().hk_check_twice, SUCCESS, OUT_OF_MEMORY)
    assert code == OUT_OF_MEMORY and msg == f"second call: {hip_string(OUT_OF_MEMORY)}"


def test_a_status_takes_over_another_ones_first_failure():
    """What an engine does with its network's status after a failed forward."""
    code, msg = text(shim().hk_adopt, SUCCESS, LAUNCH_FAILURE)
    assert code == LAUNCH_FAILURE and msg == f"other call: {hip_string(LAUNCH_FAILURE)}"
    code, msg = text(shim().hk_adopt, INVALID_VALUE, LAUNCH_FAILURE)
    assert code == INVALID_VALUE and msg == f"own call: {hip_string(INVALID_VALUE)}"
    code, msg = text(shim().hk_adopt, SUCCESS, SUCCESS)
    assert code == SUCCESS and msg == ""


def test_failed_status_becomes_the_abi_answer():
    rc, msg = text(shim().hk_convert, ILLEGAL_ADDRESS, b"select failed")
    assert rc == M0_ERR_HIP and msg == f"select failed: inject(code): {hip_string(ILLEGAL_ADDRESS)}"
    rc, msg = text(shim().hk_convert, ILLEGAL_ADDRESS, None)
    assert rc == M0_ERR_HIP and msg == f"inject(code): {hip_string(ILLEGAL_ADDRESS)}"


def test_sanitizer_build_over_the_same_properties():
    """The header as a stand-alone host program (its own main, never loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "host_shim"), "../_build/check_shim_san"])
    out = subprocess.run([os.path.join(HERE, "_build", "check_shim_san")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
    assert out.stdout.strip().endswith("\n0 failures") and out.stdout.count(" ok\n") == 11, out.stdout
