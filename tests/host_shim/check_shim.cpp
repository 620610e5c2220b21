// Host build of csrc/hip_check.h: HipStatus / M0_HIP / m0_hip_error driven with injected hipError_t values
// (tests/test_hip_check.py).  The only HIP runtime call is hipGetErrorString, which needs no device.  The product's
// m0_set_error lives in capi_net.hip; here it is a thread-local string the test reads back.
// With -DCHECK_SHIM_MAIN the file is a stand-alone program (the one to build with -fsanitize=address,undefined) that runs the
// same properties and prints one line each.
#include <stdio.h>
#include <string.h>
#include "../../matrix0_amd/csrc/hip_check.h"

static thread_local std::string g_last_error;
void m0_set_error(const std::string& s) { g_last_error = s; }

namespace {
int g_evaluated = 0;      // how often a call expression handed to M0_HIP was evaluated
hipError_t inject(int code) { ++g_evaluated; return (hipError_t)code; }
void give(const std::string& s, char* out, int cap) {
    if (out && cap > 0) { strncpy(out, s.c_str(), (size_t)cap - 1); out[cap - 1] = 0; }
}
}  // namespace

extern "C" {

// M0_HIP over codes[0..n) on one fresh status.  oks[i] = what the i-th M0_HIP yielded; returns how many call expressions were
// evaluated; *code / msg = the status afterwards.
int hk_run(const int* codes, int n, int* oks, int* code, char* msg, int cap) {
    HipStatus st;
    g_evaluated = 0;
    for (int i = 0; i < n; ++i) oks[i] = M0_HIP(st, inject(codes[i])) ? 1 : 0;
    *code = (int)st.code();
    give(st.message(), msg, cap);
    return g_evaluated;
}

// a fresh status: ok(), hipSuccess as code, an empty message -> 1
int hk_fresh(void) {
    HipStatus st;
    return st.ok() && st.code() == hipSuccess && st.message().empty() ? 1 : 0;
}

// check() called directly (no macro): the first failure stays when a different one follows; returns the code kept
int hk_check_twice(int first, int second, char* msg, int cap) {
    HipStatus st;
    st.check((hipError_t)first, "first call");
    st.check((hipError_t)second, "second call");
    give(st.message(), msg, cap);
    return (int)st.code();
}

// a status that takes over another one's failure, and keeps its own when it already has one
int hk_adopt(int own, int other, char* msg, int cap) {
    HipStatus a, b;
    a.check((hipError_t)own, "own call");
    b.check((hipError_t)other, "other call");
    a.check(b);
    give(a.message(), msg, cap);
    return (int)a.code();
}

// m0_hip_error of a status that failed with `code`; context may be null.  The error string it set goes to `out`.
int hk_convert(int code, const char* context, char* out, int cap) {
    HipStatus st;
    M0_HIP(st, inject(code));
    g_last_error.clear();
    const int rc = m0_hip_error(st, context);
    give(g_last_error, out, cap);
    return rc;
}

void hk_error_string(int code, char* out, int cap) { give(hipGetErrorString((hipError_t)code), out, cap); }

}  // extern "C"

#ifdef CHECK_SHIM_MAIN
namespace {
int failures = 0;
void expect(const char* what, bool ok) {
    printf("%-72s %s\n", what, ok ? "ok" : "WRONG");
    failures += !ok;
}
}  // namespace

int main() {
    char msg[512], want[256];
    const int oom = (int)hipErrorOutOfMemory, bad = (int)hipErrorInvalidValue;
    expect("a fresh status is ok", hk_fresh() == 1);
    {
        const int codes[3] = {0, 0, 0};
        int oks[3], code = -1;
        expect("hipSuccess keeps it ok and every call is evaluated",
               hk_run(codes, 3, oks, &code, msg, sizeof(msg)) == 3 && oks[0] && oks[1] && oks[2] && code == 0 && !msg[0]);
    }
    {
        const int codes[5] = {0, oom, bad, 0, bad};
        int oks[5], code = -1;
        const int evaluated = hk_run(codes, 5, oks, &code, msg, sizeof(msg));
        hk_error_string(oom, want, sizeof(want));
        expect("after a failure M0_HIP evaluates no call expression", evaluated == 2);
        expect("M0_HIP yields ok() before and after", oks[0] == 1 && !oks[1] && !oks[2] && !oks[3] && !oks[4]);
        expect("the first failure's code is kept", code == oom);
        expect("the message holds the call's text and HIP's string", strstr(msg, "inject(codes[i])") && strstr(msg, want));
    }
    expect("check() keeps the first of two different failures", hk_check_twice(bad, oom, msg, sizeof(msg)) == bad && strstr(msg, "first call"));
    expect("a status takes over another one's failure", hk_adopt(0, oom, msg, sizeof(msg)) == oom && strstr(msg, "other call"));
    expect("... and keeps its own when it has one", hk_adopt(bad, oom, msg, sizeof(msg)) == bad && strstr(msg, "own call"));
    hk_error_string(bad, want, sizeof(want));
    expect("m0_hip_error returns M0_ERR_HIP and prefixes the context",
           hk_convert(bad, "select failed", msg, sizeof(msg)) == -3 && strstr(msg, "select failed: inject(code)") == msg && strstr(msg, want));
    expect("... and without a context the message alone", hk_convert(bad, nullptr, msg, sizeof(msg)) == -3 && strstr(msg, "inject(code)") == msg);
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
#endif
