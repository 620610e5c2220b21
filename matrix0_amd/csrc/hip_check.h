// The one way the host units make a HIP call.  A HipStatus keeps the FIRST failure of a sequence of calls; M0_HIP issues a call
// only while the status is still good, so a straight run of copies and launches is a run of M0_HIP lines and one test at the
// end, and nothing more is started on the GPU once a call has failed.  A network and an engine each own one for their whole life
// (the handle is refused at the door afterwards, m0_engine.h); a stateless entry point has one on its stack.  Only teardown
// (hipFree / *Destroy and the synchronise before them) may still drop a result with (void).
// Host-only and free of the project's other headers: g++ -D__HIP_PLATFORM_AMD__ compiles it (tests/host_shim/check_shim.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <string>

class HipStatus {
public:
    bool ok() const { return code_ == hipSuccess; }
    // records `e` when it is the first failure, as "<what>: <HIP's text for e>"; returns ok()
    bool check(hipError_t e, const char* what) {
        if (ok() && e != hipSuccess) { code_ = e; msg_ = std::string(what) + ": " + hipGetErrorString(e); }
        return ok();
    }
    // a failure that another status recorded (a network's forward on behalf of an engine) counts here too
    bool check(const HipStatus& other) {
        if (ok()) *this = other;
        return ok();
    }
    hipError_t code() const { return code_; }
    const std::string& message() const { return msg_; }

private:
    hipError_t code_ = hipSuccess;
    std::string msg_;
};

// `call` is evaluated only while `status` is good; yields status.ok()
#define M0_HIP(status, call) ((status).ok() && (status).check((call), #call))

#ifndef M0_ERR_HIP
#define M0_ERR_HIP (-3)   // include/m0_engine.h
#endif
void m0_set_error(const std::string& s);   // the thread's m0_last_error text (capi_net.hip)

// A failed status as the ABI's answer: the error string is "[<context>: ]<first failure>", the result M0_ERR_HIP.
inline int m0_hip_error(const HipStatus& status, const char* context = nullptr) {
    m0_set_error(context ? std::string(context) + ": " + status.message() : status.message());
    return M0_ERR_HIP;
}
