// Retrograde generation of the endgame tables on the GPU: one thread per entry, an init kernel and a sweep kernel per
// table (tb_core.h holds the per-entry work), tables built in dependency order on a stream of the build's own.  Integer and
// latency bound: no LDS, nothing shared between threads but the table itself.
#include <hip/hip_runtime.h>
#include <chrono>
#include <map>
#include "hip_check.h"
#include "tb.h"

namespace m0 {

static constexpr int TB_BLOCK = 256;

__global__ __launch_bounds__(TB_BLOCK) void tb_init_kernel(TbSig sig, uint8_t* tab, uint32_t total) {
    const uint32_t idx = blockIdx.x * (uint32_t)TB_BLOCK + threadIdx.x;
    if (idx < total) tab[idx] = tb_init_entry(sig, idx);
}

// counters[0] += entries decided by this launch; counters[1] |= TB_WHY_* bits of failed successor lookups
__global__ __launch_bounds__(TB_BLOCK) void tb_sweep_kernel(TbSig sig, const TbSet* set, uint8_t* tab, uint32_t total, int n,
                                                            unsigned int* counters) {
    const uint32_t idx = blockIdx.x * (uint32_t)TB_BLOCK + threadIdx.x;
    int changed = 0, missing = 0;
    if (idx < total) changed = tb_step(sig, *set, tab, idx, n, &missing);
    const int c = __syncthreads_count(changed);
    if (threadIdx.x == 0 && c) atomicAdd(&counters[0], (unsigned int)c);
    if (missing) atomicOr(&counters[1], (unsigned int)missing);
}

namespace {

struct DeviceBuild {
    hipStream_t stream = nullptr;
    TbSet* set_dev = nullptr;
    unsigned int* counters_dev = nullptr;
    // finished tables on the device.  They stay until the build is over (a full 4-man set is under 1 GiB): hipFree in the
    // middle of the build would synchronise the whole device, other engines' streams included.
    std::map<std::string, uint8_t*> resident;
    ~DeviceBuild() {
        for (auto& kv : resident) (void)hipFree(kv.second);
        if (set_dev) (void)hipFree(set_dev);
        if (counters_dev) (void)hipFree(counters_dev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

int tb_build_on_device(int hip_device, const std::vector<std::string>& order, m0_tb* tb, std::string& err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { err = "no HIP device available (the tables are built on the GPU)"; return M0_ERR_HIP; }
    if (hip_device < 0 || hip_device >= ndev) { err = "hip_device out of range"; return M0_ERR_INVALID; }
    HipStatus hs;                                    // of this build: tested wherever the host waits for the stream
    auto failed = [&] { err = hs.message(); return M0_ERR_HIP; };
    M0_HIP(hs, hipSetDevice(hip_device));
    DeviceBuild B;
    M0_HIP(hs, hipStreamCreateWithFlags(&B.stream, hipStreamNonBlocking));
    M0_HIP(hs, hipMalloc((void**)&B.set_dev, sizeof(TbSet)));
    if (!M0_HIP(hs, hipMalloc((void**)&B.counters_dev, 2 * sizeof(unsigned int)))) return failed();
    TbSet set_host;
    for (auto& t : set_host.tab) t = nullptr;
    tb->tables.clear();
    tb->tables.reserve(order.size());
    for (size_t i = 0; i < order.size(); ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        TbTable T;
        T.name = order[i];
        if (!tb_parse_sig(T.name.c_str(), T.sig)) { err = "not a signature in scope: " + T.name; return M0_ERR_INVALID; }
        int max_sub_d = -1;
        for (const auto& d : tb_dependencies(T.name)) {
            if (!B.resident.count(d)) { err = T.name + " needs " + d + ", which is not built"; return M0_ERR_STATE; }
            for (const auto& done : tb->tables) if (done.name == d) max_sub_d = std::max(max_sub_d, done.maxd);
        }
        const uint32_t total = tb_entries(T.sig.n);
        uint8_t* tab = nullptr;
        if (!M0_HIP(hs, hipMalloc((void**)&tab, total))) return failed();
        B.resident[T.name] = tab;
        set_host.tab[tb_material_code(T.sig)] = tab;
        M0_HIP(hs, hipMemcpyAsync(B.set_dev, &set_host, sizeof(TbSet), hipMemcpyHostToDevice, B.stream));
        M0_HIP(hs, hipStreamSynchronize(B.stream));             // set_host changes again below
        const unsigned int blocks = (total + TB_BLOCK - 1) / TB_BLOCK;
        M0_HIP(hs, (tb_init_kernel<<<blocks, TB_BLOCK, 0, B.stream>>>(T.sig, tab, total), hipGetLastError()));
        // sweep n decides the entries with d == n; stop after two sweeps in a row that change nothing, once n has passed
        // every d + 1 of the tables this one reads (a later d of theirs could still decide an entry here)
        int quiet = 0, n = 0;
        for (;;) {
            ++n;
            if (n + 1 >= TB_INVALID) { err = T.name + ": a distance to mate does not fit the entry byte"; return M0_ERR_STATE; }
            unsigned int counters[2] = {0, 0};
            M0_HIP(hs, hipMemsetAsync(B.counters_dev, 0, sizeof(counters), B.stream));
            M0_HIP(hs, (tb_sweep_kernel<<<blocks, TB_BLOCK, 0, B.stream>>>(T.sig, B.set_dev, tab, total, n, B.counters_dev), hipGetLastError()));
            M0_HIP(hs, hipMemcpyAsync(counters, B.counters_dev, sizeof(counters), hipMemcpyDeviceToHost, B.stream));
            if (!M0_HIP(hs, hipStreamSynchronize(B.stream))) return failed();
            if (counters[1] & TB_WHY_NO_TABLE) { err = T.name + ": a move leads into a table that is not in the set"; return M0_ERR_STATE; }
            if (counters[1] & TB_WHY_BAD_ENTRY) { err = T.name + ": a legal move reaches an invalid entry (index or decode bug)"; return M0_ERR_STATE; }
            if (counters[0]) { quiet = 0; T.maxd = n; } else ++quiet;
            if (quiet >= 2 && n > max_sub_d + 1) break;
        }
        T.sweeps = n;
        T.bytes.resize(total);
        M0_HIP(hs, hipMemcpyAsync(T.bytes.data(), tab, total, hipMemcpyDeviceToHost, B.stream));
        if (!M0_HIP(hs, hipStreamSynchronize(B.stream))) return failed();
        if (T.maxd < 0)                                   // no sweep decided anything: d = 0 if there is a checkmate at all
            for (uint8_t v : T.bytes) if (v == 1) { T.maxd = 0; break; }
        T.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        tb->tables.push_back(std::move(T));
    }
    tb->index_tables();
    return M0_OK;
}

}  // namespace m0
