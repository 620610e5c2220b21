// extern "C" entry points of the resident row store (include/m0_batch.h) and of its batches with SSL target maps
// (include/m0_batch_ssl.h: the same path with two more outputs and the SSL instantiation of the kernel).  A store owns its segments (one allocation each, a
// SegView in front: batch_host.h), a ring of descriptor slots, and the staging outputs of batches that go to host memory.
//
// A batch resolves its ids to row references on the host, writes them into a slot's pinned buffer, copies them to the slot's
// device buffer on the caller's stream and launches batch_rows_kernel behind the copy; an event recorded behind the launch marks
// the slot busy.  A slot is reused SLOTS batches later, after a wait for its event, so the host runs at most SLOTS batches ahead
// of the device and a pinned buffer is never rewritten under a copy.  Eviction waits for the events of all slots before it frees a
// segment: a batch still running on any stream never reads freed memory.  The price is that of the hipFree itself, which
// synchronises the device: evict between epochs, not between batches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <deque>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "augment_kernels.h"
#include "batch_host.h"
#include "batch_kernels.h"
#include "capi_common.h"
#include "rowstore.h"
#include "rowpack_kernels.h"
#include "tree.h"

using namespace m0batch;
using namespace m0store;
using m0rowpack::pack_host;

namespace {

void free_outputs(m0_rowstore* s) {
    (void)hipFree(s->o_planes); (void)hipFree(s->o_pi); (void)hipFree(s->o_z); (void)hipFree(s->o_mask);
    s->o_planes = s->o_pi = s->o_z = nullptr; s->o_mask = nullptr; s->o_cap = 0;
}

void free_ssl_outputs(m0_rowstore* s) {
    (void)hipFree(s->o_ssl); (void)hipFree(s->o_status);
    s->o_ssl = nullptr; s->o_status = nullptr; s->o_ssl_cap = 0;
}

}  // namespace

// ---- what capi_batch_weighted.hip uses too (rowstore.h) ----
namespace m0store {

int invalid(const std::string& why) { m0_set_error(why); return M0_ERR_INVALID; }

bool drain(m0_rowstore* s) {
    for (Slot& sl : s->slots)
        if (sl.busy) { M0_HIP(s->hs, hipEventSynchronize(sl.done)); sl.busy = false; }
    return s->hs.ok();
}

Slot* take_slot(m0_rowstore* s, int B) {
    if (s->slots[0].cap < B) {                                            // a larger batch than any before: all slots grow at once
        drain(s);
        for (Slot& g : s->slots) {
            if (g.pinned) (void)hipHostFree(g.pinned);
            if (g.dev) (void)hipFree(g.dev);
            g.pinned = g.dev = nullptr; g.cap = 0;
            if (!g.done) M0_HIP(s->hs, hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
            M0_HIP(s->hs, hipHostMalloc((void**)&g.pinned, (size_t)B * sizeof(RowRef), hipHostMallocDefault));
            M0_HIP(s->hs, hipMalloc((void**)&g.dev, (size_t)B * sizeof(RowRef)));
        }
        if (!s->hs.ok()) return nullptr;
        for (Slot& g : s->slots) g.cap = B;
    }
    Slot& sl = s->slots[s->turn++ % SLOTS];
    if (sl.busy) { M0_HIP(s->hs, hipEventSynchronize(sl.done)); sl.busy = false; }
    return s->hs.ok() ? &sl : nullptr;
}

bool resolve(const m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, RowRef* refs, int64_t* missing) {
    for (int b = 0; b < B; ++b) {
        const int64_t id = rows[b];
        auto it = std::upper_bound(s->segs.begin(), s->segs.end(), id, [](int64_t v, const Segment& g) { return v < g.first; });
        if (it == s->segs.begin() || id >= (it - 1)->first + (it - 1)->rows) { *missing = id; return false; }
        --it;
        refs[b] = RowRef{it->view(), (int32_t)(id - it->first), kinds ? (int32_t)kinds[b] : M0_AUG_NONE};
    }
    return true;
}

int stage_outputs(m0_rowstore* s, int B, bool outputs_on_device, BatchOut& dev) {
    if (outputs_on_device) return M0_OK;
    if (dev.ssl.asked) {
        if (s->o_ssl_cap < B) {
            drain(s);
            free_ssl_outputs(s);
            M0_HIP(s->hs, hipMalloc((void**)&s->o_ssl, (size_t)B * SSL_FLOATS * sizeof(float)));
            M0_HIP(s->hs, hipMalloc((void**)&s->o_status, (size_t)B * sizeof(int32_t)));
            if (!s->hs.ok()) return m0_hip_error(s->hs, "hipMalloc failed");
            s->o_ssl_cap = B;
        }
        dev.ssl.maps = s->o_ssl; dev.ssl.status = s->o_status;
    }
    if (s->o_cap < B) {
        drain(s);
        free_outputs(s);
        const size_t N = (size_t)B;
        M0_HIP(s->hs, hipMalloc((void**)&s->o_planes, N * PLANE_FLOATS * sizeof(float)));
        M0_HIP(s->hs, hipMalloc((void**)&s->o_pi, N * COLS * sizeof(float)));
        M0_HIP(s->hs, hipMalloc((void**)&s->o_z, N * sizeof(float)));
        if (s->with_mask) M0_HIP(s->hs, hipMalloc((void**)&s->o_mask, N * COLS));
        if (!s->hs.ok()) return m0_hip_error(s->hs, "hipMalloc failed");
        s->o_cap = B;
    }
    dev.planes = s->o_planes; dev.pi = s->o_pi; dev.z = s->o_z; dev.mask = s->o_mask;
    return M0_OK;
}

int finish_batch(m0_rowstore* s, Slot* sl, int B, const BatchOut& dev, const BatchOut& user, bool outputs_on_device, hipStream_t stream) {
    M0_HIP(s->hs, dev.ssl.asked ? launch_batch_rows_ssl(sl->dev, B, dev.planes, dev.pi, dev.z, dev.mask, dev.ssl.maps, dev.ssl.status, stream)
                                : launch_batch_rows(sl->dev, B, dev.planes, dev.pi, dev.z, dev.mask, stream));
    if (M0_HIP(s->hs, hipEventRecord(sl->done, stream))) sl->busy = true;
    if (!s->hs.ok()) return m0_hip_error(s->hs, "batch launch failed");
    if (outputs_on_device) return M0_OK;
    // into the caller's arrays only when the kernel has run: a failure leaves them untouched
    if (!M0_HIP(s->hs, hipEventSynchronize(sl->done))) return m0_hip_error(s->hs, "batch kernel failed");
    sl->busy = false;
    const size_t N = (size_t)B;
    M0_HIP(s->hs, hipMemcpy(user.planes, dev.planes, N * PLANE_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
    M0_HIP(s->hs, hipMemcpy(user.pi, dev.pi, N * COLS * sizeof(float), hipMemcpyDeviceToHost));
    M0_HIP(s->hs, hipMemcpy(user.z, dev.z, N * sizeof(float), hipMemcpyDeviceToHost));
    if (user.mask) M0_HIP(s->hs, hipMemcpy(user.mask, dev.mask, N * COLS, hipMemcpyDeviceToHost));
    if (user.ssl.asked) {
        M0_HIP(s->hs, hipMemcpy(user.ssl.maps, dev.ssl.maps, N * SSL_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
        M0_HIP(s->hs, hipMemcpy(user.ssl.status, dev.ssl.status, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "download failed");
}

}  // namespace m0store

namespace {

// the argument checks of a batch that need no store
int check_batch(const int64_t* rows, const uint8_t* kinds, int B, const float* planes, const float* pi, const float* z, const uint8_t* mask,
                bool with_mask, const SslOut& ssl = SslOut()) {
    if (B <= 0) return invalid("batch must be positive");
    if (!rows || !planes || !pi || !z || (ssl.asked && (!ssl.maps || !ssl.status))) return invalid("null argument");
    if ((mask != nullptr) != with_mask) return invalid(with_mask ? "the rows have masks: a mask output is required" : "the rows have no masks: no mask output");
    if (kinds)
        if (const char* why = m0_bad_kinds(kinds, B)) return invalid(why);
    return M0_OK;
}

int device_batch(m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z, uint8_t* mask,
                 const SslOut& ssl, bool outputs_on_device, hipStream_t stream) {
    if (!M0_HIP(s->hs, hipSetDevice(s->device))) return m0_hip_error(s->hs);
    if (!outputs_on_device) stream = nullptr;
    Slot* sl = take_slot(s, B);
    if (!sl) return m0_hip_error(s->hs, "row store staging failed");
    int64_t missing = 0;
    if (!resolve(s, rows, kinds, B, sl->pinned, &missing)) return invalid("row " + std::to_string(missing) + " is not resident");
    const BatchOut user{planes, pi, z, mask, ssl};
    BatchOut dev = user;
    if (const int rc = stage_outputs(s, B, outputs_on_device, dev)) return rc;
    M0_HIP(s->hs, hipMemcpyAsync(sl->dev, sl->pinned, (size_t)B * sizeof(RowRef), hipMemcpyHostToDevice, stream));
    return finish_batch(s, sl, B, dev, user, outputs_on_device, stream);
}

// m0_rowstore_batch and m0_rowstore_batch_ssl
int store_batch(m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z, uint8_t* mask,
                const SslOut& ssl, int outputs_on_device, void* stream) {
    if (!s) return invalid("null handle");
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->hs.ok()) return m0_hip_error(s->hs);
    if (const int rc = check_batch(rows, kinds, B, planes, pi, z, mask, s->with_mask, ssl)) return rc;
    if (outputs_on_device && !s->on_device()) return invalid("a host store fills host memory");
    if (outputs_on_device && (((uintptr_t)planes | (uintptr_t)pi | (uintptr_t)mask | (uintptr_t)ssl.maps) & 15) != 0)
        return invalid("device outputs must lie on 16-byte boundaries");
    if (s->on_device()) return device_batch(s, rows, kinds, B, planes, pi, z, mask, ssl, outputs_on_device != 0, (hipStream_t)stream);
    s->refs.resize((size_t)B);
    int64_t missing = 0;
    if (!resolve(s, rows, kinds, B, s->refs.data(), &missing)) return invalid("row " + std::to_string(missing) + " is not resident");
    batch_rows_host(s->refs.data(), B, planes, pi, z, mask, ssl.maps, ssl.status);
    return M0_OK;
}

// m0_rowstore_batch_host and m0_rowstore_batch_ssl_host
int arrays_batch(const m0_rowpack_arrays* in, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z,
                 uint8_t* mask, const SslOut& ssl) {
    if (!in) return invalid("null argument");
    if (B <= 0) return invalid("batch must be positive");
    SegBlock block;
    const std::string why = build_segment(in, mask != nullptr, block);
    if (!why.empty()) return invalid("packed rows: " + why);
    if (const int rc = check_batch(rows, kinds, B, planes, pi, z, mask, mask != nullptr, ssl)) return rc;
    const SegView* view = reinterpret_cast<const SegView*>(block.bytes.data());
    std::vector<RowRef> refs((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (rows[b] < 0 || rows[b] >= in->n) return invalid("row " + std::to_string(rows[b]) + " is not one of the packed rows");
        refs[b] = RowRef{view, (int32_t)rows[b], kinds ? (int32_t)kinds[b] : M0_AUG_NONE};
    }
    batch_rows_host(refs.data(), B, planes, pi, z, mask, ssl.maps, ssl.status);
    return M0_OK;
}

// The rows of the two benches: those of m0_rowpack_bench (every row PACKED with a LEGAL mask) in their packed form, a store of its
// own that holds them, and the references of a batch of all B of them, kinds 0, 1, 2 in turn, in order and in a seeded shuffle.
struct BenchRows {
    std::vector<m0_rowpack_pos> hq;
    std::vector<int64_t> hpo, hmo;
    std::vector<uint16_t> hidx;
    std::vector<float> hval, hz;
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    std::vector<uint8_t> hk;
    m0_rowstore* store = nullptr;
    DevBuf<RowRef> dorder, dshuffled;

    ~BenchRows() { m0_rowstore_destroy(store); }

    int build(HipStatus& hs, int hip_device, int B) {
        const size_t N = (size_t)B;
        std::vector<float> planes, pi, z(N, 0.f);
        std::vector<uint8_t> mask;
        m0_rowpack_bench_rows(N, planes, pi, mask);
        // their packed form: the sizes first, then the arrays
        int64_t sizes[3];
        m0_rowpack_arrays a = {};
        a.n = B;
        (void)pack_host(planes.data(), pi.data(), z.data(), mask.data(), N, &a, sizes);
        hq.resize(N); hpo.resize(N + 1); hmo.resize(N + 1); hidx.resize((size_t)sizes[0]); hval.resize((size_t)sizes[0]); hz.resize(N);
        a.pi_n = sizes[0]; a.pos = hq.data(); a.z = hz.data(); a.pi_off = hpo.data(); a.mask_off = hmo.data(); a.pi_idx = hidx.data();
        a.pi_val = hval.data();
        if (sizes[1] != 0 || sizes[2] != 0 || !pack_host(planes.data(), pi.data(), z.data(), mask.data(), N, &a, sizes).empty())
            return invalid("the bench rows did not pack as positions with legal masks");
        const std::string why = check_arrays(&a, positions, raw_slot);
        if (!why.empty()) return invalid(why);
        store = m0_rowstore_create(hip_device, 1);
        int64_t first = 0;
        if (!store) return M0_ERR_HIP;
        if (const int rc = m0_rowstore_append(store, &a, &first)) return rc;
        std::vector<RowRef> order(N), shuffled(N);
        hk.resize(N);
        BenchRng rng;
        for (size_t i = 0; i < N; ++i) { hk[i] = (uint8_t)(i % m0aug::KINDS); order[i] = RowRef{store->segs.back().view(), (int32_t)i, (int32_t)hk[i]}; }
        shuffled = order;
        for (size_t i = N - 1; i > 0; --i) std::swap(shuffled[i].row, shuffled[rng.next() % (i + 1)].row);
        dorder.upload(hs, order.data(), N); dshuffled.upload(hs, shuffled.data(), N);
        return hs.ok() ? M0_OK : m0_hip_error(hs, "upload failed");
    }
};

}  // namespace

extern "C" {

m0_rowstore* m0_rowstore_create(int hip_device, int with_mask) {
    if (hip_device < M0_ROWSTORE_HOST) { m0_set_error("hip_device must be a device or M0_ROWSTORE_HOST"); return nullptr; }
    if (hip_device >= 0) {
        HipStatus hs;
        if (m0_select_device(hs, hip_device, "M0_ROWSTORE_HOST keeps the rows in host memory") != M0_OK) return nullptr;
    }
    m0_rowstore* s = new m0_rowstore;
    s->device = hip_device;
    s->with_mask = with_mask != 0;
    return s;
}

void m0_rowstore_destroy(m0_rowstore* s) {
    if (!s) return;
    if (s->on_device()) {
        (void)hipSetDevice(s->device);
        for (Slot& sl : s->slots) {
            if (sl.busy) (void)hipEventSynchronize(sl.done);
            if (sl.done) (void)hipEventDestroy(sl.done);
            if (sl.pinned) (void)hipHostFree(sl.pinned);
            if (sl.dev) (void)hipFree(sl.dev);
        }
        free_outputs(s);
        free_ssl_outputs(s);
        weights_destroy(s);
        for (Segment& g : s->segs) (void)hipFree(g.dev);
    }
    delete s;
}

int m0_rowstore_append(m0_rowstore* s, const m0_rowpack_arrays* in, int64_t* first_row) {
    if (!s) return invalid("null handle");
    if (!in || !first_row) return invalid("null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->hs.ok()) return m0_hip_error(s->hs);
    Segment g;
    const std::string why = build_segment(in, s->with_mask, g.host);
    if (!why.empty()) return invalid("packed rows: " + why);
    g.first = s->next_id; g.rows = g.host.rows; g.raw_rows = g.host.raw_rows; g.bytes = g.host.bytes.size();
    if (s->on_device()) {
        // a failed allocation is the caller's to handle (evict and try again): it does not end the store
        HipStatus hs;
        if (!M0_HIP(hs, hipSetDevice(s->device)) || !M0_HIP(hs, hipMalloc((void**)&g.dev, g.bytes))) return m0_hip_error(hs, "segment allocation failed");
        rebase_segment(g.host, g.dev);
        if (!M0_HIP(s->hs, hipMemcpy(g.dev, g.host.bytes.data(), g.bytes, hipMemcpyHostToDevice))) {
            (void)hipFree(g.dev);
            return m0_hip_error(s->hs, "segment upload failed");
        }
        g.host = SegBlock();
    }
    const int64_t rows = g.rows;
    s->segs.push_back(std::move(g));
    if (const int rc = weights_append(s)) {                               // a weighted store: the new rows get weight 1
        if (s->segs.back().dev) (void)hipFree(s->segs.back().dev);
        s->segs.pop_back();
        return rc;
    }
    *first_row = s->next_id;
    s->next_id += rows;
    return M0_OK;
}

int m0_rowstore_evict(m0_rowstore* s, int64_t keep_rows) {
    if (!s) return invalid("null handle");
    if (keep_rows < 0) return invalid("keep_rows must not be negative");
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->hs.ok()) return m0_hip_error(s->hs);
    size_t drop = 0;
    int64_t left = s->resident();
    while (drop < s->segs.size() && left - s->segs[drop].rows >= keep_rows) left -= s->segs[drop++].rows;
    if (drop == 0) return M0_OK;
    if (s->on_device()) {
        if (!M0_HIP(s->hs, hipSetDevice(s->device)) || !drain(s)) return m0_hip_error(s->hs, "waiting for the batches in flight failed");
    }
    for (size_t i = 0; i < drop; ++i) {
        weights_free_segment(s, s->segs.front());
        if (s->segs.front().dev) (void)hipFree(s->segs.front().dev);
        s->segs.pop_front();
    }
    return weights_evicted(s);
}

int m0_rowstore_info(m0_rowstore* s, int64_t* info) {
    if (!s) return invalid("null handle");
    if (!info) return invalid("null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    int64_t raw = 0, bytes = 0;
    for (const Segment& g : s->segs) { raw += g.raw_rows; bytes += (int64_t)g.bytes; }
    info[0] = s->resident();
    info[1] = s->segs.empty() ? s->next_id : s->segs.front().first;
    info[2] = s->next_id;
    info[3] = (int64_t)s->segs.size();
    info[4] = raw;
    info[5] = bytes;
    return M0_OK;
}

int m0_rowstore_batch(m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z, uint8_t* mask,
                      int outputs_on_device, void* stream) {
    return store_batch(s, rows, kinds, B, planes, pi, z, mask, SslOut(), outputs_on_device, stream);
}

int m0_rowstore_batch_ssl(m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z,
                          uint8_t* mask, float* ssl, int32_t* ssl_status, int outputs_on_device, void* stream) {
    return store_batch(s, rows, kinds, B, planes, pi, z, mask, SslOut{true, ssl, ssl_status}, outputs_on_device, stream);
}

int m0_rowstore_batch_host(const m0_rowpack_arrays* in, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi,
                           float* z, uint8_t* mask) {
    return arrays_batch(in, rows, kinds, B, planes, pi, z, mask, SslOut());
}

int m0_rowstore_batch_ssl_host(const m0_rowpack_arrays* in, const int64_t* rows, const uint8_t* kinds, int B, float* planes,
                               float* pi, float* z, uint8_t* mask, float* ssl, int32_t* ssl_status) {
    return arrays_batch(in, rows, kinds, B, planes, pi, z, mask, SslOut{true, ssl, ssl_status});
}

int m0_rowstore_bench(int hip_device, int B, int iters, float* fused_us, float* chain_us, double* dense_bytes) {
    if (B <= 0 || iters <= 0 || !fused_us || !chain_us || !dense_bytes) return invalid("invalid argument");
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t N = (size_t)B;
    BenchRows r;
    if (const int rc = r.build(hs, hip_device, B)) return rc;
    // the chain's inputs beside the store
    DevBuf<Pos> dpos;
    DevBuf<m0_rowpack_pos> dq;
    DevBuf<int64_t> dpo, dmo;
    DevBuf<uint16_t> didx, dmidx;
    DevBuf<int32_t> dslot;
    DevBuf<uint8_t> dk, um, cm, fm;
    DevBuf<float> dval, upl, upi, cpl, cpi, fpl, fpi, fz;
    dpos.upload(hs, r.positions.data(), N); dq.upload(hs, r.hq.data(), N);
    dpo.upload(hs, r.hpo.data(), N + 1); dmo.upload(hs, r.hmo.data(), N + 1);
    didx.upload(hs, r.hidx.data(), r.hidx.size()); dval.upload(hs, r.hval.data(), r.hval.size()); dmidx.upload(hs, nullptr, 0);
    dslot.upload(hs, r.raw_slot.data(), N); dk.upload(hs, r.hk.data(), N);
    if (!hs.ok() ||!upl.alloc(hs, N * PLANE_FLOATS) || !upi.alloc(hs, N * COLS) || !um.alloc(hs, N * COLS) || !cpl.alloc(hs, N * PLANE_FLOATS) ||
        !cpi.alloc(hs, N * COLS) || !cm.alloc(hs, N * COLS) || !fpl.alloc(hs, N * PLANE_FLOATS) || !fpi.alloc(hs, N * COLS) ||
        !fm.alloc(hs, N * COLS) || !fz.alloc(hs, N)) return m0_hip_error(hs, "hipMalloc or upload failed");
    const RowRef* refs = r.dorder.p;
    auto fused = [&]() { return M0_HIP(hs, launch_batch_rows(refs, B, fpl.p, fpi.p, fz.p, fm.p, nullptr)); };
    auto chain = [&]() {
        M0_HIP(hs, launch_encode_positions(dpos.p, B, upl.p, nullptr, um.p, nullptr, nullptr, nullptr, nullptr));
        M0_HIP(hs, launch_rowpack_unpack(dq.p, dpo.p, didx.p, dval.p, dmo.p, dmidx.p, dslot.p, nullptr, nullptr, nullptr, B, upl.p, upi.p,
                                         um.p, nullptr));
        return M0_HIP(hs, launch_augment_rows(upl.p, upi.p, um.p, dk.p, M0_AUG_NONE, B, M0_PLANES, cpl.p, cpi.p, cm.p, nullptr));
    };
    // the warm-up is the check: the rows in order give the chain's bytes
    fused(); chain();
    std::vector<uint8_t> got(N * COLS * sizeof(float)), want(N * COLS * sizeof(float));
    const struct { const void* f; const void* c; size_t bytes; } outs[3] = {{fpl.p, cpl.p, N * PLANE_FLOATS * sizeof(float)},
                                                                            {fpi.p, cpi.p, N * COLS * sizeof(float)}, {fm.p, cm.p, N * COLS}};
    for (const auto& o : outs) {
        M0_HIP(hs, hipMemcpy(got.data(), o.f, o.bytes, hipMemcpyDeviceToHost));
        M0_HIP(hs, hipMemcpy(want.data(), o.c, o.bytes, hipMemcpyDeviceToHost));
        if (!hs.ok()) return m0_hip_error(hs, "row store bench failed");
        if (memcmp(got.data(), want.data(), o.bytes) != 0) return invalid("the fused batch is not the chain's");
    }
    refs = r.dshuffled.p;
    fused();
    for (int run = 0; run < 2; ++run) {
        fused_us[run] = m0_time_iterations(hs, nullptr, iters, fused) * 1000.f;
        chain_us[run] = m0_time_iterations(hs, nullptr, iters, chain) * 1000.f;
    }
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "row store bench failed");
    *dense_bytes = (double)B * (PLANE_FLOATS * 4.0 + COLS * 4.0 + COLS + 4.0);
    return M0_OK;
}

int m0_rowstore_bench_ssl(int hip_device, int B, int iters, float* fused_us, float* chain_us, double* dense_bytes) {
    if (B <= 0 || iters <= 0 || !fused_us || !chain_us || !dense_bytes) return invalid("invalid argument");
    HipStatus hs;
    if (const int rc = m0_select_device(hs, hip_device)) return rc;
    const size_t N = (size_t)B;
    BenchRows r;
    if (const int rc = r.build(hs, hip_device, B)) return rc;
    // one set of outputs for the launch with the maps (f), one for the launch without them and the targets kernel behind it (c)
    DevBuf<uint8_t> fm, cm;
    DevBuf<float> fpl, fpi, fz, fssl, cpl, cpi, cz, cssl;
    DevBuf<int32_t> fst, cst;
    if (!fpl.alloc(hs, N * PLANE_FLOATS) || !fpi.alloc(hs, N * COLS) || !fm.alloc(hs, N * COLS) || !fz.alloc(hs, N) || !fssl.alloc(hs, N * SSL_FLOATS) ||
        !fst.alloc(hs, N) || !cpl.alloc(hs, N * PLANE_FLOATS) || !cpi.alloc(hs, N * COLS) || !cm.alloc(hs, N * COLS) || !cz.alloc(hs, N) ||
        !cssl.alloc(hs, N * SSL_FLOATS) || !cst.alloc(hs, N)) return m0_hip_error(hs, "hipMalloc failed");
    const RowRef* refs = r.dshuffled.p;
    auto fused = [&]() { return M0_HIP(hs, launch_batch_rows_ssl(refs, B, fpl.p, fpi.p, fz.p, fm.p, fssl.p, fst.p, nullptr)); };
    auto chain = [&]() {
        M0_HIP(hs, launch_batch_rows(refs, B, cpl.p, cpi.p, cz.p, cm.p, nullptr));
        return M0_HIP(hs, launch_ssl_targets_planes(cpl.p, B, cssl.p, cst.p, nullptr));
    };
    // the warm-up is the check: both give the same bytes (every row is a position, so the targets kernel writes every map)
    fused(); chain();
    std::vector<uint8_t> got(N * COLS * sizeof(float)), want(N * COLS * sizeof(float));
    const struct { const void* f; const void* c; size_t bytes; } outs[6] = {
        {fpl.p, cpl.p, N * PLANE_FLOATS * sizeof(float)}, {fpi.p, cpi.p, N * COLS * sizeof(float)}, {fm.p, cm.p, N * COLS},
        {fz.p, cz.p, N * sizeof(float)}, {fssl.p, cssl.p, N * SSL_FLOATS * sizeof(float)}, {fst.p, cst.p, N * sizeof(int32_t)}};
    for (const auto& o : outs) {
        M0_HIP(hs, hipMemcpy(got.data(), o.f, o.bytes, hipMemcpyDeviceToHost));
        M0_HIP(hs, hipMemcpy(want.data(), o.c, o.bytes, hipMemcpyDeviceToHost));
        if (!hs.ok()) return m0_hip_error(hs, "row store bench failed");
        if (memcmp(got.data(), want.data(), o.bytes) != 0) return invalid("the batch with the maps is not the chain's");
    }
    for (int run = 0; run < 2; ++run) {
        fused_us[run] = m0_time_iterations(hs, nullptr, iters, fused) * 1000.f;
        chain_us[run] = m0_time_iterations(hs, nullptr, iters, chain) * 1000.f;
    }
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "row store bench failed");
    *dense_bytes = (double)B * (PLANE_FLOATS * 4.0 + COLS * 4.0 + COLS + 4.0 + SSL_FLOATS * 4.0 + 4.0);
    return M0_OK;
}

}  // extern "C"
