// extern "C" entry points of the weighted row store (include/m0_batch_weighted.h): a weight per resident row, written, drawn from
// and gathered on the device.  The store is that of capi_batch.hip (rowstore.h); the kernels are sample_kernels.hip, a host store
// runs sample_host.h, and both run the rules of sample_core.h.
//
// A store becomes weighted at its first call here (enable): every resident segment gets one allocation of weights and block sums,
// filled with weight 1, and the segment table goes to device memory.  From then on append adds the new segment's entry behind the
// others (entries in flight are not touched) and eviction, behind its drain, rewrites the table.  Every slot of the store's ring
// carries a block-prefix buffer, sized with the table, so a draw allocates nothing.  A draw, and a weight write from device
// memory, take a slot and record its event as a batch does: the host runs at most SLOTS of them ahead, and eviction's drain
// covers them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "batch_host.h"
#include "capi_common.h"
#include "rowstore.h"
#include "sample_host.h"
#include "sample_kernels.h"

using namespace m0store;
using namespace m0sample;
using m0batch::COLS;

namespace {

size_t weight_floats_bytes(int64_t rows) { return ((size_t)rows * sizeof(float) + 15) / 16 * 16; }

// s->table and s->blocks from the resident segments
void rebuild_table(m0_rowstore* s) {
    s->table.clear();
    int block0 = 0;
    for (Segment& g : s->segs) {
        SegEntry e;
        e.first = g.first; e.rows = g.rows; e.view = g.view();
        e.w = g.wdev ? reinterpret_cast<float*>(g.wdev) : g.hw.data();
        e.bsum = g.wdev ? reinterpret_cast<uint64_t*>(g.wdev + weight_floats_bytes(g.rows)) : g.hbsum.data();
        e.block0 = block0; e.blocks = blocks_of(g.rows);
        block0 += e.blocks;
        s->table.push_back(e);
    }
    s->blocks = block0;
}

// memory for the weights of a segment that has none; false with a message when it cannot be had (the store goes on)
bool alloc_weights(m0_rowstore* s, Segment& g) {
    if (s->on_device()) {
        HipStatus hs;
        if (!M0_HIP(hs, hipMalloc((void**)&g.wdev, weight_floats_bytes(g.rows) + (size_t)blocks_of(g.rows) * sizeof(uint64_t)))) {
            g.wdev = nullptr;
            m0_hip_error(hs, "weight allocation failed");
            return false;
        }
    } else {
        g.hw.assign((size_t)g.rows, 1.f);
        g.hbsum.assign((size_t)blocks_of(g.rows), 0);
    }
    return true;
}

// the device copy of the table from entry `from` on, and prefix buffers that hold its blocks; both grow behind a drain
bool upload_table(m0_rowstore* s, size_t from) {
    const size_t n = s->table.size();
    if ((size_t)s->table_cap < n) {
        drain(s);
        (void)hipFree(s->table_dev);
        s->table_dev = nullptr;
        s->table_cap = (int)std::max<size_t>(2 * n, 16);
        M0_HIP(s->hs, hipMalloc((void**)&s->table_dev, (size_t)s->table_cap * sizeof(SegEntry)));
        from = 0;
    }
    if (s->pre_cap < s->blocks + 1) {
        drain(s);
        s->pre_cap = std::max(2 * (s->blocks + 1), 64);
        for (Slot& sl : s->slots) {
            (void)hipFree(sl.pre);
            sl.pre = nullptr;
            M0_HIP(s->hs, hipMalloc((void**)&sl.pre, (size_t)s->pre_cap * sizeof(uint64_t)));
        }
    }
    if (from < n) M0_HIP(s->hs, hipMemcpy(s->table_dev + from, s->table.data() + from, (n - from) * sizeof(SegEntry), hipMemcpyHostToDevice));
    return s->hs.ok();
}

// blocks k0 .. k0 + nk - 1 filled or scaled, done when it returns
int rewrite_blocks(m0_rowstore* s, int k0, int nk, bool scale, int64_t lo, int64_t hi, float value) {
    if (nk <= 0) return M0_OK;
    const int nseg = (int)s->table.size();
    if (!s->on_device()) {
        host_rewrite_blocks(s->table.data(), nseg, k0, nk, scale, lo, hi, value);
        return M0_OK;
    }
    M0_HIP(s->hs, launch_rewrite_blocks(s->table_dev, nseg, k0, nk, scale ? M0_REWRITE_SCALE : M0_REWRITE_FILL, lo, hi, value, nullptr));
    M0_HIP(s->hs, hipStreamSynchronize(nullptr));
    return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "weight kernel failed");
}

// what every call here does first, under the store's mutex: the store is usable, its device current, and it has weights
int enable(m0_rowstore* s) {
    if (!s->hs.ok()) return m0_hip_error(s->hs);
    if (s->resident() > (int64_t)M0_WEIGHT_ROWS_MAX) return invalid("more than 2^23 resident rows: no weights");
    if (s->on_device() && !M0_HIP(s->hs, hipSetDevice(s->device))) return m0_hip_error(s->hs);
    if (s->weighted) return M0_OK;
    for (Segment& g : s->segs)
        if (!alloc_weights(s, g)) {
            for (Segment& h : s->segs) weights_free_segment(s, h);
            return M0_ERR_HIP;
        }
    rebuild_table(s);
    if (s->on_device()) {
        M0_HIP(s->hs, hipMalloc((void**)&s->counters_dev, 2 * sizeof(uint64_t)));
        M0_HIP(s->hs, hipMemset(s->counters_dev, 0, 2 * sizeof(uint64_t)));
        if (!upload_table(s, 0)) return m0_hip_error(s->hs, "weight staging failed");
    }
    s->weighted = true;
    return rewrite_blocks(s, 0, s->blocks, false, INT64_MIN, INT64_MAX, 1.f);
}

// the block of a resident id
int block_of_id(const m0_rowstore* s, int64_t id) {
    const SegEntry& e = s->table[(size_t)segment_of(s->table.data(), (int)s->table.size(), id)];
    return e.block0 + (int)((id - e.first) / BLOCK_ROWS);
}

bool resident_id(const m0_rowstore* s, int64_t id) { return !s->segs.empty() && id >= s->segs.front().first && id < s->next_id; }

// outputs of a draw that goes to host memory
bool stage_draw(m0_rowstore* s, int B) {
    if (s->o_draw_cap >= B) return true;
    drain(s);
    (void)hipFree(s->o_ids); (void)hipFree(s->o_prob);
    s->o_ids = nullptr; s->o_prob = nullptr; s->o_draw_cap = 0;
    M0_HIP(s->hs, hipMalloc((void**)&s->o_ids, (size_t)B * sizeof(int64_t)));
    M0_HIP(s->hs, hipMalloc((void**)&s->o_prob, (size_t)B * sizeof(float)));
    if (s->hs.ok()) s->o_draw_cap = B;
    return s->hs.ok();
}

int check_draw(const m0_rowstore* s, int B, const int64_t* ids_out, const float* prob_out, int outputs_on_device) {
    if (B <= 0) return invalid("batch must be positive");
    if (!ids_out || !prob_out) return invalid("null argument");
    if (outputs_on_device && !s->on_device()) return invalid("a host store fills host memory");
    if (s->segs.empty()) return invalid("nothing is resident: nothing to draw from");
    return M0_OK;
}

int download_draw(m0_rowstore* s, int B, int64_t* ids_out, float* prob_out) {
    M0_HIP(s->hs, hipMemcpy(ids_out, s->o_ids, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToHost));
    M0_HIP(s->hs, hipMemcpy(prob_out, s->o_prob, (size_t)B * sizeof(float), hipMemcpyDeviceToHost));
    return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "download failed");
}

// a host store's draw: ids, prob and, when not null, the references
void host_store_draw(m0_rowstore* s, int B, uint64_t seed, uint64_t draw, int stratified, int64_t* ids_out, float* prob_out, RowRef* refs) {
    s->hpre.resize((size_t)s->blocks + 1);
    host_block_prefix(s->table.data(), (int)s->table.size(), s->blocks, s->hpre.data());
    if (host_draw(s->table.data(), (int)s->table.size(), s->blocks, s->hpre.data(), B, seed, draw, stratified != 0, ids_out, prob_out, refs))
        s->counters[1] += 1;
}

}  // namespace

namespace m0store {

int score_gather(m0_rowstore* s, const int64_t* ids, const uint8_t* kinds, int B, float* planes, float* pi, float* z, uint8_t* mask,
                 bool with_weights, hipStream_t st, Slot** slot) {
    if (!s->hs.ok()) return m0_hip_error(s->hs);
    if (with_weights) {
        if (const int rc = enable(s)) return rc;
    } else if (!M0_HIP(s->hs, hipSetDevice(s->device))) {
        return m0_hip_error(s->hs);
    }
    Slot* sl = take_slot(s, B);
    if (!sl) return m0_hip_error(s->hs, "row store staging failed");
    int64_t missing = 0;
    if (!resolve(s, ids, kinds, B, sl->pinned, &missing)) return invalid("row " + std::to_string(missing) + " is not resident");
    BatchOut dev;
    dev.planes = planes; dev.pi = pi; dev.z = z; dev.mask = mask;
    M0_HIP(s->hs, hipMemcpyAsync(sl->dev, sl->pinned, (size_t)B * sizeof(RowRef), hipMemcpyHostToDevice, st));
    *slot = sl;
    return finish_batch(s, sl, B, dev, dev, true, st);
}

int score_weights(m0_rowstore* s, Slot* slot, int B, const float* score_rows_dev, const m0_weight_rule& rule, hipStream_t st) {
    M0_HIP(s->hs, launch_score_weights(s->table_dev, (int)s->table.size(), slot->dev, score_rows_dev, B, rule, st));
    if (M0_HIP(s->hs, hipEventRecord(slot->done, st))) slot->busy = true;  // the slot is free once this kernel has run, too
    return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "weight launch failed");
}

int weights_append(m0_rowstore* s) {
    if (!s->weighted) return M0_OK;
    Segment& g = s->segs.back();
    if (s->on_device() && !M0_HIP(s->hs, hipSetDevice(s->device))) return m0_hip_error(s->hs);
    if (!alloc_weights(s, g)) return M0_ERR_HIP;
    const int k0 = s->blocks;
    rebuild_table(s);
    if (s->on_device() && !upload_table(s, s->table.size() - 1)) return m0_hip_error(s->hs, "weight staging failed");
    return rewrite_blocks(s, k0, s->blocks - k0, false, g.first, g.first + g.rows, 1.f);
}

void weights_free_segment(m0_rowstore* s, Segment& g) {
    (void)s;
    if (g.wdev) (void)hipFree(g.wdev);
    g.wdev = nullptr;
    g.hw.clear(); g.hbsum.clear();
}

int weights_evicted(m0_rowstore* s) {
    if (!s->weighted) return M0_OK;
    rebuild_table(s);
    if (s->on_device() && !upload_table(s, 0)) return m0_hip_error(s->hs, "weight staging failed");
    return M0_OK;
}

void weights_destroy(m0_rowstore* s) {
    for (Slot& sl : s->slots) { (void)hipFree(sl.pre); sl.pre = nullptr; }
    (void)hipFree(s->table_dev); (void)hipFree(s->counters_dev); (void)hipFree(s->o_ids); (void)hipFree(s->o_prob);
    for (Segment& g : s->segs) weights_free_segment(s, g);
}

}  // namespace m0store

extern "C" {

int m0_rowstore_set_weights(m0_rowstore* s, const int64_t* ids, const float* values, int64_t n, int on_device, void* stream) {
    if (!s) return invalid("null handle");
    if (n < 0 || (n > 0 && (!ids || !values))) return invalid(n < 0 ? "n must not be negative" : "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    if (on_device && !s->on_device()) return invalid("a host store takes weights from host memory");
    if (const int rc = enable(s)) return rc;
    if (n == 0) return M0_OK;
    const int nseg = (int)s->table.size();
    if (on_device) {
        if (nseg == 0) return invalid("nothing is resident");
        Slot* sl = take_slot(s, std::max(s->slots[0].cap, 1));
        if (!sl) return m0_hip_error(s->hs, "row store staging failed");
        M0_HIP(s->hs, launch_set_weights(s->table_dev, nseg, ids, values, n, s->counters_dev, (hipStream_t)stream));
        if (M0_HIP(s->hs, hipEventRecord(sl->done, (hipStream_t)stream))) sl->busy = true;
        return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "weight launch failed");
    }
    for (int64_t i = 0; i < n; ++i) {
        if (!resident_id(s, ids[i])) return invalid("row " + std::to_string(ids[i]) + " is not resident");
        if (!valid_weight(values[i])) return invalid("a weight must be finite and lie in [0, 65536]: value " + std::to_string(i));
    }
    std::vector<int64_t> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end()) return invalid("row " + std::to_string(*twice) + " occurs more than once");
    if (!s->on_device()) {
        host_set_weights(s->table.data(), nseg, ids, values, n);
        return M0_OK;
    }
    DevBuf<int64_t> dids;
    DevBuf<float> dvalues;
    HipStatus hs;                                                         // a failed allocation here does not end the store
    if (!dids.upload(hs, ids, (size_t)n) || !dvalues.upload(hs, values, (size_t)n) || !M0_HIP(hs, hipStreamSynchronize(nullptr)))
        return m0_hip_error(hs, "weight upload failed");
    M0_HIP(s->hs, launch_set_weights(s->table_dev, nseg, dids.p, dvalues.p, n, s->counters_dev, nullptr));
    M0_HIP(s->hs, hipStreamSynchronize(nullptr));
    return s->hs.ok() ? M0_OK : m0_hip_error(s->hs, "weight kernel failed");
}

int m0_rowstore_fill_weights(m0_rowstore* s, int64_t first_id, int64_t n, float value) {
    if (!s) return invalid("null handle");
    if (n < 0) return invalid("n must not be negative");
    if (!valid_weight(value)) return invalid("a weight must be finite and lie in [0, 65536]");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = enable(s)) return rc;
    if (n == 0) return M0_OK;
    if (!resident_id(s, first_id)) return invalid("row " + std::to_string(first_id) + " is not resident");
    if (n > s->next_id - first_id) return invalid("row " + std::to_string(s->next_id) + " is not resident");
    const int k0 = block_of_id(s, first_id), k1 = block_of_id(s, first_id + n - 1);
    return rewrite_blocks(s, k0, k1 - k0 + 1, false, first_id, first_id + n, value);
}

int m0_rowstore_scale_weights(m0_rowstore* s, float factor) {
    if (!s) return invalid("null handle");
    if (!(factor >= 0.f) || isinf(factor)) return invalid("factor must be finite and not negative");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = enable(s)) return rc;
    return rewrite_blocks(s, 0, s->blocks, true, 0, 0, factor);
}

int m0_rowstore_get_weights(m0_rowstore* s, const int64_t* ids, int64_t n, float* out_host) {
    if (!s) return invalid("null handle");
    if (n < 0 || (n > 0 && (!ids || !out_host))) return invalid(n < 0 ? "n must not be negative" : "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = enable(s)) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (!resident_id(s, ids[i])) return invalid("row " + std::to_string(ids[i]) + " is not resident");
    if (n == 0) return M0_OK;
    const int nseg = (int)s->table.size();
    // a device store: the weights of the segments the ids touch, downloaded once each
    std::vector<std::vector<float>> copy((size_t)nseg);
    if (s->on_device()) M0_HIP(s->hs, hipDeviceSynchronize());
    for (int64_t i = 0; i < n; ++i) {
        const int g = segment_of(s->table.data(), nseg, ids[i]);
        const SegEntry& e = s->table[(size_t)g];
        if (s->on_device() && copy[(size_t)g].empty()) {
            copy[(size_t)g].resize((size_t)e.rows);
            M0_HIP(s->hs, hipMemcpy(copy[(size_t)g].data(), e.w, (size_t)e.rows * sizeof(float), hipMemcpyDeviceToHost));
            if (!s->hs.ok()) return m0_hip_error(s->hs, "download failed");
        }
        out_host[i] = s->on_device() ? copy[(size_t)g][(size_t)(ids[i] - e.first)] : e.w[ids[i] - e.first];
    }
    return M0_OK;
}

int m0_rowstore_weights_info(m0_rowstore* s, int64_t* info) {
    if (!s) return invalid("null handle");
    if (!info) return invalid("null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = enable(s)) return rc;
    uint64_t total = 0, counters[2] = {s->counters[0], s->counters[1]};
    int64_t with_ticks = 0;
    if (s->on_device()) {
        M0_HIP(s->hs, hipDeviceSynchronize());
        M0_HIP(s->hs, hipMemcpy(counters, s->counters_dev, sizeof(counters), hipMemcpyDeviceToHost));
    }
    std::vector<uint8_t> copy;
    for (const SegEntry& e : s->table) {
        const float* w = e.w;
        const uint64_t* bsum = e.bsum;
        if (s->on_device()) {
            copy.resize(weight_floats_bytes(e.rows) + (size_t)e.blocks * sizeof(uint64_t));
            M0_HIP(s->hs, hipMemcpy(copy.data(), e.w, copy.size(), hipMemcpyDeviceToHost));
            if (!s->hs.ok()) break;
            w = reinterpret_cast<const float*>(copy.data());
            bsum = reinterpret_cast<const uint64_t*>(copy.data() + weight_floats_bytes(e.rows));
        }
        for (int j = 0; j < e.blocks; ++j) total += bsum[j];
        for (int64_t i = 0; i < e.rows; ++i) with_ticks += ticks(w[i]) != 0;
    }
    if (!s->hs.ok()) return m0_hip_error(s->hs, "download failed");
    info[0] = (int64_t)total; info[1] = with_ticks; info[2] = (int64_t)counters[0]; info[3] = (int64_t)counters[1];
    return M0_OK;
}

int m0_rowstore_sample(m0_rowstore* s, int B, uint64_t seed, uint64_t draw, int stratified, int64_t* ids_out, float* prob_out,
                       int outputs_on_device, void* stream) {
    if (!s) return invalid("null handle");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = check_draw(s, B, ids_out, prob_out, outputs_on_device)) return rc;
    if (const int rc = enable(s)) return rc;
    if (!s->on_device()) {
        host_store_draw(s, B, seed, draw, stratified, ids_out, prob_out, nullptr);
        return M0_OK;
    }
    hipStream_t st = outputs_on_device ? (hipStream_t)stream : nullptr;
    Slot* sl = take_slot(s, std::max(s->slots[0].cap, 1));
    if (!sl || (!outputs_on_device && !stage_draw(s, B))) return m0_hip_error(s->hs, "row store staging failed");
    M0_HIP(s->hs, launch_draw(s->table_dev, (int)s->table.size(), s->blocks, sl->pre, B, seed, draw, stratified,
                              outputs_on_device ? ids_out : s->o_ids, outputs_on_device ? prob_out : s->o_prob, nullptr, s->counters_dev, st));
    if (M0_HIP(s->hs, hipEventRecord(sl->done, st))) sl->busy = true;
    if (!s->hs.ok()) return m0_hip_error(s->hs, "draw launch failed");
    if (outputs_on_device) return M0_OK;
    if (!M0_HIP(s->hs, hipEventSynchronize(sl->done))) return m0_hip_error(s->hs, "draw kernel failed");
    sl->busy = false;
    return download_draw(s, B, ids_out, prob_out);
}

int m0_rowstore_batch_sampled(m0_rowstore* s, int B, uint64_t seed, uint64_t draw, int stratified, const uint8_t* kinds, float* planes,
                              float* pi, float* z, uint8_t* mask, float* ssl, int32_t* ssl_status, int64_t* ids_out, float* prob_out,
                              int outputs_on_device, void* stream) {
    if (!s) return invalid("null handle");
    std::lock_guard<std::mutex> lk(s->mu);
    if (const int rc = check_draw(s, B, ids_out, prob_out, outputs_on_device)) return rc;
    if (!planes || !pi || !z || (ssl != nullptr) != (ssl_status != nullptr)) return invalid("null argument");
    if ((mask != nullptr) != s->with_mask) return invalid(s->with_mask ? "the rows have masks: a mask output is required" : "the rows have no masks: no mask output");
    if (kinds)
        if (const char* why = m0_bad_kinds(kinds, B)) return invalid(why);
    if (outputs_on_device && (((uintptr_t)planes | (uintptr_t)pi | (uintptr_t)mask | (uintptr_t)ssl) & 15) != 0)
        return invalid("device outputs must lie on 16-byte boundaries");
    if (const int rc = enable(s)) return rc;
    const SslOut maps{ssl != nullptr, ssl, ssl_status};
    if (!s->on_device()) {
        s->refs.resize((size_t)B);
        for (int b = 0; b < B; ++b) s->refs[(size_t)b] = RowRef{nullptr, 0, kinds ? (int32_t)kinds[b] : M0_AUG_NONE};
        host_store_draw(s, B, seed, draw, stratified, ids_out, prob_out, s->refs.data());
        m0batch::batch_rows_host(s->refs.data(), B, planes, pi, z, mask, ssl, ssl_status);
        return M0_OK;
    }
    hipStream_t st = outputs_on_device ? (hipStream_t)stream : nullptr;
    Slot* sl = take_slot(s, B);
    if (!sl) return m0_hip_error(s->hs, "row store staging failed");
    // the kinds cross with the descriptor copy; the draw behind it writes {seg, row} of each reference on the device
    for (int b = 0; b < B; ++b) sl->pinned[b] = RowRef{nullptr, 0, kinds ? (int32_t)kinds[b] : M0_AUG_NONE};
    const BatchOut user{planes, pi, z, mask, maps};
    BatchOut dev = user;
    if (const int rc = stage_outputs(s, B, outputs_on_device != 0, dev)) return rc;
    if (!outputs_on_device && !stage_draw(s, B)) return m0_hip_error(s->hs, "row store staging failed");
    M0_HIP(s->hs, hipMemcpyAsync(sl->dev, sl->pinned, (size_t)B * sizeof(RowRef), hipMemcpyHostToDevice, st));
    M0_HIP(s->hs, launch_draw(s->table_dev, (int)s->table.size(), s->blocks, sl->pre, B, seed, draw, stratified,
                              outputs_on_device ? ids_out : s->o_ids, outputs_on_device ? prob_out : s->o_prob, sl->dev, s->counters_dev, st));
    if (!s->hs.ok()) return m0_hip_error(s->hs, "draw launch failed");
    if (const int rc = finish_batch(s, sl, B, dev, user, outputs_on_device != 0, st)) return rc;
    return outputs_on_device ? M0_OK : download_draw(s, B, ids_out, prob_out);
}

int m0_weight_from_score(const float* rows, int B, const m0_weight_rule* rule, float* out) {
    if (!rows || !out) return invalid("null argument");
    if (B <= 0) return invalid("batch must be positive");
    if (const char* why = bad_rule(rule)) return invalid(why);
    for (int b = 0; b < B; ++b) {
        const float* c = rows + (size_t)b * M0_SCORE_COLS;
        out[b] = weight_from_score(*rule, c[0], c[1], c[2]);
    }
    return M0_OK;
}

}  // extern "C"
