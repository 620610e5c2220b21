// The resident row store as its translation units share it: capi_batch.hip (include/m0_batch.h, m0_batch_ssl.h: segments, slots,
// batches) and capi_batch_weighted.hip (include/m0_batch_weighted.h: a weight per row, draws).  Everything here is used under the
// store's mutex.
#pragma once
#include <hip/hip_runtime.h>
#include <deque>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "batch_host.h"
#include "hip_check.h"
#include "sample_core.h"

namespace m0store {

using m0batch::RowRef;
using m0batch::SegBlock;
using m0batch::SegView;

constexpr int SLOTS = 4;

struct Segment {
    int64_t first = 0, rows = 0, raw_rows = 0;
    size_t bytes = 0;
    uint8_t* dev = nullptr;               // a device store's copy of the block
    SegBlock host;                        // a host store's block
    // a weighted store's weights f32 [rows] and, behind them on a 16-byte boundary, block sums u64 [blocks]: one device
    // allocation, or the two host arrays
    uint8_t* wdev = nullptr;
    std::vector<float> hw;
    std::vector<uint64_t> hbsum;
    const SegView* view() const { return reinterpret_cast<const SegView*>(dev ? dev : host.bytes.data()); }
};

struct Slot {
    RowRef* pinned = nullptr;
    RowRef* dev = nullptr;
    int cap = 0;
    hipEvent_t done = nullptr;
    bool busy = false;
    uint64_t* pre = nullptr;              // a weighted device store: the block prefix of the draw this slot carries
};

// the two outputs m0_rowstore_batch_ssl adds; `asked` false: a batch without them
struct SslOut {
    bool asked = false;
    float* maps = nullptr;
    int32_t* status = nullptr;
};

// the outputs of a batch: the caller's, or where the kernel writes them
struct BatchOut {
    float* planes = nullptr;
    float* pi = nullptr;
    float* z = nullptr;
    uint8_t* mask = nullptr;
    SslOut ssl;
};

}  // namespace m0store

struct m0_rowstore {
    int device = M0_ROWSTORE_HOST;
    bool with_mask = false;
    HipStatus hs;
    std::mutex mu;
    std::deque<m0store::Segment> segs;
    int64_t next_id = 0;
    m0store::Slot slots[m0store::SLOTS];
    unsigned turn = 0;
    std::vector<m0store::RowRef> refs;    // a host store's descriptor
    // outputs of a batch that goes to host memory
    float* o_planes = nullptr;
    float* o_pi = nullptr;
    float* o_z = nullptr;
    uint8_t* o_mask = nullptr;
    int o_cap = 0;
    // ... and of its SSL target maps, from the first batch that asks for them (m0_rowstore_batch_ssl)
    float* o_ssl = nullptr;
    int32_t* o_status = nullptr;
    int o_ssl_cap = 0;
    // ---- weights (capi_batch_weighted.hip), from the first weighted call on ----
    bool weighted = false;
    std::vector<m0sample::SegEntry> table;        // the resident segments; a device store's copy of it is table_dev
    int blocks = 0;                               // of all segments
    m0sample::SegEntry* table_dev = nullptr;
    int table_cap = 0;
    int pre_cap = 0;                              // of every slot's pre
    uint64_t* counters_dev = nullptr;             // [2]: values sanitised or skipped, degenerate draws
    uint64_t counters[2] = {0, 0};                // a host store's
    std::vector<uint64_t> hpre;                   // a host store's block prefix
    int64_t* o_ids = nullptr;                     // outputs of a draw that goes to host memory
    float* o_prob = nullptr;
    int o_draw_cap = 0;

    bool on_device() const { return device >= 0; }
    int64_t resident() const { return segs.empty() ? 0 : segs.back().first + segs.back().rows - segs.front().first; }
};

namespace m0store {

int invalid(const std::string& why);
// every batch, draw and weight write enqueued so far has finished
bool drain(m0_rowstore* s);
// the slot of this batch, free and holding B references
Slot* take_slot(m0_rowstore* s, int B);
// refs [B] of the ids, or the first id that is not resident in *missing
bool resolve(const m0_rowstore* s, const int64_t* rows, const uint8_t* kinds, int B, RowRef* refs, int64_t* missing);
// dev: the caller's outputs on the way in; for outputs in host memory the store's staging outputs (grown when B needs it) on the
// way out
int stage_outputs(m0_rowstore* s, int B, bool outputs_on_device, BatchOut& dev);
// the batch of the references in sl->dev, launched on `stream` behind whatever filled them; the slot's event behind it; and for
// outputs in host memory the wait and the download from dev into user
int finish_batch(m0_rowstore* s, Slot* sl, int B, const BatchOut& dev, const BatchOut& user, bool outputs_on_device, hipStream_t stream);
// the hooks of a weighted store in append, evict and destroy (capi_batch_weighted.hip); none does anything for a store without
// weights and returns M0_OK.  weights_append: weight 1 for the rows of the segment just pushed (an error: they could not be had,
// the message is set and the caller drops the segment).  weights_free_segment and weights_evicted: for each segment eviction
// drops, and once after them, behind the drain.
// m0_net_score_resident (capi_net.hip), which holds the store's mutex around both.  score_gather: the batch of these ids and
// kinds written to device memory on `st` as m0_rowstore_batch writes it (mask exactly when the store has masks), *slot the slot
// that carries its references; with_weights: the store gets its weights first.  score_weights: behind the score kernel on `st`,
// every row of that batch gets the rule's weight of its columns in score_rows_dev f32 [B][M0_SCORE_COLS].
int score_gather(m0_rowstore* s, const int64_t* ids, const uint8_t* kinds, int B, float* planes, float* pi, float* z, uint8_t* mask,
                 bool with_weights, hipStream_t st, Slot** slot);
int score_weights(m0_rowstore* s, Slot* slot, int B, const float* score_rows_dev, const m0_weight_rule& rule, hipStream_t st);
int weights_append(m0_rowstore* s);
void weights_free_segment(m0_rowstore* s, Segment& g);
int weights_evicted(m0_rowstore* s);
void weights_destroy(m0_rowstore* s);

}  // namespace m0store
