// extern "C" entry points of the network seam (include/m0_engine.h).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "net.h"
#include "capi_common.h"
#include "score_core.h"
#include "score_kernels.h"
#include "ssl_score_core.h"
#include "ssl_score_kernels.h"
#include "augment_kernels.h"
#include "rowstore.h"

thread_local std::string g_m0_last_error;

void m0_set_error(const std::string& s) { g_m0_last_error = s; }

// One staging array of a network handle: where its device pointer lives and how many bytes a row takes.
struct StagedArray {
    void** p;
    size_t row_bytes;
    template <typename T>
    StagedArray(T*& ptr, size_t per_row) : p((void**)&ptr), row_bytes(per_row * sizeof(T)) {}
};

// The arrays of a group grow together and share one capacity; a call reserves only the groups it uses.
enum { STAGE_IO, STAGE_SCORE, STAGE_SSL_SCORE, STAGE_AUG, STAGE_GROUPS };
static const char* const STAGE_GROW_ERROR[STAGE_GROUPS] = {"hipMalloc failed for I/O staging", "hipMalloc failed for score staging",
                                                           "hipMalloc failed for SSL score staging",
                                                           "hipMalloc failed for augmentation staging"};

struct m0_net {
    Net* net = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    int cap[STAGE_GROUPS] = {0, 0, 0, 0};               // rows every array of the group holds; 0 after a failed growth
    // STAGE_IO: the host-facing infer call
    float *planes_dev = nullptr, *logits_dev = nullptr, *value_dev = nullptr, *ssl_dev = nullptr;
    // STAGE_SCORE, m0_net_score: the stored targets in, the score columns out
    float *score_pi_dev = nullptr, *score_z_dev = nullptr, *score_rows_dev = nullptr;
    uint8_t* score_mask_dev = nullptr;
    // STAGE_SSL_SCORE, m0_net_score_ssl: stored SSL targets in, the SSL score columns out
    float *ssl_targets_dev = nullptr, *ssl_rows_dev = nullptr;
    // STAGE_AUG, m0_net_score_aug: the kinds in, the transformed planes, pi and mask that its forward and score kernel read
    uint8_t *aug_kinds_dev = nullptr, *aug_mask_dev = nullptr;
    float *aug_planes_dev = nullptr, *aug_pi_dev = nullptr;

    // a group as (array, elements per row); a staging array is listed here and nowhere else
    std::vector<StagedArray> staging(int group) {
        const size_t planes = (size_t)net->cfg().planes * 64, sslc = net->ssl_channels_total() > 0 ? net->ssl_channels_total() : 1;
        switch (group) {
        case STAGE_IO: return {{planes_dev, planes}, {logits_dev, M0_POLICY_SIZE}, {value_dev, 1}, {ssl_dev, sslc * 64}};
        case STAGE_SCORE: return {{score_pi_dev, M0_POLICY_SIZE}, {score_z_dev, 1}, {score_mask_dev, M0_POLICY_SIZE}, {score_rows_dev, M0_SCORE_COLS}};
        case STAGE_SSL_SCORE: return {{ssl_targets_dev, (size_t)m0ssl::TARGET_CH * 64}, {ssl_rows_dev, M0_SSL_SCORE_COLS}};
        case STAGE_AUG: return {{aug_kinds_dev, 1}, {aug_planes_dev, planes}, {aug_pi_dev, M0_POLICY_SIZE}, {aug_mask_dev, M0_POLICY_SIZE}};
        }
        return {};
    }
};

Net* m0_net_impl(m0_net* n) { return n ? n->net : nullptr; }
hipStream_t m0_net_stream(m0_net* n) { return n ? n->stream : nullptr; }
int m0_net_device(m0_net* n) { return n ? n->device : 0; }
void m0_net_lock(m0_net* n) { if (n) n->mu.lock(); }
void m0_net_unlock(m0_net* n) { if (n) n->mu.unlock(); }

hipError_t create_stream_cu_mask_env(const char* env_name, hipStream_t* stream) {
    const char* mk = getenv(env_name);
    if (!mk || !*mk) return hipStreamCreateWithFlags(stream, hipStreamNonBlocking);
    uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int nw = 0;
    for (const char* q = mk; *q && nw < 8; ++nw) {
        char* end = nullptr;
        words[nw] = (uint32_t)strtoul(q, &end, 16);
        if (end == q) break;
        q = (*end == ',') ? end + 1 : end;
    }
    return hipExtStreamCreateWithCUMask(stream, 8, words);
}

// Frees a group: through the network's status when it regrows, with the results dropped (hs null) at teardown.
static void release_staging(m0_net* n, int group, HipStatus* hs) {
    for (const StagedArray& a : n->staging(group)) {
        if (*a.p && hs) M0_HIP(*hs, hipFree(*a.p));
        else if (*a.p) (void)hipFree(*a.p);
        *a.p = nullptr;
    }
    n->cap[group] = 0;
}

// Room for B rows in a group.  It grows only past its capacity, to max(B, 64) rows, and the old arrays are freed before the new
// ones are allocated, so the peak does not double.
static int reserve_staging(m0_net* n, int group, int B) {
    if (B <= n->cap[group]) return M0_OK;
    HipStatus& hs = n->net->hip();
    release_staging(n, group, &hs);
    const int rows = B < 64 ? 64 : B;
    for (const StagedArray& a : n->staging(group)) M0_HIP(hs, hipMalloc(a.p, (size_t)rows * a.row_bytes));
    if (!hs.ok()) return m0_hip_error(hs, STAGE_GROW_ERROR[group]);
    n->cap[group] = rows;
    return M0_OK;
}

extern "C" {

const char* m0_last_error(void) { return g_m0_last_error.c_str(); }
const char* m0_version(void) { return "m0engine 0.2 (gfx950)"; }
int m0_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

m0_net* m0_net_create(const m0_net_cfg* cfg, int hip_device) {
    if (!cfg) { m0_set_error("cfg is null"); return nullptr; }
    const char* why = Net::check_supported(*cfg);
    if (why) { m0_set_error(std::string("unsupported network config: ") + why); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        m0_set_error("no HIP device available (the engine has no CPU fallback)");
        return nullptr;
    }
    if (hip_device < 0 || hip_device >= ndev) { m0_set_error("hip_device out of range"); return nullptr; }
    if (hipSetDevice(hip_device) != hipSuccess) { m0_set_error("hipSetDevice failed"); return nullptr; }
    m0_net* h = new m0_net();
    h->device = hip_device;
    // M0_NET_CU_MASK: the network's stream runs on those CUs only.  Measurement switch of tools/exp_cumask.py (two networks on
    // complementary halves of the chip); read at creation, so two networks of one process can get different masks.
    const hipError_t se = create_stream_cu_mask_env("M0_NET_CU_MASK", &h->stream);
    if (se != hipSuccess) {
        m0_set_error("hipStreamCreate failed");
        delete h;
        return nullptr;
    }
    h->net = new Net(*cfg, hip_device, h->stream);
    return h;
}

void m0_net_destroy(m0_net* n) {
    if (!n) return;
    (void)hipSetDevice(n->device);
    if (n->stream) { (void)hipStreamSynchronize(n->stream); }
    for (int g = 0; g < STAGE_GROUPS; ++g) release_staging(n, g, nullptr);
    delete n->net;
    if (n->stream) (void)hipStreamDestroy(n->stream);
    delete n;
}

int m0_net_load_weight(m0_net* n, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!n) { m0_set_error("net is null"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    std::string err;
    int rc = n->net->load(name, data, dtype, shape, ndim, err);
    if (rc != M0_OK) m0_set_error(err);
    return rc;
}

int m0_net_finalize(m0_net* n) {
    if (!n) { m0_set_error("net is null"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    if (!n->net->hip().ok()) return m0_hip_error(n->net->hip());
    std::string err;
    int rc = n->net->finalize(err);
    if (rc != M0_OK) m0_set_error(err);
    return rc;
}

// The host-facing forward, under the network's lock.  tap_stream / tap_second (both or neither): the trunk tap's two buffers
// after the forward, fp16 [B][64][width] widened to f32; the caller has armed the tap.
static int infer_locked(m0_net* n, const float* planes, int B, float* policy, float* value, float* ssl,
                        float* tap_stream = nullptr, float* tap_second = nullptr, int* has_second = nullptr) {
    HipStatus& hs = n->net->hip();
    if (!M0_HIP(hs, hipSetDevice(n->device))) return m0_hip_error(hs);       // also a network that has failed before
    int rc = reserve_staging(n, STAGE_IO, B);
    if (rc != M0_OK) return rc;
    const int P = n->net->cfg().planes;
    const int sslc = n->net->ssl_channels_total();
    if (ssl && sslc == 0) { m0_set_error("ssl output requested but the net has no SSL heads"); return M0_ERR_INVALID; }
    std::string err;
    if (!M0_HIP(hs, hipMemcpyAsync(n->planes_dev, planes, (size_t)B * P * 64 * 4, hipMemcpyHostToDevice, n->stream)))
        return m0_hip_error(hs, "H2D copy");
    rc = n->net->forward(n->planes_dev, nullptr, B, n->logits_dev, n->value_dev, ssl ? n->ssl_dev : nullptr, n->stream, err);
    if (rc != M0_OK) { m0_set_error(err); return rc; }
    M0_HIP(hs, hipMemcpyAsync(policy, n->logits_dev, (size_t)B * M0_POLICY_SIZE * 4, hipMemcpyDeviceToHost, n->stream));
    M0_HIP(hs, hipMemcpyAsync(value, n->value_dev, (size_t)B * 4, hipMemcpyDeviceToHost, n->stream));
    if (ssl) M0_HIP(hs, hipMemcpyAsync(ssl, n->ssl_dev, (size_t)B * sslc * 64 * 4, hipMemcpyDeviceToHost, n->stream));
    std::vector<_Float16> th, ta;
    const size_t tn = tap_stream ? (size_t)B * 64 * n->net->trunk_width() : 0;
    if (tap_stream) {
        th.resize(tn);
        M0_HIP(hs, hipMemcpyAsync(th.data(), n->net->tap_stream(), tn * 2, hipMemcpyDeviceToHost, n->stream));
        if (n->net->tap_has_second()) {
            ta.resize(tn);
            M0_HIP(hs, hipMemcpyAsync(ta.data(), n->net->tap_second(), tn * 2, hipMemcpyDeviceToHost, n->stream));
        }
    }
    if (!M0_HIP(hs, hipStreamSynchronize(n->stream))) return m0_hip_error(hs, "forward failed");
    if (tap_stream) {
        for (size_t i = 0; i < tn; ++i) tap_stream[i] = (float)th[i];
        for (size_t i = 0; i < tn; ++i) tap_second[i] = ta.empty() ? 0.f : (float)ta[i];
        *has_second = ta.empty() ? 0 : 1;
    }
    // NaN/Inf must surface as errors (mcts.py:1165-1177, tests/test_error_handling.py:23-53)
    for (size_t i = 0, nn = (size_t)B * M0_POLICY_SIZE; i < nn; ++i)
        if (!isfinite(policy[i])) { m0_set_error("network produced non-finite policy logits"); return M0_ERR_NONFINITE; }
    for (int i = 0; i < B; ++i)
        if (!isfinite(value[i])) { m0_set_error("network produced non-finite value"); return M0_ERR_NONFINITE; }
    return M0_OK;
}

int m0_net_infer(m0_net* n, const float* planes, int B, float* policy, float* value, float* ssl) {
    if (!n || !planes || !policy || !value) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    return infer_locked(n, planes, B, policy, value, ssl);
}

// What m0_net_score, m0_net_score_packed, m0_net_score_aug and m0_net_score_ssl ask of net_score: one forward, then the score
// kernels on the buffers it left.  ssl_rows null: without the SSL heads, as m0_net_score always ran.  augmented false: the rows as
// they were uploaded, the launches m0_net_score always made; otherwise augment_rows_kernel first moves them into the second staging
// set, and the forward and the score kernel read that.  packed (planes, pi and legal_mask null then): the staging buffers that
// the dense rows would be copied into are filled by unpacking on the stream instead, and everything behind them is the same.
// store (planes, pi, legal_mask, packed and z null then; include/m0_batch_weighted.h): those staging buffers are filled by the
// batch kernel of a resident row store from ids and kinds, on the network's stream; with a rule, one more kernel behind the score
// kernel turns each row's columns into its weight in the store.  The store's mutex is taken behind the network's.
struct ScoreRequest {
    const float* planes = nullptr;                      // the rows: dense planes, pi and legal_mask (may be null) ...
    const float* pi = nullptr;
    const uint8_t* legal_mask = nullptr;
    const m0_rowpack_arrays* packed = nullptr;          // ... or packed
    const float* z = nullptr;
    int B = 0;
    const m0_score_opts* opts = nullptr;
    float* rows = nullptr;
    bool augmented = false;
    const uint8_t* kinds = nullptr;
    float* ssl_rows = nullptr;
    const float* ssl_targets = nullptr;
    m0_rowstore* store = nullptr;                       // ... or resident: ids [B], kinds [B] or null
    const int64_t* ids = nullptr;
    const m0_weight_rule* rule = nullptr;
};

static int net_score(m0_net* n, const ScoreRequest& q) {
    const int B = q.B;
    if (!n || (q.store ? !q.ids : (!q.packed && (!q.planes || !q.pi)) || !q.z) || !q.rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    const bool have_mask = q.store ? q.store->with_mask : q.packed ? q.packed->pos[0].mask_kind != M0_ROWPACK_MASK_NONE : q.legal_mask != nullptr;
    if (const char* why = m0score::bad_opts(q.opts, have_mask)) { m0_set_error(why); return M0_ERR_INVALID; }
    if ((q.packed || q.store) && n->net->cfg().planes != M0_PLANES) { m0_set_error("packed rows need the 19 planes of encode_board"); return M0_ERR_INVALID; }
    if (q.augmented || (q.store && q.kinds))
        if (const char* why = m0_bad_kinds(q.kinds, B)) { m0_set_error(why); return M0_ERR_INVALID; }
    if (q.store) {
        if (!q.store->on_device()) { m0_set_error("a host store has no rows on a device to score"); return M0_ERR_INVALID; }
        if (q.store->device != n->device) { m0_set_error("the store is on another device than the network"); return M0_ERR_INVALID; }
        if (q.rule)
            if (const char* why = m0sample::bad_rule(q.rule)) { m0_set_error(why); return M0_ERR_INVALID; }
    }
    std::lock_guard<std::mutex> lk(n->mu);
    std::unique_lock<std::mutex> store_lk;                                    // network first, then store
    if (q.store) store_lk = std::unique_lock<std::mutex>(q.store->mu);
    m0store::Slot* slot = nullptr;
    int tasks = 0;
    if (q.ssl_rows) {
        tasks = n->net->cfg().self_supervised ? n->net->cfg().ssl_tasks & m0sslscore::ALL_TASKS : 0;
        if (n->net->ssl_channels_total() == 0 || n->net->ssl_channels_total() != m0sslscore::channels(tasks)) {
            m0_set_error("the net has no SSL heads to score");
            return M0_ERR_INVALID;
        }
        if (n->net->cfg().planes != M0_PLANES) { m0_set_error("SSL targets need the 19 planes of encode_board"); return M0_ERR_INVALID; }
    }
    HipStatus& hs = n->net->hip();
    if (!M0_HIP(hs, hipSetDevice(n->device))) return m0_hip_error(hs);       // also a network that has failed before
    int rc = reserve_staging(n, STAGE_IO, B);
    if (rc == M0_OK) rc = reserve_staging(n, STAGE_SCORE, B);
    if (rc == M0_OK && q.ssl_rows) rc = reserve_staging(n, STAGE_SSL_SCORE, B);
    if (rc == M0_OK && q.augmented) rc = reserve_staging(n, STAGE_AUG, B);
    if (rc != M0_OK) return rc;
    const bool masked = q.opts->mask_mode == M0_SCORE_MASK_LEGAL;
    const size_t cells = (size_t)B * M0_POLICY_SIZE;
    if (q.store) {
        rc = m0store::score_gather(q.store, q.ids, q.kinds, B, n->planes_dev, n->score_pi_dev, n->score_z_dev,
                                   have_mask ? n->score_mask_dev : nullptr, q.rule != nullptr, n->stream, &slot);
        if (rc != M0_OK) return rc;
    } else if (q.packed) {
        rc = m0_rowpack_unpack_to_device(hs, q.packed, n->planes_dev, n->score_pi_dev, masked ? n->score_mask_dev : nullptr, n->stream);
        if (rc != M0_OK) return rc;
        M0_HIP(hs, hipMemcpyAsync(n->score_z_dev, q.z, (size_t)B * 4, hipMemcpyHostToDevice, n->stream));
    } else {
        M0_HIP(hs, hipMemcpyAsync(n->planes_dev, q.planes, (size_t)B * n->net->cfg().planes * 64 * 4, hipMemcpyHostToDevice, n->stream));
        M0_HIP(hs, hipMemcpyAsync(n->score_pi_dev, q.pi, cells * 4, hipMemcpyHostToDevice, n->stream));
        M0_HIP(hs, hipMemcpyAsync(n->score_z_dev, q.z, (size_t)B * 4, hipMemcpyHostToDevice, n->stream));
        if (masked) M0_HIP(hs, hipMemcpyAsync(n->score_mask_dev, q.legal_mask, cells, hipMemcpyHostToDevice, n->stream));
    }
    if (q.ssl_rows && q.ssl_targets)
        M0_HIP(hs, hipMemcpyAsync(n->ssl_targets_dev, q.ssl_targets, (size_t)B * m0ssl::TARGET_CH * 64 * 4, hipMemcpyHostToDevice, n->stream));
    if (q.augmented) M0_HIP(hs, hipMemcpyAsync(n->aug_kinds_dev, q.kinds, (size_t)B, hipMemcpyHostToDevice, n->stream));
    if (!hs.ok()) return m0_hip_error(hs, "H2D copy");
    const float* planes_in = n->planes_dev;
    const float* pi_in = n->score_pi_dev;
    const uint8_t* mask_in = masked ? n->score_mask_dev : nullptr;
    if (q.augmented) {
        if (!M0_HIP(hs, launch_augment_rows(planes_in, pi_in, mask_in, n->aug_kinds_dev, M0_AUG_NONE, B, n->net->cfg().planes,
                                            n->aug_planes_dev, n->aug_pi_dev, masked ? n->aug_mask_dev : nullptr, n->stream)))
            return m0_hip_error(hs, "augment kernel");
        planes_in = n->aug_planes_dev;
        pi_in = n->aug_pi_dev;
        if (masked) mask_in = n->aug_mask_dev;
    }
    std::string err;
    rc = n->net->forward(planes_in, nullptr, B, n->logits_dev, n->value_dev, q.ssl_rows ? n->ssl_dev : nullptr, n->stream, err);
    if (rc != M0_OK) { m0_set_error(err); return rc; }
    // the logits and the head outputs stay where the forward left them
    M0_HIP(hs, launch_score_rows(n->logits_dev, n->value_dev, pi_in, n->score_z_dev, mask_in, B, *q.opts, n->score_rows_dev, n->stream));
    M0_HIP(hs, hipMemcpyAsync(q.rows, n->score_rows_dev, (size_t)B * M0_SCORE_COLS * 4, hipMemcpyDeviceToHost, n->stream));
    if (q.store && q.rule && hs.ok()) {
        rc = m0store::score_weights(q.store, slot, B, n->score_rows_dev, *q.rule, n->stream);
        if (rc != M0_OK) return rc;
    }
    if (q.ssl_rows) {
        M0_HIP(hs, launch_ssl_score(n->ssl_dev, tasks, n->planes_dev, q.ssl_targets ? n->ssl_targets_dev : nullptr, B, n->ssl_rows_dev,
                                    n->stream));
        M0_HIP(hs, hipMemcpyAsync(q.ssl_rows, n->ssl_rows_dev, (size_t)B * M0_SSL_SCORE_COLS * 4, hipMemcpyDeviceToHost, n->stream));
    }
    if (!M0_HIP(hs, hipStreamSynchronize(n->stream))) return m0_hip_error(hs, "forward and score failed");
    for (int b = 0; b < B; ++b)
        if (((int)q.rows[(size_t)b * M0_SCORE_COLS + 7] & M0_SCORE_FLAG_NONFINITE) ||
            (q.ssl_rows && ((int)q.ssl_rows[(size_t)b * M0_SSL_SCORE_COLS + 15] & M0_SSL_SCORE_FLAG_NONFINITE))) {
            m0_set_error("network produced non-finite outputs (row " + std::to_string(b) + ")");
            return M0_ERR_NONFINITE;
        }
    return M0_OK;
}

// the dense rows and what every score call gives
static ScoreRequest dense_request(const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int B,
                                  const m0_score_opts* opts, float* rows) {
    ScoreRequest q;
    q.planes = planes; q.pi = pi; q.z = z; q.legal_mask = legal_mask; q.B = B; q.opts = opts; q.rows = rows;
    return q;
}

int m0_net_score(m0_net* n, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int B,
                 const m0_score_opts* opts, float* rows) {
    return net_score(n, dense_request(planes, pi, z, legal_mask, B, opts, rows));
}

int m0_net_score_packed(m0_net* n, const m0_rowpack_arrays* in, const m0_score_opts* opts, float* rows) {
    if (!in || !in->pos || !in->z || in->n <= 0 || in->n > INT_MAX) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    ScoreRequest q;
    q.packed = in; q.z = in->z; q.B = (int)in->n; q.opts = opts; q.rows = rows;
    return net_score(n, q);
}

int m0_net_score_resident(m0_net* n, m0_rowstore* store, const int64_t* ids, const uint8_t* kinds, int B, const m0_score_opts* opts,
                          float* rows, const m0_weight_rule* rule) {
    if (!store) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    ScoreRequest q;
    q.store = store; q.ids = ids; q.kinds = kinds; q.B = B; q.opts = opts; q.rows = rows; q.rule = rule;
    return net_score(n, q);
}

int m0_net_score_aug(m0_net* n, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, const uint8_t* kinds,
                     int B, const m0_score_opts* opts, float* rows) {
    ScoreRequest q = dense_request(planes, pi, z, legal_mask, B, opts, rows);
    q.augmented = true; q.kinds = kinds;
    return net_score(n, q);
}

int m0_net_score_ssl(m0_net* n, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask,
                     const float* ssl_targets, int B, const m0_score_opts* opts, float* rows, float* ssl_rows) {
    if (!ssl_rows) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    ScoreRequest q = dense_request(planes, pi, z, legal_mask, B, opts, rows);
    q.ssl_rows = ssl_rows; q.ssl_targets = ssl_targets;
    return net_score(n, q);
}

int m0_net_tap_info(const m0_net* n, int* steps, int* width) {
    if (!n || !steps || !width) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    *steps = n->net->tap_steps();
    *width = n->net->trunk_width();
    return M0_OK;
}

int m0_net_infer_tap(m0_net* n, const float* planes, int B, int step, float* policy, float* value, float* ssl, float* stream,
                     float* second, int* has_second) {
    if (!n || !planes || !policy || !value || !stream || !second || !has_second) {
        m0_set_error("null argument");
        return M0_ERR_INVALID;
    }
    if (B <= 0) { m0_set_error("batch must be positive"); return M0_ERR_INVALID; }
    if (step < 0 || step >= n->net->tap_steps()) { m0_set_error("tap step out of range"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    n->net->set_tap(step);
    const int rc = infer_locked(n, planes, B, policy, value, ssl, stream, second, has_second);
    n->net->set_tap(-1);
    return rc;
}

int m0_net_ssl_channels(const m0_net* n) { return n ? n->net->ssl_channels_total() : 0; }
int64_t m0_net_param_count(const m0_net* n) { return n ? (int64_t)n->net->param_count() : 0; }
double m0_net_flops_per_position(const m0_net* n, int with_ssl) { return n ? n->net->flops_per_position(with_ssl != 0) : 0.0; }

int m0_net_profile_enable(m0_net* n, int on) {
    if (!n) { m0_set_error("net is null"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    n->net->set_profile(on != 0);
    return M0_OK;
}

int m0_net_profile_get(m0_net* n, double* conv_ms, double* conv_flop, int64_t* launches, int reset) {
    if (!n) { m0_set_error("net is null"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    if (conv_ms) *conv_ms = n->net->prof_conv_ms();
    if (conv_flop) *conv_flop = n->net->prof_conv_flop();
    if (launches) *launches = n->net->prof_conv_launches();
    if (reset) n->net->reset_profile();
    return M0_OK;
}

int m0_net_profile_get_tail(m0_net* n, double* tail_ms, int64_t* tail_launches) {
    if (!n) { m0_set_error("net is null"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    if (tail_ms) *tail_ms = n->net->prof_tail_ms();
    if (tail_launches) *tail_launches = n->net->prof_tail_launches();
    return M0_OK;
}

int m0_net_bench_forward(m0_net* n, int B, int iters, int with_ssl, float* ms_per_forward) {
    if (!n || !ms_per_forward || B <= 0 || iters <= 0) { m0_set_error("invalid argument"); return M0_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(n->mu);
    HipStatus& hs = n->net->hip();
    if (!M0_HIP(hs, hipSetDevice(n->device))) return m0_hip_error(hs);
    int rc = reserve_staging(n, STAGE_IO, B);
    if (rc != M0_OK) return rc;
    std::string err;
    // synthetic resident input: sparse 0/1 piece planes + constant planes (with_ssl bit 1: keep the input of the previous call
    // of the same batch size -- tools/exp_cumask.py times two networks side by side without the host-side generation)
    if (!(with_ssl & 2)) {
        const int P = n->net->cfg().planes;
        std::vector<float> h((size_t)B * P * 64, 0.f);
        BenchRng rng;
        for (size_t i = 0; i < h.size(); ++i) {
            const uint64_t s = rng.next();
            int p = (int)((i / 64) % P);
            if (p < 12) h[i] = ((s >> 20) % 100) < 8 ? 1.f : 0.f;
            else h[i] = (float)((((i / 64 / P) * 7 + p) % 10) / 10.0);
        }
        if (!M0_HIP(hs, hipMemcpy(n->planes_dev, h.data(), h.size() * 4, hipMemcpyHostToDevice))) return m0_hip_error(hs, "H2D copy");
    }
    float* ssl = ((with_ssl & 1) && n->net->ssl_channels_total() > 0) ? n->ssl_dev : nullptr;
    rc = n->net->forward(n->planes_dev, nullptr, B, n->logits_dev, n->value_dev, ssl, n->stream, err);   // warm-up
    if (rc != M0_OK) { m0_set_error(err); return rc; }
    const float ms = m0_time_iterations(hs, n->stream, iters, [&]() {
        rc = n->net->forward(n->planes_dev, nullptr, B, n->logits_dev, n->value_dev, ssl, n->stream, err);
        return rc == M0_OK;
    });
    if (rc != M0_OK) { m0_set_error(err); return rc; }
    if (!hs.ok()) return m0_hip_error(hs, "bench forward failed");
    *ms_per_forward = ms;
    n->net->harvest_profile();
    return M0_OK;
}

}  // extern "C"
