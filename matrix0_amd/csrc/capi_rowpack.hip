// extern "C" entry points of the packed training rows (include/m0_rowpack.h): the stateless device calls, with a HipStatus on the
// stack like m0_decode_planes, and their host twins.  m0_net_score_packed lives with the network handle in capi_net.hip and
// unpacks through m0_rowpack_unpack_to_device below.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "rowpack_host.h"
#include "rowpack_kernels.h"
#include "tree.h"

using namespace m0rowpack;

namespace {

int invalid(const std::string& why) { m0_set_error(why); return M0_ERR_INVALID; }

}  // namespace

int m0_rowpack_unpack_to_device(HipStatus& hs, const m0_rowpack_arrays* in, float* planes_dev, float* pi_dev, uint8_t* mask_dev,
                                hipStream_t st) {
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    const std::string why = check_arrays(in, positions, raw_slot);
    if (!why.empty()) return invalid("packed rows: " + why);
    if (mask_dev && !has_masks(*in)) return invalid("packed rows: a mask is wanted of rows without masks");
    const size_t n = (size_t)in->n, raw = (size_t)in->raw_n;
    DevBuf<Pos> dpos;
    DevBuf<m0_rowpack_pos> dq;
    DevBuf<int64_t> dpo, dmo;
    DevBuf<uint16_t> dpi, dmi;
    DevBuf<float> dpv, drs, drp;
    DevBuf<uint8_t> drm;
    DevBuf<int32_t> dslot;
    dpos.upload(hs, positions.data(), n, st);
    dq.upload(hs, in->pos, n, st);
    dpo.upload(hs, in->pi_off, n + 1, st);
    dmo.upload(hs, in->mask_off, n + 1, st);
    dpi.upload(hs, in->pi_idx, (size_t)in->pi_n, st);
    dpv.upload(hs, in->pi_val, (size_t)in->pi_n, st);
    dmi.upload(hs, in->mask_idx, mask_dev ? (size_t)in->mask_n : 0, st);
    dslot.upload(hs, raw_slot.data(), n, st);
    drs.upload(hs, in->raw_planes, raw * PLANE_FLOATS, st);
    drp.upload(hs, in->raw_pi, raw * COLS, st);
    drm.upload(hs, in->raw_mask, mask_dev ? raw * COLS : 0, st);
    if (!hs.ok()) return m0_hip_error(hs, "packed rows upload failed");
    M0_HIP(hs, launch_encode_positions(dpos.p, (int)n, planes_dev, nullptr, mask_dev, nullptr, nullptr, nullptr, st));
    M0_HIP(hs, launch_rowpack_unpack(dq.p, dpo.p, dpi.p, dpv.p, dmo.p, dmi.p, dslot.p, drs.p, drp.p, drm.p, (int)n, planes_dev, pi_dev,
                                     mask_dev, st));
    // the uploads live for this call: the kernels are done before they go
    if (!M0_HIP(hs, hipStreamSynchronize(st))) return m0_hip_error(hs, "unpack kernels failed");
    return M0_OK;
}

// The rows the *_bench calls of the packed rows run on (capi_common.h): N positions of seeded legal play from the start position,
// soft pi on about two thirds of each one's legal moves, the legal moves as mask.
void m0_rowpack_bench_rows(size_t N, std::vector<float>& planes, std::vector<float>& pi, std::vector<uint8_t>& mask) {
    planes.assign(N * PLANE_FLOATS, 0.f);
    pi.assign(N * COLS, 0.f);
    mask.assign(N * COLS, 0);
    BenchRng rng;
    const char* start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
    Pos p;
    m0::parse_fen(start, p);
    for (size_t i = 0; i < N; ++i) {
        m0::Move mv[M0_MAX_MOVES];
        int k = m0::gen_legal(p, mv);
        if (k == 0 || p.halfmove > 90 || p.fullmove > 150) { m0::parse_fen(start, p); k = m0::gen_legal(p, mv); }
        m0::encode_planes_f32(p, &planes[i * PLANE_FLOATS]);
        float sum = 0.f;
        for (int j = 0; j < k; ++j) {
            const int idx = m0::move_to_index(p, mv[j]);
            mask[i * COLS + idx] = 1;
            if (rng.next() % 3 || j == 0) sum += pi[i * COLS + idx] = (float)(1 + rng.next() % 100);
        }
        for (int j = 0; j < k; ++j) pi[i * COLS + m0::move_to_index(p, mv[j])] /= sum;
        m0::make_move(p, mv[rng.next() % k]);
    }
}

extern "C" {

int m0_rowpack_pack_host(const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int n,
                         m0_rowpack_arrays* out, int64_t* sizes) {
    if (!planes || !z || !out || !sizes || n <= 0) return invalid("invalid argument");
    const std::string why = pack_host(planes, pi, z, legal_mask, (size_t)n, out, sizes);
    return why.empty() ? M0_OK : invalid(why);
}

int m0_rowpack_unpack_host(const m0_rowpack_arrays* in, float* planes, float* pi, float* z, uint8_t* legal_mask) {
    if (!in || !planes || !pi || !z) return invalid("null argument");
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    const std::string why = check_arrays(in, positions, raw_slot);
    if (!why.empty()) return invalid("packed rows: " + why);
    if ((legal_mask != nullptr) != has_masks(*in)) return invalid("packed rows: the mask output must be given exactly for rows with masks");
    unpack_host(*in, positions, raw_slot, planes, pi, z, legal_mask);
    return M0_OK;
}

int m0_rowpack_pack(int hip_device, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int n,
                    m0_rowpack_arrays* out, int64_t* sizes) {
    if (!planes || !z || !out || !sizes || n <= 0) return invalid("invalid argument");
    HipStatus hs;
    const int rc = m0_select_device(hs, hip_device, "use the _host call");
    if (rc != M0_OK) return rc;
    const size_t N = (size_t)n;
    DevBuf<float> dpl, dpi;
    DevBuf<uint8_t> dm;
    DevBuf<Pos> dpos;
    DevBuf<int32_t> dst, dfl, dnl, dcnt;
    DevBuf<m0_rowpack_pos> dq;
    dpl.upload(hs, planes, N * PLANE_FLOATS);
    if (pi) dpi.upload(hs, pi, N * COLS);
    if (legal_mask) dm.upload(hs, legal_mask, N * COLS);
    if (!dpos.alloc(hs, N) || !dst.alloc(hs, N) || !dfl.alloc(hs, N) || !dnl.alloc(hs, N) || !dcnt.alloc(hs, 2 * N) || !dq.alloc(hs, N))
        return m0_hip_error(hs, "hipMalloc or upload failed");
    M0_HIP(hs, launch_decode_planes(dpl.p, dm.p, n, dpos.p, dst.p, dfl.p, dnl.p, nullptr));
    M0_HIP(hs, launch_rowpack_count(dpi.p, dm.p, dpos.p, dst.p, n, dq.p, dcnt.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "count pass failed");
    std::vector<m0_rowpack_pos> pos(N);
    std::vector<int32_t> counts(2 * N), raw_slot;
    std::vector<int64_t> pi_off, mask_off;
    dq.download(hs, pos.data(), N);
    dcnt.download(hs, counts.data(), 2 * N);
    if (!hs.ok()) return m0_hip_error(hs, "download failed");
    scan_counts(pos.data(), counts.data(), N, pi_off, mask_off, raw_slot, sizes);
    const std::string why = check_capacity(out, sizes, legal_mask != nullptr);
    if (!why.empty()) return invalid(why);
    DevBuf<int64_t> dpo, dmo;
    DevBuf<int32_t> dslot;
    DevBuf<uint16_t> didx, dmidx;
    DevBuf<float> dval, drs, drp;
    DevBuf<uint8_t> drm;
    const size_t npi = (size_t)sizes[0], nmk = (size_t)sizes[1], raw = (size_t)sizes[2];
    dpo.upload(hs, pi_off.data(), N + 1);
    dmo.upload(hs, mask_off.data(), N + 1);
    dslot.upload(hs, raw_slot.data(), N);
    if (!didx.alloc(hs, npi + 1) || !dval.alloc(hs, npi + 1) || !dmidx.alloc(hs, nmk + 1) || !drs.alloc(hs, raw * PLANE_FLOATS + 1) ||
        !drp.alloc(hs, raw * COLS + 1) || !drm.alloc(hs, raw * COLS + 1)) return m0_hip_error(hs, "hipMalloc or upload failed");
    M0_HIP(hs, launch_rowpack_fill(dpl.p, dpi.p, dm.p, dq.p, dpo.p, dmo.p, dslot.p, n, didx.p, dval.p, dmidx.p, drs.p, drp.p, drm.p, nullptr));
    if (!M0_HIP(hs, hipDeviceSynchronize())) return m0_hip_error(hs, "fill pass failed");
    // into scratch first: nothing of the caller's is partly written when a download fails
    std::vector<uint16_t> hidx(npi), hmidx(nmk);
    std::vector<float> hval(npi);
    if (npi) { didx.download(hs, hidx.data(), npi); dval.download(hs, hval.data(), npi); }
    if (nmk) dmidx.download(hs, hmidx.data(), nmk);
    if (!hs.ok()) return m0_hip_error(hs, "download failed");
    if (raw) {
        drs.download(hs, out->raw_planes, raw * PLANE_FLOATS);
        drp.download(hs, out->raw_pi, raw * COLS);
        if (legal_mask) drm.download(hs, out->raw_mask, raw * COLS);
        if (!hs.ok()) return m0_hip_error(hs, "download failed");
    }
    if (npi) { memcpy(out->pi_idx, hidx.data(), npi * sizeof(uint16_t)); memcpy(out->pi_val, hval.data(), npi * sizeof(float)); }
    if (nmk) memcpy(out->mask_idx, hmidx.data(), nmk * sizeof(uint16_t));
    memcpy(out->pos, pos.data(), N * sizeof(m0_rowpack_pos));
    memcpy(out->z, z, N * sizeof(float));
    memcpy(out->pi_off, pi_off.data(), (N + 1) * sizeof(int64_t));
    memcpy(out->mask_off, mask_off.data(), (N + 1) * sizeof(int64_t));
    out->n = n; out->pi_n = sizes[0]; out->mask_n = sizes[1]; out->raw_n = sizes[2];
    return M0_OK;
}

int m0_rowpack_unpack(int hip_device, const m0_rowpack_arrays* in, float* planes, float* pi, float* z, uint8_t* legal_mask) {
    if (!in || !planes || !pi || !z) return invalid("null argument");
    if (in->n <= 0 || !in->pos) return invalid("packed rows: the number of rows must be positive");
    if ((legal_mask != nullptr) != has_masks(*in)) return invalid("packed rows: the mask output must be given exactly for rows with masks");
    HipStatus hs;
    int rc = m0_select_device(hs, hip_device, "use the _host call");
    if (rc != M0_OK) return rc;
    const size_t N = (size_t)in->n;
    DevBuf<float> dpl, dpi;
    DevBuf<uint8_t> dm;
    if (!dpl.alloc(hs, N * PLANE_FLOATS) || !dpi.alloc(hs, N * COLS) || (legal_mask && !dm.alloc(hs, N * COLS)))
        return m0_hip_error(hs, "hipMalloc failed");
    rc = m0_rowpack_unpack_to_device(hs, in, dpl.p, dpi.p, dm.p, nullptr);
    if (rc != M0_OK) return rc;
    dpl.download(hs, planes, N * PLANE_FLOATS);
    dpi.download(hs, pi, N * COLS);
    if (legal_mask) dm.download(hs, legal_mask, N * COLS);
    if (!hs.ok()) return m0_hip_error(hs, "download failed");
    memcpy(z, in->z, N * sizeof(float));
    return M0_OK;
}

int m0_rowpack_bench(int hip_device, int B, int iters, float* pack_us, float* unpack_us, double* dense_bytes) {
    if (B <= 0 || iters <= 0 || !pack_us || !unpack_us || !dense_bytes) return invalid("invalid argument");
    HipStatus hs;
    int rc = m0_select_device(hs, hip_device, "use the _host call");
    if (rc != M0_OK) return rc;
    const size_t N = (size_t)B;
    std::vector<float> planes, pi, z(N, 0.f);
    std::vector<uint8_t> mask;
    m0_rowpack_bench_rows(N, planes, pi, mask);
    // the packed form of these rows, once, for the offsets of the fill pass and as the input of unpacking
    int64_t sizes[3];
    m0_rowpack_arrays a = {};
    a.n = B;
    (void)pack_host(planes.data(), pi.data(), z.data(), mask.data(), N, &a, sizes);
    std::vector<m0_rowpack_pos> hq(N);
    std::vector<int64_t> hpo(N + 1), hmo(N + 1);
    std::vector<uint16_t> hidx((size_t)sizes[0]);
    std::vector<float> hval((size_t)sizes[0]), hz(N);
    a.pi_n = sizes[0]; a.pos = hq.data(); a.z = hz.data(); a.pi_off = hpo.data(); a.mask_off = hmo.data(); a.pi_idx = hidx.data();
    a.pi_val = hval.data();
    if (sizes[1] != 0 || sizes[2] != 0 || !pack_host(planes.data(), pi.data(), z.data(), mask.data(), N, &a, sizes).empty())
        return invalid("the bench rows did not pack as positions with legal masks");
    std::vector<Pos> positions;
    std::vector<int32_t> raw_slot;
    const std::string why = check_arrays(&a, positions, raw_slot);
    if (!why.empty()) return invalid(why);
    DevBuf<float> dpl, dpi, dval, opl, opi;
    DevBuf<uint8_t> dm, om;
    DevBuf<Pos> dpos;
    DevBuf<int32_t> dst, dfl, dnl, dcnt, dslot;
    DevBuf<m0_rowpack_pos> dq;
    DevBuf<int64_t> dpo, dmo;
    DevBuf<uint16_t> didx, dmidx;
    dpl.upload(hs, planes.data(), N * PLANE_FLOATS);
    dpi.upload(hs, pi.data(), N * COLS);
    dm.upload(hs, mask.data(), N * COLS);
    dpo.upload(hs, hpo.data(), N + 1);
    dmo.upload(hs, hmo.data(), N + 1);
    dslot.upload(hs, raw_slot.data(), N);
    if (!dpos.alloc(hs, N) || !dst.alloc(hs, N) || !dfl.alloc(hs, N) || !dnl.alloc(hs, N) || !dcnt.alloc(hs, 2 * N) || !dq.alloc(hs, N) ||
        !didx.alloc(hs, hidx.size() + 1) || !dval.alloc(hs, hidx.size() + 1) || !dmidx.alloc(hs, 1) || !opl.alloc(hs, N * PLANE_FLOATS) ||
        !opi.alloc(hs, N * COLS) || !om.alloc(hs, N * COLS)) return m0_hip_error(hs, "hipMalloc or upload failed");
    auto pack = [&]() {
        M0_HIP(hs, launch_decode_planes(dpl.p, dm.p, B, dpos.p, dst.p, dfl.p, dnl.p, nullptr));
        M0_HIP(hs, launch_rowpack_count(dpi.p, dm.p, dpos.p, dst.p, B, dq.p, dcnt.p, nullptr));
        return M0_HIP(hs, launch_rowpack_fill(dpl.p, dpi.p, dm.p, dq.p, dpo.p, dmo.p, dslot.p, B, didx.p, dval.p, dmidx.p, nullptr,
                                              nullptr, nullptr, nullptr));
    };
    auto unpack = [&]() {
        M0_HIP(hs, launch_encode_positions(dpos.p, B, opl.p, nullptr, om.p, nullptr, nullptr, nullptr, nullptr));
        return M0_HIP(hs, launch_rowpack_unpack(dq.p, dpo.p, didx.p, dval.p, dmo.p, dmidx.p, dslot.p, nullptr, nullptr, nullptr, B,
                                                opl.p, opi.p, om.p, nullptr));
    };
    pack(); unpack();                                                                   // warm-up
    const float ms_pack = m0_time_iterations(hs, nullptr, iters, pack);
    const float ms_unpack = m0_time_iterations(hs, nullptr, iters, unpack);
    if (!hs.ok()) return m0_hip_error(hs, "rowpack bench failed");
    // what the kernels wrote last is what the host packs and unpacks
    std::vector<float> back(N * COLS);
    opi.download(hs, back.data(), N * COLS);
    if (!hs.ok()) return m0_hip_error(hs, "download failed");
    if (memcmp(back.data(), pi.data(), N * COLS * sizeof(float)) != 0) return invalid("the bench rows did not come back");
    *pack_us = ms_pack * 1000.f;
    *unpack_us = ms_unpack * 1000.f;
    *dense_bytes = (double)B * (PLANE_FLOATS * 4.0 + COLS * 4.0 + COLS);
    return M0_OK;
}

}  // extern "C"
