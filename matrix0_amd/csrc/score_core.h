// Row arithmetic of the training-loss score (include/m0_score.h): one row of 4672 columns folded into a few numbers.  Plain C++
// without intrinsics, host and device: score_kernels.hip runs it with one lane per column slice, tests/score_shim runs the same
// code under g++ with the lanes as a loop.
//
// A row is scored in two steps over the same columns.  Scan is the one pass that needs nothing beforehand: the counts, the
// target's best move, and an ONLINE soft-max (running maximum, sums rescaled when it moves) kept twice, over the support and over
// all columns, with the pi-weighted and the plain sum of (logit - maximum) carried along, so nothing overflows and no term of a
// sum changes sign.  Tail needs the scan's result: the rank counts logits above the target's, and the entropy of the smoothed
// target needs |support|.  Both have add (one column), merge (two partial results; the caller fixes the order) and end in finish.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/m0_engine.h"

#if defined(__HIPCC__)
#define M0_SCORE_HD __host__ __device__ inline
#else
#define M0_SCORE_HD inline
#endif

namespace m0score {

constexpr int COLS = M0_POLICY_SIZE;
constexpr int LANES = 64;
constexpr int F4 = COLS / 4;                              // a row as 16-byte pieces: 1168
constexpr int SWEEPS = (F4 + LANES - 1) / LANES;          // piece k * 64 + lane belongs to lane `lane`: 19 sweeps, the last partial
static_assert(COLS % 4 == 0, "rows are read in 16-byte pieces");

M0_SCORE_HD bool is_finite(float x) { return fabsf(x) <= FLT_MAX; }       // false for NaN

M0_SCORE_HD bool in_support(int mode, float pi, bool in_mask) {
    return mode == M0_SCORE_MASK_LEGAL ? (in_mask || pi > 0.f) : mode == M0_SCORE_MASK_TARGET ? pi > 0.f : true;
}

// log-sum-exp as (maximum, sum of exp(x - maximum)); sum == 0 means empty
struct OnlineLse {
    float m = -FLT_MAX, s = 0.f;
    // Folds x in; returns old maximum - new maximum (<= 0; 0 for the first x), which sums taken relative to the maximum must be
    // moved by.  Selects, one exp2f and no branch: every lane of a wave comes through here for every column.  The argument of the
    // exponential is <= 0 and its rounding error (|arg| * 2^-24 relative) weighs on a term of size exp(arg): below 5e-8 of the sum.
    M0_SCORE_HD float add(float x) {
        const bool up = x > m;
        const float e = exp2f(-fabsf(x - m) * 1.4426950408889634f);      // 0 for the first x: m is below every finite logit
        const float d = (up && s != 0.f) ? m - x : 0.f;
        s = up ? s * e + 1.f : s + e;
        m = up ? x : m;
        return d;
    }
};

struct Scan {
    int mode = M0_SCORE_MASK_LEGAL;
    OnlineLse sup, all;                 // over the support, over all 4672 columns
    int n = 0, nq = 0;                  // |support|, |smoothing set|
    float ps = 0.f, a = 0.f;            // over the support: sum pi, sum pi * (logit - sup.m)
    float u = 0.f;                      // over the smoothing set: sum (logit - sup.m)
    float p_all = 0.f;                  // sum pi over every column (the zero-sum test of train.py:210)
    float best_pi = -INFINITY, best_logit = 0.f;        // argmax(pi) over the support, lowest index among equals: the target's
    int best_idx = COLS;                                // best move, and under the zero-sum fallback the lowest legal column
    float poison = 0.f;                                 // sum of logit * 0: NaN once a logit is not finite

    // in_mask: the row's legal_mask byte under M0_SCORE_MASK_LEGAL, false otherwise.  A non-finite logit makes the sums
    // meaningless and `poison` NaN; finish then zeroes the row's loss columns.
    M0_SCORE_HD void add(int col, float logit, float pi, bool in_mask) {
        const bool s_in = in_support(mode, pi, in_mask);
        p_all += pi;
        poison += logit * 0.f;
        all.add(logit);
        if (!s_in) return;                              // most columns of most rows: a wave skips the rest together
        ++n;
        if (pi > best_pi || (pi == best_pi && col < best_idx)) { best_pi = pi; best_idx = col; best_logit = logit; }
        const float d = sup.add(logit);
        a += ps * d;                                    // ps and nq are 0 while the support is empty
        u += (float)nq * d;
        const float rel = logit - sup.m;
        ps += pi;
        a += pi * rel;
        if (mode != M0_SCORE_MASK_NONE || pi > 0.f) { ++nq; u += rel; }          // train.py:508-512
    }

    M0_SCORE_HD void merge(const Scan& o) {
        if (o.all.s != 0.f) {
            if (all.s == 0.f) all = o.all;
            else {
                const float m = fmaxf(all.m, o.all.m);
                all.s = all.s * expf(all.m - m) + o.all.s * expf(o.all.m - m);
                all.m = m;
            }
        }
        if (o.sup.s != 0.f) {
            if (sup.s == 0.f) { sup = o.sup; a = o.a; u = o.u; }
            else {
                const float m = fmaxf(sup.m, o.sup.m), da = sup.m - m, db = o.sup.m - m;
                sup.s = sup.s * expf(da) + o.sup.s * expf(db);
                a = (a + ps * da) + (o.a + o.ps * db);
                u = (u + (float)nq * da) + (o.u + (float)o.nq * db);
                sup.m = m;
            }
        }
        ps += o.ps;
        n += o.n; nq += o.nq; p_all += o.p_all; poison += o.poison;
        if (o.best_pi > best_pi || (o.best_pi == best_pi && o.best_idx < best_idx)) {
            best_pi = o.best_pi; best_idx = o.best_idx; best_logit = o.best_logit;
        }
    }
};

// What the second step needs of the first
struct Plan {
    int mode = M0_SCORE_MASK_LEGAL;
    bool uniform = false;               // the zero-sum fallback: pi = uniform over the legal moves (then the whole support)
    float target_logit = 0.f;
    float keep = 1.f, c = 0.f;          // pi_s = keep * pi + c on the smoothing set

    M0_SCORE_HD Plan() {}
    M0_SCORE_HD Plan(const m0_score_opts& o, const Scan& s) {
        mode = o.mask_mode;
        uniform = o.mask_mode == M0_SCORE_MASK_LEGAL && s.p_all <= 0.f && s.n > 0;
        target_logit = s.best_logit;
        keep = 1.f - o.label_smoothing;
        c = (o.label_smoothing > 0.f && s.nq > 0) ? o.label_smoothing / (float)s.nq : 0.f;
    }
};

struct Tail {
    int rank = 0, npos = 0;             // support columns above the target's logit; columns with pi > 0
    float h = 0.f;                      // -sum over pi > 0 of pi_s * log(pi_s)

    M0_SCORE_HD void add(const Plan& p, float logit, float pi, bool in_mask) {
        rank += in_support(p.mode, pi, in_mask) && logit > p.target_logit;
        if (pi > 0.f) {                             // few columns of a row; they lie in the smoothing set under every mode
            ++npos;
            const float q = p.keep * pi + p.c;
            h -= q * logf(q);
        }
    }
    M0_SCORE_HD void merge(const Tail& o) { rank += o.rank; npos += o.npos; h += o.h; }
};

// The row's M0_SCORE_COLS columns
M0_SCORE_HD void finish(const m0_score_opts& o, const Scan& s, const Plan& p, const Tail& t, float value, float z, float* out) {
    int flags = 0;
    if (s.n == 0) flags |= M0_SCORE_FLAG_EMPTY;
    if (!is_finite(s.poison) || !is_finite(value)) flags |= M0_SCORE_FLAG_NONFINITE;
    if (p.uniform) flags |= M0_SCORE_FLAG_UNIFORM;
    const float v = is_finite(value) ? value : 0.f;
    float policy = 0.f, entropy = 0.f, vloss = 0.f, rank = 0.f, mass = 0.f;
    if (!(flags & (M0_SCORE_FLAG_EMPTY | M0_SCORE_FLAG_NONFINITE))) {
        const float log_z = logf(s.sup.s);                      // log-softmax of a support column: (logit - sup.m) - log_z
        const float eps = o.label_smoothing;
        if (p.uniform) {                                        // pi_s = 1 / n on the support, smoothed or not
            policy = log_z - s.u / (float)s.n;
            entropy = logf((float)s.n);
        } else {
            policy = (1.f - eps) * (s.ps * log_z - s.a);
            entropy = t.h;
            if (p.c > 0.f) {
                policy += eps * (log_z - s.u / (float)s.nq);
                entropy -= (float)(s.nq - t.npos) * p.c * logf(p.c);
            }
        }
        const float d = v - z, ad = fabsf(d);
        vloss = o.value_loss == 0 ? d * d : (ad < o.huber_delta ? 0.5f * d * d / o.huber_delta : ad - 0.5f * o.huber_delta);
        rank = (float)t.rank;
        mass = s.sup.s * expf(s.sup.m - s.all.m) / s.all.s;
    }
    out[0] = policy; out[1] = entropy; out[2] = vloss; out[3] = rank; out[4] = mass;
    out[5] = (float)s.n; out[6] = v; out[7] = (float)flags;
}

// the argument checks of m0_score_rows / m0_net_score on the options; nullptr when they are fine
inline const char* bad_opts(const m0_score_opts* o, bool have_mask) {
    if (!o) return "opts is null";
    if (o->mask_mode < M0_SCORE_MASK_LEGAL || o->mask_mode > M0_SCORE_MASK_NONE) return "mask_mode out of range";
    if (o->mask_mode == M0_SCORE_MASK_LEGAL && !have_mask) return "M0_SCORE_MASK_LEGAL needs a legal_mask";
    if (!(o->label_smoothing >= 0.f && o->label_smoothing < 1.f)) return "label_smoothing outside [0, 1)";
    if (!(o->huber_delta > 0.f)) return "huber_delta must be positive";
    if (o->value_loss != 0 && o->value_loss != 1) return "value_loss must be 0 (mse) or 1 (huber)";
    return nullptr;
}

}  // namespace m0score
