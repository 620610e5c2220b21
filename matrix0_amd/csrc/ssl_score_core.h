// Square arithmetic of the SSL score (include/m0_ssl_score.h): the reference's SSL losses (azchess/model/resnet.py:892-1130, as
// matrix0_amd/ssl_loss.py restates them) for ONE square of one row, and the merge of a row's 64 squares.  Plain C++ without
// intrinsics, host and device: ssl_score_kernels.hip runs it with one lane per square, tests/ssl_score_shim runs the same code
// under g++ with the lanes as a loop.
//
// The exponential and the logarithm are written out here (range reduction and a polynomial in fmaf, no library call, nothing the
// compiler may contract differently), so that a row has the same bits on the device and on the host.  Their arguments are
// narrow: exp only of x <= 0 (a logit minus the maximum, -|z|), log only of a soft-max denominator in [1, 13] and of 1 + e with
// e in (0, 1]; both are good to about 2 ulp there.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "ssl_targets_core.h"

namespace m0sslscore {

constexpr int LANES = 64;
constexpr int ALL_TASKS = M0_SSL_PIECE | M0_SSL_THREAT | M0_SSL_PIN | M0_SSL_FORK | M0_SSL_CONTROL;
constexpr int COUNTS = 10;                    // columns 5-14

// channels of the heads of `tasks`, in the order piece 13, threat 1, pin 1, fork 1, control 3
M0_SSL_HD int channels(int tasks) {
    return (tasks & M0_SSL_PIECE ? 13 : 0) + (tasks & M0_SSL_THREAT ? 1 : 0) + (tasks & M0_SSL_PIN ? 1 : 0) +
           (tasks & M0_SSL_FORK ? 1 : 0) + (tasks & M0_SSL_CONTROL ? 3 : 0);
}

M0_SSL_HD float bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
M0_SSL_HD uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// e^x for x <= 0; 0 below -87 (where e^x leaves the normal numbers) and for NaN
M0_SSL_HD float exp_le0(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!(x >= -87.f)) return 0.f;
    const float n = rintf(x * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, x);                  // x - n ln 2 in two pieces: |r| <= 0.347
    r = fmaf(n, -1.428606765330187045e-06f, r);
    float p = 1.f / 5040.f;                                     // Taylor to r^7: the next term is below 5e-9
    p = fmaf(p, r, 1.f / 720.f);
    p = fmaf(p, r, 1.f / 120.f);
    p = fmaf(p, r, 1.f / 24.f);
    p = fmaf(p, r, 1.f / 6.f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.f);
    p = fmaf(p, r, 1.f);
    return p * bits_float((uint32_t)((int)n + 127) << 23);      // n >= -126: the scale and the product are normal
}

// log(1 + f) for f in [-0.3, 1] as 2 atanh(s), s = f / (2 + f): |s| <= 1/3, the series to s^17
M0_SSL_HD float log1p_series(float f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float s = f / (2.f + f);
    const float s2 = s * s;
    float p = 1.f / 17.f;
    p = fmaf(p, s2, 1.f / 15.f);
    p = fmaf(p, s2, 1.f / 13.f);
    p = fmaf(p, s2, 1.f / 11.f);
    p = fmaf(p, s2, 1.f / 9.f);
    p = fmaf(p, s2, 1.f / 7.f);
    p = fmaf(p, s2, 1.f / 5.f);
    p = fmaf(p, s2, 1.f / 3.f);
    const float t = s + s;
    return fmaf(t * s2, p, t);
}

// log(x) for a normal x >= 1 (any other x gives some finite number or NaN; such rows are zeroed by their flag)
M0_SSL_HD float log_ge1(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t u = float_bits(x);
    int k = (int)(u >> 23) - 127;
    float m = bits_float((u & 0x007fffffu) | 0x3f800000u);      // x = 2^k m, m in [1, 2)
    if (m > 1.41421354f) { m *= 0.5f; ++k; }
    const float kf = (float)k;
    return fmaf(kf, 0.693145751953125f, fmaf(kf, 1.428606765330187045e-06f, log1p_series(m - 1.f)));
}

// ---- one square's inputs ----
struct Logits {
    float piece[13];
    float threat, pin, fork;
    float control[3];
};

// heads_row: f32 [channels(tasks)][64] as Net::forward leaves a row; channel c of square sq at c * 64 + sq
M0_SSL_HD Logits load_logits(int tasks, const float* heads_row, int sq) {
    Logits z = {};
    const float* h = heads_row + sq;
    if (tasks & M0_SSL_PIECE) { for (int k = 0; k < 13; ++k) z.piece[k] = h[k * 64]; h += 13 * 64; }
    if (tasks & M0_SSL_THREAT) { z.threat = h[0]; h += 64; }
    if (tasks & M0_SSL_PIN) { z.pin = h[0]; h += 64; }
    if (tasks & M0_SSL_FORK) { z.fork = h[0]; h += 64; }
    if (tasks & M0_SSL_CONTROL) { for (int k = 0; k < 3; ++k) z.control[k] = h[k * 64]; }
    return z;
}

// 0 (of either sign) while every logit of a scored task is finite, NaN otherwise; sums of it keep that
M0_SSL_HD float poison_of(const Logits& z) {
    float p = z.threat * 0.f + z.pin * 0.f + z.fork * 0.f;
    for (int k = 0; k < 13; ++k) p += z.piece[k] * 0.f;
    for (int k = 0; k < 3; ++k) p += z.control[k] * 0.f;
    return p;
}

struct Targets {
    int piece;                             // class 0..12 (12: empty)
    float threat, pin, fork, control;      // as stored: clamped or thresholded where they are used
};

M0_SSL_HD Targets targets_of(const m0ssl::SquareTargets& t) {
    return Targets{t.piece < 0 ? 12 : t.piece, t.threat ? 1.f : 0.f, 0.f, t.fork ? 1.f : 0.f, (float)t.control};
}

// targets_row: f32 [17][64], the layout of m0_game_record.ssl; the piece class is the first maximum of the 13 channels
M0_SSL_HD Targets stored_targets(const float* targets_row, int sq) {
    const float* t = targets_row + sq;
    int cls = 0;
    float best = t[0];
    for (int k = 1; k < 13; ++k) { const float v = t[k * 64]; if (v > best) { best = v; cls = k; } }
    return Targets{cls, t[13 * 64], t[14 * 64], t[15 * 64], t[16 * 64]};
}

M0_SSL_HD int control_class(float t) { return t < -0.5f ? 0 : (t > 0.5f ? 2 : 1); }

// do two squares' targets fall into different classes for a task of `tasks`
M0_SSL_HD bool classes_differ(int tasks, const Targets& a, const Targets& b) {
    bool d = false;
    if (tasks & M0_SSL_PIECE) d = d || a.piece != b.piece;
    if (tasks & M0_SSL_THREAT) d = d || (a.threat >= 0.5f) != (b.threat >= 0.5f);
    if (tasks & M0_SSL_PIN) d = d || (a.pin >= 0.5f) != (b.pin >= 0.5f);
    if (tasks & M0_SSL_FORK) d = d || (a.fork >= 0.5f) != (b.fork >= 0.5f);
    if (tasks & M0_SSL_CONTROL) d = d || control_class(a.control) != control_class(b.control);
    return d;
}

// ---- one square's result, and the sum of squares ----
struct Cell {
    float loss[5] = {0.f, 0.f, 0.f, 0.f, 0.f};         // piece, threat, pin, fork, control
    int n[COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};    // columns 5-14
    M0_SSL_HD void merge(const Cell& o) {
        for (int i = 0; i < 5; ++i) loss[i] += o.loss[i];
        for (int i = 0; i < COUNTS; ++i) n[i] += o.n[i];
    }
};

// cross-entropy of N logits against class cls; *top is the arg-max, the lowest index among equals
template <int N>
M0_SSL_HD float cross_entropy(const float* z, int cls, int* top) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float m = z[0], zc = z[0], s = 0.f;
    int am = 0;
    for (int k = 1; k < N; ++k) {
        if (z[k] > m) { m = z[k]; am = k; }
        zc = k == cls ? z[k] : zc;
    }
    for (int k = 0; k < N; ++k) s += exp_le0(z[k] - m);
    *top = am;
    return log_ge1(s) - (zc - m);
}

// binary cross-entropy with logits as torch writes it, the target clamped to [0, 1]
M0_SSL_HD float bce(float z, float t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float tc = fminf(fmaxf(t, 0.f), 1.f);
    return (fmaxf(z, 0.f) - z * tc) + log1p_series(exp_le0(-fabsf(z)));
}

M0_SSL_HD Cell score_square(int tasks, const Logits& z, const Targets& t) {
    Cell c;
    int top;
    if (tasks & M0_SSL_PIECE) {
        c.loss[0] = cross_entropy<13>(z.piece, t.piece, &top);
        const bool hit = top == t.piece, occupied = t.piece != 12;
        c.n[0] = hit; c.n[1] = hit && occupied; c.n[2] = occupied;
    }
    if (tasks & M0_SSL_THREAT) {
        c.loss[1] = bce(z.threat, t.threat);
        const bool says = z.threat > 0.f, is = t.threat >= 0.5f;
        c.n[3] = says && is; c.n[4] = says; c.n[5] = is;
    }
    if (tasks & M0_SSL_PIN) c.loss[2] = bce(z.pin, t.pin);
    if (tasks & M0_SSL_FORK) {
        c.loss[3] = bce(z.fork, t.fork);
        const bool says = z.fork > 0.f, is = t.fork >= 0.5f;
        c.n[6] = says && is; c.n[7] = says; c.n[8] = is;
    }
    if (tasks & M0_SSL_CONTROL) {
        const int cls = control_class(t.control);
        c.loss[4] = cross_entropy<3>(z.control, cls, &top);
        c.n[9] = top == cls;
    }
    return c;
}

// The row's M0_SSL_SCORE_COLS columns from the sum of its squares.  unusable: the planes are (flag 1); poisoned: a scored logit
// is not finite (flag 2); stored: targets were given; differ: they disagree with the planes' somewhere (flag 4 if those are usable).
M0_SSL_HD void finish(const Cell& sum, bool unusable, bool poisoned, bool stored, bool differ, float* out) {
    int flags = 0;
    if (unusable) flags |= M0_SSL_SCORE_FLAG_PLANES;
    if (poisoned) flags |= M0_SSL_SCORE_FLAG_NONFINITE;
    if (stored && !unusable && differ) flags |= M0_SSL_SCORE_FLAG_MISMATCH;
    const bool zero = poisoned || (unusable && !stored);
    for (int i = 0; i < 5; ++i) out[i] = zero ? 0.f : sum.loss[i] * (1.f / 64.f);
    for (int i = 0; i < COUNTS; ++i) out[5 + i] = zero ? 0.f : (float)sum.n[i];
    out[15] = (float)flags;
}

// tasks: a non-empty subset of the five M0_SSL_* bits
inline bool bad_tasks(int tasks) { return tasks <= 0 || (tasks & ~ALL_TASKS) != 0; }

}  // namespace m0sslscore
