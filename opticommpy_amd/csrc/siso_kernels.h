// siso_kernels.h -- single-input adaptive equalizers of the direct-detection chain (ffe, dfe, volterra) and anorm: the per-symbol
// bodies as host/device-neutral inline functions.  engine_siso.hip wraps them in gfx950 kernels; tests/emu/emu_siso.cpp loops the
// same functions over lanes and symbols with g++.
// Reference: optic/dsp/equalization.py:1176-2143 (dfe, ffe, volterra and their cores), optic/dsp/core.py:720 (anorm).
// Arithmetic is double whatever the input type and whatever `prec`.
//
// One formulation: LMS over a regressor phi(k) of `ncoef` entries, each a product of up to three samples of the window (or, for
// the feedback part of dfe, one earlier reference):  y = w . phi,  e = r - y,  w += mu_s e conj(phi).  The concatenated
// coefficient vector is  ffe: f;  dfe: [f ; b];  volterra: [h1 ; h2 row-major ; h3 row-major (order 3 only)].
//
// The window of symbol k of a pass is stream[k SpS .. k SpS + nTaps): in the first pass the stream is the zero-padded input under
// the reference's fill rule (live()); a later pass of the pre-convergence starts from the window the pass before ended with
// (the reference does not reload its buffer), so its first nTaps samples are stream_before[(nTrain + 1) SpS ..) and the rest is
// the padded input again.
//
// Lane layout of the serial kernel: coefficient c sits in lane c % 64, slot c / 64 (R slots per lane).  Per symbol a lane sums its
// products in the order of the slots; the 64 lane sums are added in a butterfly over lane distances 32, 16, 8, 4, 2, 1.
// The frozen kernel (one symbol per thread, coefficients fixed) sums taps in ascending order, the quadratic and cubic sections
// nested as  sum_i x_i sum_j x_j sum_l h3 x_l.
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace sk {

using mk::Cplx;

enum { kFfe = 0, kDfe = 1, kVolterra = 2, kAnorm = 3 };       // ssf_siso_kind
enum { kDataAided = 0, kFulltime = 1 };                       // ssf_siso_mode

// limits the kernels are built for (checked by ssf_siso_eq before anything is allocated)
constexpr int kWave = 64;
constexpr int kMaxR = 24;                     // coefficients per lane: what the serial kernel holds without spilling (32 spilled)
constexpr int kMaxCoeffs = kWave * kMaxR;     // 1536 per call
constexpr int kMaxTaps = 256;                 // the window: nTaps, nTapsFF, n1Taps
constexpr int kMaxFb = 256;                   // nTapsFB
constexpr int kMaxSpS = 8, kMaxM = 1024;
constexpr int kChunk = 64;                    // symbols staged per chunk of the serial kernel: one per lane
constexpr int kPre = 12;                      // window samples a lane holds in flight for the next chunk
constexpr int kStageElems = kWave * kPre;     // 768 >= (kChunk - 1) kMaxSpS + kMaxTaps
constexpr int kTile = 256;                    // symbols per workgroup of the frozen kernel

static_assert((kChunk - 1) * kMaxSpS + kMaxTaps <= kStageElems, "a chunk's window samples fit the staging buffer");

// a value of the signal: real kinds never touch im
template <bool CX> struct V {
    double re, im;
};
template <bool CX> MK_HD V<CX> vzero() { return V<CX>{0.0, 0.0}; }
// acc += h x
template <bool CX> MK_HD void vfma(V<CX> &acc, V<CX> h, V<CX> x) {
    if (CX) {
        acc.re += h.re * x.re - h.im * x.im;
        acc.im += h.re * x.im + h.im * x.re;
    } else {
        acc.re += h.re * x.re;
    }
}
// h += w conj(x)
template <bool CX> MK_HD void vupdate(V<CX> &h, V<CX> w, V<CX> x) {
    if (CX) {
        h.re += w.re * x.re + w.im * x.im;
        h.im += w.im * x.re - w.re * x.im;
    } else {
        h.re += w.re * x.re;
    }
}

// what a call works on
struct Geo {
    long long n;              // input samples
    long long L;              // padded samples: n + 2 Lpad
    long long N;              // output symbols: n / SpS
    long long nTrain;
    int kind, cx, fulltime, order;
    int nTaps;                // window length: nTaps, nTapsFF or n1Taps
    int nFB, n2, n3, t2, t3;
    int SpS, Lpad, M, prec32;
    int ncoef;                // entries of the regressor: nTaps | nTapsFF + nTapsFB | n1 + n2^2 (+ n3^3 at order 3)
    int passes;               // preconvIters where a restart happens (nTrain < N), else 1
    double mu;
};

MK_HD int coeffs_per_lane(int ncoef) { return (ncoef + kWave - 1) / kWave; }

// the slot counts the serial kernel is compiled for
MK_HD int slots_for(int ncoef) {
    const int r = coeffs_per_lane(ncoef);
    return r <= 1 ? 1 : r <= 2 ? 2 : r <= 4 ? 4 : r <= 8 ? 8 : r <= 16 ? 16 : 24;
}

// entry c of the regressor: the number of window samples it multiplies (1 .. 3) and their offsets in the window, or (fb) the
// reference of symbol k - 1 - i0
struct Entry {
    int deg, i0, i1, i2;
    bool fb;
};
MK_HD Entry entry_of(const Geo &g, int c) {
    Entry e{1, c, 0, 0, false};
    if (g.kind == kDfe) {
        if (c >= g.nTaps) e.i0 = c - g.nTaps, e.fb = true;
    } else if (g.kind == kVolterra && c >= g.nTaps) {
        int q = c - g.nTaps;
        if (q < g.n2 * g.n2) {
            e.deg = 2, e.i0 = g.t2 + q / g.n2, e.i1 = g.t2 + q % g.n2;
        } else {
            q -= g.n2 * g.n2;
            e.deg = 3, e.i0 = g.t3 + q / (g.n3 * g.n3), e.i1 = g.t3 + (q / g.n3) % g.n3, e.i2 = g.t3 + q % g.n3;
        }
    }
    return e;
}
// the step of an entry: mu, mu / 2, mu / 7 by degree
MK_HD double step_of(double mu, int deg) { return deg == 1 ? mu : deg == 2 ? mu / 2 : mu / 7; }

// whether position q of the padded input holds data: the reference fills the SpS samples behind symbol k from the input only
// if k SpS + nTaps + SpS < L, and with zeros otherwise
MK_HD bool live(const Geo &g, long long q) {
    if (q < g.nTaps) return true;
    const long long k = (q - g.nTaps) / g.SpS;
    return k * g.SpS + g.nTaps + g.SpS < g.L;
}

// the scales of a call, kept on the device: [0] sqrt(mean |sigIn|^2), [1] sqrt(mean |symbRef|^2), [2] max |rounded normalised
// sigIn| (volterra), [3] sqrt(mean sigOut^2) (volterra)
constexpr int kScalN = 4;

MK_HD double round_prec(double v, int prec32) { return prec32 ? (double)(float)v : v; }

// a raw input value -> what the recursion works on: pnorm, rounded to prec; for volterra anorm of that, rounded again
template <bool CX> MK_HD V<CX> normalise(const Geo &g, double sx, double mx, double re, double im) {
    V<CX> v{round_prec(re / sx, g.prec32), CX ? round_prec(im / sx, g.prec32) : 0.0};
    if (g.kind == kVolterra) v.re = round_prec(v.re / mx, g.prec32);
    return v;
}
template <bool CX> MK_HD V<CX> normalise_ref(const Geo &g, double sr, double re, double im) {
    return V<CX>{round_prec(re / sr, g.prec32), CX ? round_prec(im / sr, g.prec32) : 0.0};
}

// position q of the first pass's stream, raw (not normalised): the padded input under the fill rule
MK_HD void padded_raw(const Geo &g, int dtype, const void *x, long long q, double &re, double &im) {
    re = 0.0, im = 0.0;
    const long long s = q - g.Lpad;
    if (s >= 0 && s < g.n && live(g, q)) mk::load(dtype, x, s, re, im);
}

// distance of an output to a table point: |y - c| for real data, |y - c|^2 for complex data (the same first minimum unless two
// distances differ by less than a rounding)
template <bool CX> MK_HD double dist(V<CX> y, double cr, double ci) {
    if (CX) {
        const double dr = y.re - cr, di = y.im - ci;
        return dr * dr + di * di;
    }
    return std::fabs(y.re - cr);
}
// the better of two (distance, index) candidates: the smaller distance, the lower index on a tie (np.argmin)
MK_HD void argmin_merge(double &d, int &i, double d2, int i2) {
    if (d2 < d || (d2 == d && i2 < i)) d = d2, i = i2;
}
// first minimum over the whole table by one thread (the frozen kernel)
template <bool CX> MK_HD int nearest(const double *tab, int M, V<CX> y) {
    int bi = 0;
    double bd = dist<CX>(y, tab[0], tab[1]);
    for (int m = 1; m < M; ++m) {
        const double d = dist<CX>(y, tab[2 * m], tab[2 * m + 1]);
        if (d < bd) bd = d, bi = m;
    }
    return bi;
}

// e = r - y and |e|^2
template <bool CX> MK_HD V<CX> error_of(V<CX> r, V<CX> y, double &esq) {
    V<CX> e{r.re - y.re, CX ? r.im - y.im : 0.0};
    esq = CX ? e.re * e.re + e.im * e.im : e.re * e.re;
    return e;
}

// a lane's part of y: its R products in the order of the slots
template <int R, bool CX> MK_HD V<CX> lane_output(const V<CX> *h, const V<CX> *phi) {
    V<CX> y = vzero<CX>();
#pragma unroll
    for (int r = 0; r < R; ++r) vfma<CX>(y, h[r], phi[r]);
    return y;
}

// the butterfly of the wave's reductions on 64 values held in an array (host): after it every entry is the sum
inline void butterfly_sum(double *v) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        double t[kWave];
        for (int l = 0; l < kWave; ++l) t[l] = v[l] + v[l ^ o];
        for (int l = 0; l < kWave; ++l) v[l] = t[l];
    }
}
inline void butterfly_argmin(double *d, int *i) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
        double td[kWave];
        int ti[kWave];
        for (int l = 0; l < kWave; ++l) {
            td[l] = d[l], ti[l] = i[l];
            argmin_merge(td[l], ti[l], d[l ^ o], i[l ^ o]);
        }
        for (int l = 0; l < kWave; ++l) d[l] = td[l], i[l] = ti[l];
    }
}

// the frozen kernel's output of one symbol: w the window (nTaps values, normalised), coef the concatenated coefficients
template <bool CX> MK_HD V<CX> frozen_output(const Geo &g, const V<CX> *coef, const V<CX> *w) {
    V<CX> y = vzero<CX>();
    for (int t = 0; t < g.nTaps; ++t) vfma<CX>(y, coef[t], w[t]);
    if (g.kind != kVolterra) return y;
    const V<CX> *h2 = coef + g.nTaps, *h3 = h2 + g.n2 * g.n2;
    double quad = 0.0, cub = 0.0;
    for (int i = 0; i < g.n2; ++i) {
        double s = 0.0;
        for (int j = 0; j < g.n2; ++j) s += h2[i * g.n2 + j].re * w[g.t2 + j].re;
        quad += w[g.t2 + i].re * s;
    }
    if (g.order == 3) {
        for (int i = 0; i < g.n3; ++i) {
            double si = 0.0;
            for (int j = 0; j < g.n3; ++j) {
                double sj = 0.0;
                for (int l = 0; l < g.n3; ++l) sj += h3[(i * g.n3 + j) * g.n3 + l].re * w[g.t3 + l].re;
                si += w[g.t3 + j].re * sj;
            }
            cub += w[g.t3 + i].re * si;
        }
    }
    y.re = (y.re + quad) + cub;
    return y;
}

// how the symbols of a call are divided: every pass but the last walks symbols 0 .. nTrain serially; the last pass walks
// `serial_last` symbols serially and leaves the rest (from `frozen_from` on) to the frozen kernel
struct Split {
    long long serial_last, frozen_from, frozen_count, serial_total;
};
MK_HD Split split_of(const Geo &g, bool frozen_allowed) {
    Split s{g.N, g.N, 0, 0};
    if (frozen_allowed && !g.fulltime && g.kind != kDfe) {
        long long from = g.nTrain;
        // after a restart the first windows still hold the carried buffer: they stay with the serial kernel
        const long long plain = g.passes > 1 ? (g.nTaps + g.SpS - 1) / g.SpS : 0;
        if (from < plain) from = plain;
        if (from < g.N) s.serial_last = from, s.frozen_from = from, s.frozen_count = g.N - from;
    }
    s.serial_total = (long long)(g.passes - 1) * (g.nTrain + 1) + s.serial_last;
    return s;
}

}  // namespace sk
}  // namespace ssf
