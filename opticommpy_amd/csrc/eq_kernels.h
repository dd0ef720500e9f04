// eq_kernels.h -- adaptive MIMO equalizer (NLMS, CMA, RDE, data-aided RDE, DD-LMS, static): the per-symbol bodies as
// host/device-neutral inline functions.  engine_eq.hip wraps them in gfx950 kernels (one wavefront per output mode, its
// coefficients in registers); tests/emu/emu_eq.cpp loops the same functions over lanes and symbols with g++.
// Reference: optic/dsp/equalization.py:125-351 (mimoAdaptEqualizer), 354-516 (coreAdaptEq), 519-572 (nlmsUp), 647-708 (ddlmsUp),
// 788-843 (cmaUp), 846-909 (rdeUp), 912-973 (dardeUp).
// Arithmetic is double whatever the input type; single-precision inputs are widened on load (metrics_kernels.h: load).
//
// Why one wave per output mode: in every update rule row k + N nModes of H changes by a factor that depends on y_k (and the
// reference or decision of mode k) times conj(x_N).  The nModes rows that make y_k are therefore a filter of their own: an
// nModes x nModes equalizer is nModes independent multiple-input single-output recursions.
//
// Lane layout: the nModes nTaps coefficients of an output mode are numbered j = N nTaps + t (input mode N, tap t); lane l holds
// j = l + 64 r for r = 0 .. R - 1, R = ceil(nModes nTaps / 64).  Per symbol a lane sums its R products in the order of r; the 64
// lane sums are added in a butterfly over lane distances 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace eqk {

using mk::Cplx;
using mk::load;

enum { kNlms = 0, kCma = 1, kRde = 2, kDaRde = 3, kDdLms = 4, kStatic = 5 };            // ssf_eq_alg

// limits the kernels are built for (checked by ssf_mimo_eq before anything is allocated)
constexpr int kMaxModes = 4, kMaxTaps = 64, kMaxSpS = 8, kMaxM = 1024, kMaxRadii = 1024;
constexpr int kWave = 64;
constexpr int kMaxR = kMaxModes * kMaxTaps / kWave;     // coefficients per lane: 4
constexpr int kChunk = 64;        // output symbols staged per chunk: one per lane, so a chunk's outputs leave in one store
constexpr int kPre = 16;          // padded input elements a lane holds in flight for the next chunk
constexpr int kStageElems = kWave * kPre;               // the staging buffer: 1024 complex values, 16 KiB of LDS

// one stretch of symbols the serial kernel walks: `reps` times over symbols start .. start + len - 1 with one rule and step size
struct Seg {
    long long start, len;
    int alg, reps;
    double mu;
};

// output symbols of one chunk: kChunk, or fewer where ((c - 1) SpS + nTaps) nModes input values would not fit the buffer
MK_HD int chunk_symbols(int nModes, int nTaps, int SpS) {
    const int c = (kStageElems / nModes - nTaps) / SpS + 1;
    return c < kChunk ? c : kChunk;
}

MK_HD int coeffs_per_lane(int nModes, int nTaps) { return (nModes * nTaps + kWave - 1) / kWave; }

// coefficient r of a lane: input mode N and tap t, or nothing (the lane layout above)
MK_HD bool lane_coeff(int lane, int r, int nModes, int nTaps, int &N, int &t) {
    const int j = lane + kWave * r;
    if (j >= nModes * nTaps) {
        N = 0, t = 0;
        return false;
    }
    N = j / nTaps, t = j - N * nTaps;
    return true;
}

// sample p of the zero-padded input of mode N (Lpad zeros ahead of the n samples and behind them)
MK_HD Cplx padded(int dtype, const void *x, long long n, int nModes, int Lpad, long long p, int N) {
    Cplx v{0.0, 0.0};
    const long long g = p - Lpad;
    if (g >= 0 && g < n) load(dtype, x, g * nModes + N, v.re, v.im);
    return v;
}

// a lane's part of y = sum_j h_j x_j (numpy's complex product, summed in the order of r)
template <int R>
MK_HD void lane_output(const Cplx *h, const Cplx *x, double &yr, double &yi) {
    yr = 0.0, yi = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        yr += h[r].re * x[r].re - h[r].im * x[r].im;
        yi += h[r].re * x[r].im + h[r].im * x[r].re;
    }
}

// ... and of ||x_N||^2 for every input mode N (NLMS): pw[N] takes |x_r|^2 of the coefficients that belong to mode N
template <int R>
MK_HD void lane_power(const Cplx *x, const int *mode, double *pw) {
#pragma unroll
    for (int m = 0; m < kMaxModes; ++m) pw[m] = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double p = x[r].re * x[r].re + x[r].im * x[r].im;
#pragma unroll
        for (int m = 0; m < kMaxModes; ++m) pw[m] += mode[r] == m ? p : 0.0;
    }
}

// np.linalg.norm(x) ** 2 from the sum of squares, then the reciprocal numpy's complex / real division multiplies by
MK_HD double nlms_scale(double sum_sq) {
    const double nr = std::sqrt(sum_sq);
    return 1.0 / (nr * nr);
}

// the factor g of the update H += (mu g) conj(x) and |e|^2
struct Err {
    double gr, gi, esq;
};
// NLMS, DD-LMS: e = target - y, g = e
MK_HD Err err_linear(double tr, double ti, double yr, double yi) {
    const double er = tr - yr, ei = ti - yi;
    return Err{er, ei, er * er + ei * ei};
}
// CMA, RDE, DA-RDE: e = r2 - |y|^2 (real), g = e y
MK_HD Err err_radius(double r2, double yr, double yi) {
    const double e = r2 - (yr * yr + yi * yi);
    return Err{e * yr, e * yi, e * e};
}

// the better of two (distance, index) candidates: the smaller distance, the lower index on a tie (np.argmin)
MK_HD void argmin_merge(double &d, int &i, double d2, int i2) {
    if (d2 < d || (d2 == d && i2 < i)) d = d2, i = i2;
}
MK_HD double dist_point(double cr, double ci, double yr, double yi) {
    const double dr = yr - cr, di = yi - ci;
    return dr * dr + di * di;
}
MK_HD double dist_radius(double R, double a) { return std::fabs(R - a); }

// h += w conj(x), w = mu g
MK_HD void update(Cplx &h, double wr, double wi, double xr, double xi) {
    h.re += wr * xr + wi * xi;
    h.im += wi * xr - wr * xi;
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

// static stage: output symbol i of mode k with H fixed, summed over input modes and taps in order
MK_HD Cplx static_output(const Cplx *H, int dtype, const void *x, long long n, int nModes, int nTaps, int SpS, int Lpad, long long i,
                         int k) {
    Cplx y{0.0, 0.0};
    for (int N = 0; N < nModes; ++N) {
        const Cplx *h = H + (long long)(k + N * nModes) * nTaps;
        for (int t = 0; t < nTaps; ++t) {
            const Cplx v = padded(dtype, x, n, nModes, Lpad, i * SpS + t, N);
            y.re += h[t].re * v.re - h[t].im * v.im;
            y.im += h[t].re * v.im + h[t].im * v.re;
        }
    }
    return y;
}

}  // namespace eqk
}  // namespace ssf
