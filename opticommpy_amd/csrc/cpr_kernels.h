// cpr_kernels.h -- carrier phase recovery (blind phase search, unwrap, phase compensation, 4th-power frequency offset
// estimation): the per-element bodies as host/device-neutral inline functions.  engine_cpr.hip wraps them in gfx950 kernels;
// tests/emu/emu_cpr.cpp loops the same functions over the symbols with g++.
// Reference: optic/dsp/carrierRecovery.py:37-169 (cpr), 172-223 (bps), 333-371 (fourthPowerFOE);
// optic/dsp/carrierRecoveryGPU.py:17-68 (bpsGPU); numpy's unwrap.
// Arithmetic is double whatever the input type; single-precision inputs are widened on load (metrics_kernels.h: load).
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace ck {

using mk::Cplx;
using mk::load;

// limits the kernels are built for (checked by ssf_cpr / ssf_bps / ssf_foe before anything is allocated)
constexpr int kMaxM = 1024;       // constellation points (table in LDS: 16 KiB)
constexpr int kMaxB = 1024;       // test phases
constexpr int kMaxNh = 1023;      // half window: the window holds 2 Nh + 1 <= 2047 symbols
constexpr int kMaxModes = 64;
constexpr int kMaxPower = 1024;   // FOE: x ** P
constexpr int kTile = 256;        // output symbols of one workgroup of the search (one per lane)
constexpr int kScanPer = 4;       // elements per lane of the unwrap's block scan
constexpr int kScanBlock = 256 * kScanPer;

constexpr double kPiD = 3.141592653589793;

MK_HD void sincos_d(double t, double &s, double &c) {
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincos(t, &s, &c);                  // (full-range argument reduction in double precision)
#else
    s = std::sin(t), c = std::cos(t);
#endif
}

// x e^{j phi} given (cos, sin), numpy's complex product
MK_HD void rotate(double xr, double xi, double c, double s, double &yr, double &yi) {
    yr = xr * c - xi * s;
    yi = xr * s + xi * c;
}

// ---- blind phase search: min_m |x e^{j phi} - c_m|^2 over the whole table (tab: M interleaved (re, im) pairs)
MK_HD double dmin_full(const double *tab, int M, double xr, double xi, double c, double s) {
    double yr, yi;
    rotate(xr, xi, c, s, yr, yi);
    double best = INFINITY;
    for (int m = 0; m < M; ++m) {
        const double dr = yr - tab[2 * m], di = yi - tab[2 * m + 1];
        const double d = dr * dr + di * di;
        best = d < best ? d : best;
    }
    return best;
}

// ... and for a table that is the full product of nr real and ni imaginary levels (square QAM): the minimum over the product is
// the sum of the minima of the two axes -- rounding is monotonic, so this is the value dmin_full finds (2 sqrt(M) comparisons)
MK_HD double dmin_sep(const double *lre, int nr, const double *lim, int ni, double xr, double xi, double c, double s) {
    double yr, yi;
    rotate(xr, xi, c, s, yr, yi);
    double br = INFINITY, bi = INFINITY;
    for (int m = 0; m < nr; ++m) {
        const double d = yr - lre[m], q = d * d;
        br = q < br ? q : br;
    }
    for (int m = 0; m < ni; ++m) {
        const double d = yi - lim[m], q = d * d;
        bi = q < bi ? q : bi;
    }
    return br + bi;
}

// window sum of the 2 Nh + 1 values first .. first + 2 Nh of a row, from the row's inclusive prefix sums c.  A row starts Nh
// symbols ahead of its tile, so every symbol of a tile has its whole window in the row, the one at a tile border as any other.
// The prefix sums carry a rounding error of a few ulp of the row's total (at most (256 + 2 Nh) / (2 Nh + 1) windows long): the
// argmin is that of exact sums wherever the two smallest differ by more than about 1e-14 relative.
MK_HD double window_from_prefix(const double *c, int first, int Nh) {
    const double hi = c[first + 2 * Nh];
    return first ? hi - c[first - 1] : hi;
}

// ---- np.unwrap(p) with the default period 2 pi: the correction that symbol k adds to the running sum (p = 4 phi)
MK_HD double unwrap_corr(double prev, double cur) {
    const double twoPi = 2.0 * kPiD;
    const double dd = cur - prev;
    double m = std::fmod(dd + kPiD, twoPi);        // numpy's mod: the sign of the divisor
    if (m < 0.0) m += twoPi;
    double ddmod = m - kPiD;
    if (ddmod == -kPiD && dd > 0.0) ddmod = kPiD;
    return std::fabs(dd) < kPiD ? 0.0 : ddmod - dd;
}

// ---- frequency offset estimation
// (xr + j xi) ** P by binary exponentiation, P >= 1
MK_HD void cpow_int(double xr, double xi, int P, double &yr, double &yi) {
    double br = xr, bi = xi, rr = 1.0, ri = 0.0;
    bool first = true;
    while (P > 0) {
        if (P & 1) {
            if (first) {
                rr = br, ri = bi, first = false;
            } else {
                const double t = rr * br - ri * bi;
                ri = rr * bi + ri * br, rr = t;
            }
        }
        P >>= 1;
        if (P) {
            const double t = br * br - bi * bi;
            bi = br * bi + bi * br, br = t;
        }
    }
    yr = rr, yi = ri;
}

// position i of the fftshift-ed spectrum of length n: the transform's bin, and its signed frequency index
MK_HD long long shifted_bin(long long i, long long n) {
    const long long b = i - n / 2;
    return b < 0 ? b + n : b;
}
MK_HD long long signed_index(long long bin, long long n) { return bin < (n - 1) / 2 + 1 ? bin : bin - n; }

// fo = fftshift(Fs fftfreq(n))[i] / P with numpy's operations in numpy's order
inline double foe_frequency(long long i, long long n, double Fs, int P) {
    const double val = 1.0 / ((double)n * 1.0);
    const double f = Fs * ((double)signed_index(shifted_bin(i, n), n) * val);
    return f / (double)P;
}
// the reference's exp(-1j * 2 * np.pi * fo * t) has the angle a t with a = -(2 pi fo), t = k / Fs
inline double foe_slope(double fo) { return -(2.0 * kPiD * fo); }

MK_HD void derotate(double xr, double xi, double a, long long k, double Fs, double &yr, double &yi) {
    const double t = (double)k / Fs;
    double s, c;
    sincos_d(a * t, s, c);
    rotate(xr, xi, c, s, yr, yi);
}

// the better of two (|X|^2, position) candidates: the larger magnitude, the earlier position on a tie (np.argmax)
MK_HD void argmax_merge(double &m, long long &i, double m2, long long i2) {
    if (m2 > m || (m2 == m && i2 < i)) m = m2, i = i2;
}

}  // namespace ck
}  // namespace ssf
