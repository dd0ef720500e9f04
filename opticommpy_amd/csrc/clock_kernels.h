// clock_kernels.h -- the sampling clock: the converters that put a clock offset on a signal (clockSamplingInterp, quantizer, the
// clip of adc, the min/max of dac) and the stage that takes it off again (gardnerClockRecovery, calcClockDrift): the per-element
// and per-output bodies as host/device-neutral inline functions.  engine_clock.hip wraps them in gfx950 kernels;
// tests/emu/emu_clock.cpp walks the same functions in the launch geometry with g++.
// Reference: optic/dsp/core.py:272-349 (clockSamplingInterp, quantizer), optic/models/devices.py:793-1022 (adc, dac),
// optic/dsp/clockRecovery.py:24-232 (gardnerTED, gardnerTEDnyquist, interpolator, gardnerClockRecovery, calcClockDrift).
// Arithmetic is double; single-precision data are widened on load and rounded on store.  Every expression is written in the
// order numpy evaluates it and the translation unit is compiled without contraction of multiply-adds: results are the reference's
// (the converters) or the restatement's (tests/clock_restatement.py: the clock recovery) bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace ck {

using mk::Cplx;
using mk::CplxF;

constexpr int kBlock = 256;       // lanes per workgroup of the element-wise passes and of the reductions
constexpr int kMaxBlocks = 4096;  // workgroups of a grid-stride pass; the min/max partials of one call
constexpr int kWave = 64;
constexpr int kChunk = 256;       // input samples of one column the clock recovery stages in LDS per chunk
constexpr int kWin = kChunk + 4;  // ... with the four neighbours an output at the chunk's last sample reads (x[m-2] .. x[m+2])
constexpr int kPre = (kWin + kWave - 1) / kWave;      // values a lane holds in flight for the next chunk: 5
constexpr int kRing = 256;        // outputs (and timing values) of a column held in LDS, a ring indexed by n mod kRing
constexpr int kFlush = 64;        // outputs that leave in one store: [f, f + kFlush) goes once n >= f + kLag
constexpr int kLag = 128;         // so an output is still in LDS while n is less than kLag - kFlush = 64 places ahead of it

enum { kFormReal = 0, kFormComplex = 1, kFormComponents = 2 };        // ssf_clock_params.form
enum { kGardnerOk = 0, kGardnerBackrun = 1 };                          // status of a column of the clock recovery

// ---- clockSamplingInterp: np.interp(tout, tin, x) with tin[j] = double(j) inTs
// j with tin[j] <= t < tin[j+1] for tin[0] <= t <= tin[N-1]: a guess from t inFs (a product: the guess may be one off, a quotient
// would cost a division per output), corrected against double(j) inTs so that it is the index a binary search over tin finds
MK_HD long long interp_index(double t, double inTs, double inFs, long long N) {
    double g = std::floor(t * inFs);
    long long j = !(g > 0.0) ? 0 : g > (double)(N - 1) ? N - 1 : (long long)g;
    while (j + 1 < N && (double)(j + 1) * inTs <= t) ++j;
    while (j > 0 && (double)j * inTs > t) --j;
    return j;
}

// which of numpy's cases an output time falls in: j, and whether x[j] is the result as it is
MK_HD bool interp_locate(double t, double inTs, double inFs, long long N, long long &j) {
    if (t < 0.0) {                                     // tin[0] = 0
        j = 0;
        return true;
    }
    if (!(t <= (double)(N - 1) * inTs)) {              // beyond the end (a NaN time ends here too: locate() marks it)
        j = N - 1;
        return true;
    }
    j = interp_index(t, inTs, inFs, N);
    return j == N - 1 || t == (double)j * inTs;
}

// numpy's real rule: the slope is a quotient
MK_HD double interp_real(double a, double b, double tj, double tj1, double t) { return ((b - a) / (tj1 - tj)) * (t - tj) + a; }
// numpy's complex rule, per component: the slope is a product with the reciprocal
MK_HD double interp_recip(double a, double b, double inv, double tj, double t) { return ((b - a) * inv) * (t - tj) + a; }

// an output time located among the input times: the two samples it lies between (row j, and j + 1 unless x[j] is the result)
struct Located {
    long long j;
    bool exact;
    bool nan;                     // a NaN time among two or more input times: numpy hands the time itself on
    double t;
};
MK_HD Located locate(double t, double inTs, double inFs, long long N) {
    Located l;
    l.t = t;
    l.nan = t != t && N > 1;      // (one input time: numpy compares, and a NaN that is neither below nor above gives x[0])
    l.exact = interp_locate(t, inTs, inFs, N, l.j);
    return l;
}
// component `comp` of the output located at l, from the samples a = x[j] and b = x[j + 1] of the column
MK_HD double interp_component(const Located &l, const double *a, const double *b, int comp, double inTs, bool recip) {
    if (l.nan) return recip && comp == 1 ? 0.0 : l.t;        // numpy's complex rule: NaN + 0j; its real rule: NaN
    if (l.exact) return a[comp];
    const double tj = (double)l.j * inTs, tj1 = (double)(l.j + 1) * inTs;
    return recip ? interp_recip(a[comp], b[comp], 1.0 / (tj1 - tj), tj, l.t) : interp_real(a[comp], b[comp], tj, tj1, l.t);
}
// the two samples of a column around l (b only where it is read)
MK_HD void interp_samples(int dtype, const void *x, int ncols, int col, const Located &l, double *a, double *b) {
    mk::load(dtype, x, l.j * ncols + col, a[0], a[1]);
    b[0] = 0.0, b[1] = 0.0;
    if (!l.exact) mk::load(dtype, x, (l.j + 1) * ncols + col, b[0], b[1]);
}

// ---- np.clip
MK_HD double clip_real(double v, double lo, double hi) {
    if (v != v) return v;
    v = lo < v ? v : lo;
    return v < hi ? v : hi;
}
// numpy's order of complex numbers: the real parts decide, the imaginary parts only between equal real parts
MK_HD bool complex_less(double ar, double ai, double br, double bi) { return ar < br || (ar == br && ai < bi); }
// np.clip(z, lo + 1j lo, hi + 1j hi): a value below the lower bound in that order becomes the bound entirely
MK_HD void clip_complex(double &re, double &im, double lo, double hi) {
    if (re != re || im != im) return;
    if (!complex_less(lo, lo, re, im)) re = lo, im = lo;
    if (!complex_less(re, im, hi, hi)) re = hi, im = hi;
}

// ---- quantizer: d[i] = qmin + double(i) qdelta for i < levels (np.arange), the output d[argmin |x - d|], the first minimum
MK_HD double quant_level(long long i, double qmin, double qdelta) { return qmin + (double)i * qdelta; }
MK_HD double quantize(double x, double qmin, double qdelta, long long levels) {
    if (x != x) return qmin;                                           // np.argmin of all-NaN distances is 0
    double g = std::nearbyint((x - qmin) / qdelta);
    long long c = !(g > 0.0) ? 0 : g > (double)(levels - 1) ? levels - 1 : (long long)g;
    const long long first = c > 0 ? c - 1 : 0, last = c + 1 < levels ? c + 1 : levels - 1;
    long long best = first;
    double dbest = std::fabs(x - quant_level(first, qmin, qdelta));
    for (long long i = first + 1; i <= last; ++i) {
        const double d = std::fabs(x - quant_level(i, qmin, qdelta));
        if (d < dbest) dbest = d, best = i;
    }
    return quant_level(best, qmin, qdelta);
}

// rounding of a double to the precision the data are stored in
MK_HD double round_to(bool single, double v) { return single ? (double)(float)v : v; }
MK_HD bool is_single(int dtype) { return dtype == mk::kC64 || dtype == mk::kF32; }
MK_HD bool is_complex(int dtype) { return dtype == mk::kC128 || dtype == mk::kC64; }

// the converter chain on one element: interpolate (to the data's precision), clip, quantise
struct Chain {
    long long n_in, n_out;
    int ncols, dtype, form, clip, quantize;
    double inTs, outTs, lo, hi, qmin, qdelta;
    long long levels;
    double inFs;                  // 1 / inTs: the index guess only
};
// element q = row ncols + col of the output; t_re / t_im: the output times (NULL: double(row) outTs)
MK_HD void chain_element(const Chain &c, const void *x, const double *t_re, const double *t_im, long long q, double &re, double &im) {
    const long long row = q / c.ncols;
    const int col = (int)(q - row * c.ncols);
    const bool single = is_single(c.dtype), cplx = is_complex(c.dtype);
    const double tr = t_re ? t_re[row] : (double)row * c.outTs;
    const bool recip = c.form == kFormComplex;
    double a[2], b[2];
    Located l = locate(tr, c.inTs, c.inFs, c.n_in);
    interp_samples(c.dtype, x, c.ncols, col, l, a, b);
    re = round_to(single, interp_component(l, a, b, 0, c.inTs, recip));
    im = 0.0;
    if (cplx) {
        if (c.form == kFormComponents && t_im) {        // the imaginary parts at times of their own
            l = locate(t_im[row], c.inTs, c.inFs, c.n_in);
            interp_samples(c.dtype, x, c.ncols, col, l, a, b);
        }
        im = round_to(single, interp_component(l, a, b, 1, c.inTs, recip));
        if (c.form == kFormComponents && im != im) re = im;     // the parts are put together as re + 1j im: numpy's product 1j NaN is NaN + NaN j
    }
    if (c.clip) {
        if (cplx) clip_complex(re, im, c.lo, c.hi);
        else re = clip_real(re, c.lo, c.hi);
    }
    if (c.quantize) {
        re = quantize(re, c.qmin, c.qdelta, c.levels);
        if (cplx) im = quantize(im, c.qmin, c.qdelta, c.levels);
    }
}

// ---- clock recovery
// the Farrow structure's cubic coefficients at t (optic/dsp/clockRecovery.py:77-82), every product and sum in the stated order
struct Farrow {
    double c0, c1, c2, c3;
};
MK_HD Farrow farrow(double t) {
    const double t2 = t * t, t3 = t2 * t;
    Farrow f;
    f.c0 = (-1.0 / 6.0) * t3 + (1.0 / 6.0) * t;
    f.c1 = ((0.5 * t3) + (0.5 * t2)) - t;
    f.c2 = (((-0.5 * t3) - t2) + 0.5 * t) + 1.0;
    f.c3 = ((1.0 / 6.0) * t3 + 0.5 * t2) + (1.0 / 3.0) * t;
    return f;
}
MK_HD double farrow_apply(const Farrow &f, double x0, double x1, double x2, double x3) {
    return ((x0 * f.c0 + x1 * f.c1) + x2 * f.c2) + x3 * f.c3;
}
// the interpolated sample, rounded to single precision as it is stored
MK_HD CplxF interpolate(const Cplx *w, double t) {
    const Farrow f = farrow(t);
    return CplxF{(float)farrow_apply(f, w[0].re, w[1].re, w[2].re, w[3].re), (float)farrow_apply(f, w[0].im, w[1].im, w[2].im, w[3].im)};
}
// the timing error from the stored outputs a = out[n-2], b = out[n-1], c = out[n], widened
MK_HD double ted_nyquist(CplxF a, CplxF b, CplxF c) {
    const double pa = (double)a.re * (double)a.re + (double)a.im * (double)a.im;
    const double pb = (double)b.re * (double)b.re + (double)b.im * (double)b.im;
    const double pc = (double)c.re * (double)c.re + (double)c.im * (double)c.im;
    return pb * (pa - pc);
}
MK_HD double ted_gardner(CplxF a, CplxF b, CplxF c) {
    return (double)b.re * ((double)c.re - (double)a.re) + (double)b.im * ((double)c.im - (double)a.im);
}

// the loop filter: the state of one column's loop is t_nco and intPart, and the indices n (output) and m (input)
MK_HD void loop_filter(double &t_nco, double &intPart, double ted, double kp, double ki) {
    intPart = ki * ted + intPart;
    t_nco -= kp * ted + intPart;
}
// the NCO's clock gap: the three branches of clockRecovery.py:161-171.  Returns the step of n: -1 (m stays), 2 or 1 (m moves on).
MK_HD int nco_gap(double &t_nco) {
    if (t_nco > 1.0) {
        t_nco -= 1.0;
        return -1;
    }
    if (t_nco < -1.0) {
        t_nco += 1.0;
        return 2;
    }
    return 1;
}
// the loop runs while this holds (the reference's condition; it raises where n falls below 1, here the column ends)
MK_HD bool loop_runs(long long n, long long m, long long Ln, long long nSamples) { return n >= 1 && n < Ln - 1 && m < nSamples - 2; }

// sample p of the column's input with lpad zeros behind its n samples
MK_HD Cplx padded(int dtype, const void *x, long long n, int nModes, int col, long long p) {
    Cplx v{0.0, 0.0};
    if (p >= 0 && p < n) mk::load(dtype, x, p * nModes + col, v.re, v.im);
    return v;
}

// ---- calcClockDrift: d[i] = |(t[i+1] - mean) - (t[i] - mean)|, i < n - 1; scipy.signal.find_peaks(d, height=0.5): a peak is a
// run d[i] .. d[j] of equal values with d[i-1] < d[i] and d[j+1] < d[j], both neighbours inside the array; its index the middle
MK_HD double drift_diff(const double *t, long long n, int ncols, int col, double mean, long long i) {
    return std::fabs((t[(i + 1) * ncols + col] - mean) - (t[i * ncols + col] - mean));
}
// whether a peak starts at i (1 <= i <= nd - 2, nd = n - 1 differences), and the peak's index
MK_HD bool drift_peak(const double *t, long long n, int ncols, int col, double mean, long long i, long long &at) {
    const long long nd = n - 1;
    const double v = drift_diff(t, n, ncols, col, mean, i);
    if (!(v >= 0.5) || !(drift_diff(t, n, ncols, col, mean, i - 1) < v)) return false;
    long long j = i;
    while (j + 1 < nd && drift_diff(t, n, ncols, col, mean, j + 1) == v) ++j;
    if (j + 1 >= nd || !(drift_diff(t, n, ncols, col, mean, j + 1) < v)) return false;
    at = (i + j) / 2;
    return true;
}
// ppm of a column from its peaks: sign(mean) 1e6 / ((last - first) / (count - 1)), NaN with fewer than two peaks
MK_HD double drift_ppm(long long count, long long first, long long last, double mean_all) {
    if (count < 2) return NAN;
    const double period = (double)(last - first) / (double)(count - 1);
    const double sign = mean_all > 0.0 ? 1.0 : mean_all < 0.0 ? -1.0 : mean_all;
    return sign * (1.0 / period) * 1e6;
}

}  // namespace ck
}  // namespace ssf
