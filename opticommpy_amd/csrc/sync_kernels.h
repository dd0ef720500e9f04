// sync_kernels.h -- sequence synchronisation (symbolSync in both modes, finddelay): the per-element bodies and the decisions as
// host/device-neutral inline functions.  engine_sync.hip wraps them in gfx950 kernels around rocFFT's transforms;
// tests/emu/emu_sync.cpp loops the same functions with g++ around a radix-2 transform of its own.
// Reference: optic/dsp/core.py:552-675 (symbolSync), 678-698 (finddelay); scipy.signal.correlate, mode "full".
//
// Every correlation is one circular correlation of length L >= n_tx + n_rx - 1.  The transmitted sequence sits n_rx - 1 places
// into its zero-padded buffer, so element j of ifft(A conj(B)) IS element j of scipy's full correlation: no wrap, no index map.
// Real sequences ride in pairs: ifft(A conj(B) + j A conj(B')) carries correlate(a, b) in its real and correlate(a, b') in its
// imaginary part ('amp'); with a complex a and a real b the two parts are correlate(Re a, b) and correlate(Im a, b) ('real').
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace sk {

using mk::Cplx;
using mk::CplxF;
using mk::load;

constexpr int kMaxModes = 8;
constexpr int kBlock = 256;        // lanes of every kernel of the engine
constexpr int kMaxBlocks = 1024;   // workgroups of one grid round of the reductions and of the gather
enum { kAmp = 0, kReal = 1, kDelay = 2 };           // what the call computes (ssf_sync_params.mode; kDelay: ssf_finddelay)
enum { kRotP1 = 0, kRotM1 = 1, kRotPJ = 2, kRotMJ = 3 };   // 1, -1, 1j, -1j

// the record of one call as the decisions leave it in device memory; the gather reads it there, the host copies it once
struct Record {
    long long delay[kMaxModes];
    int swap[kMaxModes], rot[kMaxModes], conj[kMaxModes];
    int rotmat[kMaxModes * kMaxModes];               // 'real': rot[m, n] of every pair
    double corr[kMaxModes * kMaxModes];              // corrMatrix[m, n], row-major (nModes, nModes)
    long long peak_index[kMaxModes];                 // the lag index the delay was taken from (lags: nothing finite was found)
};

// one peak: max |c| over the lags, its lowest index and the signed value there
struct Peak {
    double mag;
    long long idx;
    double val;
};
MK_HD Peak peak_none(long long lags) { return Peak{-1.0, lags, 0.0}; }
// the larger magnitude, the lower index among equal ones (np.argmax): the result does not depend on the order of the merges
MK_HD void peak_merge(Peak &p, const Peak &q) {
    if (q.mag > p.mag || (q.mag == p.mag && q.idx < p.idx)) p = q;
}

// ---- preparation
// np.abs of one element.  A complex64 sequence stays single precision in the reference (np.abs, np.mean and the subtraction are
// float32 operations there): the same operations here, widened afterwards.  numpy's vectorised |z| of a complex64 is not the
// correctly rounded hypotf but max sqrt(fma(r, r, 1)) with r = min / max, each step rounded to single (found by experiment,
// numpy 2.2 on x86-64 with FMA: equal at 200 000 of 200 000 random values; a third of them differ from hypotf by an ulp, which
// moves corrMatrix by several 1e-9).  Division and square root are IEEE-rounded on the device too (hipcc's default for HIP).
MK_HD float amp_f32(float re, float im) {
    const float a = std::fabs(re), b = std::fabs(im);
    const float mx = a > b ? a : b, mn = a > b ? b : a;
    if (mx == 0.f) return 0.f;
    const float r = mn / mx;
    return mx * std::sqrt(std::fma(r, r, 1.f));
}
MK_HD double amp_value(double re, double im, bool f32) {
    if (f32) return (double)amp_f32((float)re, (float)im);
    return std::hypot(re, im);
}
MK_HD double center_value(double v, double mean, bool f32) {
    if (f32) return (double)((float)v - (float)mean);
    return v - mean;
}
// np.mean of float32: float32(float64(sum) / n), the sum being numpy's pairwise sum in float32 (metrics_kernels.h: pw_combine)
MK_HD double mean_f32(float sum, long long n) { return (double)(float)((double)sum / (double)n); }

// one leaf (at most 128 elements) of numpy's pairwise sum over the real parts of a transform buffer, which hold float32 values
MK_HD float pw_leaf_re(const Cplx *a, long long n) {
    if (n < 8) {
        float r = 0.f;
        for (long long i = 0; i < n; ++i) r += (float)a[i].re;
        return r;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = (float)a[j].re;
    long long i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += (float)a[i + j].re;
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += (float)a[i].re;
    return res;
}

// ---- layout of the transform buffers
// sequences: tx_m -> m;  rx_n (|rx_n| or Re rx_n or y) -> nModes + n;  'real': Im rx_n -> 2 nModes + n
MK_HD int n_sequences(int mode, int nModes) { return mode == kAmp ? 2 * nModes : mode == kReal ? 3 * nModes : 2; }
// correlations of the first round: 'amp' packs two received modes per transform
MK_HD int pairs_per_row(int mode, int nModes) { return mode == kAmp ? (nModes + 1) / 2 : nModes; }
MK_HD int n_slots(int mode, int nModes) { return mode == kDelay ? 1 : nModes * pairs_per_row(mode, nModes); }
// the peak of the pair (m, n): its slot and channel (0: real part, 1: imaginary part) -> index into the peak array
MK_HD int pair_peak(int mode, int nModes, int m, int n) {
    if (mode == kAmp) return 2 * (m * pairs_per_row(mode, nModes) + n / 2) + (n & 1);
    return 2 * (m * nModes + n);
}

// the sequences a slot multiplies: A conj(B) + j A conj(B2) (b2 < 0: none).  swap: the record's, for the second round
MK_HD void slot_sequences(int mode, int round, int nModes, int slot, const int *swap, int &a, int &b, int &b2) {
    b2 = -1;
    if (mode == kDelay) {
        a = 0, b = 1;
    } else if (round == 2) {                         // 'real': tx[:, swap[k]] against Im rx_k
        a = swap[slot], b = 2 * nModes + slot;
    } else if (mode == kAmp) {
        const int nq = pairs_per_row(mode, nModes), m = slot / nq, q = slot - m * nq;
        a = m, b = nModes + 2 * q;
        if (2 * q + 1 < nModes) b2 = b + 1;
    } else {
        const int m = slot / nModes;
        a = m, b = nModes + (slot - m * nModes);
    }
}

MK_HD Cplx spectral_product(Cplx A, Cplx B, double scale) {
    Cplx r;
    r.re = (A.re * B.re + A.im * B.im) * scale;
    r.im = (A.im * B.re - A.re * B.im) * scale;
    return r;
}
MK_HD Cplx spectral_pair(Cplx A, Cplx B, Cplx B2, double scale) {                // P + j P2
    const Cplx p = spectral_product(A, B, scale), q = spectral_product(A, B2, scale);
    Cplx r;
    r.re = p.re - q.im, r.im = p.im + q.re;
    return r;
}

// ---- peak search: the two channels of lag j of one correlation.  kDelay: |c|^2 of the complex correlation in channel 0
MK_HD void peak_channels(int mode, Cplx c, long long j, Peak &p0, Peak &p1) {
    if (mode == kDelay) {
        const double m = c.re * c.re + c.im * c.im;
        peak_merge(p0, Peak{m, j, m});
    } else {
        peak_merge(p0, Peak{std::fabs(c.re), j, c.re});
        peak_merge(p1, Peak{std::fabs(c.im), j, c.im});
    }
}

// ---- decisions (one thread)
// corrMatrix column argmax: the first maximum (np.argmax)
MK_HD void decide_swap(int nModes, Record &r) {
    for (int n = 0; n < nModes; ++n) {
        int best = 0;
        for (int m = 1; m < nModes; ++m)
            if (r.corr[m * nModes + n] > r.corr[best * nModes + n]) best = m;
        r.swap[n] = best;
    }
}
// 'amp' (core.py:603-622): the delays are the peaks of the correlations of the pairs (swap[k], k), already there
MK_HD void decide_amp(int nModes, long long n_tx, const Peak *pk, Record &r) {
    for (int m = 0; m < nModes; ++m)
        for (int n = 0; n < nModes; ++n) r.corr[m * nModes + n] = pk[pair_peak(kAmp, nModes, m, n)].mag;
    decide_swap(nModes, r);
    for (int k = 0; k < nModes; ++k) {
        const Peak &p = pk[pair_peak(kAmp, nModes, r.swap[k], k)];
        r.peak_index[k] = p.idx;
        r.delay[k] = p.idx - (n_tx - 1);
        r.rot[k] = kRotP1, r.conj[k] = 0;
    }
}
// 'real', first round (core.py:625-651): channel 0 is crr, channel 1 cir
MK_HD void decide_real_rot(int nModes, const Peak *pk, Record &r) {
    for (int m = 0; m < nModes; ++m)
        for (int n = 0; n < nModes; ++n) {
            const Peak &cr = pk[pair_peak(kReal, nModes, m, n)], &ci = pk[pair_peak(kReal, nModes, m, n) + 1];
            r.corr[m * nModes + n] = cr.mag > ci.mag ? cr.mag : ci.mag;
            int rot;
            if (cr.mag > ci.mag) rot = cr.val > 0 ? kRotP1 : kRotM1;
            else rot = ci.val > 0 ? kRotMJ : kRotPJ;
            r.rotmat[m * nModes + n] = rot;
        }
    decide_swap(nModes, r);
}
// 'real', second round (core.py:653-665).  Column k is tx[:, swap[k]] times rot[k, swap[k]] -- the reference's indexing, not
// rot[swap[k], k].  Its real part is +-Re or +-Im of tx[:, swap[k]], so finddelay's correlation is +-crr or +-cir of the pair
// (swap[k], k); its imaginary part against Im rx_k is a part of the second round's correlation pk2[2 k], pk2[2 k + 1].
MK_HD void decide_real_delay(int nModes, long long n_tx, const Peak *pk, const Peak *pk2, Record &r) {
    for (int k = 0; k < nModes; ++k) {
        const int s = r.swap[k], rot = r.rotmat[k * nModes + s];
        const bool quarter = rot == kRotPJ || rot == kRotMJ;
        const Peak &p = pk[pair_peak(kReal, nModes, s, k) + (quarter ? 1 : 0)];
        r.peak_index[k] = p.idx;
        r.delay[k] = p.idx - (n_tx - 1);
        const Peak &q = pk2[2 * k + (quarter ? 0 : 1)];
        const double cii = (rot == kRotP1 || rot == kRotPJ) ? q.val : -q.val;
        r.rot[k] = rot, r.conj[k] = cii < 0 ? 1 : 0;
    }
}

// ---- gather: out[i, k] = f(tx[(i + delay[k]) mod n_tx, swap[k]]) (np.roll by -delay)
MK_HD long long roll_source(long long i, long long delay, long long n) {
    long long d = delay % n;
    if (d < 0) d += n;
    const long long s = i + d;
    return s >= n ? s - n : s;
}
template <class T> MK_HD void rotate_conj(T &re, T &im, int rot, int conj) {
    const T a = re, b = im;
    if (rot == kRotM1) re = -a, im = -b;
    else if (rot == kRotPJ) re = -b, im = a;
    else if (rot == kRotMJ) re = b, im = -a;
    if (conj) im = -im;
}

}  // namespace sk
}  // namespace ssf
