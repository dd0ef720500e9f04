// metrics_kernels.h -- link metrics (BER, SER, SNR, GMI, NGMI, MI, EVM) of received against transmitted symbols:
// the per-symbol bodies and the combine steps as host/device-neutral inline functions.  engine_metrics.hip wraps them
// in gfx950 kernels (one symbol per lane, wave shuffle -> LDS -> one partial per workgroup, partials summed in a fixed
// order); tests/emu/emu_metrics.cpp loops the same functions over the symbols with g++.
// Reference: optic/comm/metrics.py:111-195 (fastBERcalc), 198-239 (calcLLR), 329-426 (monteCarloGMI), 429-547
// (monteCarloMI, calcMI), 572-637 (calcEVM); optic/comm/modulation.py:271-299, 369-408 (minEuclid, demodulateGray).
// Arithmetic is double whatever the input type; single-precision inputs are widened on load.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MK_HD __host__ __device__ inline
#else
#define MK_HD inline
#endif

namespace ssf {
namespace mk {

enum { kC128 = 0, kC64 = 1, kF64 = 2, kF32 = 3 };                       // ssf_metrics_params.dtype
enum { kWantBer = 1, kWantGmi = 2, kWantMi = 4, kWantEvm = 8, kWantEvmBlind = 16 };
constexpr int kMaxModes = 64, kMaxBits = 10;
constexpr int kStatN = 4, kDecN = 8, kSoftN = 2;                        // values per partial of the three passes
constexpr int kScalN = 12;                                              // doubles per mode of the scalars kept on the device
constexpr int kPwBlock = 128;                                           // leaf length of numpy's pairwise summation
constexpr long long kPwChunk = 8192;                                    // numpy reduces in chunks of its buffer size (np.getbufsize())

struct alignas(16) Cplx {
    double re, im;
};
struct alignas(8) CplxF {
    float re, im;
};

// bytes of one element of the given type
MK_HD size_t elem_size(int dtype) { return dtype == kC128 ? 16 : dtype == kF32 ? 4 : 8; }

// element `off` of an array of the given type (16 B per lane for complex128)
MK_HD void load(int dtype, const void *p, long long off, double &re, double &im) {
    if (dtype == kC128) {
        const Cplx v = ((const Cplx *)p)[off];
        re = v.re, im = v.im;
    } else if (dtype == kC64) {
        const CplxF v = ((const CplxF *)p)[off];
        re = (double)v.re, im = (double)v.im;
    } else if (dtype == kF64) {
        re = ((const double *)p)[off], im = 0.0;
    } else {
        re = (double)((const float *)p)[off], im = 0.0;
    }
}

// numpy's complex division (Smith), tx / rx
MK_HD void cdiv(double ar, double ai, double br, double bi, double &qr, double &qi) {
    if (std::fabs(br) >= std::fabs(bi)) {
        const double rat = bi / br, scl = 1.0 / (br + bi * rat);
        qr = (ar + ai * rat) * scl, qi = (ai - ar * rat) * scl;
    } else {
        const double rat = br / bi, scl = 1.0 / (bi + br * rat);
        qr = (ar * rat + ai) * scl, qi = (ai * rat - ar) * scl;
    }
}

// ---- pass 1: statistics.  acc = [Re sum tx/rx, Im sum tx/rx, sum |rx|^2, sum |tx|^2]
MK_HD void stats_body(double *acc, bool rotate, bool has_tx, double rr, double ri, double tr, double ti) {
    acc[2] += rr * rr + ri * ri;
    if (!has_tx) return;
    acc[3] += tr * tr + ti * ti;
    if (rotate) {
        double qr, qi;
        cdiv(tr, ti, rr, ri, qr, qi);
        acc[0] += qr, acc[1] += qi;
    }
}

// scalars of one mode: [0,1] rot, [2] s_rx, [3] s_tx  (fastBERcalc / monteCarloGMI / monteCarloMI: rotation by mean(tx / rx), then
// each column to unit power);  [4,5] rotation, [6] joint norm of symb, [7] joint norm of symbTx  (calcEVM: pnorm over the whole
// array first, rotation after it and no second normalisation);  [8] sigma^2 (written by the second combine)
// tot: kStatN sums per mode, n symbols per mode
MK_HD void stats_combine(const double *tot, int nModes, long long n, bool rotate, bool has_tx, double *scal) {
    double jrx = 0.0, jtx = 0.0;
    for (int k = 0; k < nModes; ++k) jrx += tot[k * kStatN + 2], jtx += tot[k * kStatN + 3];
    jrx = std::sqrt(jrx / (double)(n * nModes));
    jtx = std::sqrt(jtx / (double)(n * nModes));
    for (int k = 0; k < nModes; ++k) {
        const double *t = tot + k * kStatN;
        double *s = scal + k * kScalN;
        double qr = 1.0, qi = 0.0;
        if (rotate && has_tx) qr = t[0] / (double)n, qi = t[1] / (double)n;
        s[0] = qr, s[1] = qi;
        s[2] = std::sqrt((qr * qr + qi * qi) * (t[2] / (double)n));
        s[3] = std::sqrt(t[3] / (double)n);
        const double g = (rotate && has_tx) ? jrx / jtx : 1.0;
        s[4] = (rotate && has_tx) ? g * qr : 1.0;
        s[5] = (rotate && has_tx) ? g * qi : 0.0;
        s[6] = jrx, s[7] = jtx;
        s[8] = 0.0;
    }
}

// index of the nearest point, first minimum (tab: M interleaved (re, im) pairs)
MK_HD int nearest(const double *tab, int M, double re, double im) {
    int best = 0;
    double dbest = INFINITY;
    for (int m = 0; m < M; ++m) {
        const double dr = re - tab[2 * m], di = im - tab[2 * m + 1];
        const double d = dr * dr + di * di;
        if (d < dbest) dbest = d, best = m;
    }
    return best;
}

MK_HD int popcount32(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// rx, tx as stored -> the reference's rotated and normalised columns
MK_HD void normalise(const double *s, double rr, double ri, double tr, double ti, double &xr, double &xi, double &yr, double &yi) {
    xr = (s[0] * rr - s[1] * ri) / s[2], xi = (s[0] * ri + s[1] * rr) / s[2];
    yr = tr / s[3], yi = ti / s[3];
}

// ---- pass 2: decisions.  acc = [Re sum d, Im sum d, sum |d|^2, sum |tx_n|^2, bit errors, symbol errors, EVM numerator, EVM
// denominator] with d = rx_n - tx_n; the error counts are integers held in doubles (exact below 2^53)
MK_HD void decide_body(double *acc, const double *s, const double *raw, int M, double sqrtEs, int want, double rr, double ri,
                       double tr, double ti) {
    double xr, xi, yr, yi;
    normalise(s, rr, ri, tr, ti, xr, xi, yr, yi);
    const double dr = xr - yr, di = xi - yi;
    acc[0] += dr, acc[1] += di, acc[2] += dr * dr + di * di, acc[3] += yr * yr + yi * yi;
    if (want & kWantBer) {
        const int irx = nearest(raw, M, sqrtEs * xr, sqrtEs * xi), itx = nearest(raw, M, sqrtEs * yr, sqrtEs * yi);
        acc[4] += (double)popcount32((unsigned)(irx ^ itx));            // bitMap is the binary expansion of the point index
        acc[5] += irx != itx ? 1.0 : 0.0;
    }
    if (want & kWantEvm) {
        const double ur = rr / s[6], ui = ri / s[6], vr = tr / s[7], vi = ti / s[7];
        const double er = s[4] * ur - s[5] * ui - vr, ei = s[4] * ui + s[5] * ur - vi;
        acc[6] += er * er + ei * ei, acc[7] += vr * vr + vi * vi;
    }
}

// per-mode results after pass 2; res = [BER, SER, SNR, GMI, NGMI, MI, EVM, bit errors, symbol errors, n]
constexpr int kResN = 10;
MK_HD void decide_combine(const double *tot, long long n, int bits, double *s, double *res) {
    const double dn = (double)n;
    const double mr = tot[0] / dn, mi = tot[1] / dn;
    s[8] = tot[2] / dn - (mr * mr + mi * mi);                            // np.var of the complex residual
    res[0] = tot[4] / (dn * (double)bits);
    res[1] = tot[5] / dn;
    res[2] = 10.0 * std::log10((tot[3] / dn) / (tot[2] / dn));
    res[6] = (tot[6] / dn) / (tot[7] / dn);
    res[7] = tot[4], res[8] = tot[5], res[9] = dn;
}

// ---- pass 3: soft demapping.  The reference's direct form: M likelihoods exp(-|r - c|^2 / sigma^2) px, per bit position the
// sums over the points whose label has a 0 / a 1 there, LLR = log(sum0) - log(sum1) with +-inf clipped to +-500 (the sums
// underflow at high SNR; a max-shifted log-sum-exp would give another GMI there).  Rounding-level differences only: the
// exponent is |r - c|^2 times -1 / sigma^2 (one ulp from the quotient: 1e-13 relative in a term at the underflow edge) and the
// terms are added group-wise.
// cn: normalised table, M interleaved pairs; acc = [sum over bits of log2(1 + exp(+-LLR)), sum of the MI term]
template <int B>
MK_HD void soft_body(double *acc, const double *s, const double *raw, const double *cn, const double *px, const double *log2px, int M,
                     double sqrtEs, double rr, double ri, double tr, double ti) {
    double xr, xi, yr, yi;
    normalise(s, rr, ri, tr, ti, xr, xi, yr, yi);
    const double sigma2 = s[8];
    const int itx = nearest(raw, M, sqrtEs * yr, sqrtEs * yi);
    const double ninv = -1.0 / sigma2;                                   // (-|r - c|^2) / sigma^2 as one multiplication per term
    // The M terms go in groups of G = min(M, 16) consecutive points: inside a group the low log2(G) label bits are known at
    // compile time (no selects), the high bits are those of the group and take the group's sum.
    constexpr int LB = B < 4 ? B : 4, G = 1 << LB;
    double p0[B], p1[B], pY = 0.0;
#pragma unroll
    for (int j = 0; j < B; ++j) p0[j] = 0.0, p1[j] = 0.0;
    for (int m0 = 0; m0 < M; m0 += G) {
        double p[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double dr = xr - cn[2 * (m0 + g)], di = xi - cn[2 * (m0 + g) + 1];
            p[g] = std::exp((dr * dr + di * di) * ninv) * px[m0 + g];
        }
        double tot = 0.0;
#pragma unroll
        for (int l = 0; l < LB; ++l) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if ((g >> l) & 1)
                    s1 += p[g];
                else
                    s0 += p[g];
            }
            p0[B - 1 - l] += s0, p1[B - 1 - l] += s1;
            tot = s0 + s1;
        }
        pY += tot;
#pragma unroll
        for (int j = 0; j < B - LB; ++j) {
            if ((m0 >> (B - 1 - j)) & 1)
                p1[j] += tot;
            else
                p0[j] += tot;
        }
    }
    double g = 0.0;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        double llr = std::log(p0[j]) - std::log(p1[j]);
        if (llr == INFINITY) llr = 500.0;
        if (llr == -INFINITY) llr = -500.0;
        const double sg = ((itx >> (B - 1 - j)) & 1) ? 1.0 : -1.0;
        g += std::log2(1.0 + std::exp(sg * llr));
    }
    acc[0] += g;
    const double dr = xr - yr, di = xi - yi;
    const double log2_pYgX = -(1.0 / sigma2) * (dr * dr + di * di) * 1.4426950408889634;
    acc[1] += log2_pYgX + log2px[itx] - std::log2(pY);
}

template <int B = 1> struct SoftDispatch {
    MK_HD static void run(int bits, double *acc, const double *s, const double *raw, const double *cn, const double *px,
                          const double *log2px, int M, double sqrtEs, double rr, double ri, double tr, double ti) {
        if (bits == B)
            soft_body<B>(acc, s, raw, cn, px, log2px, M, sqrtEs, rr, ri, tr, ti);
        else
            SoftDispatch<B + 1>::run(bits, acc, s, raw, cn, px, log2px, M, sqrtEs, rr, ri, tr, ti);
    }
};
template <> struct SoftDispatch<kMaxBits + 1> {
    MK_HD static void run(int, double *, const double *, const double *, const double *, const double *, const double *, int, double,
                          double, double, double, double) {}
};

MK_HD void soft_combine(const double *tot, long long n, double H, double *res) {
    res[3] = H - tot[0] / (double)n;
    res[4] = res[3] / H;
    res[5] = H + tot[1] / (double)n;                                     // H(X) - H(X|Y), H(X|Y) = -mean(term)
}

// ---- blind EVM (no transmitted symbols): decisions against pnorm(table), which the reference keeps in single precision; the
// denominator mean(|decided|^2) is a float32 np.mean, i.e. numpy's pairwise summation in float32, reproduced operation for
// operation below (w32[m] = float32 |c_m|^2, idx = decided point per symbol).
// acc = [sum |symb_n - c|^2]; returns the decided index
MK_HD int blind_body(double *acc, double jrx, const double *tab, int M, double rr, double ri) {
    const double ur = rr / jrx, ui = ri / jrx;
    const int i = nearest(tab, M, ur, ui);
    const double er = ur - tab[2 * i], ei = ui - tab[2 * i + 1];
    acc[0] += er * er + ei * ei;
    return i;
}

// The order: the sequence is cut into chunks of 8192 elements (numpy's reduction buffer; found by experiment, numpy 2.2: np.sum of
// float32 equals this order in 140 of 140 random trials at lengths 8193 .. 40000, one undivided recursion in 84); the chunk sums
// are added one after the other onto 0; within a chunk numpy's pairwise_sum: at most 128 elements are a leaf (eight interleaved
// running sums, then the rest one by one), more are split in two and the halves added.
// numpy's pairwise_sum splits n > 128 into n2 = (n / 2) rounded down to a multiple of 8 and the rest
MK_HD long long pw_split(long long n) {
    long long n2 = n / 2;
    return n2 - n2 % 8;
}

// number of leaves of one chunk of n elements; starts (may be NULL) receives their first elements
inline long long pw_chunk_leaves(long long n, long long first, long long *starts, long long count = 0) {
    if (n <= kPwBlock) {
        if (starts) starts[count] = first;
        return count + 1;
    }
    const long long n2 = pw_split(n);
    count = pw_chunk_leaves(n2, first, starts, count);
    return pw_chunk_leaves(n - n2, first + n2, starts, count);
}
// ... of a whole sequence (starts needs one more entry than leaves: the caller sets the last to n)
inline long long pw_leaves(long long n, long long *starts) {
    long long count = 0;
    for (long long first = 0; first < n; first += kPwChunk) count = pw_chunk_leaves(n - first < kPwChunk ? n - first : kPwChunk, first, starts, count);
    return count;
}

MK_HD float pw_leaf(const float *w, const int32_t *idx, long long n) {
    if (n < 8) {
        float r = 0.f;
        for (long long i = 0; i < n; ++i) r += w[idx[i]];
        return r;
    }
    float r0 = w[idx[0]], r1 = w[idx[1]], r2 = w[idx[2]], r3 = w[idx[3]], r4 = w[idx[4]], r5 = w[idx[5]], r6 = w[idx[6]], r7 = w[idx[7]];
    long long i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += w[idx[i]], r1 += w[idx[i + 1]], r2 += w[idx[i + 2]], r3 += w[idx[i + 3]];
        r4 += w[idx[i + 4]], r5 += w[idx[i + 5]], r6 += w[idx[i + 6]], r7 += w[idx[i + 7]];
    }
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += w[idx[i]];
    return res;
}

// the leaf sums combined in the order of the recursion (explicit stack: depth <= 64; the kernel keeps it in LDS)
struct PwFrame {
    long long n;
    float left;
    int state;
};
MK_HD float pw_chunk_combine(const float *leaf, long long &next, long long n, PwFrame *stk) {
    int sp = 0;
    float ret = 0.f;
    stk[0].n = n, stk[0].state = 0;
    while (sp >= 0) {
        PwFrame &f = stk[sp];
        if (f.state == 0) {
            if (f.n <= kPwBlock) {
                ret = leaf[next++];
                --sp;
            } else {
                f.state = 1;
                stk[sp + 1].n = pw_split(f.n), stk[sp + 1].state = 0;
                ++sp;
            }
        } else if (f.state == 1) {
            f.left = ret, f.state = 2;
            stk[sp + 1].n = f.n - pw_split(f.n), stk[sp + 1].state = 0;
            ++sp;
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}
MK_HD float pw_combine(const float *leaf, long long n, PwFrame *stk) {
    long long next = 0;
    float total = 0.f;
    for (long long first = 0; first < n; first += kPwChunk) total += pw_chunk_combine(leaf, next, n - first < kPwChunk ? n - first : kPwChunk, stk);
    return total;
}

}  // namespace mk
}  // namespace ssf
