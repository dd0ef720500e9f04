// Device bodies of the IM/DD transmitter and the AWGN channel.  Same convention as rx_kernels.h: every body is a template over a
// Ctx (HIP: RxCtx of engine_rx.hip, tests: a host walk, tests/emu/emu_imddtx.cpp), so the code the GPU runs is the code the CPU
// tests execute.
//
// Reference (file:line under the reference checkout):
//   pamTransmitter       optic/models/tx.py:231-352      pam_peak_body, pam_mzm_body, pam_finish_body (after the stuffed filter)
//   pm, mzm, iqm         optic/models/devices.py:56-220  modulate_body   (calcMZM / calcPM: optic/dsp/core.py:1076-1139)
//   awgn                 optic/models/channels.py:522-565  power_body, awgn_body
//   upsample, voa        optic/dsp/core.py:395-432, optic/models/devices.py:263-286  stuff_body
// Sums and maxima over a launch are per-workgroup partials in a fixed order (fused::block_sum2 / block_max); the launch that needs
// the value adds the partials itself, every workgroup in the same order (fused::global_sum / global_max): no host wait in between,
// and a result repeats bit for bit.
#pragma once
#include <cmath>

#include "rx_kernels.h"

namespace ssf {
namespace rx {

constexpr int kTxBlocks = 1024;            // most workgroups of a reduction pass (and partials the next pass adds up)
constexpr int kTxBlock = 256;              // lanes per workgroup of every kernel here
constexpr unsigned kAwgnTag = 0x4157u;     // span tag of awgn's Philox streams (edfa: 0 and the span numbers, photodiodes 0x5044, laser walk 0x504E)
constexpr double kTxPi = 3.14159265358979323846;

// workgroups of a pass over n elements: one per kTxBlock elements, at most kTxBlocks (the host and the tests use the same rule)
inline int tx_blocks(long long n) {
    const long long g = (n + kTxBlock - 1) / kTxBlock;
    return (int)(g < 1 ? 1 : g > kTxBlocks ? kTxBlocks : g);
}

// ... and of an element-wise pass: at most kTxEwBlocks, grid-stride beyond kTxEwBlocks * kTxBlock elements
constexpr int kTxEwBlocks = 4096;
inline int tx_ew_blocks(long long n) {
    const long long g = (n + kTxBlock - 1) / kTxBlock;
    return (int)(g < 1 ? 1 : g > kTxEwBlocks ? kTxEwBlocks : g);
}
// calcMZM's sqrt(1 + gamma), sqrt(1 - gamma) from the extinction ratio in dB, in double precision on the host (core.py:1105-1106)
inline void mzm_arms(double ER, double *sp, double *sm) {
    const double erLin = std::pow(10.0, ER / 10), gamma = 2 * std::sqrt(erLin) / (erLin + 1);
    *sp = std::sqrt(1 + gamma);
    *sm = std::sqrt(1 - gamma);
}

// calcPM's factor exp(1j * (z / Vpi) * pi) for z = zr + j zi, rounded as numpy rounds it: (z / Vpi) * pi per part; a real drive
// (CX = false) has modulus one
template <bool CX> SSF_HD Cd pm_factor(double zr, double zi, double Vpi) {
    double c, s;
    fused::sincos_d((zr / Vpi) * kTxPi, s, c);
    if (CX) {
        const double m = exp(-(zi / Vpi) * kTxPi);
        return mk<double>(m * c, m * s);
    }
    return mk<double>(c, s);
}
// calcMZM (core.py:1105-1110): sqrt(1 + g) (E / 2) pm((u + Vb) / 2) + sqrt(1 - g) (E / 2) pm(-(u + Vb) / 2), sp = sqrt(1 + g), sm = sqrt(1 - g)
template <bool CX> SSF_HD Cd mzm_field(Cd e, double ur, double ui, double Vb, double Vpi, double sp, double sm) {
    const double vr = (ur + Vb) / 2, vi = ui / 2;
    const Cd h = mk<double>(e.re / 2, e.im / 2);
    const Cd fu = pm_factor<CX>(vr, vi, Vpi);
    const Cd fl = CX ? pm_factor<CX>(-vr, -vi, Vpi) : mk<double>(fu.re, -fu.im);
    const Cd a = h * fu, b = h * fl;
    return mk<double>(sp * a.re + sm * b.re, sp * a.im + sm * b.im);
}

// ---- pamTransmitter, one polarisation mode: sig is the pulse-shaped symbol stream (real: the transform's imaginary residue is
// dropped, the reference's signal has none)
struct PamPeakArgs {
    const Cd *sig;
    double *part;        // one maximum of |sig| per workgroup
    long long N;
};
template <class Ctx> SSF_HD void pam_peak_body(Ctx &ctx, const PamPeakArgs &a) {
    double m = 0;                                                // (a workgroup without samples leaves the neutral 0)
    for (long long n = (long long)ctx.bid * ctx.nthreads + ctx.tid; n < a.N; n += (long long)ctx.nblocks * ctx.nthreads) {
        const double v = fabs(a.sig[n].re);
        m = v > m ? v : m;
    }
    m = fused::block_max(ctx, m, (double *)ctx.lds);
    if (ctx.tid == 0) a.part[ctx.bid] = m;
}
// E = mzm(1, mzmScale * (Vpi * sig / max|sig|), Vpi, Vb, ER) into column `col` of out (N, ld), and the partial sums of |E|^2
struct PamMzmArgs {
    const Cd *sig;
    Cd *out;
    const double *pmax;  // nb partial maxima
    double *ppow;        // one partial sum per workgroup
    long long N;
    int nb, ld, col;
    double mzmScale, Vpi, Vb, sp, sm;
};
template <class Ctx> SSF_HD void pam_mzm_body(Ctx &ctx, const PamMzmArgs &a) {
    const double mx = fused::global_max(ctx, a.pmax, a.nb, (double *)ctx.lds);
    double acc = 0, unused = 0;
    for (long long n = (long long)ctx.bid * ctx.nthreads + ctx.tid; n < a.N; n += (long long)ctx.nblocks * ctx.nthreads) {
        const double u = a.mzmScale * (a.Vpi * a.sig[n].re / mx);                       // tx.py:335, 338
        const Cd e = mzm_field<false>(mk<double>(1.0, 0.0), u, 0.0, a.Vb, a.Vpi, a.sp, a.sm);
        a.out[n * a.ld + a.col] = e;
        acc += e.re * e.re + e.im * e.im;
    }
    fused::block_sum2(ctx, acc, unused, (double *)ctx.lds);
    if (ctx.tid == 0) a.ppow[ctx.bid] = acc;
}
// out[:, col] = amp * (E / sqrt(mean |E|^2)), amp = sqrt(dBm2W(power))                  (tx.py:341 with pnorm, core.py:717)
struct PamFinishArgs {
    Cd *out;
    const double *ppow;
    long long N;
    int nb, ld, col;
    double amp;
};
template <class Ctx> SSF_HD void pam_finish_body(Ctx &ctx, const PamFinishArgs &a) {
    const double rms = sqrt(fused::global_sum(ctx, a.ppow, a.nb, (double *)ctx.lds) / (double)a.N);
    for (long long n = (long long)ctx.bid * ctx.nthreads + ctx.tid; n < a.N; n += (long long)ctx.nblocks * ctx.nthreads) {
        Cd &d = a.out[n * a.ld + a.col];
        d = mk<double>(a.amp * (d.re / rms), a.amp * (d.im / rms));
    }
}

// ---- pm / mzm / iqm, element-wise
enum { MOD_PM = 0, MOD_MZM = 1, MOD_IQM = 2 };
struct ModArgs {
    const double *u;     // n float64, or n complex128 interleaved (u_cx)
    const Cd *Ei;        // n values, or null: the scalar ei0
    Cd *out;
    long long n;
    int kind, u_cx;
    Cd ei0;
    double Vpi, VbI, VbQ, spI, smI, spQ, smQ;       // mzm: the I set; pm: Vpi only
    Cd rotQ;             // iqm: exp(1j * (Vphi / Vpi) * pi)
};
inline ModArgs mod_args(int kind, long long n, int u_cx, const double *u, const Cd *Ei, double ei_re, double ei_im, double Vpi, double VbI,
                        double VbQ, double Vphi, double ERI, double ERQ, Cd *out) {
    ModArgs a{};
    a.u = u;
    a.Ei = Ei;
    a.out = out;
    a.n = n;
    a.kind = kind;
    a.u_cx = u_cx;
    a.ei0 = mk<double>(ei_re, ei_im);
    a.Vpi = Vpi;
    a.VbI = VbI;
    a.VbQ = VbQ;
    mzm_arms(ERI, &a.spI, &a.smI);
    mzm_arms(ERQ, &a.spQ, &a.smQ);
    const double ang = (Vphi / Vpi) * kTxPi;               // calcPM on Vphi * ones: one value
    a.rotQ = mk<double>(std::cos(ang), std::sin(ang));
    return a;
}
template <int KIND, bool CX, class Ctx> SSF_HD void modulate_loop(Ctx &ctx, const ModArgs &a) {
    for (long long n = (long long)ctx.bid * ctx.nthreads + ctx.tid; n < a.n; n += (long long)ctx.nblocks * ctx.nthreads) {
        const double ur = CX ? a.u[2 * n] : a.u[n], ui = CX ? a.u[2 * n + 1] : 0.0;
        const Cd e = a.Ei ? a.Ei[n] : a.ei0;
        if (KIND == MOD_PM) {
            a.out[n] = e * pm_factor<CX>(ur, ui, a.Vpi);
        } else if (KIND == MOD_MZM) {
            a.out[n] = mzm_field<CX>(e, ur, ui, a.VbI, a.Vpi, a.spI, a.smI);
        } else {                                                                        // devices.py:214-218
            const Cd h = mk<double>(e.re / 1.4142135623730951, e.im / 1.4142135623730951);
            const Cd eI = mzm_field<false>(h, ur, 0.0, a.VbI, a.Vpi, a.spI, a.smI);
            const Cd eQ = mzm_field<false>(h, ui, 0.0, a.VbQ, a.Vpi, a.spQ, a.smQ);
            a.out[n] = eI + eQ * a.rotQ;
        }
    }
}
template <class Ctx> SSF_HD void modulate_body(Ctx &ctx, const ModArgs &a) {
    if (a.kind == MOD_IQM) {
        if (a.u_cx) modulate_loop<MOD_IQM, true>(ctx, a);
        else modulate_loop<MOD_IQM, false>(ctx, a);
    } else if (a.kind == MOD_MZM) {
        if (a.u_cx) modulate_loop<MOD_MZM, true>(ctx, a);
        else modulate_loop<MOD_MZM, false>(ctx, a);
    } else {
        if (a.u_cx) modulate_loop<MOD_PM, true>(ctx, a);
        else modulate_loop<MOD_PM, false>(ctx, a);
    }
}

// ---- awgn: sum |x|^2 over every element of every column (sigPow, core.py:50-66), as a sum over the float64 values
struct PowerArgs {
    const double *x;
    double *part;
    long long cnt;       // float64 values: elements, or twice that for complex input
};
template <class Ctx> SSF_HD void power_body(Ctx &ctx, const PowerArgs &a) {
    double acc = 0, unused = 0;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < a.cnt; i += (long long)ctx.nblocks * ctx.nthreads) acc += a.x[i] * a.x[i];
    fused::block_sum2(ctx, acc, unused, (double *)ctx.lds);
    if (ctx.tid == 0) a.part[ctx.bid] = acc;
}
// out = x + s (zr + j zi), s = sqrt(((Fs / B) * (mean |x|^2 / snr_lin)) / 2)            (channels.py:556-565, core.py:761, 788)
// un: the caller's unit normals -- `total` for the real parts, then `total` for the imaginary parts when the noise is complex --
// or null: Philox, counter = sample, row = column, span tag kAwgnTag
struct AwgnArgs {
    const double *x;
    double *out;
    const double *un;
    const double *part;
    long long total;     // elements (samples * columns)
    int nb, ncols, in_cx, out_cx, cnoise;
    double FsB, snr_lin;
    unsigned long long seed;
};
template <class Ctx> SSF_HD void awgn_body(Ctx &ctx, const AwgnArgs &a) {
    const double pw = fused::global_sum(ctx, a.part, a.nb, (double *)ctx.lds) / (double)a.total;
    const double s = sqrt((a.FsB * (pw / a.snr_lin)) / 2);
    for (long long e = (long long)ctx.bid * ctx.nthreads + ctx.tid; e < a.total; e += (long long)ctx.nblocks * ctx.nthreads) {
        const double xr = a.in_cx ? a.x[2 * e] : a.x[e], xi = a.in_cx ? a.x[2 * e + 1] : 0.0;
        double nr, ni;
        if (a.un) {
            nr = s * a.un[e];
            ni = a.cnoise ? s * a.un[a.total + e] : 0.0;
        } else {
            const long long smp = a.ncols == 1 ? e : e / a.ncols;
            gauss_pair((unsigned long long)smp, (unsigned)(e - smp * a.ncols), kAwgnTag, a.seed, s, nr, ni);
            if (!a.cnoise) ni = 0.0;
        }
        if (a.out_cx) {
            a.out[2 * e] = xr + nr;
            a.out[2 * e + 1] = xi + ni;
        } else {
            a.out[e] = xr + nr;
        }
    }
}

// ---- upsample / voa on 8-byte words (a complex128 column is two of them): out (rows * factor, w) gets scale * in (rows, w) in the
// rows that are multiples of `factor` and zeros elsewhere.  scale == 1 copies the bits (complex64 pairs travel as one word).
struct StuffArgs {
    const double *in;
    double *out;
    long long total;     // words of out = rows * factor * w
    int factor, w;
    double scale;
};
template <class Ctx> SSF_HD void stuff_body(Ctx &ctx, const StuffArgs &a) {
    const unsigned long long *bits = (const unsigned long long *)a.in;
    unsigned long long *obits = (unsigned long long *)a.out;
    for (long long o = (long long)ctx.bid * ctx.nthreads + ctx.tid; o < a.total; o += (long long)ctx.nblocks * ctx.nthreads) {
        const long long r = o / a.w, c = o - r * a.w;
        if (a.factor > 1 && r % a.factor != 0) {
            obits[o] = 0ull;
            continue;
        }
        const long long i = (r / a.factor) * a.w + c;
        if (a.scale == 1.0) obits[o] = bits[i];
        else a.out[o] = a.in[i] * a.scale;
    }
}

}  // namespace rx
}  // namespace ssf
