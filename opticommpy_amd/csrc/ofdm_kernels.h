// ofdm_kernels.h -- the per-lane bodies of the OFDM engine (engine_ofdm.hip), written against an execution context `Ctx` (tid / bid /
// nthreads / lds / sync()) like the bodies of fused_kernels.h: hipcc launches them on gfx950, tests/emu/emu_ofdm.cpp walks them
// with g++.  Reference semantics: optic/comm/ofdm.py (modulateOFDM, demodulateOFDM).
//
// A frame is one transform.  Where its length is a power of two, 16 .. 8192, a group of L / 16 lanes keeps it in registers (sixteen
// values per lane) and exchanges through LDS with fft_dit / fft_dif of fused_kernels.h, as the overlap-save filter does; a
// workgroup of 256 lanes (512 at 8192 points) takes as many frames as that gives groups.
//   modulator     the transform's input k is read THROUGH the carrier map (a code per input: zero, data symbol d, the pilot, or the
//                 conjugate of either), so the zero padding, the fftshift and the Hermitian mirror never exist in memory; the
//                 inverse transform runs DIT (digit-reversed in, natural out): lane b ends up with samples b, b + L/16, ..., which it
//                 stores scaled by sqrt(L) / L behind the prefix and, the last SpS G of them, a second time as the prefix.
//   demodulator   the frame is loaded behind its prefix; the forward transform runs DIF (natural in, digit-reversed out), and the
//                 stores go through a table that sends bin k to its carrier after fftshift and the Hermitian slice, or nowhere.
// The maps come in REGISTER order (value idx of lane b: entry idx * L/16 + b), so a wave reads consecutive entries.
// Every other length takes the same loads and stores as element-wise kernels around a rocFFT batch (natural-order maps).
// All arithmetic is double: complex64 input is widened on load, complex64 output rounded once on store.
#pragma once
#include <vector>

#include "fused_kernels.h"

namespace ssf {
namespace ofdm {

using fused::cx;
using fused::mk;

constexpr int kBlock = 256;                   // lanes per workgroup (the 8192-point transform: 512)
constexpr int kMinLg = 4, kMaxLg = 13;        // transforms of 16 .. 8192 points run in registers and LDS

// a carrier-map code of the modulator: kind in bits 0-1, conjugate in bit 2, the data index above
enum { SRC_ZERO = 0, SRC_DATA = 1, SRC_PILOT = 2, SRC_CONJ = 4 };

SSF_HD int log2_exact(long long n) {          // log2 n for a power of two, else -1
    int lg = 0;
    while ((1ll << lg) < n) ++lg;
    return (1ll << lg) == n ? lg : -1;
}
// the transform length the register-and-LDS kernels take (else rocFFT)
SSF_HD bool lds_length(long long L) {
    const int lg = log2_exact(L);
    return lg >= kMinLg && lg <= kMaxLg;
}
constexpr int threads_for(int lg) { return (1 << (lg - 4)) > kBlock ? (1 << (lg - 4)) : kBlock; }
constexpr int frames_per_workgroup(int lg) { return threads_for(lg) >> (lg - 4); }
SSF_HD size_t lds_bytes_for(int lg) { return (size_t)frames_per_workgroup(lg) * fused::lds_slots_per_fft(1 << lg) * sizeof(cx<double>); }

SSF_HD cx<double> load_cx(const void *p, long long i, int c64) {
    if (c64) {
        const cx<float> v = ((const cx<float> *)p)[i];
        return mk<double>((double)v.re, (double)v.im);
    }
    return ((const cx<double> *)p)[i];
}
SSF_HD void store_cx(void *p, long long i, int c64, cx<double> v) {
    if (c64) ((cx<float> *)p)[i] = mk<float>((float)v.re, (float)v.im);
    else ((cx<double> *)p)[i] = v;
}
SSF_HD cx<double> cdiv(cx<double> a, cx<double> b) {
    const double d = 1.0 / (b.re * b.re + b.im * b.im);
    return mk<double>((a.re * b.re + a.im * b.im) * d, (a.im * b.re - a.re * b.im) * d);
}

// ------------------------------------------------------------------------------------------------------------------- modulator
struct ModArgs {
    const int *map;               // L codes: register order (LDS kernels) or natural order (scatter kernel)
    const void *symb;             // nframes x Ni symbols
    void *out;                    // nframes x SpS (Nfft + G) samples
    cx<double> *work;             // rocFFT route: nframes x L
    long long nframes;
    int L, Ni, pre;               // pre = SpS G samples of prefix
    int in_c64, out_c64;
    double pilot_re, pilot_im;    // as the frame holds it: rounded to single precision
    double scale;                 // sqrt(L) / L
};

// what transform input `code` of frame f is: the frame's values are complex64 in the reference, so a complex128 symbol is rounded here
SSF_HD cx<double> mod_source(const ModArgs &a, long long f, int code) {
    const int kind = code & 3;
    if (kind == SRC_ZERO) return mk<double>(0.0, 0.0);
    cx<double> v;
    if (kind == SRC_PILOT) {
        v = mk<double>(a.pilot_re, a.pilot_im);
    } else {
        v = load_cx(a.symb, f * a.Ni + (code >> 3), a.in_c64);
        v = mk<double>((double)(float)v.re, (double)(float)v.im);
    }
    return (code & SRC_CONJ) ? fused::conj(v) : v;
}
// sample n of frame f: behind the prefix, and where it is one of the last `pre`, in the prefix too
SSF_HD void mod_store(const ModArgs &a, long long f, int n, cx<double> v) {
    const long long base = f * ((long long)a.L + a.pre);
    v = v * a.scale;
    store_cx(a.out, base + a.pre + n, a.out_c64, v);
    if (n >= a.L - a.pre) store_cx(a.out, base + (n - (a.L - a.pre)), a.out_c64, v);
}

template <int LG, class Ctx> SSF_HD void mod_body(Ctx &ctx, const ModArgs &a) {
    const fused::PassPlan p = fused::make_plan(LG);
    const int gpw = ctx.nthreads / p.tpf;
    const int g = ctx.tid / p.tpf, b = ctx.tid - g * p.tpf;
    const long long f = (long long)ctx.bid * gpw + g;
    const bool live = f < a.nframes;                         // idle groups still take part in the barriers
    cx<double> *l = (cx<double> *)ctx.lds + (size_t)g * fused::lds_slots_per_fft(p.L);
    cx<double> v[16];
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) v[idx] = live ? mod_source(a, f, a.map[idx * p.tpf + b]) : mk<double>(0.0, 0.0);
    fused::TwSrc<double> tws;
    fused::fft_dit<+1, 16, false, 1>(ctx, p, b, v, l, tws);
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) mod_store(a, f, b + p.tpf * q, v[q]);
}

// rocFFT route: work[f L + k] = the frame's input k, then (after the batch) the same stores
template <class Ctx> SSF_HD void mod_scatter_body(Ctx &ctx, const ModArgs &a) {
    const long long total = a.nframes * a.L;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < total; i += (long long)ctx.nblocks * ctx.nthreads) {
        const long long f = i / a.L;
        a.work[i] = mod_source(a, f, a.map[(int)(i - f * a.L)]);
    }
}
template <class Ctx> SSF_HD void mod_store_body(Ctx &ctx, const ModArgs &a) {
    const long long total = a.nframes * a.L;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < total; i += (long long)ctx.nblocks * ctx.nthreads) {
        const long long f = i / a.L;
        mod_store(a, f, (int)(i - f * a.L), a.work[i]);
    }
}

// ----------------------------------------------------------------------------------------------------------------- demodulator
struct DemodArgs {
    const int *dest;              // Nfft entries (register or natural order): where bin k goes, or -1.  Without pilots the index of
                                  // the data symbol in the frame's output, with pilots the carrier 0 .. Ns - 1
    const int *pidx;              // Ns: the rank of carrier c among the sorted pilots, or -1
    const void *sig;              // nframes x (Nfft + G)
    void *out;                    // nframes x Ni
    cx<double> *Y;                // with pilots: nframes x Ns, the spectrum of every frame
    double *habs, *hpha;          // with pilots: Np x nframes, |H_est| and its angle per pilot and frame
    cx<double> *work;             // rocFFT route: nframes x Nfft
    long long nframes;
    int Nfft, G, Ns, Ni, Np;
    int in_c64;                   // the output has the input's type
    double pilot_re, pilot_im, scale;         // scale = 1 / sqrt(Nfft)
};

SSF_HD cx<double> demod_load(const DemodArgs &a, long long f, int n) {
    return load_cx(a.sig, f * ((long long)a.Nfft + a.G) + a.G + n, a.in_c64);
}
// bin value v of frame f, whose table entry is d
SSF_HD void demod_store(const DemodArgs &a, long long f, int d, cx<double> v) {
    if (d < 0) return;
    v = v * a.scale;
    if (a.Np == 0) {
        store_cx(a.out, f * a.Ni + d, a.in_c64, v);
        return;
    }
    a.Y[f * a.Ns + d] = v;
    const int j = a.pidx[d];
    if (j >= 0) {
        const cx<double> h = cdiv(v, mk<double>(a.pilot_re, a.pilot_im));
        a.habs[(long long)j * a.nframes + f] = std::hypot(h.re, h.im);
        a.hpha[(long long)j * a.nframes + f] = std::atan2(h.im, h.re);
    }
}

template <int LG, class Ctx> SSF_HD void demod_body(Ctx &ctx, const DemodArgs &a) {
    const fused::PassPlan p = fused::make_plan(LG);
    const int gpw = ctx.nthreads / p.tpf;
    const int g = ctx.tid / p.tpf, b = ctx.tid - g * p.tpf;
    const long long f = (long long)ctx.bid * gpw + g;
    const bool live = f < a.nframes;
    cx<double> *l = (cx<double> *)ctx.lds + (size_t)g * fused::lds_slots_per_fft(p.L);
    cx<double> v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = live ? demod_load(a, f, b + p.tpf * q) : mk<double>(0.0, 0.0);
    fused::TwSrc<double> tws;
    fused::fft_dif<-1, 16, false, 1>(ctx, p, b, v, l, tws);
    if (!live) return;
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) demod_store(a, f, a.dest[idx * p.tpf + b], v[idx]);
}

template <class Ctx> SSF_HD void demod_gather_body(Ctx &ctx, const DemodArgs &a) {
    const long long total = a.nframes * a.Nfft;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < total; i += (long long)ctx.nblocks * ctx.nthreads) {
        const long long f = i / a.Nfft;
        a.work[i] = demod_load(a, f, (int)(i - f * a.Nfft));
    }
}
template <class Ctx> SSF_HD void demod_store_body(Ctx &ctx, const DemodArgs &a) {
    const long long total = a.nframes * a.Nfft;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < total; i += (long long)ctx.nblocks * ctx.nthreads) {
        const long long f = i / a.Nfft;
        demod_store(a, f, a.dest[(int)(i - f * a.Nfft)], a.work[i]);
    }
}

// ---- the channel: the pilots' mean magnitude and mean angle, joined by straight lines over the carriers (interp1d, kind 'linear',
// fill_value 'extrapolate': the end segments run on).  hi[c] is the upper pilot of carrier c's segment, 1 .. Np - 1 (host: searchsorted
// on the sorted pilots, clipped).
struct ChanArgs {
    const double *habs, *hpha;    // Np x nframes
    double *mean;                 // 2 Np: mean magnitude, then mean angle, per sorted pilot
    const int *pilots, *hi;       // Np sorted carriers; Ns segment indices
    cx<double> *H;                // Ns
    long long nframes;
    int Np, Ns;
};
SSF_HD double chan_line(const double *y, const int *x, int hi, int c) {
    const double slope = (y[hi] - y[hi - 1]) / (double)(x[hi] - x[hi - 1]);
    return slope * (double)(c - x[hi - 1]) + y[hi - 1];
}
SSF_HD cx<double> chan_value(const ChanArgs &a, int c) {
    const double mag = chan_line(a.mean, a.pilots, a.hi[c], c), ang = chan_line(a.mean + a.Np, a.pilots, a.hi[c], c);
    double s, co;
    fused::sincos_d(ang, s, co);
    return mk<double>(mag * co, mag * s);
}

// ---- single-tap equalisation and the data carriers: out[f Ni + d] = Y[f Ns + carrier[d]] / H[carrier[d]]
struct EqArgs {
    const cx<double> *Y, *H;
    const int *carrier;           // Ni data carriers
    void *out;
    long long nframes;
    int Ns, Ni, out_c64;
};
template <class Ctx> SSF_HD void equalize_body(Ctx &ctx, const EqArgs &a) {
    const long long total = a.nframes * a.Ni;
    for (long long i = (long long)ctx.bid * ctx.nthreads + ctx.tid; i < total; i += (long long)ctx.nblocks * ctx.nthreads) {
        const long long f = i / a.Ni;
        const int c = a.carrier[(int)(i - f * a.Ni)];
        store_cx(a.out, i, a.out_c64, cdiv(a.Y[f * a.Ns + c], a.H[c]));
    }
}

// ---- host side: natural-order tables -> the order the register kernels read
// modulator (DIT): value idx of lane b is the transform's input rev_pos(reg_pos(last pass, b, idx)); demodulator (DIF): the same
// index is the bin that value idx of lane b holds afterwards
inline void register_order(const int *natural, int *reg, int lg) {
    const fused::PassPlan p = fused::make_plan(lg);
    for (int b = 0; b < p.tpf; ++b)
        for (int idx = 0; idx < 16; ++idx) reg[idx * p.tpf + b] = natural[fused::rev_pos(p, fused::reg_pos(p, p.npass - 1, b, idx))];
}
// the modulator's map as its kernels read it (lg > 0: the register kernel of 2^lg points)
inline void mod_table(const int *src_map, int L, int lg, std::vector<int> &h) {
    h.assign(src_map, src_map + L);
    if (lg > 0) register_order(src_map, h.data(), lg);
}
// the demodulator's tables, one block of ints: [dest Nfft | pidx Ns | carrier Ni | pilots Np | hi Ns]
struct DemodTables {
    int dest, pidx, carrier, pilots, hi;      // offsets into the block
};
inline DemodTables demod_tables(const int *bin_carrier, const int *data_carriers, const int *pilot_carriers, const int *pilot_hi, int Nfft,
                                int Ns, int Ni, int Np, int lg, std::vector<int> &h) {
    const DemodTables t{0, Nfft, Nfft + Ns, Nfft + Ns + Ni, Nfft + Ns + Ni + Np};
    h.assign((size_t)t.hi + Ns, -1);
    std::vector<int> nat(bin_carrier, bin_carrier + Nfft);
    for (int d = 0; d < Ni; ++d) h[t.carrier + d] = data_carriers[d];
    for (int j = 0; j < Np; ++j) h[t.pilots + j] = pilot_carriers[j], h[t.pidx + pilot_carriers[j]] = j;
    for (int c = 0; c < Ns; ++c) h[t.hi + c] = Np ? pilot_hi[c] : 0;
    if (!Np) {                                // no pilots: a bin goes straight to its data symbol's place
        std::vector<int> rank((size_t)Ns, -1);
        for (int d = 0; d < Ni; ++d) rank[data_carriers[d]] = d;
        for (int k = 0; k < Nfft; ++k) nat[k] = nat[k] >= 0 ? rank[nat[k]] : -1;
    }
    if (lg > 0) register_order(nat.data(), h.data() + t.dest, lg);
    else for (int k = 0; k < Nfft; ++k) h[t.dest + k] = nat[k];
    return t;
}

}  // namespace ofdm
}  // namespace ssf
