// emu_sync.cpp -- the arithmetic of engine_sync.hip without a GPU: the per-element bodies and the decisions of
// opticommpy_amd/csrc/sync_kernels.h looped with g++, around a radix-2 transform written here (the engine's lengths are powers of
// two).  The received signal arrives at one sample per symbol: the decimation is the receiver engine's and has its own emulator.
//   in:  int64 mode (0 amp, 1 real, 2 finddelay), nModes, n_x, n_y, x_dtype, y_dtype, x_f32, y_f32; x (n_x, nModes); y (n_y, nModes)
//   out: int64 delay[8], swap[8], rot[8], conj[8]; double corrMatrix[64]; then (n_x, nModes) of x's type unless finddelay
// g++ -O2 -std=c++17 -ffp-contract=off -I opticommpy_amd/csrc tests/emu/emu_sync.cpp
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sync_kernels.h"

using namespace ssf::sk;
namespace mk = ssf::mk;
typedef std::complex<double> zc;

static void fft(zc *a, long long n, bool inverse) {
    for (long long i = 1, j = 0; i < n; ++i) {
        long long bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    const double pi = 3.14159265358979323846;
    for (long long len = 2; len <= n; len <<= 1) {
        std::vector<zc> w(len / 2);
        for (long long k = 0; k < len / 2; ++k) {
            const double t = (inverse ? 2.0 : -2.0) * pi * (double)k / (double)len;
            w[k] = zc(std::cos(t), std::sin(t));
        }
        for (long long i = 0; i < n; i += len)
            for (long long k = 0; k < len / 2; ++k) {
                const zc u = a[i + k], v = a[i + k + len / 2] * w[k];
                a[i + k] = u + v, a[i + k + len / 2] = u - v;
            }
    }
}

static size_t elem_size(int dtype) { return dtype == mk::kC128 ? 16 : dtype == mk::kC64 || dtype == mk::kF64 ? 8 : 4; }

struct Emu {
    int mode, nModes;
    long long L, lags, n_tx;
    std::vector<Cplx> F, G;
    std::vector<Peak> peak;
    Record rec{};

    void prepare(int side, const void *x, int dtype, bool f32, long long n, long long off) {
        const int base = side ? nModes : 0;
        for (long long i = 0; i < n; ++i)
            for (int m = 0; m < nModes; ++m) {
                double re, im;
                load(dtype, x, i * nModes + m, re, im);
                Cplx v;
                if (mode == kAmp) {
                    v.re = amp_value(re, im, f32), v.im = 0.0;
                } else if (mode == kReal && side) {
                    v.re = re, v.im = 0.0;
                    F[(long long)(2 * nModes + m) * L + i] = Cplx{im, 0.0};
                } else {
                    v.re = re, v.im = im;
                }
                F[(long long)(base + m) * L + off + i] = v;
            }
        if (mode != kAmp) return;
        for (int m = 0; m < nModes; ++m) {
            Cplx *f = F.data() + (long long)(base + m) * L + off;
            double mean;
            if (f32) {
                const long long nleaf = mk::pw_leaves(n, nullptr);
                std::vector<long long> starts(nleaf + 1, n);
                mk::pw_leaves(n, starts.data());
                std::vector<float> leaf(nleaf);
                for (long long t = 0; t < nleaf; ++t) leaf[t] = pw_leaf_re(f + starts[t], starts[t + 1] - starts[t]);
                mk::PwFrame stk[64];
                mean = mean_f32(mk::pw_combine(leaf.data(), n, stk), n);
            } else {
                double s = 0.0;                  // (the kernels add workgroup partials: another order, the same decisions)
                for (long long i = 0; i < n; ++i) s += f[i].re;
                mean = s / (double)n;
            }
            for (long long i = 0; i < n; ++i) f[i].re = center_value(f[i].re, mean, f32);
        }
    }

    void correlate(int round, int nslots, int peak_base) {
        const double scale = 1.0 / (double)L;
        for (int slot = 0; slot < nslots; ++slot) {
            int sa, sb, sb2;
            slot_sequences(mode, round, nModes, slot, rec.swap, sa, sb, sb2);
            const Cplx *A = F.data() + (long long)sa * L, *B = F.data() + (long long)sb * L, *B2 = F.data() + (long long)(sb2 < 0 ? sb : sb2) * L;
            Cplx *g = G.data() + (long long)slot * L;
            for (long long j = 0; j < L; ++j) g[j] = sb2 < 0 ? spectral_product(A[j], B[j], scale) : spectral_pair(A[j], B[j], B2[j], scale);
            fft((zc *)g, L, true);
            Peak p0 = peak_none(lags), p1 = peak_none(lags);
            for (long long j = lags - 1; j >= 0; --j) peak_channels(mode, g[j], j, p0, p1);      // (any order gives the same peak)
            peak[peak_base + 2 * slot] = p0, peak[peak_base + 2 * slot + 1] = p1;
        }
        const int first = 2 * n_slots(mode, nModes);
        if (mode == kAmp) decide_amp(nModes, n_tx, peak.data(), rec);
        else if (mode == kReal && round == 1) decide_real_rot(nModes, peak.data(), rec);
        else if (mode == kReal) decide_real_delay(nModes, n_tx, peak.data(), peak.data() + first, rec);
        else rec.peak_index[0] = peak[0].idx, rec.delay[0] = peak[0].idx - (n_tx - 1);
    }
};

template <class T> static void gather(const Emu &e, const void *x, long long n, std::vector<char> &out) {
    out.resize((size_t)n * e.nModes * sizeof(T));
    const T *tx = (const T *)x;
    T *o = (T *)out.data();
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < e.nModes; ++k) {
            T v = tx[roll_source(i, e.rec.delay[k], n) * e.nModes + e.rec.swap[k]];
            rotate_conj(v.re, v.im, e.rec.rot[k], e.rec.conj[k]);
            o[i * e.nModes + k] = v;
        }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    long long h[8];
    if (std::fread(h, sizeof(long long), 8, f) != 8) return 2;
    Emu e;
    e.mode = (int)h[0], e.nModes = (int)h[1];
    const long long n_x = h[2], n_y = h[3];
    const int x_dtype = (int)h[4], y_dtype = (int)h[5];
    std::vector<char> x((size_t)n_x * e.nModes * elem_size(x_dtype)), y((size_t)n_y * e.nModes * elem_size(y_dtype));
    if (std::fread(x.data(), 1, x.size(), f) != x.size() || std::fread(y.data(), 1, y.size(), f) != y.size()) return 2;
    std::fclose(f);

    e.n_tx = n_x, e.lags = n_x + n_y - 1;
    e.L = 4;
    while (e.L < e.lags) e.L <<= 1;
    const int nseq = n_sequences(e.mode, e.nModes), nslots = n_slots(e.mode, e.nModes);
    e.F.assign((size_t)nseq * e.L, Cplx{0.0, 0.0});
    e.G.assign((size_t)nslots * e.L, Cplx{0.0, 0.0});
    e.peak.assign(2 * (size_t)(nslots + e.nModes), peak_none(e.lags));
    e.prepare(0, x.data(), x_dtype, h[6] != 0, n_x, n_y - 1);
    e.prepare(1, y.data(), y_dtype, h[7] != 0, n_y, 0);
    for (int s = 0; s < nseq; ++s) fft((zc *)(e.F.data() + (long long)s * e.L), e.L, false);
    e.correlate(1, nslots, 0);
    if (e.mode == kReal) e.correlate(2, e.nModes, 2 * nslots);

    std::vector<char> out;
    if (e.mode != kDelay) {
        if (x_dtype == mk::kC64) gather<mk::CplxF>(e, x.data(), n_x, out);
        else gather<Cplx>(e, x.data(), n_x, out);
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    long long rec[32];
    for (int k = 0; k < 8; ++k) rec[k] = e.rec.delay[k], rec[8 + k] = e.rec.swap[k], rec[16 + k] = e.rec.rot[k], rec[24 + k] = e.rec.conj[k];
    std::fwrite(rec, sizeof(long long), 32, o);
    std::fwrite(e.rec.corr, sizeof(double), 64, o);
    std::fwrite(out.data(), 1, out.size(), o);
    std::fclose(o);
    return 0;
}
