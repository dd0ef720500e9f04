// emu_cpr.cpp -- the carrier-recovery kernel bodies of opticommpy_amd/csrc/cpr_kernels.h looped over the symbols on the host
// (g++, no GPU): the same per-element functions the gfx950 kernels of engine_cpr.hip call, in the same sequence of passes, with
// one running sum where the kernels keep one partial per workgroup, one sequential prefix sum per row of minimum distances
// where the workgroup cuts the row into segments, a plain DFT where the library calls rocFFT, and a
// sequential scan inside a block of the unwrap where the workgroup scans in a tree.  tests/test_cpr_emu.py compiles this file,
// feeds it a fixture and holds the results to the bounds of the GPU test.
//
// usage: emu_cpr <input file> <output file>
//   int64 n, nModes, dtype, Nh, B, M, runFOE, P, what (0 = cpr, 1 = bps alone, 2 = FOE alone, 3 = derotation alone by the given
//   offset, the first symbol counted as number Nh);  double Fs, fo;  double table[2M];  x
// output (binary): what = 0: sigOut (n, nModes) complex128, phase (n, nModes), raw (n, nModes), fo[nModes]
//                  what = 1: raw (n, nModes);   what = 2: sigOut (n, nModes) complex128, fo[nModes];   what = 3: sigOut
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cpr_kernels.h"

using namespace ssf::ck;

static void read_or_die(void *dst, size_t bytes, FILE *f) {
    if (bytes && std::fread(dst, 1, bytes, f) != bytes) {
        std::fprintf(stderr, "emu_cpr: short input\n");
        std::exit(2);
    }
}

// the table as the product of its levels, as engine_cpr.hip decides it
static bool separable(const std::vector<double> &tab, int M, std::vector<double> &lre, std::vector<double> &lim) {
    auto add = [](std::vector<double> &v, double x) {
        for (double y : v)
            if (y == x) return;
        v.push_back(x);
    };
    for (int m = 0; m < M; ++m) add(lre, tab[2 * m]), add(lim, tab[2 * m + 1]);
    if (lre.size() * lim.size() != (size_t)M) return false;
    for (int m = 0; m < M; ++m)
        for (int q = 0; q < m; ++q)
            if (tab[2 * m] == tab[2 * q] && tab[2 * m + 1] == tab[2 * q + 1]) return false;
    return true;
}

struct Signal {
    const void *p;
    int dtype;
};

static void bps(const Signal &x, long long n, int nModes, int Nh, int B, int M, const std::vector<double> &tab, std::vector<double> &raw) {
    std::vector<double> lre, lim, rot(2 * B), testph(B);
    const bool sep = separable(tab, M, lre, lim);
    for (int b = 0; b < B; ++b) {
        testph[b] = (double)b * (kPiD / 2.0) / (double)B;
        rot[2 * b] = std::cos(testph[b]), rot[2 * b + 1] = std::sin(testph[b]);
    }
    const int W = kTile + 2 * Nh;
    std::vector<double> d((size_t)B * W);
    raw.assign((size_t)n * nModes, 0.0);
    for (int m = 0; m < nModes; ++m) {
        for (long long t0 = 0; t0 < n; t0 += kTile) {              // a tile of output symbols and its halo, as a workgroup takes it
            for (int j = 0; j < W; ++j) {
                const long long g = t0 - Nh + j;
                double xr = 0.0, xi = 0.0;
                if (g >= 0 && g < n) load(x.dtype, x.p, g * nModes + m, xr, xi);
                for (int b = 0; b < B; ++b)
                    d[(size_t)b * W + j] = sep ? dmin_sep(lre.data(), (int)lre.size(), lim.data(), (int)lim.size(), xr, xi, rot[2 * b], rot[2 * b + 1])
                                               : dmin_full(tab.data(), M, xr, xi, rot[2 * b], rot[2 * b + 1]);
            }
            for (int b = 0; b < B; ++b) {                          // rows -> inclusive prefix sums (the kernel: in 16 segments)
                double run = 0.0;
                for (int j = 0; j < W; ++j) run += d[(size_t)b * W + j], d[(size_t)b * W + j] = run;
            }
            for (int t = 0; t < kTile && t0 + t < n; ++t) {
                double best = INFINITY;
                int bi = 0;
                for (int b = 0; b < B; ++b) {
                    const double sum = window_from_prefix(d.data() + (size_t)b * W, t, Nh);
                    if (sum < best) best = sum, bi = b;
                }
                raw[(t0 + t) * nModes + m] = testph[bi];
            }
        }
    }
}

static void normalise(std::vector<Cplx> &y) {
    double acc = 0.0;
    for (const Cplx &v : y) acc += v.re * v.re + v.im * v.im;
    const double s = std::sqrt(acc / (double)y.size());
    for (Cplx &v : y) v.re = v.re / s, v.im = v.im / s;
}

static void foe(const Signal &x, long long n, int nModes, int P, double Fs, std::vector<Cplx> &y, std::vector<double> &fo) {
    std::vector<double> tw(2 * n);
    for (long long q = 0; q < n; ++q) tw[2 * q] = std::cos(-2.0 * kPiD * (double)q / (double)n), tw[2 * q + 1] = std::sin(-2.0 * kPiD * (double)q / (double)n);
    std::vector<Cplx> f(n), F(n);
    y.resize((size_t)n * nModes), fo.assign(nModes, 0.0);
    for (int m = 0; m < nModes; ++m) {
        for (long long k = 0; k < n; ++k) {
            double xr, xi;
            load(x.dtype, x.p, k * nModes + m, xr, xi);
            cpow_int(xr, xi, P, f[k].re, f[k].im);
        }
        for (long long b = 0; b < n; ++b) {
            double sr = 0.0, si = 0.0;
            for (long long k = 0; k < n; ++k) {
                const long long q = (b * k) % n;
                sr += f[k].re * tw[2 * q] - f[k].im * tw[2 * q + 1];
                si += f[k].re * tw[2 * q + 1] + f[k].im * tw[2 * q];
            }
            F[b].re = sr, F[b].im = si;
        }
        double mag = -1.0;
        long long pos = n;
        for (long long i = 0; i < n; ++i) {
            const Cplx v = F[shifted_bin(i, n)];
            argmax_merge(mag, pos, v.re * v.re + v.im * v.im, i);
        }
        fo[m] = foe_frequency(pos, n, Fs, P);
        const double a = foe_slope(fo[m]);
        for (long long k = 0; k < n; ++k) {
            double xr, xi;
            load(x.dtype, x.p, k * nModes + m, xr, xi);
            derotate(xr, xi, a, k, Fs, y[k * nModes + m].re, y[k * nModes + m].im);
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[9];
    double dh[2];
    read_or_die(h, sizeof(h), f);
    read_or_die(dh, sizeof(dh), f);
    const double Fs = dh[0], fo_given = dh[1];
    const long long n = h[0];
    const int nModes = (int)h[1], dtype = (int)h[2], Nh = (int)h[3], B = (int)h[4], M = (int)h[5], runFOE = (int)h[6], P = (int)h[7],
              what = (int)h[8];
    std::vector<double> tab(2 * (size_t)M);
    read_or_die(tab.data(), tab.size() * 8, f);
    std::vector<char> xin((size_t)n * nModes * (dtype == ssf::mk::kC128 ? 16 : 8));
    read_or_die(xin.data(), xin.size(), f);
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    Signal x{xin.data(), dtype};
    std::vector<Cplx> work, y((size_t)n * nModes);
    std::vector<double> fo(nModes, 0.0), raw, phase((size_t)n * nModes);

    if (what == 1) {
        bps(x, n, nModes, Nh, B, M, tab, raw);
        std::fwrite(raw.data(), 8, raw.size(), o);
    } else if (what == 3) {
        const double a = foe_slope(fo_given);
        for (long long k = 0; k < n; ++k)
            for (int m = 0; m < nModes; ++m) {
                double xr, xi;
                load(dtype, xin.data(), k * nModes + m, xr, xi);
                derotate(xr, xi, a, (long long)Nh + k, Fs, y[k * nModes + m].re, y[k * nModes + m].im);
            }
        std::fwrite(y.data(), 16, y.size(), o);
    } else if (what == 2) {
        foe(x, n, nModes, P, Fs, work, fo);
        std::fwrite(work.data(), 16, work.size(), o);
        std::fwrite(fo.data(), 8, fo.size(), o);
    } else {
        if (runFOE) {
            foe(x, n, nModes, P, Fs, work, fo);
            normalise(work);
            x = Signal{work.data(), ssf::mk::kC128};
        }
        bps(x, n, nModes, Nh, B, M, tab, raw);
        // unwrap: scan inside blocks of kScanBlock symbols, block sums scanned in order, then applied
        const long long nblk = (n + kScanBlock - 1) / kScanBlock;
        std::vector<double> loc((size_t)n), bsum(nblk);
        for (int m = 0; m < nModes; ++m) {
            for (long long b = 0; b < nblk; ++b) {
                double run = 0.0;
                for (long long k = b * kScanBlock; k < (b + 1) * kScanBlock && k < n; ++k) {
                    if (k >= 1) run += unwrap_corr(4.0 * raw[(k - 1) * nModes + m], 4.0 * raw[k * nModes + m]);
                    loc[k] = run;
                }
                bsum[b] = run;
            }
            double off = 0.0;
            for (long long b = 0; b < nblk; ++b) {
                const double v = bsum[b];
                bsum[b] = off, off += v;
            }
            for (long long k = 0; k < n; ++k) {
                const double cum = bsum[k / kScanBlock] + loc[k];
                const double ph = (4.0 * raw[k * nModes + m] + cum) / 4.0;
                phase[k * nModes + m] = ph;
                double xr, xi, s, c;
                load(x.dtype, x.p, k * nModes + m, xr, xi);
                sincos_d(ph, s, c);
                rotate(xr, xi, c, s, y[k * nModes + m].re, y[k * nModes + m].im);
            }
        }
        normalise(y);
        std::fwrite(y.data(), 16, y.size(), o);
        std::fwrite(phase.data(), 8, phase.size(), o);
        std::fwrite(raw.data(), 8, raw.size(), o);
        std::fwrite(fo.data(), 8, fo.size(), o);
    }
    std::fclose(o);
    return 0;
}
