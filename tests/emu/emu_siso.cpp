// emu_siso.cpp -- the ffe / dfe / volterra kernels' arithmetic on the host: the per-symbol bodies of
// opticommpy_amd/csrc/siso_kernels.h looped over lanes and symbols in the layout and order of engine_siso.hip (coefficient c in lane
// c % 64, slot c / 64; a lane's products summed in slot order, the 64 lane sums in a butterfly; the frozen tail one symbol at a
// time with frozen_output).  Built by tests/test_siso_emu.py with g++; also the one-core comparison of tools/bench_siso.py.
//   emu_siso in.bin out.bin [reps]
// in.bin:  20 int64 (n, nref, nTrain, kind, mode, cx, prec32, order, nTaps, nFB, n2, n3, SpS, M, preconvIters, ncoef, no_frozen, 0, 0, 0),
//          then doubles: mu, table (2 M), coefficients (ncoef, or 2 ncoef for complex data), x (n or 2 n), ref (nref or 2 nref)
// out.bin: doubles: sigOut (N or 2 N), coefficients, mse (N), then serial symbols, frozen symbols, R, seconds of the last repetition
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "siso_kernels.h"

using namespace ssf::sk;
namespace mk = ssf::mk;

struct Problem {
    Geo g;
    long long nref;
    bool no_frozen;
    std::vector<double> table, coef, x, ref;
};

template <bool CX> static V<CX> value_at(const std::vector<double> &a, long long i) { return V<CX>{CX ? a[2 * i] : a[i], CX ? a[2 * i + 1] : 0.0}; }

template <int R, bool CX> static void walk(Problem &p, std::vector<double> &y, std::vector<double> &mse, double *info) {
    const Geo &g = p.g;
    const int dtype = CX ? mk::kC128 : mk::kF64, nTaps = g.nTaps, SpS = g.SpS, M = g.M;
    const Split sp = split_of(g, !p.no_frozen);
    // the scales
    double sx = 0.0, sr = 0.0, mx = 0.0;
    for (size_t i = 0; i < p.x.size(); ++i) sx += p.x[i] * p.x[i];
    sx = std::sqrt(sx / (double)g.n);
    for (size_t i = 0; i < p.ref.size(); ++i) sr += p.ref[i] * p.ref[i];
    sr = p.nref ? std::sqrt(sr / (double)p.nref) : 1.0;
    if (g.kind == kVolterra) {
        for (long long i = 0; i < g.n; ++i) mx = std::fmax(mx, std::fabs(round_prec(p.x[i] / sx, g.prec32)));
    }

    // the lanes' registers
    static V<CX> h[kWave][R];
    static Entry ent[kWave][R];
    static bool has[kWave][R];
    for (int l = 0; l < kWave; ++l)
        for (int r = 0; r < R; ++r) {
            const int c = l + kWave * r;
            has[l][r] = c < g.ncoef;
            h[l][r] = has[l][r] ? value_at<CX>(p.coef, c) : vzero<CX>();
            ent[l][r] = has[l][r] ? entry_of(g, c) : Entry{0, 0, 0, 0, false};
        }
    std::vector<V<CX>> head[2] = {std::vector<V<CX>>(nTaps), std::vector<V<CX>>(nTaps)};      // raw, as in the kernel
    std::vector<V<CX>> fb(kMaxFb + 1, vzero<CX>());                                            // fb[j]: the reference of symbol k - 1 - j
    auto stream_raw = [&](int pass, long long q) {
        if (pass > 0 && q < nTaps) return head[pass & 1][q];
        double re, im;
        padded_raw(g, dtype, p.x.data(), q, re, im);
        return V<CX>{re, im};
    };
    for (int pass = 0; pass < g.passes; ++pass) {
        const long long len = pass + 1 < g.passes ? g.nTrain + 1 : sp.serial_last;
        if (pass + 1 < g.passes)
            for (int t = 0; t < nTaps; ++t) head[(pass + 1) & 1][t] = stream_raw(pass, (g.nTrain + 1) * SpS + t);
        std::vector<V<CX>> w(nTaps);
        for (long long k = 0; k < len; ++k) {
            for (int t = 0; t < nTaps; ++t) {
                const V<CX> raw = stream_raw(pass, k * SpS + t);
                w[t] = normalise<CX>(g, sx, mx, raw.re, raw.im);
            }
            static V<CX> phi[kWave][R];
            double yr[kWave], yi[kWave];
            for (int l = 0; l < kWave; ++l) {
                for (int r = 0; r < R; ++r) {
                    V<CX> v = vzero<CX>();
                    const Entry &e = ent[l][r];
                    if (has[l][r]) {
                        if (e.fb) v = fb[e.i0];
                        else {
                            v = w[e.i0];
                            if (e.deg >= 2) v.re *= w[e.i1].re;
                            if (e.deg >= 3) v.re *= w[e.i2].re;
                        }
                    }
                    phi[l][r] = v;
                }
                const V<CX> part = lane_output<R, CX>(h[l], phi[l]);
                yr[l] = part.re, yi[l] = part.im;
            }
            butterfly_sum(yr);
            if (CX) butterfly_sum(yi);
            const V<CX> yv{yr[0], CX ? yi[0] : 0.0};
            V<CX> rf;
            if (k < g.nTrain) {
                const V<CX> raw = value_at<CX>(p.ref, k);
                rf = normalise_ref<CX>(g, sr, raw.re, raw.im);
            } else {
                double d[kWave];
                int bi[kWave];
                for (int l = 0; l < kWave; ++l) {
                    d[l] = INFINITY, bi[l] = kMaxM;
                    for (int m = l; m < M; m += kWave) argmin_merge(d[l], bi[l], dist<CX>(yv, p.table[2 * m], p.table[2 * m + 1]), m);
                }
                butterfly_argmin(d, bi);
                const int b = bi[0] < M ? bi[0] : M - 1;
                rf = V<CX>{p.table[2 * b], CX ? p.table[2 * b + 1] : 0.0};
            }
            double esq;
            const V<CX> e = error_of<CX>(rf, yv, esq);
            if (g.fulltime || k < g.nTrain) {
                for (int l = 0; l < kWave; ++l)
                    for (int r = 0; r < R; ++r) {
                        const double mu = step_of(g.mu, ent[l][r].deg >= 2 && !ent[l][r].fb ? ent[l][r].deg : 1);
                        vupdate<CX>(h[l][r], V<CX>{mu * e.re, CX ? mu * e.im : 0.0}, phi[l][r]);
                    }
            }
            if (g.nFB > 0) {
                for (int j = g.nFB - 1; j > 0; --j) fb[j] = fb[j - 1];
                fb[0] = rf;
            }
            if (CX) y[2 * k] = yv.re, y[2 * k + 1] = yv.im;
            else y[k] = yv.re;
            mse[k] = esq;
        }
    }
    for (int l = 0; l < kWave; ++l)
        for (int r = 0; r < R; ++r)
            if (has[l][r]) {
                const int c = l + kWave * r;
                if (CX) p.coef[2 * c] = h[l][r].re, p.coef[2 * c + 1] = h[l][r].im;
                else p.coef[c] = h[l][r].re;
            }
    // the frozen tail
    if (sp.frozen_count > 0) {
        std::vector<V<CX>> coef(g.ncoef), w(nTaps);
        for (int c = 0; c < g.ncoef; ++c) coef[c] = value_at<CX>(p.coef, c);
        for (long long k = sp.frozen_from; k < g.N; ++k) {
            for (int t = 0; t < nTaps; ++t) {
                double re, im;
                padded_raw(g, dtype, p.x.data(), k * SpS + t, re, im);
                w[t] = normalise<CX>(g, sx, mx, re, im);
            }
            const V<CX> yv = frozen_output<CX>(g, coef.data(), w.data());
            const int b = nearest<CX>(p.table.data(), M, yv);
            double esq;
            error_of<CX>(V<CX>{p.table[2 * b], CX ? p.table[2 * b + 1] : 0.0}, yv, esq);
            if (CX) y[2 * k] = yv.re, y[2 * k + 1] = yv.im;
            else y[k] = yv.re;
            mse[k] = esq;
        }
    }
    if (g.kind == kVolterra) {
        double s = 0.0;
        for (long long k = 0; k < g.N; ++k) s += y[k] * y[k];
        s = std::sqrt(s / (double)g.N);
        for (long long k = 0; k < g.N; ++k) y[k] /= s;
    }
    info[0] = (double)sp.serial_total, info[1] = (double)sp.frozen_count, info[2] = sp.serial_total > 0 ? R : 0;
}

template <bool CX> static void walk_r(Problem &p, std::vector<double> &y, std::vector<double> &mse, double *info) {
    switch (slots_for(p.g.ncoef)) {
    case 1: return walk<1, CX>(p, y, mse, info);
    case 2: return walk<2, CX>(p, y, mse, info);
    case 4: return walk<4, CX>(p, y, mse, info);
    case 8: return walk<8, CX>(p, y, mse, info);
    case 16: return walk<16, CX>(p, y, mse, info);
    default: return walk<24, CX>(p, y, mse, info);
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    long long hd[20];
    if (std::fread(hd, sizeof(long long), 20, f) != 20) return 4;
    Problem p{};
    Geo &g = p.g;
    g.n = hd[0], p.nref = hd[1], g.nTrain = hd[2], g.kind = (int)hd[3], g.fulltime = hd[4] == kFulltime, g.cx = (int)hd[5];
    g.prec32 = (int)hd[6], g.order = (int)hd[7], g.nTaps = (int)hd[8], g.nFB = g.kind == kDfe ? (int)hd[9] : 0, g.n2 = (int)hd[10], g.n3 = (int)hd[11];
    g.SpS = (int)hd[12], g.M = (int)hd[13], g.ncoef = (int)hd[15], p.no_frozen = hd[16] != 0;
    g.Lpad = g.nTaps / 2, g.L = g.n + 2 * g.Lpad, g.N = g.n / g.SpS, g.t2 = (g.nTaps - g.n2) / 2, g.t3 = (g.nTaps - g.n3) / 2;
    g.passes = g.nTrain < g.N ? (int)hd[14] : 1;
    if (g.ncoef > kMaxCoeffs || g.nTaps > kMaxTaps || g.nFB > kMaxFb || g.M > kMaxM || g.SpS > g.nTaps || g.SpS < 1 || g.N < 1) return 5;
    const int w = g.cx ? 2 : 1;
    auto rd = [&](std::vector<double> &v, size_t count) {
        v.resize(count);
        return count == 0 || std::fread(v.data(), sizeof(double), count, f) == count;
    };
    double mu;
    if (std::fread(&mu, sizeof(double), 1, f) != 1) return 4;
    g.mu = mu;
    if (!rd(p.table, 2 * (size_t)g.M) || !rd(p.coef, (size_t)w * g.ncoef) || !rd(p.x, (size_t)w * g.n) || !rd(p.ref, (size_t)w * p.nref)) return 4;
    std::fclose(f);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 1;
    std::vector<double> y((size_t)w * g.N), mse((size_t)g.N), coef0 = p.coef;
    double info[4] = {0, 0, 0, 0};
    for (int r = 0; r < reps; ++r) {
        p.coef = coef0;
        const auto t0 = std::chrono::steady_clock::now();
        if (g.cx) walk_r<true>(p, y, mse, info);
        else walk_r<false>(p, y, mse, info);
        info[3] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    std::fwrite(y.data(), sizeof(double), y.size(), o);
    std::fwrite(p.coef.data(), sizeof(double), p.coef.size(), o);
    std::fwrite(mse.data(), sizeof(double), mse.size(), o);
    std::fwrite(info, sizeof(double), 4, o);
    std::fclose(o);
    return 0;
}
