// emu_eq.cpp -- the adaptive-equalizer kernel bodies of opticommpy_amd/csrc/eq_kernels.h looped over lanes and symbols on the
// host (g++, no GPU): the same per-symbol functions the gfx950 kernels of engine_eq.hip call, with the kernel's lane layout (lane
// l holds coefficients l + 64 r) and its reduction order (a lane sums its R products in order, the 64 lane sums go through the
// butterfly over distances 32 .. 1).  The chunking of the kernel moves data only and is left out.  tests/test_eq_emu.py compiles
// this file, feeds it a fixture as the package hands it to the library and holds the results to the bounds of the GPU test.
//
// usage: emu_eq <input file> <output file>
//   int64 n, total, nref, nModes, nTaps, SpS, dtype, ref_dtype, nStages, numIter, M, nRadii;  double Rcma;
//   per stage: int64 L, int64 alg, double mu;  double table[2 M];  double radii[nRadii];  complex128 H[nModes^2 nTaps];  x;  ref
// output (binary): sigOut (total, nModes) complex128, H (nModes^2, nTaps) complex128, errSq (nModes, total) float64;
// stdout: the seconds the loops took, without reading and writing the files (tools/bench_eq.py's CPU comparator), then the
// header's chunk_symbols and coeffs_per_lane for the geometry (the chunking itself is not emulated; tests/test_eq_shapes_emu.py
// holds the two numbers to the rows' literals)
// usage: emu_eq --nlms-scale <sum of squares as a hexadecimal float> ...   prints nlms_scale of each, as a hexadecimal float
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "eq_kernels.h"

using namespace ssf::eqk;

static void read_or_die(void *dst, size_t bytes, FILE *f) {
    if (bytes && std::fread(dst, 1, bytes, f) != bytes) {
        std::fprintf(stderr, "emu_eq: short input\n");
        std::exit(2);
    }
}

struct Problem {
    long long n, total, nref;
    int nModes, nTaps, SpS, dtype, rdtype, M, nRad;
    double Rcma;
    std::vector<double> tab, rad;
    std::vector<char> x, ref;
};

// one output mode over one stretch of symbols: what a wave of k_eq_serial<R> does
template <int R>
static void serial(const Problem &p, int k, const Seg &sg, Cplx *H, Cplx *y, double *esq) {
    const int nModes = p.nModes, nTaps = p.nTaps, Lpad = nTaps / 2;
    Cplx h[kWave][R];
    int mode[kWave][R], tap[kWave][R];
    bool has[kWave][R];
    for (int l = 0; l < kWave; ++l)
        for (int r = 0; r < R; ++r) {
            has[l][r] = lane_coeff(l, r, nModes, nTaps, mode[l][r], tap[l][r]);
            h[l][r] = has[l][r] ? H[(long long)(k + mode[l][r] * nModes) * nTaps + tap[l][r]] : Cplx{0.0, 0.0};
        }
    for (int rep = 0; rep < sg.reps; ++rep)
        for (long long i = sg.start; i < sg.start + sg.len; ++i) {
            Cplx x[kWave][R];
            double vr[kWave], vi[kWave], pw[kMaxModes][kWave], scl[kMaxModes] = {1.0, 1.0, 1.0, 1.0};
            for (int l = 0; l < kWave; ++l) {
                for (int r = 0; r < R; ++r)
                    x[l][r] = has[l][r] ? padded(p.dtype, p.x.data(), p.n, nModes, Lpad, i * p.SpS + tap[l][r], mode[l][r]) : Cplx{0.0, 0.0};
                lane_output<R>(h[l], x[l], vr[l], vi[l]);
                double q[kMaxModes];
                lane_power<R>(x[l], mode[l], q);
                for (int m = 0; m < kMaxModes; ++m) pw[m][l] = q[m];
            }
            butterfly_sum(vr), butterfly_sum(vi);
            const double yr = vr[0], yi = vi[0];
            Cplx rf{0.0, 0.0};
            if (sg.alg == kNlms || sg.alg == kDaRde) load(p.rdtype, p.ref.data(), i * nModes + k, rf.re, rf.im);
            Err e;
            if (sg.alg == kNlms) {
                for (int m = 0; m < nModes; ++m) {
                    butterfly_sum(pw[m]);
                    scl[m] = nlms_scale(pw[m][0]);
                }
                e = err_linear(rf.re, rf.im, yr, yi);
            } else if (sg.alg == kDdLms || sg.alg == kRde) {
                const bool points = sg.alg == kDdLms;
                const int cnt = points ? p.M : p.nRad;
                const double ay = std::sqrt(yr * yr + yi * yi);
                double d[kWave];
                int bi[kWave];
                for (int l = 0; l < kWave; ++l) {
                    d[l] = INFINITY, bi[l] = points ? kMaxM : kMaxRadii;
                    for (int m = l; m < cnt; m += kWave)
                        argmin_merge(d[l], bi[l], points ? dist_point(p.tab[2 * m], p.tab[2 * m + 1], yr, yi) : dist_radius(p.rad[m], ay), m);
                }
                butterfly_argmin(d, bi);
                e = points ? err_linear(p.tab[2 * bi[0]], p.tab[2 * bi[0] + 1], yr, yi) : err_radius(p.rad[bi[0]] * p.rad[bi[0]], yr, yi);
            } else if (sg.alg == kDaRde) {
                e = err_radius(rf.re * rf.re + rf.im * rf.im, yr, yi);
            } else {
                e = err_radius(p.Rcma, yr, yi);
            }
            const double wr = sg.mu * e.gr, wi = sg.mu * e.gi;
            for (int l = 0; l < kWave; ++l)
                for (int r = 0; r < R; ++r) {
                    const double s = scl[mode[l][r]];
                    update(h[l][r], wr, wi, sg.alg == kNlms ? x[l][r].re * s : x[l][r].re, sg.alg == kNlms ? x[l][r].im * s : x[l][r].im);
                }
            y[i * nModes + k] = Cplx{yr, yi};
            esq[(long long)k * p.total + i] = e.esq;
        }
    for (int l = 0; l < kWave; ++l)
        for (int r = 0; r < R; ++r)
            if (has[l][r]) H[(long long)(k + mode[l][r] * nModes) * nTaps + tap[l][r]] = h[l][r];
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "--nlms-scale") {       // nlms_scale of every further argument, bit for bit (%a)
        for (int i = 2; i < argc; ++i) std::printf("%a\n", nlms_scale(std::strtod(argv[i], nullptr)));
        return 0;
    }
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[12];
    Problem p;
    read_or_die(h, sizeof(h), f);
    read_or_die(&p.Rcma, 8, f);
    p.n = h[0], p.total = h[1], p.nref = h[2];
    p.nModes = (int)h[3], p.nTaps = (int)h[4], p.SpS = (int)h[5], p.dtype = (int)h[6], p.rdtype = (int)h[7];
    const int nStages = (int)h[8], numIter = (int)h[9];
    p.M = (int)h[10], p.nRad = (int)h[11];
    std::vector<Seg> segs;
    long long start = 0;
    for (int s = 0; s < nStages; ++s) {
        int64_t la[2];
        double mu;
        read_or_die(la, sizeof(la), f);
        read_or_die(&mu, 8, f);
        segs.push_back(Seg{start, (long long)la[0], (int)la[1], s == 0 ? numIter : 1, mu});
        start += la[0];
    }
    p.tab.resize(2 * (size_t)p.M), p.rad.resize(p.nRad);
    read_or_die(p.tab.data(), p.tab.size() * 8, f);
    read_or_die(p.rad.data(), p.rad.size() * 8, f);
    std::vector<Cplx> H((size_t)p.nModes * p.nModes * p.nTaps), y((size_t)p.total * p.nModes, Cplx{0.0, 0.0});
    std::vector<double> esq((size_t)p.total * p.nModes, 0.0);
    read_or_die(H.data(), H.size() * 16, f);
    p.x.resize((size_t)p.n * p.nModes * (p.dtype == ssf::mk::kC128 ? 16 : 8));
    read_or_die(p.x.data(), p.x.size(), f);
    p.ref.resize((size_t)p.nref * p.nModes * (p.rdtype == ssf::mk::kC128 ? 16 : 8));
    read_or_die(p.ref.data(), p.ref.size(), f);
    std::fclose(f);

    const int R = coeffs_per_lane(p.nModes, p.nTaps);
    const auto t0 = std::chrono::steady_clock::now();
    for (const Seg &sg : segs) {
        if (sg.alg == kStatic) {
            for (long long i = sg.start; i < sg.start + sg.len; ++i)
                for (int k = 0; k < p.nModes; ++k)
                    y[i * p.nModes + k] = static_output(H.data(), p.dtype, p.x.data(), p.n, p.nModes, p.nTaps, p.SpS, p.nTaps / 2, i, k);
            continue;
        }
        for (int k = 0; k < p.nModes; ++k) {
            if (R == 1) serial<1>(p, k, sg, H.data(), y.data(), esq.data());
            else if (R == 2) serial<2>(p, k, sg, H.data(), y.data(), esq.data());
            else serial<4>(p, k, sg, H.data(), y.data(), esq.data());
        }
    }
    std::printf("loop_s %.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    std::printf("chunk %d coeffs_per_lane %d\n", chunk_symbols(p.nModes, p.nTaps, p.SpS), R);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(y.data(), 16, y.size(), o);
    std::fwrite(H.data(), 16, H.size(), o);
    std::fwrite(esq.data(), 8, esq.size(), o);
    std::fclose(o);
    return 0;
}
