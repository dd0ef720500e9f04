// emu_clock.cpp -- the bodies of opticommpy_amd/csrc/clock_kernels.h walked on the CPU in the launch geometry of engine_clock.hip:
// the grid-stride element-wise passes, the two-launch min/max, the clock recovery's chunked input window and output ring (one
// "wavefront" per column) and the two launches of the clock drift.  Built by tests/clock_cases.py:build_emu with g++ (no
// contraction of multiply-adds: x86-64 without -march has none).
//   emu_clock const                           prints kChunk kWin kRing kFlush kLag kBlock kMaxBlocks
//   emu_clock <op> in.bin out.bin             op: chain | quantize | clip | minmax | gardner | drift
// in.bin: 16 int64, 8 float64, then the arrays the op reads (tests/clock_cases.py writes them); out.bin: the op's arrays.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "clock_kernels.h"

using namespace ssf;
using namespace ssf::ck;

static std::vector<char> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> buf(sz > 0 ? sz : 1);
    if (sz > 0 && fread(buf.data(), 1, sz, f) != (size_t)sz) { perror("read"); exit(2); }
    fclose(f);
    return buf;
}
static void write_out(FILE *f, const void *p, size_t bytes) {
    if (bytes && fwrite(p, 1, bytes, f) != bytes) { perror("write"); exit(2); }
}
static long long blocks_for(long long count) {
    const long long nb = (count + kBlock - 1) / kBlock;
    return nb < 1 ? 1 : nb < kMaxBlocks ? nb : kMaxBlocks;
}
static void store_element(int dtype, bool as_double, void *out, long long q, double re, double im) {
    if (is_complex(dtype)) {
        if (as_double || dtype == mk::kC128) ((mk::Cplx *)out)[q] = mk::Cplx{re, im};
        else ((mk::CplxF *)out)[q] = mk::CplxF{(float)re, (float)im};
    } else {
        if (as_double || dtype == mk::kF64) ((double *)out)[q] = re;
        else ((float *)out)[q] = (float)re;
    }
}

// one column of the clock recovery as k_gardner walks it
static void gardner_column(int dtype, const void *x, long long n, long long nSamples, long long Ln, int nModes, int col, int nyquist,
                           double kp, double ki, mk::CplxF *out, double *tv, long long *last_n, int *status_out) {
    std::vector<mk::Cplx> xs(kWin), pre(kWin);
    std::vector<mk::CplxF> ring(kRing, mk::CplxF{0.0f, 0.0f});
    std::vector<double> tring(kRing, 0.0);
    const long long kMask = kRing - 1;
    auto fetch = [&](long long chunk) {
        for (int idx = 0; idx < kWin; ++idx) pre[idx] = padded(dtype, x, n, nModes, col, chunk * kChunk + idx);
    };
    auto to_lds = [&]() { xs = pre; };
    auto flush = [&](long long f) {
        for (int lane = 0; lane < kWave; ++lane) {
            const long long q = f + lane;
            if (q < Ln) out[q * nModes + col] = ring[q & kMask], tv[q * nModes + col] = tring[q & kMask];
            ring[q & kMask] = mk::CplxF{0.0f, 0.0f}, tring[q & kMask] = 0.0;
        }
    };
    double t_nco = 0.0, intPart = 0.0;
    long long nn = 2, m = 2, chunk = 0, f = 0;
    int status = kGardnerOk;
    fetch(0);
    to_lds();
    fetch(1);
    mk::Cplx w[5];
    for (int i = 0; i < 5; ++i) w[i] = xs[i];
    while (loop_runs(nn, m, Ln, nSamples)) {
        const mk::CplxF pa = ring[(nn - 2) & kMask], pb = ring[(nn - 1) & kMask];
        const mk::CplxF y = interpolate(w, t_nco);
        ring[nn & kMask] = y;
        if ((nn & 1) == 0) loop_filter(t_nco, intPart, nyquist ? ted_nyquist(pa, pb, y) : ted_gardner(pa, pb, y), kp, ki);
        const int step = nco_gap(t_nco);
        nn += step;
        if (f > 0 && nn < f + 2) {
            status = kGardnerBackrun;
            break;
        }
        if (nn < Ln) tring[nn & kMask] = t_nco;
        if (step > 0) {
            ++m;
            if (m >= 2 + (chunk + 1) * kChunk) {
                ++chunk;
                to_lds();
                fetch(chunk + 1);
                for (int i = 0; i < 5; ++i) w[i] = xs[i];
            } else {
                w[0] = w[1], w[1] = w[2], w[2] = w[3], w[3] = w[4];
                w[4] = xs[(int)(m + 2 - chunk * kChunk)];
            }
        }
        while (nn >= f + kLag) flush(f), f += kFlush;
    }
    for (int r = 0; r < kRing / kFlush; ++r) flush(f + r * kFlush);
    last_n[col] = nn, status_out[col] = status;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "const") {
        printf("%d %d %d %d %d %d %d\n", kChunk, kWin, kRing, kFlush, kLag, kBlock, kMaxBlocks);
        return 0;
    }
    if (argc != 4) {
        fprintf(stderr, "usage: emu_clock const | emu_clock <op> in.bin out.bin\n");
        return 2;
    }
    const std::string op = argv[1];
    std::vector<char> in = read_file(argv[2]);
    const long long *I = (const long long *)in.data();
    const double *D = (const double *)(in.data() + 16 * sizeof(long long));
    const char *payload = in.data() + 16 * sizeof(long long) + 8 * sizeof(double);
    FILE *fo = fopen(argv[3], "wb");
    if (!fo) { perror(argv[3]); return 2; }

    if (op == "chain") {
        // I: n_in n_out ncols dtype form clip quantize qlevels has_tre has_tim; D: inTs outTs lo hi qmin qdelta
        Chain c{I[0], I[1], (int)I[2], (int)I[3], (int)I[4], (int)I[5], (int)I[6], D[0], D[1], D[2], D[3], D[4], D[5], I[7], 1.0 / D[0]};
        const void *x = payload;
        const char *p = payload + (size_t)c.n_in * c.ncols * mk::elem_size(c.dtype);
        const double *t_re = I[8] ? (const double *)p : nullptr;
        if (I[8]) p += (size_t)c.n_out * sizeof(double);
        const double *t_im = I[9] ? (const double *)p : nullptr;
        const long long count = c.n_out * c.ncols;
        const size_t esz = c.quantize ? (is_complex(c.dtype) ? 16 : 8) : mk::elem_size(c.dtype);
        std::vector<char> out((size_t)count * esz + 1);
        const long long nb = blocks_for(count);
        for (long long b = 0; b < nb; ++b)
            for (int th = 0; th < kBlock; ++th)
                for (long long q = b * kBlock + th; q < count; q += nb * kBlock) {
                    double re, im;
                    chain_element(c, x, t_re, t_im, q, re, im);
                    store_element(c.dtype, c.quantize != 0, out.data(), q, re, im);
                }
        write_out(fo, out.data(), (size_t)count * esz);
    } else if (op == "quantize") {
        // I: count dtype qlevels; D: qmin qdelta   (a complex dtype: the real part, stride 2)
        const long long count = I[0];
        const int dtype = (int)I[1], stride = is_complex(dtype) ? 2 : 1;
        std::vector<double> out(count + 1);
        const long long nb = blocks_for(count);
        for (long long b = 0; b < nb; ++b)
            for (int th = 0; th < kBlock; ++th)
                for (long long q = b * kBlock + th; q < count; q += nb * kBlock) {
                    const double v = is_single(dtype) ? (double)((const float *)payload)[q * stride] : ((const double *)payload)[q * stride];
                    out[q] = quantize(v, D[0], D[1], I[2]);
                }
        write_out(fo, out.data(), (size_t)count * sizeof(double));
    } else if (op == "clip") {
        // I: count dtype; D: lo hi
        const long long count = I[0];
        const int dtype = (int)I[1];
        std::vector<char> out((size_t)count * mk::elem_size(dtype) + 1);
        for (long long q = 0; q < count; ++q) {
            double re, im;
            mk::load(dtype, payload, q, re, im);
            if (is_complex(dtype)) clip_complex(re, im, D[0], D[1]);
            else re = clip_real(re, D[0], D[1]);
            store_element(dtype, false, out.data(), q, re, im);
        }
        write_out(fo, out.data(), (size_t)count * mk::elem_size(dtype));
    } else if (op == "minmax") {
        // I: count dtype: the partial pair of every workgroup, then their fold
        const int dtype = (int)I[1];
        const long long reals = I[0] * (is_complex(dtype) ? 2 : 1), nb = blocks_for(reals);
        std::vector<double> part(2 * nb);
        for (long long b = 0; b < nb; ++b) {
            double mn = INFINITY, mx = -INFINITY;
            for (int th = 0; th < kBlock; ++th)
                for (long long q = b * kBlock + th; q < reals; q += nb * kBlock) {
                    const double v = is_single(dtype) ? (double)((const float *)payload)[q] : ((const double *)payload)[q];
                    mn = v < mn ? v : mn, mx = v > mx ? v : mx;
                }
            part[2 * b] = mn, part[2 * b + 1] = mx;
        }
        double res[2] = {INFINITY, -INFINITY};
        for (long long b = 0; b < nb; ++b) res[0] = part[2 * b] < res[0] ? part[2 * b] : res[0], res[1] = part[2 * b + 1] > res[1] ? part[2 * b + 1] : res[1];
        write_out(fo, res, sizeof(res));
    } else if (op == "gardner") {
        // I: n lpad Ln nModes dtype nyquist; D: kp ki
        const long long n = I[0], lpad = I[1], Ln = I[2];
        const int nModes = (int)I[3], dtype = (int)I[4];
        std::vector<mk::CplxF> out((size_t)Ln * nModes + 1, mk::CplxF{0.0f, 0.0f});
        std::vector<double> tv((size_t)Ln * nModes + 1, 0.0);
        std::vector<long long> last(nModes);
        std::vector<int> status(nModes);
        const auto t0 = std::chrono::steady_clock::now();
        for (int col = 0; col < nModes; ++col)
            gardner_column(dtype, payload, n, n + lpad, Ln, nModes, col, (int)I[5], D[0], D[1], out.data(), tv.data(), last.data(), status.data());
        if (getenv("EMU_CLOCK_TIME"))            // tools/bench_clock.py: the loop alone, without the files
            printf("loop_seconds %.9f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        write_out(fo, out.data(), (size_t)Ln * nModes * sizeof(mk::CplxF));
        write_out(fo, tv.data(), (size_t)Ln * nModes * sizeof(double));
        write_out(fo, last.data(), (size_t)nModes * sizeof(long long));
        write_out(fo, status.data(), (size_t)nModes * sizeof(int));
    } else if (op == "drift") {
        // I: n ncols per_column
        const long long n = I[0];
        const int ncols = (int)I[1], per_column = (int)I[2];
        const double *t = (const double *)payload;
        std::vector<double> sums(ncols), ppm(ncols);
        for (int col = 0; col < ncols; ++col) {          // k_drift_sum: a lane's rows in order, the lanes by block_reduce.h's tree
            double lane[kBlock];
            for (int th = 0; th < kBlock; ++th) {
                lane[th] = 0.0;
                for (long long r = th; r < n; r += kBlock) lane[th] += t[r * ncols + col];
            }
            double wave[kBlock / 64];
            for (int wv = 0; wv < kBlock / 64; ++wv) {
                double v[64];
                for (int l = 0; l < 64; ++l) v[l] = lane[wv * 64 + l];
                for (int o = 32; o > 0; o >>= 1)
                    for (int l = 0; l < 64; ++l) v[l] = v[l] + (l + o < 64 ? v[l + o] : v[l]);
                wave[wv] = v[0];
            }
            sums[col] = ((wave[0] + wave[1]) + wave[2]) + wave[3];
        }
        double total = 0.0;
        for (int k = 0; k < ncols; ++k) total += sums[k];
        for (int col = 0; col < ncols; ++col) {
            const double mean = per_column ? sums[col] / (double)n : total / (double)(n * ncols);
            long long count = 0, first = n, last = -1;
            for (int th = 0; th < kBlock; ++th)
                for (long long i = 1 + th; i + 1 < n - 1; i += kBlock) {
                    long long at;
                    if (drift_peak(t, n, ncols, col, mean, i, at)) ++count, first = at < first ? at : first, last = at > last ? at : last;
                }
            ppm[col] = drift_ppm(count, first, last, mean);
        }
        write_out(fo, ppm.data(), (size_t)ncols * sizeof(double));
    } else {
        fprintf(stderr, "unknown op %s\n", op.c_str());
        return 2;
    }
    fclose(fo);
    return 0;
}
