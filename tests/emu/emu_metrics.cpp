// emu_metrics.cpp -- the link-metrics kernel bodies of opticommpy_amd/csrc/metrics_kernels.h looped over the symbols on the host
// (g++, no GPU): the same per-symbol functions and combine steps the gfx950 kernels call, with one running sum per mode where
// the kernels keep one partial per workgroup.  tests/test_metrics_emu.py compiles this file, feeds it a fixture and holds the
// printed results to the bounds of the GPU test.
//
// usage: emu_metrics <input file>
//   int64 n, nModes, dtype, transposed, rotate, M, discard, want (ssf_metrics_want; 32 = hard demodulation of a 1-D sequence)
//   double Es, H;  double raw[2M], norm[2M], px[M];  float w32[M];  rx, then tx unless want is 16 or 32
// output: one line per value, "<name> <mode> <hexfloat>"; for want = 32 one line "bits" followed by the bits
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "metrics_kernels.h"

using namespace ssf::mk;

static void read_or_die(void *dst, size_t bytes, FILE *f) {
    if (bytes && std::fread(dst, 1, bytes, f) != bytes) {
        std::fprintf(stderr, "emu_metrics: short input\n");
        std::exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[8];
    double eh[2];
    read_or_die(h, sizeof(h), f);
    read_or_die(eh, sizeof(eh), f);
    const long long n = h[0], discard = h[6];
    const int nModes = (int)h[1], dtype = (int)h[2], transposed = (int)h[3], rotate = (int)h[4], M = (int)h[5], want = (int)h[7];
    const double Es = eh[0], H = eh[1], sqrtEs = std::sqrt(Es);
    std::vector<double> raw(2 * M), norm(2 * M), px(M), log2px(M);
    std::vector<float> w32(M);
    read_or_die(raw.data(), raw.size() * 8, f);
    read_or_die(norm.data(), norm.size() * 8, f);
    read_or_die(px.data(), px.size() * 8, f);
    read_or_die(w32.data(), w32.size() * 4, f);
    for (int m = 0; m < M; ++m) log2px[m] = std::log2(px[m]);
    const size_t esize = dtype == kC128 ? 16 : (dtype == kF32 ? 4 : 8);
    const bool has_tx = !(want == kWantEvmBlind || want == 32);
    std::vector<char> rx((size_t)n * nModes * esize), tx(has_tx ? rx.size() : 0);
    read_or_die(rx.data(), rx.size(), f);
    read_or_die(tx.data(), tx.size(), f);
    std::fclose(f);
    int bits = 0;
    while ((1 << bits) < M) ++bits;

    if (want == 32) {
        std::printf("bits");
        for (long long i = 0; i < n; ++i) {
            double rr, ri;
            load(dtype, rx.data(), i, rr, ri);
            const int m = nearest(raw.data(), M, rr, ri);
            for (int j = 0; j < bits; ++j) std::printf(" %d", (m >> (bits - 1 - j)) & 1);
        }
        std::printf("\n");
        return 0;
    }

    const long long n0 = discard, ne = n - 2 * discard;
    const long long sn = transposed ? 1 : nModes, sm = transposed ? n : 1;
    std::vector<double> stat(nModes * kStatN, 0.0), scal(nModes * kScalN, 0.0), res(nModes * kResN, 0.0);
    for (int k = 0; k < nModes; ++k)
        for (long long i = 0; i < ne; ++i) {
            const long long off = (n0 + i) * sn + k * sm;
            double rr, ri, tr = 0.0, ti = 0.0;
            load(dtype, rx.data(), off, rr, ri);
            if (has_tx) load(dtype, tx.data(), off, tr, ti);
            stats_body(&stat[k * kStatN], rotate != 0, has_tx, rr, ri, tr, ti);
        }
    stats_combine(stat.data(), nModes, ne, rotate != 0, has_tx, scal.data());

    if (want == kWantEvmBlind) {
        std::vector<long long> starts(pw_leaves(ne, nullptr) + 1);
        const long long nleaf = pw_leaves(ne, starts.data());
        starts[nleaf] = ne;
        for (int k = 0; k < nModes; ++k) {
            std::vector<int32_t> idx(ne);
            double acc[1] = {0.0};
            for (long long i = 0; i < ne; ++i) {
                double rr, ri;
                load(dtype, rx.data(), (n0 + i) * sn + k * sm, rr, ri);
                idx[i] = blind_body(acc, scal[k * kScalN + 6], norm.data(), M, rr, ri);
            }
            std::vector<float> leaf(nleaf);
            for (long long t = 0; t < nleaf; ++t) leaf[t] = pw_leaf(w32.data(), idx.data() + starts[t], starts[t + 1] - starts[t]);
            PwFrame stk[64];
            const float s32 = pw_combine(leaf.data(), ne, stk);
            const float mean32 = (float)((double)s32 / (double)ne);
            std::printf("EVM %d %a\n", k, (acc[0] / (double)ne) / (double)mean32);
        }
        return 0;
    }

    for (int k = 0; k < nModes; ++k) {
        double acc[kDecN] = {0.0};
        for (long long i = 0; i < ne; ++i) {
            const long long off = (n0 + i) * sn + k * sm;
            double rr, ri, tr, ti;
            load(dtype, rx.data(), off, rr, ri);
            load(dtype, tx.data(), off, tr, ti);
            decide_body(acc, &scal[k * kScalN], raw.data(), M, sqrtEs, want, rr, ri, tr, ti);
        }
        decide_combine(acc, ne, bits, &scal[k * kScalN], &res[k * kResN]);
    }
    if (want & (kWantGmi | kWantMi))
        for (int k = 0; k < nModes; ++k) {
            double acc[kSoftN] = {0.0};
            for (long long i = 0; i < ne; ++i) {
                const long long off = (n0 + i) * sn + k * sm;
                double rr, ri, tr, ti;
                load(dtype, rx.data(), off, rr, ri);
                load(dtype, tx.data(), off, tr, ti);
                SoftDispatch<1>::run(bits, acc, &scal[k * kScalN], raw.data(), norm.data(), px.data(), log2px.data(), M, sqrtEs, rr, ri,
                                     tr, ti);
            }
            soft_combine(acc, ne, H, &res[k * kResN]);
        }
    const char *names[7] = {"BER", "SER", "SNR", "GMI", "NGMI", "MI", "EVM"};
    for (int k = 0; k < nModes; ++k)
        for (int v = 0; v < 7; ++v) std::printf("%s %d %a\n", names[v], k, res[k * kResN + v]);
    return 0;
}
