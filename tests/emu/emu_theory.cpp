// emu_theory.cpp -- the bodies of opticommpy_amd/csrc/theory_kernels.h walked on the host (g++, no GPU) in the layout of the
// kernels of engine_theory.hip: k_theory_mi's tiles of 256 nodes with one node per lane, the wave's shuffle tree and the
// ((w0 + w1) + w2) + w3 of block_reduce.h, then the tiles and the points in k_theory_fin's order; k_calc_mi's grid-stride lanes.
// tests/test_theory_emu.py compiles this file and runs it against the fixtures and the shape rows.
//
// usage: emu_theory <input file> <output file>
//   mode 0: int64 {0, M, nS, nPts};  table[2M], px[M], sigma[nS] doubles;  int64 points[nPts]
//           output: nS values of MI -- or, with nPts > 0, nS x nPts values px_i (sum_t w log2 S - W log2 px_i) of those points
//   mode 1: int64 {1, n, M, dtype};  sigma2, table[2M], px[M] doubles;  rx[n], tx[n] of dtype
//           output: MI
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "theory_kernels.h"

using namespace ssf::tk;
namespace mk = ssf::mk;

constexpr int kBlock = 256, kMaxBlocks = 512;

static void read_or_die(void *dst, size_t bytes, FILE *f) {
    if (bytes && std::fread(dst, 1, bytes, f) != bytes) {
        std::fprintf(stderr, "emu_theory: short input\n");
        std::exit(2);
    }
}

// lane 0 of br::wave_sum_down over v[0 .. 64)
static double wave_sum(double *v) {
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l + o < 64; ++l) v[l] += v[l + o];
    return v[0];
}
// br::block_sum_store of one value per lane of a workgroup
static double block_sum(std::vector<double> &lane) {
    double w[4];
    for (int k = 0; k < 4; ++k) w[k] = wave_sum(lane.data() + 64 * k);
    return ((w[0] + w[1]) + w[2]) + w[3];
}

static int theory(FILE *f, FILE *out, int M, int nS, int nPts) {
    if (M < 1 || M > kMaxM || nS < 1 || nS > kMaxS || nPts < 0 || nPts > M) return 2;
    std::vector<double> tab(2 * (size_t)M), px(M), sigma(nS);
    std::vector<int64_t> pts(nPts);
    read_or_die(tab.data(), tab.size() * 8, f);
    read_or_die(px.data(), px.size() * 8, f);
    read_or_die(sigma.data(), sigma.size() * 8, f);
    read_or_die(pts.data(), pts.size() * 8, f);
    for (int64_t p : pts)
        if (p < 0 || p >= M) return 2;
    std::vector<double> row((size_t)kRow * M), part(2 * (size_t)kTiles), la(kBlock), lw(kBlock), term(M);
    const double H = entropy(px.data(), M);
    for (int s = 0; s < nS; ++s) {
        const int count = nPts ? nPts : M;
        for (int c = 0; c < count; ++c) {
            const int i = nPts ? (int)pts[c] : c;
            for (int j = 0; j < M; ++j) row_entry(tab.data(), px.data(), i, j, sigma[s], row.data() + kRow * j);
            for (int t = 0; t < kTiles; ++t) {
                for (int lane = 0; lane < kBlock; ++lane) {
                    double acc[2] = {0.0, 0.0};
                    const int q = t * kTile + lane;
                    if (q < kNodes) node_body(acc, row.data(), M, q);
                    la[lane] = acc[0], lw[lane] = acc[1];
                }
                part[2 * t] = block_sum(la), part[2 * t + 1] = block_sum(lw);
            }
            term[c] = point_term(part.data(), px[i]);
        }
        if (nPts) {
            std::fwrite(term.data(), 8, nPts, out);
            continue;
        }
        std::vector<double> lane(kBlock, 0.0);                          // k_theory_fin: lane-strided over the points
        for (int l = 0; l < kBlock; ++l)
            for (int i = l; i < M; i += kBlock) lane[l] += term[i];
        const double mi = H - block_sum(lane);
        std::fwrite(&mi, 8, 1, out);
    }
    return 0;
}

static int calc(FILE *f, FILE *out, long long n, int M, int dtype) {
    if (n < 1 || M < 1 || M > kMaxM || dtype < 0 || dtype > 3) return 2;
    double sigma2;
    std::vector<double> tab(2 * (size_t)M), px(M), l2(M);
    read_or_die(&sigma2, 8, f);
    read_or_die(tab.data(), tab.size() * 8, f);
    read_or_die(px.data(), px.size() * 8, f);
    std::vector<char> rx((size_t)n * mk::elem_size(dtype)), tx(rx.size());
    read_or_die(rx.data(), rx.size(), f);
    read_or_die(tx.data(), tx.size(), f);
    for (int m = 0; m < M; ++m) l2[m] = std::log2(px[m]);
    const double ninv = -(1.0 / sigma2);
    const long long nb = std::min<long long>((n + kBlock - 1) / kBlock, kMaxBlocks);
    std::vector<double> part(nb), lane(kBlock);
    for (long long b = 0; b < nb; ++b) {
        for (int l = 0; l < kBlock; ++l) {
            double acc[1] = {0.0};
            for (long long k = b * kBlock + l; k < n; k += nb * kBlock) {
                double rr, ri, tr, ti;
                mk::load(dtype, rx.data(), k, rr, ri);
                mk::load(dtype, tx.data(), k, tr, ti);
                calc_body(acc, tab.data(), px.data(), l2.data(), M, ninv, rr, ri, tr, ti);
            }
            lane[l] = acc[0];
        }
        part[b] = block_sum(lane);
    }
    double v[64] = {0.0};                                               // br::wave_sum_partials
    for (int l = 0; l < 64; ++l)
        for (long long b = l; b < nb; b += 64) v[l] += part[b];
    const double mi = calc_combine(wave_sum(v), n, entropy(px.data(), M));
    std::fwrite(&mi, 8, 1, out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    FILE *out = std::fopen(argv[2], "wb");
    if (!f || !out) return 2;
    int64_t h[4];
    read_or_die(h, sizeof(h), f);
    const int rc = h[0] == 0 ? theory(f, out, (int)h[1], (int)h[2], (int)h[3]) : calc(f, out, h[1], (int)h[2], (int)h[3]);
    std::fclose(f);
    std::fclose(out);
    return rc;
}
