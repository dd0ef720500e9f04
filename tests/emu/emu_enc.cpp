// emu_enc.cpp -- the encoder kernels of engine_enc.hip without a GPU (test-only): includes opticommpy_amd/csrc/enc_kernels.h, the
// per-lane bodies the gfx950 kernels call, and walks them with g++ in the engine's tiling -- workgroups of 256 lanes in waves of 64,
// a wave's ballot built from its lanes' bits, LDS as an array per workgroup.
//   emu_enc enc in.bin out.bin    int32 header [form, k, rows, copy, nnz, N, n, transposed], then (dense) rows x W uint64 words or
//                                 (sparse) rows + 1 and nnz int32, then the k N message bytes;  out: n N bytes
//   emu_enc mod in.bin out.bin    int32 header [M, b], int64 nsymb, 2 M doubles, nsymb b bytes;  out: 2 nsymb doubles
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "enc_kernels.h"

using namespace ssf::enc;

static void need(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "emu_enc: %s\n", what);
        std::exit(2);
    }
}

template <class T> static void rd(FILE *f, T *p, size_t n) { need(n == 0 || std::fread(p, sizeof(T), n, f) == n, "short input"); }

struct Args {
    const uint64_t *P;
    const int *ptr, *idx;
    int k, rows, W, copy;
    const unsigned char *in;
    unsigned char *out;
    int N, n, transposed;
};

// one wave's ballot: bit l is lane l's value
template <class F> static uint64_t ballot(F bit_of_lane) {
    uint64_t w = 0;
    for (int l = 0; l < kWave; ++l) w |= (uint64_t)(bit_of_lane(l) & 1u) << l;
    return w;
}

static void wg_dense(const Args &a, int bx, int by) {
    std::vector<uint64_t> s_msg((size_t)kTile * a.W);
    const int c0 = by * kTile;
    for (int wave = 0; wave < kBlock / kWave; ++wave)
        for (int p = wave; p < kTile * a.W; p += kBlock / kWave) {
            const int t = p / a.W, w = p - t * a.W;
            s_msg[p] = ballot([&](int lane) { return load_bit(a.in, w * kWave + lane, c0 + t, a.k, a.N, a.transposed); });
        }
    const int nt = a.N - c0 < kTile ? a.N - c0 : kTile;
    for (int tid = 0; tid < kBlock; ++tid) {
        if (a.copy && bx == 0)
            for (int j = tid; j < a.k && j < a.n; j += kBlock)
                for (int t = 0; t < nt; ++t)
                    a.out[user_index(j, c0 + t, a.n, a.N, a.transposed)] = (unsigned char)word_bit(s_msg.data() + (size_t)t * a.W, j);
        const int i = bx * kRows + tid;
        const int row = (a.copy ? a.k : 0) + i;
        if (i >= a.rows || row >= a.n) continue;
        uint64_t acc[kTile];
        dense_row(a.P + (size_t)i * a.W, s_msg.data(), a.W, acc);
        for (int t = 0; t < nt; ++t) a.out[user_index(row, c0 + t, a.n, a.N, a.transposed)] = (unsigned char)parity64(acc[t]);
    }
}

static void wg_accum(const Args &a, int c) {
    std::vector<uint64_t> s_msg((size_t)a.W);
    const int Wm = (a.rows + kWave - 1) / kWave;
    std::vector<uint64_t> s_par((size_t)Wm, ~0ull);
    std::vector<unsigned char> s_cin((size_t)Wm, 0xEE);
    for (int w = 0; w < a.W; ++w) s_msg[w] = ballot([&](int lane) { return load_bit(a.in, w * kWave + lane, c, a.k, a.N, a.transposed); });
    for (int j = 0; j < a.k && j < a.n; ++j) a.out[user_index(j, c, a.n, a.N, a.transposed)] = (unsigned char)word_bit(s_msg.data(), j);
    for (int base = 0; base < a.rows; base += kSpan)                    // the parities, a span of 256 at a time: four ballots
        for (int wave = 0; wave < kBlock / kWave; ++wave) {
            const uint64_t word = ballot([&](int lane) {
                const int i = base + wave * kWave + lane;
                return i < a.rows ? row_parity(s_msg.data(), a.idx, a.ptr[i], a.ptr[i + 1]) : 0u;
            });
            if (base + wave * kWave < a.rows) s_par[base / kWave + wave] = word;
        }
    unsigned carry = 0;                                                 // wave 0: the carry into every ballot, 64 ballots at a time
    for (int s = 0; s < Wm; s += kWave) {
        const uint64_t word = ballot([&](int lane) { return s + lane < Wm ? scan_total(s_par[s + lane]) : 0u; });
        for (int lane = 0; lane < kWave; ++lane)
            if (s + lane < Wm) s_cin[s + lane] = (unsigned char)(scan_lane(word, lane) ^ scan_total(s_par[s + lane]) ^ carry);
        carry ^= scan_total(word);
    }
    for (int i = 0; i < a.rows && a.k + i < a.n; ++i)
        a.out[user_index(a.k + i, c, a.n, a.N, a.transposed)] = (unsigned char)(scan_lane(s_par[i / kWave], i & (kWave - 1)) ^ s_cin[i / kWave]);
}

static int run_enc(FILE *fi, FILE *fo) {
    int h[8];
    rd(fi, h, 8);
    const int form = h[0], k = h[1], rows = h[2], copy = h[3], nnz = h[4], N = h[5], n = h[6], transposed = h[7];
    const int W = (k + kWave - 1) / kWave;
    need(k >= 1 && rows >= 1 && N >= 1 && n >= 1 && n <= rows + (copy ? k : 0), "bad header");
    need(W <= (form == kDense ? kMaxWordsDense : kMaxWordsSparse), "k beyond the engine's limit");
    need(form == kDense || rows <= kMaxChecksSparse, "m beyond the engine's limit");
    std::vector<uint64_t> P;
    std::vector<int> ptr, idx;
    if (form == kDense) {
        P.resize((size_t)rows * W);
        rd(fi, P.data(), P.size());
    } else {
        ptr.resize((size_t)rows + 1), idx.resize((size_t)nnz + 1);
        rd(fi, ptr.data(), (size_t)rows + 1);
        rd(fi, idx.data(), (size_t)nnz);
        need(ptr[0] == 0 && ptr[rows] == nnz, "bad CSR");
        for (int e = 0; e < nnz; ++e) need(idx[e] >= 0 && idx[e] < k, "index out of range");
    }
    std::vector<unsigned char> in((size_t)k * N), out((size_t)n * N, 0xEE);
    rd(fi, in.data(), in.size());
    Args a{P.data(), ptr.data(), idx.data(), k, rows, W, form == kSparse || copy, in.data(), out.data(), N, n, transposed};
    if (form == kDense) {
        for (int by = 0; by < (N + kTile - 1) / kTile; ++by)
            for (int bx = 0; bx < (rows + kRows - 1) / kRows; ++bx) wg_dense(a, bx, by);
    } else {
        for (int c = 0; c < N; ++c) wg_accum(a, c);
    }
    need(std::fwrite(out.data(), 1, out.size(), fo) == out.size(), "short output");
    return 0;
}

static int run_mod(FILE *fi, FILE *fo) {
    int h[2];
    long long nsymb;
    rd(fi, h, 2);
    rd(fi, &nsymb, 1);
    const int M = h[0], b = h[1];
    need(M >= 2 && M <= kModMaxM && (1 << b) == M && nsymb >= 1, "bad header");
    std::vector<double> tab(2 * (size_t)M), out(2 * (size_t)nsymb);
    std::vector<unsigned char> bits((size_t)nsymb * b);
    rd(fi, tab.data(), tab.size());
    rd(fi, bits.data(), bits.size());
    for (long long i = 0; i < nsymb; ++i) {
        const int s = symbol_index(bits.data(), i, b);
        out[2 * i] = tab[2 * s], out[2 * i + 1] = tab[2 * s + 1];
    }
    need(std::fwrite(out.data(), sizeof(double), out.size(), fo) == out.size(), "short output");
    return 0;
}

int main(int argc, char **argv) {
    need(argc == 4, "usage: emu_enc enc|mod in.bin out.bin");
    FILE *fi = std::fopen(argv[2], "rb"), *fo = std::fopen(argv[3], "wb");
    need(fi && fo, "cannot open files");
    const int rc = argv[1][0] == 'e' ? run_enc(fi, fo) : run_mod(fi, fo);
    std::fclose(fi);
    std::fclose(fo);
    return rc;
}
