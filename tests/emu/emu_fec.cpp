// emu_fec.cpp -- the soft-decision FEC kernels without a GPU: includes opticommpy_amd/csrc/fec_kernels.h, the text the gfx950
// kernels of engine_fec.hip run, and walks it over nodes and codewords as the two engines do.
//   emu_fec ldpc in.bin out.bin     in:  int64 m, n, E, n_, ncw, maxIter, alg, prec, in_dtype, transposed, engine (1 LDS, 2 global)
//                                        int32 check_offsets[m + 1], edge_var[E], var_offsets[n + 1], var_edge_indices[E]
//                                        llrs: n_ ncw values of in_dtype in the caller's orientation
//                                   out: posterior (n_ ncw of prec), bits (n_ ncw int8), fail (ncw int8), iter (ncw uint32)
//   emu_fec llr in.bin out.bin      in:  int64 n, dtype, M; double sigma2, table[2 M], px[M]; int32 bitmap[M log2 M]; x
//                                   out: n log2 M doubles
//   emu_fec time in.bin out.bin reps    the ldpc decode repeated, seconds per decode on stdout (the CPU figure of tools/bench_fec.py)
// The LDS walk keeps one codeword's messages in a padded array (fec::Padded) and leaves its loop at convergence; the global walk
// keeps msg[e][cw] for all codewords (fec::Strided) and follows the launches of engine_fec.hip, workgroup by workgroup: k_check
// (parity of the iteration before, then the check update, speculative for a codeword that has just converged), k_var (which
// finds the convergence and freezes the codeword), a last parity pass and k_finish.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fec_kernels.h"
#include "metrics_kernels.h"

using namespace ssf::fec;

namespace {
constexpr int kBlock = 256;

struct Graph {
    int m, n, E;
    std::vector<int> co, ev, vo, ve;
};
struct Job {
    Graph g;
    int n_, ncw, maxIter, alg, prec, in_dtype, transposed, engine;
    std::vector<unsigned char> in;
};

std::vector<unsigned char> slurp(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> b((size_t)sz);
    if (sz && std::fread(b.data(), 1, (size_t)sz, f) != (size_t)sz) std::exit(2);
    std::fclose(f);
    return b;
}

template <class T, int MODE>
void walk_lds(const Job &j, T *out, int8_t *bits, int8_t *fail, uint32_t *iter) {
    const Graph &g = j.g;
    const Padded idx;
    std::vector<T> msg((size_t)Padded::slots(g.E)), llr((size_t)g.n), post((size_t)g.n);
    std::vector<unsigned char> hard((size_t)g.n);
    for (int cw = 0; cw < j.ncw; ++cw) {
        for (int v = 0; v < g.n; ++v) llr[v] = load_llr<T>(j.in.data(), j.in_dtype, v, cw, j.n_, j.ncw, j.transposed);
        for (int e = 0; e < g.E; ++e) msg[idx(e)] = llr[g.ev[e]];
        int it = 0, failed = 1;
        for (; it < j.maxIter; ++it) {
            for (int c = 0; c < g.m; ++c) check_update<T, MODE>(msg.data(), g.co[c], g.co[c + 1], idx);
            for (int v = 0; v < g.n; ++v) var_update<T>(msg.data(), g.ve.data(), g.vo[v], g.vo[v + 1], llr[v], post[v], hard[v], idx);
            int odd = 0;
            for (int c = 0; c < g.m; ++c) odd |= check_parity(hard.data(), g.ev.data(), g.co[c], g.co[c + 1], Plain());
            failed = odd;
            if (!failed) break;
        }
        for (int v = 0; v < j.n_; ++v) {
            const long long o = user_index(v, cw, j.n_, j.ncw, j.transposed);
            out[o] = post[v], bits[o] = (int8_t)hard[v];
        }
        fail[cw] = failed ? 1 : 0;
        iter[cw] = (uint32_t)(failed ? j.maxIter - 1 : it);
    }
}

template <class T, int MODE>
void walk_global(const Job &j, T *out, int8_t *bits, int8_t *fail, uint32_t *iter) {
    const Graph &g = j.g;
    const long long ncw = j.ncw;
    std::vector<T> msg((size_t)ncw * g.E), llr((size_t)ncw * g.n), post((size_t)ncw * g.n);         // codeword-minor: x[i][cw]
    std::vector<unsigned char> hard((size_t)ncw * g.n);
    std::vector<int> unsat((size_t)j.maxIter * ncw, 0), done((size_t)ncw, 0), d_fail((size_t)ncw, 0);
    std::vector<uint32_t> d_iter((size_t)ncw, 0);
    for (long long t = 0; t < (long long)(g.n > g.E ? g.n : g.E) * ncw; ++t) {                         // k_init
        const long long i = t / ncw;
        const int cw = (int)(t % ncw);
        if (i < g.n) llr[(size_t)t] = load_llr<T>(j.in.data(), j.in_dtype, (int)i, cw, j.n_, j.ncw, j.transposed);
        if (i < g.E) msg[(size_t)t] = load_llr<T>(j.in.data(), j.in_dtype, g.ev[i], cw, j.n_, j.ncw, j.transposed);
    }
    auto k_check = [&](int it, int parity_only) {
        const long long total = (long long)g.m * ncw;
        for (long long b0 = 0; b0 < total; b0 += kBlock) {              // one workgroup: kBlock consecutive (check, codeword) pairs
            const long long b1 = b0 + kBlock < total ? b0 + kBlock : total;
            if (it > 0) {
                int s_odd[kBlock] = {0};
                for (long long t = b0; t < b1; ++t) {
                    const int c = (int)(t / ncw), cw = (int)(t % ncw);
                    if (!done[cw] && check_parity(hard.data(), g.ev.data(), g.co[c], g.co[c + 1], Strided{ncw, cw}))
                        s_odd[ncw < kBlock ? cw : (int)(t - b0)] = 1;
                }
                for (long long t = b0; t < b1 && t - b0 < ncw; ++t) {
                    const int cw = (int)(t % ncw);
                    if (!done[cw] && s_odd[ncw < kBlock ? cw : (int)(t - b0)]) unsat[(size_t)(it - 1) * ncw + cw] = 1;
                }
            }
            if (parity_only) continue;
            for (long long t = b0; t < b1; ++t) {
                const int c = (int)(t / ncw), cw = (int)(t % ncw);
                if (!done[cw]) check_update<T, MODE>(msg.data(), g.co[c], g.co[c + 1], Strided{ncw, cw});
            }
        }
    };
    auto k_var = [&](int it) {
        const std::vector<int> was_done = done;                          // (a thread that reads the flag late skips all the same)
        for (long long t = 0; t < (long long)g.n * ncw; ++t) {
            const int v = (int)(t / ncw), cw = (int)(t % ncw);
            if (was_done[cw]) continue;
            if (it > 0 && unsat[(size_t)(it - 1) * ncw + cw] == 0) {
                if (v == 0) done[cw] = 1, d_fail[cw] = 0, d_iter[cw] = (uint32_t)(it - 1);
                continue;
            }
            var_update<T>(msg.data(), g.ve.data(), g.vo[v], g.vo[v + 1], llr[(size_t)t], post[(size_t)t], hard[(size_t)t], Strided{ncw, cw});
        }
    };
    int it = 0;
    for (; it < j.maxIter; ++it) k_check(it, 0), k_var(it);
    k_check(it, 1);
    const int last = it - 1;
    for (int cw = 0; cw < j.ncw; ++cw) {                                 // k_finish
        if (!done[cw]) d_fail[cw] = unsat[(size_t)last * ncw + cw] ? 1 : 0, d_iter[cw] = (uint32_t)last;
        fail[cw] = (int8_t)d_fail[cw], iter[cw] = d_iter[cw];
        for (int v = 0; v < j.n_; ++v) {
            const long long o = user_index(v, cw, j.n_, j.ncw, j.transposed);
            out[o] = post[(size_t)v * ncw + cw], bits[o] = (int8_t)hard[(size_t)v * ncw + cw];
        }
    }
}

template <class T, int MODE>
void walk(const Job &j, void *out, int8_t *bits, int8_t *fail, uint32_t *iter) {
    if (j.engine == kEngineLds) walk_lds<T, MODE>(j, (T *)out, bits, fail, iter);
    else walk_global<T, MODE>(j, (T *)out, bits, fail, iter);
}

template <class T>
void decode(const Job &j, int max_dc, void *out, int8_t *bits, int8_t *fail, uint32_t *iter) {
    const int mode = j.alg == kMSA ? -1 : spa_mode(max_dc);
    if (mode < 0) walk<T, -1>(j, out, bits, fail, iter);
    else if (mode == 8) walk<T, 8>(j, out, bits, fail, iter);
    else if (mode == 32) walk<T, 32>(j, out, bits, fail, iter);
    else walk<T, 0>(j, out, bits, fail, iter);
}

int run_ldpc(const char *inpath, const char *outpath, int reps) {
    const std::vector<unsigned char> raw = slurp(inpath);
    const long long *h = (const long long *)raw.data();
    Job j;
    Graph &g = j.g;
    g.m = (int)h[0], g.n = (int)h[1], g.E = (int)h[2];
    j.n_ = (int)h[3], j.ncw = (int)h[4], j.maxIter = (int)h[5], j.alg = (int)h[6], j.prec = (int)h[7], j.in_dtype = (int)h[8];
    j.transposed = (int)h[9], j.engine = (int)h[10];
    const int *p = (const int *)(h + 11);
    g.co.assign(p, p + g.m + 1), p += g.m + 1;
    g.ev.assign(p, p + g.E), p += g.E;
    g.vo.assign(p, p + g.n + 1), p += g.n + 1;
    g.ve.assign(p, p + g.E), p += g.E;
    const size_t count = (size_t)j.n_ * j.ncw, isz = j.in_dtype == kF64 ? 8 : 4, wsz = j.prec == kF64 ? 8 : 4;
    const unsigned char *in = (const unsigned char *)p;
    if ((size_t)(in - raw.data()) + count * isz != raw.size()) return 3;
    j.in.assign(in, in + count * isz);
    int max_dc = 0;
    for (int c = 0; c < g.m; ++c) max_dc = g.co[c + 1] - g.co[c] > max_dc ? g.co[c + 1] - g.co[c] : max_dc;
    std::vector<unsigned char> out(count * wsz);
    std::vector<int8_t> bits(count), fail((size_t)j.ncw);
    std::vector<uint32_t> iter((size_t)j.ncw);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
        if (j.prec == kF64) decode<double>(j, max_dc, out.data(), bits.data(), fail.data(), iter.data());
        else decode<float>(j, max_dc, out.data(), bits.data(), fail.data(), iter.data());
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (reps > 0) std::printf("%.9g\n", sec / reps);
    FILE *f = std::fopen(outpath, "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 1, out.size(), f);
    std::fwrite(bits.data(), 1, bits.size(), f);
    std::fwrite(fail.data(), 1, fail.size(), f);
    std::fwrite(iter.data(), sizeof(uint32_t), iter.size(), f);
    std::fclose(f);
    return 0;
}

int run_llr(const char *inpath, const char *outpath) {
    const std::vector<unsigned char> raw = slurp(inpath);
    const long long *h = (const long long *)raw.data();
    const long long n = h[0];
    const int dtype = (int)h[1], M = (int)h[2];
    int b = 0;
    while ((1 << b) < M) ++b;
    const double *d = (const double *)(h + 3);
    const double sigma2 = d[0], *tab = d + 1, *px = tab + 2 * M;
    const int *bitmap = (const int *)(px + M);
    const void *x = bitmap + (size_t)M * b;
    std::vector<unsigned> z((size_t)M), o((size_t)M);
    for (int i = 0; i < M; ++i) {                                        // the masks as engine_fec.hip packs them
        z[i] = o[i] = 0;
        for (int k = 0; k < b; ++k) {
            z[i] |= bitmap[(size_t)i * b + k] == 0 ? 1u << k : 0u;
            o[i] |= bitmap[(size_t)i * b + k] == 1 ? 1u << k : 0u;
        }
    }
    std::vector<double> out((size_t)n * b);
    for (long long i = 0; i < n; ++i) {
        double re, im, llr[kMaxBits];
        ssf::mk::load(dtype, x, i, re, im);
        llr_body(re, im, sigma2, M, b, tab, px, z.data(), o.data(), llr);
        for (int k = 0; k < b; ++k) out[(size_t)i * b + k] = llr[k];
    }
    FILE *f = std::fopen(outpath, "wb");
    if (!f) return 2;
    std::fwrite(out.data(), sizeof(double), out.size(), f);
    std::fclose(f);
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) return 1;
    if (!std::strcmp(argv[1], "ldpc")) return run_ldpc(argv[2], argv[3], 0);
    if (!std::strcmp(argv[1], "time") && argc > 4) return run_ldpc(argv[2], argv[3], std::atoi(argv[4]));
    if (!std::strcmp(argv[1], "llr")) return run_llr(argv[2], argv[3]);
    return 1;
}
