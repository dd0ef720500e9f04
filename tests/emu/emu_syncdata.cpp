// emu_syncdata.cpp -- host emulator of engine_syncdata.hip: the bodies of syncdata_kernels.h walked over the kernels' workgroups and
// lanes with g++ (tests/syncdata_cases.py builds and runs it; a stand-alone program, so it can also be built with
// -fsanitize=address,undefined and run directly).
//   in.bin:  int64 head (op first), then the arrays as raw bytes, head and arrays each padded to 16 bytes;  out.bin: float64 values
//   op 0 tile:     head op, n_rx, n_tx, n_pad, modes, SpS, rx_dtype, tx_dtype; rx, tx            -> rx_out, tx_out (complex128)
//   op 1 extract:  head op, n, modes, n_out, cx_out, normalize; x (complex128)                  -> out, kept per column
//   op 2 average:  head op, n, cols, N, dtype; x                                                -> out
//   op 3 bert:     head op, n; Irx (float64), bits (uint8)                                       -> the ten scalars
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "syncdata_kernels.h"

using namespace ssf;
using namespace ssf::sd;

// ---- the order of a launch-wide sum as block_reduce.h takes it (device only, so walked here): lane 0 of a wave's __shfl_down tree,
// ((w0 + w1) + w2) + w3 over the waves, the partials lane-strided by one wave and then the tree
static double tree64(const double *v) {
    double t[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l];
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) t[l] += t[l + o];
    return t[0];
}
static double block_tree(const double *v) { return ((tree64(v) + tree64(v + 64)) + tree64(v + 128)) + tree64(v + 192); }
// a lane-strided sum of nb partials (stride apart) by one wave, then the tree
static double partials_tree(const double *part, long long nb, long long stride) {
    double a[64];
    for (int l = 0; l < 64; ++l) {
        a[l] = 0.0;
        for (long long b = l; b < nb; b += 64) a[l] += part[b * stride];
    }
    return tree64(a);
}

// the workgroup's ranks as engine_syncdata.hip's block_rank takes them: every wave's shuffle scan step by step, the waves' totals,
// then rank_before
static void block_ranks(const int *count, int *before, int &total) {
    int inc[kBlock], wtot[kBlock / 64];
    for (int t = 0; t < kBlock; ++t) inc[t] = count[t];
    for (int o = 1; o < 64; o <<= 1) {
        int nxt[kBlock];
        for (int t = 0; t < kBlock; ++t) {
            const int lane = t & 63;
            nxt[t] = scan_step(inc[t], lane >= o ? inc[t - o] : inc[t], lane, o);       // (__shfl_up below lane o returns the lane's own value)
        }
        for (int t = 0; t < kBlock; ++t) inc[t] = nxt[t];
    }
    for (int w = 0; w < kBlock / 64; ++w) wtot[w] = inc[64 * w + 63];
    for (int t = 0; t < kBlock; ++t) before[t] = rank_before(wtot, kBlock / 64, t >> 6, inc[t], count[t], total);
}

static std::vector<char> read_all(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> b((size_t)sz);
    if (sz && fread(b.data(), 1, (size_t)sz, f) != (size_t)sz) { perror("read"); exit(2); }
    fclose(f);
    return b;
}

static int grid_blocks(long long count, int block, int max_blocks) {
    const long long nb = (count + block - 1) / block;
    return (int)(nb < max_blocks ? nb : max_blocks);
}

static void run_tile(const int64_t *h, const char *data, std::vector<double> &out) {
    const long long nRx = h[1], nTx = h[2], nPad = h[3];
    const int modes = (int)h[4], SpS = (int)h[5], rxd = (int)h[6], txd = (int)h[7];
    const void *rx = data, *tx = data + ((size_t)nRx * modes * mk::elem_size(rxd) + 15) / 16 * 16;
    const long long total = nPad * modes;
    out.assign((size_t)total * 4, 0.0);
    Cplx *rxo = (Cplx *)out.data(), *txo = rxo + total;
    const int nb = grid_blocks(total, kBlock, kElemMaxBlocks);
    for (int b = 0; b < nb; ++b)
        for (int t = 0; t < kBlock; ++t)
            for (long long g = (long long)b * kBlock + t; g < total; g += (long long)nb * kBlock) {
                const long long i = g / modes;
                const int m = (int)(g % modes);
                txo[g] = tile_tx(txd, tx, i, m, modes, nTx, SpS);
                rxo[g] = pad_rx(rxd, rx, i, m, modes, nRx);
            }
}

static void run_extract(const int64_t *h, const char *data, std::vector<double> &out) {
    const long long n = h[1], nOut = h[3];
    const int modes = (int)h[2], cx = (int)h[4], normalize = (int)h[5];
    const Cplx *x = (const Cplx *)data;
    const long long nb = ext_blocks(n);
    const size_t cnt_out = (size_t)nOut * modes * (cx ? 2 : 1);
    out.assign(cnt_out + modes, 0.0);                     // (the engine clears the output first)
    std::vector<int> cnt((size_t)modes * nb);
    std::vector<long long> off((size_t)modes * nb);
    std::vector<double> pw((size_t)modes * nb), norm(modes);
    // count
    for (int col = 0; col < modes; ++col)
        for (long long b = 0; b < nb; ++b) {
            double lane_pw[kBlock];
            int count[kBlock], before[kBlock], total = 0;
            for (int t = 0; t < kBlock; ++t) count[t] = popcount4(lane_flags(x, n, modes, col, b * kSpan + (long long)t * kItems, lane_pw[t]));
            block_ranks(count, before, total);
            cnt[col * nb + b] = total;
            pw[col * nb + b] = block_tree(lane_pw);
        }
    // offsets
    for (int col = 0; col < modes; ++col) {
        long long chunk[kBlock], total = 0;
        for (int t = 0; t < kBlock; ++t) {
            long long lo, hi;
            offsets_chunk(nb, t, lo, hi);
            chunk[t] = 0;
            for (long long b = lo; b < hi; ++b) chunk[t] += cnt[col * nb + b];
        }
        for (int t = 0; t < kBlock; ++t) {
            long long lo, hi, before = 0;
            offsets_chunk(nb, t, lo, hi);
            for (int l = 0; l < t; ++l) before += chunk[l];
            for (long long b = lo; b < hi; ++b) off[col * nb + b] = before, before += cnt[col * nb + b];
            total += chunk[t];
        }
        const double p = partials_tree(pw.data() + col * nb, nb, 1);
        norm[col] = normalize ? column_norm(p, total) : 1.0;
        out[cnt_out + col] = (double)total;
    }
    // scatter
    for (int col = 0; col < modes; ++col)
        for (long long b = 0; b < nb; ++b) {
            int flags[kBlock], count[kBlock], before[kBlock], total = 0;
            for (int t = 0; t < kBlock; ++t) {
                double unused;
                flags[t] = lane_flags(x, n, modes, col, b * kSpan + (long long)t * kItems, unused);
                count[t] = popcount4(flags[t]);
            }
            block_ranks(count, before, total);
            for (int t = 0; t < kBlock; ++t)
                lane_scatter(x, modes, col, b * kSpan + (long long)t * kItems, flags[t], off[col * nb + b] + before[t], norm[col], cx != 0, out.data(), nOut);
        }
}

template <bool CX> static void run_average_t(long long n, int cols, int N, int dtype, const void *x, std::vector<double> &out) {
    std::vector<double> w((size_t)(kMaTile + kMaMaxN - 1) * (CX ? 2 : 1));
    out.assign((size_t)n * cols * (CX ? 2 : 1), 0.0);
    for (int col = 0; col < cols; ++col)
        for (long long t0 = 0; t0 < n; t0 += kMaTile) {
            const long long left = n - t0;
            const int cnt = left < kMaTile ? (int)left : kMaTile, have = cnt + N - 1;
            for (int j = 0; j < have; ++j) {
                const long long r = t0 - N / 2 + j;
                double re = 0.0, im = 0.0;
                if (r >= 0 && r < n) mk::load(dtype, x, r * cols + col, re, im);
                if (CX) w[2 * j] = re, w[2 * j + 1] = im;
                else w[j] = re;
            }
            for (int o = 0; o < cnt; ++o) {
                double re, im;
                window_mean<CX>(w.data(), o, N, re, im);
                const long long g = (t0 + o) * cols + col;
                if (CX) out[2 * g] = re, out[2 * g + 1] = im;
                else out[g] = re;
            }
        }
}

static void run_bert(const int64_t *h, const char *data, std::vector<double> &out) {
    const long long n = h[1];
    const double *x = (const double *)data;
    const uint8_t *bits = (const uint8_t *)(data + ((size_t)n * sizeof(double) + 15) / 16 * 16);
    const int nb = grid_blocks(n, kBlock, kBertMaxBlocks);
    std::vector<double> part((size_t)nb * 3, 0.0);
    out.assign(kBertScal, 0.0);
    double *s = out.data();
    for (int pass = 0; pass < 3; ++pass) {
        for (int b = 0; b < nb; ++b) {
            double lanes[3][kBlock];
            for (int t = 0; t < kBlock; ++t) {
                double acc[3] = {0.0, 0.0, 0.0};
                for (long long i = (long long)b * kBlock + t; i < n; i += (long long)nb * kBlock) {
                    if (pass == 0) bert_stats(acc, x[i], bits[i] == 1);
                    else if (pass == 1) bert_dev(acc, x[i], bits[i] == 1, s[2], s[3]);
                    else acc[0] += bert_error(x[i], bits[i] == 1, s[6]);
                }
                for (int k = 0; k < 3; ++k) lanes[k][t] = acc[k];
            }
            const int K = pass == 0 ? 3 : pass == 1 ? 2 : 1;
            for (int k = 0; k < K; ++k) part[3 * b + k] = block_tree(lanes[k]);
        }
        double tot[3];
        for (int k = 0; k < 3; ++k) tot[k] = partials_tree(part.data() + k, nb, 3);
        if (pass == 0) bert_means(tot, n, s);
        else if (pass == 1) bert_threshold(tot, s);
        else s[8] = tot[0], s[9] = 0.0;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<char> in = read_all(argv[1]);
    const int64_t *h = (const int64_t *)in.data();
    std::vector<double> out;
    switch ((int)h[0]) {
    case 0: run_tile(h, in.data() + 8 * sizeof(int64_t), out); break;
    case 1: run_extract(h, in.data() + 6 * sizeof(int64_t), out); break;
    case 2: {
        const void *x = in.data() + 6 * sizeof(int64_t);    // (the head is padded to 16 bytes)
        if ((int)h[4] == mk::kF64) run_average_t<false>(h[1], (int)h[2], (int)h[3], (int)h[4], x, out);
        else run_average_t<true>(h[1], (int)h[2], (int)h[3], (int)h[4], x, out);
        break;
    }
    case 3: run_bert(h, in.data() + 2 * sizeof(int64_t), out); break;
    default: return 2;
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), sizeof(double), out.size(), f);
    fclose(f);
    return 0;
}
