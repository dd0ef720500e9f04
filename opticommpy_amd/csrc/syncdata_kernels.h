// syncdata_kernels.h -- the glue of syncDataSequences, movingAverage and bert: the per-sample and per-lane bodies as
// host/device-neutral inline functions.  engine_syncdata.hip wraps them in gfx950 kernels; tests/emu/emu_syncdata.cpp walks the
// same functions over workgroups and lanes with g++.
// Reference: optic/dsp/synchronization.py:30-170 (syncDataSequences), optic/dsp/core.py:829-880 (movingAverage),
// optic/comm/metrics.py:37-105 (bert).  Arithmetic is double whatever the input type.
//
// tile      T[i, m] = tx[(i / SpS) mod nTx, m] where i mod SpS == 0, else 0, as complex128; rx widened and zero-padded beside it.
// extract   per column the non-zero samples keep their order: a workgroup owns kSpan rows, a lane kItems consecutive ones; the
//           rank of a sample is (kept in the workgroups before) + (kept by the lanes before) + (kept among the lane's own before).
// average   y[i] = (1 / N) sum_{j = i - N/2}^{i + (N-1)/2} x[j], zeros outside [0, n): a workgroup holds kMaTile rows of a column
//           and the N - 1 rows around them; every output adds its N values from the lowest row upwards.
// bert      three passes over (Irx, bits): counts and sums per class, squared deviations per class, decisions against Id.
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace sd {

using mk::Cplx;

constexpr int kBlock = 256;                   // lanes of every workgroup here (block_reduce.h's)
constexpr int kItems = 4, kSpan = kBlock * kItems;        // B: rows of a column one workgroup scans
constexpr int kMaTile = 1024;                 // T: outputs of a column per workgroup
constexpr int kMaMaxN = 2048;                 // longest window: (T + N - 1) complex values fit the 64 KiB of static LDS
constexpr int kMaxModes = 8;                  // symbolSync's limit
constexpr int kBertMaxBlocks = 1024, kElemMaxBlocks = 1 << 16;
constexpr int kBertScal = 10;                 // n1, n0, I1, I0, std1, std0, Id, Q, errors, (spare)

MK_HD bool nonzero(const Cplx &v) { return v.re != 0.0 || v.im != 0.0; }

// ---- tile / stuff / widen
MK_HD Cplx tile_tx(int dtype, const void *tx, long long i, int m, int modes, long long nTx, int SpS) {
    Cplx v{0.0, 0.0};
    if (i % SpS == 0) mk::load(dtype, tx, ((i / SpS) % nTx) * modes + m, v.re, v.im);
    return v;
}
MK_HD Cplx pad_rx(int dtype, const void *rx, long long i, int m, int modes, long long nRx) {
    Cplx v{0.0, 0.0};
    if (i < nRx) mk::load(dtype, rx, i * modes + m, v.re, v.im);
    return v;
}

// ---- a block of `width` columns from one row-major array into another: element g of the block (row g / width, column g % width)
MK_HD void column_block_index(long long g, int width, int src_cols, int src_first, int dst_cols, int dst_first, long long &from, long long &to) {
    const long long i = g / width;
    const int j = (int)(g % width);
    from = i * src_cols + src_first + j, to = i * dst_cols + dst_first + j;
}

// ---- extraction
MK_HD long long ext_blocks(long long n) { return (n + kSpan - 1) / kSpan; }
// the lane's kItems rows from row0 on: bit e of the result is set where row0 + e holds a non-zero sample; pw: their |.|^2, added
// in row order
MK_HD int lane_flags(const Cplx *x, long long n, int modes, int col, long long row0, double &pw) {
    int f = 0;
    pw = 0.0;
    for (int e = 0; e < kItems; ++e) {
        if (row0 + e >= n) break;
        const Cplx v = x[(row0 + e) * modes + col];
        if (nonzero(v)) f |= 1 << e, pw += v.re * v.re + v.im * v.im;
    }
    return f;
}
// the workgroup's exclusive scan of the lanes' counts.  Within a wave the inclusive scan takes the steps o = 1, 2, .. 32: a lane adds
// the value that lane - o held before the step (lanes below o keep theirs); the last lane of every wave then leaves the wave's
// total, and a lane's rank is the waves before it + its inclusive value - its own count.
MK_HD int scan_step(int inc, int from_below, int lane, int o) { return lane >= o ? inc + from_below : inc; }
MK_HD int rank_before(const int *wave_total, int waves, int wave, int inc, int own, int &total) {
    int before = 0;
    total = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) before += wave_total[w];
        total += wave_total[w];
    }
    return before + inc - own;
}
MK_HD int popcount4(int f) { return (f & 1) + ((f >> 1) & 1) + ((f >> 2) & 1) + ((f >> 3) & 1); }
// writes the lane's kept samples from rank `at` on, divided by `norm` (1 leaves the bits as they are); rows >= nOut are never
// written
MK_HD void lane_scatter(const Cplx *x, int modes, int col, long long row0, int f, long long at, double norm, bool cx_out, void *out, long long nOut) {
    for (int e = 0; e < kItems; ++e) {
        if (!(f >> e & 1)) continue;
        const Cplx v = x[(row0 + e) * modes + col];
        if (at < nOut) {
            if (cx_out) ((Cplx *)out)[at * modes + col] = Cplx{v.re / norm, v.im / norm};
            else ((double *)out)[at * modes + col] = v.re / norm;
        }
        ++at;
    }
}
// the share of the workgroups' counts that lane `lane` of the offsets workgroup scans: [lo, hi)
MK_HD void offsets_chunk(long long nb, int lane, long long &lo, long long &hi) {
    const long long per = (nb + kBlock - 1) / kBlock;
    lo = per * lane < nb ? per * lane : nb;
    hi = lo + per < nb ? lo + per : nb;
}
MK_HD double column_norm(double power, long long kept) { return kept > 0 ? std::sqrt(power / (double)kept) : 1.0; }

// ---- windowed mean.  w: the tile's rows with the halo in front, row t0 - N / 2 at w[0] (interleaved (re, im) where CX); the
// window of local output o is w[o .. o + N)
template <bool CX> MK_HD void window_mean(const double *w, int o, int N, double &re, double &im) {
    double sr = 0.0, si = 0.0;
    if (CX) {
        const Cplx *c = (const Cplx *)w + o;
        for (int j = 0; j < N; ++j) sr += c[j].re, si += c[j].im;
    } else {
        for (int j = 0; j < N; ++j) sr += w[o + j];
    }
    re = sr / (double)N, im = si / (double)N;
}

// ---- bert
// (a bit is 1 where its byte equals 1, as the reference's bitsTx == 1; the callers pass byte == 1)
MK_HD void bert_stats(double *acc, double x, int bit) {                 // acc: n1, sum1, sum0
    if (bit) acc[0] += 1.0, acc[1] += x;
    else acc[2] += x;
}
MK_HD void bert_dev(double *acc, double x, int bit, double I1, double I0) {     // acc: ss1, ss0
    const double d = x - (bit ? I1 : I0);
    acc[bit ? 0 : 1] += d * d;
}
MK_HD double bert_error(double x, int bit, double Id) { return ((x > Id) ? 1 : 0) != bit ? 1.0 : 0.0; }
// s: n1, n0, I1, I0 from the first pass' totals (n samples)
MK_HD void bert_means(const double *tot, long long n, double *s) {
    s[0] = tot[0], s[1] = (double)n - tot[0];
    s[2] = tot[1] / s[0], s[3] = tot[2] / s[1];
}
// s: std1, std0, Id, Q from the second pass' totals
MK_HD void bert_threshold(const double *tot, double *s) {
    s[4] = std::sqrt(tot[0] / s[0]), s[5] = std::sqrt(tot[1] / s[1]);
    s[6] = (s[4] * s[3] + s[5] * s[2]) / (s[4] + s[5]);
    s[7] = (s[2] - s[3]) / (s[4] + s[5]);
}

}  // namespace sd
}  // namespace ssf
