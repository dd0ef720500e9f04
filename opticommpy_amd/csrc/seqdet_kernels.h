// seqdet_kernels.h -- sequence and symbol detection of the direct-detection chain (mlse, detector) and the autocorrelation behind
// estimateWhiteningFilter: the per-state, per-symbol and per-lag bodies as host/device-neutral inline functions.
// engine_seqdet.hip wraps them in gfx950 kernels; tests/emu/emu_seqdet.cpp loops the same functions over lanes, steps and chunks
// with g++.  Both are compiled without contraction of multiply-adds: two candidates the reference computes as equal stay equal.
// Reference: optic/comm/modulation.py:412-481 (detector), 582-680 (mlse); optic/dsp/core.py:1143-1254 (levinson, autocorr,
// estimateWhiteningFilter).  Arithmetic is double.
//
// mlse.  The trellis has S = M^L states (L = taps - 1; one state at L = 0).  State s holds the last L symbols, the newest in its
// lowest digit.  Next state ns is reached from the M predecessors  ns / M + j M^(L-1), j = 0 .. M-1, all with the decided symbol
// ns % M; the expected output of candidate j is  base(ns) + h[L] c[j]  with  base(ns) = h[0] c[ns % M] + sum_{i=1}^{L-1} h[i]
// c[digit i-1 of ns / M], the reference's summation order.  At L = 0 the candidates of the one state are the M symbols themselves
// (expected output h[0] c[j], decided symbol j, predecessor 0).  Either way a step keeps one byte per state: j of the survivor,
// the lowest j among equal metrics (the reference walks the predecessors upwards with a strict <).
//
// Survivors: row n of a column is Sp = S rounded up to 4 bytes; rows of kSurvChunk steps form a chunk.  The traceback is three
// integer passes: the end-state -> start-state map of every chunk, the composition of the maps from the final state, and one
// walker per chunk that writes the chunk's decisions.
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace sq {

using mk::Cplx;

// limits the kernels are built for (checked by ssf_mlse / ssf_detector / ssf_autocorr before anything is allocated)
constexpr int kMaxM = 64, kMaxStates = 1024, kMaxTaps = 11, kMaxCols = 64;
constexpr int kSurvChunk = 32;                // T: steps whose survivors are gathered in LDS and flushed together
constexpr int kStageChunk = 256;              // C: samples of y staged in LDS at a time (a multiple of T)
constexpr int kComposeLds = 16384;            // map entries (uint16) the composing workgroup stages at a time
constexpr int kDetBlock = 256;                // detector: symbols per workgroup
constexpr int kAcMaxTaps = 256, kAcTile = 4096, kAcBlock = 256, kAcMaxBlocks = 1024;
static_assert(kStageChunk % kSurvChunk == 0, "a staging chunk holds whole survivor chunks");

struct Trellis {
    int M, L, S, Sp, stride, cx;              // stride = M^(L-1): the weight of a predecessor's highest digit (0 at L = 0)
};

// S = M^L, or 0 where it exceeds the cap
MK_HD int states_of(int M, int L) {
    long long s = 1;
    for (int i = 0; i < L; ++i) {
        s *= M;
        if (s > kMaxStates) return 0;
    }
    return (int)s;
}
MK_HD Trellis trellis_of(int M, int taps, int cx) {
    Trellis t{};
    t.M = M, t.L = taps - 1, t.S = states_of(M, t.L), t.Sp = (t.S + 3) & ~3, t.cx = cx;
    t.stride = t.L > 0 ? t.S / M : 0;
    return t;
}

// a += h c, as numpy multiplies and adds complex values (real tables have zero imaginary parts: the imaginary sums stay zero)
MK_HD void add_product(double &ar, double &ai, const double *h, const double *c) {
    ar += h[0] * c[0] - h[1] * c[1];
    ai += h[0] * c[1] + h[1] * c[0];
}

// the part of a next state's expected outputs that all its candidates share (h, c: interleaved (re, im) pairs)
MK_HD void state_base(const Trellis &t, const double *h, const double *c, int ns, double &br, double &bi) {
    br = 0.0, bi = 0.0;
    if (t.L == 0) return;
    br = h[0] * c[2 * (ns % t.M)] - h[1] * c[2 * (ns % t.M) + 1];
    bi = h[0] * c[2 * (ns % t.M) + 1] + h[1] * c[2 * (ns % t.M)];
    int rest = ns / t.M;
    for (int i = 1; i < t.L; ++i) {
        add_product(br, bi, h + 2 * i, c + 2 * (rest % t.M));
        rest /= t.M;
    }
}
// the part candidate j adds: h[L] c[j]
MK_HD void candidate_term(const Trellis &t, const double *h, const double *c, int j, double &tr, double &ti) {
    tr = h[2 * t.L] * c[2 * j] - h[2 * t.L + 1] * c[2 * j + 1];
    ti = h[2 * t.L] * c[2 * j + 1] + h[2 * t.L + 1] * c[2 * j];
}

MK_HD int predecessor(const Trellis &t, int ns, int j) { return t.L == 0 ? 0 : ns / t.M + j * t.stride; }
MK_HD int decided_symbol(const Trellis &t, int ns, int j) { return t.L == 0 ? j : ns % t.M; }

// add-compare-select of next state ns: pm the metrics before the step, term the M candidate terms; returns the survivor's j.
// MT: the number of candidates where the caller knows it at compile time (the loop unrolls and the M reads of pm are in flight
// together), 0 otherwise.  The operations and their order do not depend on MT.
template <bool CX, int MT> MK_HD int acs(const Trellis &t, const double *pm, const double *term, int ns, double br, double bi, double yr,
                                         double yi, double &best) {
    const int M = MT ? MT : t.M;
    const int p0 = t.L == 0 ? 0 : ns / M;
    int bj = 0;
    best = INFINITY;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const double er = br + term[2 * j], dr = yr - er;
        double bm = dr * dr;
        if (CX) {
            const double ei = bi + term[2 * j + 1], di = yi - ei;
            bm += di * di;
        }
        const double cand = pm[p0 + j * t.stride] + bm;
        if (j == 0 || cand < best) best = cand, bj = j;
    }
    return bj;
}
// the same with the common constellation sizes unrolled
template <bool CX> MK_HD int acs_any(const Trellis &t, const double *pm, const double *term, int ns, double br, double bi, double yr, double yi,
                                     double &best) {
    switch (t.M) {
    case 2: return acs<CX, 2>(t, pm, term, ns, br, bi, yr, yi, best);
    case 4: return acs<CX, 4>(t, pm, term, ns, br, bi, yr, yi, best);
    case 8: return acs<CX, 8>(t, pm, term, ns, br, bi, yr, yi, best);
    }
    return acs<CX, 0>(t, pm, term, ns, br, bi, yr, yi, best);
}

// lowest-index minimum: (d, i) takes (d2, i2) where that is smaller, or equal with the lower index
MK_HD void argmin_merge(double &d, int &i, double d2, int i2) {
    if (d2 < d || (d2 == d && i2 < i)) d = d2, i = i2;
}

// one traceback step through a survivor row
MK_HD int step_back(const Trellis &t, const uint8_t *row, int state) { return predecessor(t, state, row[state]); }

// ---- detector: index of the decision for one received value.  tab: M (re, im) pairs; logpx: M log priors (MAP)
enum { kRuleML = 0, kRuleMAP = 1 };
MK_HD int detect(const double *tab, const double *logpx, int M, int rule, double sigma2, double re, double im) {
    if (rule == kRuleML) return mk::nearest(tab, M, re, im);
    int best = 0;
    double vbest = -INFINITY;
    for (int m = 0; m < M; ++m) {
        const double dr = re - tab[2 * m], di = im - tab[2 * m + 1];
        const double v = -(dr * dr + di * di) / sigma2 + logpx[m];
        if (v > vbest) vbest = v, best = m;
    }
    return best;
}

// ---- autocorr: the range of samples workgroup b of nb sums (whole tiles, so that a sum's order does not depend on n alone)
MK_HD long long ac_tiles_per_block(long long n, int nb) {
    const long long tiles = (n + kAcTile - 1) / kAcTile;
    return (tiles + nb - 1) / nb;
}
MK_HD int ac_blocks(long long n) {
    const long long tiles = (n + kAcTile - 1) / kAcTile;
    return (int)(tiles < kAcMaxBlocks ? (tiles < 1 ? 1 : tiles) : kAcMaxBlocks);
}
// one lane's share of lag k over the tile that starts at sample t0 (w: the tile with the kAcMaxTaps - 1 samples before it in
// front, zeros where there are none): samples t0 + lane, t0 + lane + 64, ..
MK_HD double ac_lane_sum(const double *w, int k, int lane, long long t0, int cnt) {
    double a = 0.0;
    for (int i = lane; i < cnt; i += 64)
        if (t0 + i >= k) a += w[kAcMaxTaps - 1 + i] * w[kAcMaxTaps - 1 + i - k];
    return a;
}

}  // namespace sq
}  // namespace ssf
