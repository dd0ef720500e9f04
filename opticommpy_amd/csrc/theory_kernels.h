// theory_kernels.h -- mutual information of a constellation on the AWGN channel by quadrature (ssf_theory_mi) and the Monte-Carlo
// calcMI (ssf_calc_mi): the per-node and per-symbol bodies as host/device-neutral inline functions.  engine_theory.hip wraps them
// in gfx950 kernels; tests/emu/emu_theory.cpp walks the same functions over the kernels' tiles and lanes with g++.
// Reference: optic/comm/metrics.py:497-547 (calcMI), 689-747 (condEntropy), 770-848 (theoryMI).
//
// The rule.  With y = x_i + sqrt(2) sigma t (t complex, density e^{-|t|^2} / pi) the ratio p(y | x_j) / p(y | x_i) is e^{e_ij(t)},
//     e_ij(t) = -(|d_ij|^2 + 2 sqrt(2) sigma Re(conj(d_ij) t)) / (2 sigma^2),   d_ij = x_i - x_j,
// and H(X | Y) = sum_i px_i E_t[ log2( sum_j px_j e^{e_ij(t)} ) - log2 px_i ].  The expectation is a uniform grid in t: spacing
// kStep, |Re t|, |Im t| <= kTmax, weight e^{-|t|^2} kStep^2 / pi, not renormalised (the integrand is analytic with Gaussian decay:
// the trapezoid rule's best case; measured bound in profiles/theory_quadrature.json).
#pragma once
#include <cmath>

#include "metrics_kernels.h"

namespace ssf {
namespace tk {

constexpr double kStep = 0.1, kTmax = 6.5;
constexpr int kK = 65, kSide = 2 * kK + 1, kNodes = kSide * kSide;     // 131 x 131 nodes
constexpr int kTile = 256, kTiles = (kNodes + kTile - 1) / kTile;      // one node per lane, 68 tiles
constexpr int kMaxM = 1024, kMaxS = 4096;
constexpr int kRow = 3;                                                // doubles per j of a point's row
constexpr double kLog2e = 1.4426950408889634, kSqrt2 = 1.4142135623730951, kPi = 3.141592653589793;

// entry j of point i's row: Re d_ij / sigma, Im d_ij / sigma, -|d_ij|^2 / (2 sigma^2) + ln px_j
MK_HD void row_entry(const double *tab, const double *px, int i, int j, double sigma, double *e) {
    const double dr = tab[2 * i] - tab[2 * j], di = tab[2 * i + 1] - tab[2 * j + 1];
    e[0] = dr / sigma, e[1] = di / sigma;
    e[2] = -(dr * dr + di * di) / (2.0 * sigma * sigma) + std::log(px[j]);
}

// node q of the grid: acc = [w log2( sum_j px_j e^{e_ij(t)} ), w]
// The exponent cannot overflow: with u = d_ij / (sqrt(2) sigma), e_ij = |t|^2 - |u + t|^2 <= |t|^2 <= 2 kTmax^2 = 84.5; the term
// j = i is px_i e^0, so the sum is positive and its logarithm finite.
MK_HD void node_body(double *acc, const double *row, int M, int q) {
    const double tr = (double)(q / kSide - kK) * kStep, ti = (double)(q % kSide - kK) * kStep;
    const double w = std::exp(-(tr * tr + ti * ti)) * (kStep * kStep / kPi);
    const double ur = -kSqrt2 * tr, ui = -kSqrt2 * ti;
    double S = 0.0;
    for (int j = 0; j < M; ++j) S += std::exp(row[kRow * j] * ur + (row[kRow * j + 1] * ui + row[kRow * j + 2]));
    acc[0] += w * std::log2(S), acc[1] += w;
}

// point i from its tile sums (added in the order of the tiles): px_i (sum_t w log2 S - W log2 px_i), W the grid's own weight sum
MK_HD double point_term(const double *part, double pxi) {
    double T = 0.0, W = 0.0;
    for (int t = 0; t < kTiles; ++t) T += part[2 * t], W += part[2 * t + 1];
    return pxi * (T - W * std::log2(pxi));
}

// H(X) = -sum px log2 px, one term after the other
inline double entropy(const double *px, int M) {
    double H = 0.0;
    for (int m = 0; m < M; ++m) H -= px[m] * std::log2(px[m]);
    return H;
}

// ---- calcMI: one symbol.  The reference's direct form: index of the first minimum of |tx - c|, the M likelihoods
// exp(-(1 / sigma^2) |rx - c|^2) px added as they come, no log-sum-exp rescue.  ninv = -(1 / sigma^2).
// acc += log2 p(y | x) + log2 px[index] - log2 p(y)
MK_HD void calc_body(double *acc, const double *tab, const double *px, const double *log2px, int M, double ninv, double rr, double ri,
                     double tr, double ti) {
    const int ind = mk::nearest(tab, M, tr, ti);
    const double er = rr - tr, ei = ri - ti;
    double pY = 0.0;
    for (int m = 0; m < M; ++m) {
        const double dr = rr - tab[2 * m], di = ri - tab[2 * m + 1];
        pY += std::exp(ninv * (dr * dr + di * di)) * px[m];
    }
    acc[0] += ninv * (er * er + ei * ei) * kLog2e + log2px[ind] - std::log2(pY);
}

// MI = H(X) - H(X | Y), H(X | Y) = -sum / n
MK_HD double calc_combine(double sum, long long n, double H) { return H + sum / (double)n; }

}  // namespace tk
}  // namespace ssf
