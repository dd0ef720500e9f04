// nlin_kernels.h -- the per-lane bodies of the perturbation-model engine (engine_nlin.hip), written against an execution context
// `Ctx` (tid / bid / nthreads / nblocks / lds / sync()) like the bodies of ofdm_kernels.h: hipcc launches them on gfx950,
// tests/emu/emu_nlin.cpp walks them with g++.  Reference semantics: optic/models/perturbation.py (calcNLINperturbation,
// calcNLINperturbationSimplified, perturbationNLIN).
//
// With m = j - L, n = L - i and x zero outside [0, N) the reference's sum over its (2L+1)^2 window is
//     P[s, m] = x[s] conj(x[s+m]) + y[s] conj(y[s+m])
//     dx[t]   = sum_m x[t+m] sum_n C_ifwm[L-n, L+m] P[t+n, m]  +  x[t] sum_n C_ixpm[L-n, L] |y[t+n]|^2       (dy: x <-> y)
// A *pass* is one inner sum: a line q[s] over the symbols (P[., m], or |y|^2, or |x|^2), a list of coefficients over n, and the
// symbol the result multiplies.  A workgroup of kLanes lanes takes a tile of kTile = kLanes kOut consecutive symbols and a share
// of the passes: x and y of the tile plus 2L on either side go to LDS once (the zero padding is the guard of that load: no index
// outside [0, N) becomes an address); per pass the line over [t0 - L, t0 + kTile + L) is formed cooperatively into one of two LDS
// buffers while the pass before is summed out of the other; a lane holds kOut consecutive outputs in registers, so that in a dense
// pass (every n, mode 'AM') one 16-byte LDS read of the line feeds kOut complex multiply-adds -- the window of kOut line values
// slides by one per n -- next to one broadcast read of the coefficient, which is formed into LDS with the line.  A sparse pass
// ('AMR') reads its n from a list there too.  The line is stored residue-major (index i at (i mod kOut) S + i / kOut), so the lanes of a wave, kOut indices apart,
// read consecutive 16-byte slots.  Every sum has a fixed order; the shares of the passes are added in order by finish_body, which
// also forms the phases and, for perturbationNLIN, the field.  All arithmetic is double; of what the reference rounds to complex64
// (prec) the normalised symbols are rounded on the way in and dx, dy on the way out.  Its float32 products and powers are not
// imitated (numpy's single-precision |.| is not one formula on every machine): they run in double on the rounded symbols.
#pragma once
#include "fused_core.h"

namespace ssf {
namespace nlin {

using fused::cx;
using fused::mk;

constexpr int kMaxL = 128;                    // largest matrixOrder
constexpr int kLanes = 64, kOut = 4;          // lanes of a workgroup of the main kernel, consecutive outputs per lane
constexpr int kTile = kLanes * kOut;          // symbols per workgroup
constexpr int kBlock = 256;                   // lanes of the element-wise kernels and of the power sums
constexpr int kMaxBlocks = 1024;              // ... and the most workgroups they take: the number of partial sums of a mean
constexpr int kMaxSplit = 16;                 // most shares the passes are dealt into
constexpr int kTargetGroups = 2048;           // workgroups the main kernel aims at
enum { PASS_IFWM = 0, PASS_IXPM_X = 1, PASS_IXPM_Y = 2 };

SSF_HD long long tiles_for(long long N) { return (N + kTile - 1) / kTile; }
// shares of the passes: enough to reach kTargetGroups workgroups, at most kMaxSplit and at most one per pass.  It depends on N
// and the plan only, so a result does not depend on the device it was computed on.
SSF_HD int split_for(long long N, int npass) {
    const long long t = tiles_for(N);
    long long s = (kTargetGroups + t - 1) / t;
    if (s > kMaxSplit) s = kMaxSplit;
    if (s > npass) s = npass;
    return (int)s;                            // 0 without passes
}
SSF_HD int line_slots(int L) { return (kTile + 2 * L + kOut - 1) / kOut; }                  // S: slots per residue
SSF_HD int coef_slots(int L) { return 2 * L + 1 + kOut; }            // a pass's coefficients, and what the sum reads ahead
// x and y of the tile, two lines, and the coefficients (with their n) of two passes
SSF_HD size_t lds_bytes_for(int L) {
    return ((size_t)2 * (kTile + 4 * L) + (size_t)2 * kOut * line_slots(L) + (size_t)2 * coef_slots(L)) * sizeof(cx<double>) +
           (size_t)2 * coef_slots(L) * sizeof(int);
}
SSF_HD int line_pos(int i, int S) { return (i & (kOut - 1)) * S + (i >> 2); }
static_assert(kOut == 4, "line_pos shifts by log2 kOut");

SSF_HD cx<double> load_in(const void *p, long long i, int c64) {
    if (c64) {
        const cx<float> v = ((const cx<float> *)p)[i];
        return mk<double>((double)v.re, (double)v.im);
    }
    return ((const cx<double> *)p)[i];
}
// A += c v in four multiply-adds
SSF_HD void cmac(cx<double> &A, cx<double> c, cx<double> v) {
    A.re = fused::fma_s<double>(c.re, v.re, A.re);
    A.re = fused::fma_s<double>(-c.im, v.im, A.re);
    A.im = fused::fma_s<double>(c.re, v.im, A.im);
    A.im = fused::fma_s<double>(c.im, v.re, A.im);
}
SSF_HD cx<double> round32(cx<double> v) { return mk<double>((double)(float)v.re, (double)(float)v.im); }
SSF_HD void store_out(void *p, long long i, int c64, cx<double> v) {
    if (c64) ((cx<float> *)p)[i] = mk<float>((float)v.re, (float)v.im);
    else ((cx<double> *)p)[i] = v;
}

// ---- normalisation: out[col][t] = in[t stride + col] / sqrt(total[col] / N), rounded to single precision where the reference's
// array is complex64 (numpy divides by a real scalar through its reciprocal)
struct StageArgs {
    const void *in[2];            // the two columns (the same array with stride 2, or two arrays)
    long long stride;
    int in_c64, round;
    const double *total;          // 2: sum |x|^2, sum |y|^2
    cx<double> *out;              // 2 x N
    long long N;
};
template <class Ctx> SSF_HD void stage_body(Ctx &ctx, const StageArgs &a, int col) {
    const double r = 1.0 / std::sqrt(a.total[col] / (double)a.N);
    for (long long t = (long long)ctx.bid * ctx.nthreads + ctx.tid; t < a.N; t += (long long)ctx.nblocks * ctx.nthreads) {
        cx<double> v = load_in(a.in[col], t * a.stride, a.in_c64) * r;
        a.out[(long long)col * a.N + t] = a.round ? round32(v) : v;
    }
}
// |.|^2 of element t of a column, as the power sums add it
SSF_HD double power_term(const void *p, long long i, int c64) { return fused::norm2(load_in(p, i, c64)); }

// ---- the sums
struct MainArgs {
    const cx<double> *xs;         // 2 x N: the normalised x, then y
    cx<double> *part;             // split x 2 x N: each share's dx, dy
    const int *pass;              // npass x {kind, m, first, count}
    const cx<double> *coef;       // ncoef
    const int *nidx;              // ncoef: the n of a coefficient (sparse plans)
    long long N;
    int L, npass, split;
};

template <bool DENSE, class Ctx> SSF_HD void main_body(Ctx &ctx, const MainArgs &a, long long tile, int share) {
    const int L = a.L, S = line_slots(L), W = kTile + 4 * L, LW = kTile + 2 * L, CW = coef_slots(L);
    cx<double> *xl = (cx<double> *)ctx.lds, *yl = xl + W, *line = yl + W, *cl = line + (size_t)2 * kOut * S;
    int *nl = (int *)(cl + 2 * CW);
    const long long t0 = tile * kTile;
    for (int i = ctx.tid; i < W; i += ctx.nthreads) {
        const long long s = t0 - 2 * L + i;
        const bool in = s >= 0 && s < a.N;
        xl[i] = in ? a.xs[s] : mk<double>(0.0, 0.0);
        yl[i] = in ? a.xs[a.N + s] : mk<double>(0.0, 0.0);
    }
    ctx.sync();
    const int p0 = (int)((long long)share * a.npass / a.split), p1 = (int)((long long)(share + 1) * a.npass / a.split);
    // line value i is the symbol t0 - L + i, which the tile holds at i + L.  The pass's coefficients come along into LDS: read
    // from there, the same address in every lane, they share the line reads' in-order counter, where scalar loads inside the
    // sum would make every wait a wait for everything.
    auto form = [&](int p, int buf) {
        const int kind = a.pass[4 * p], m = a.pass[4 * p + 1], first = a.pass[4 * p + 2], count = a.pass[4 * p + 3];
        cx<double> *dst = line + (size_t)buf * kOut * S;
        for (int i = ctx.tid; i < count; i += ctx.nthreads) {
            cl[buf * CW + i] = a.coef[first + i];
            if (!DENSE) nl[buf * CW + i] = a.nidx[first + i];
        }
        for (int i = ctx.tid; i < LW; i += ctx.nthreads) {
            const int j = i + L;
            cx<double> v;
            if (kind == PASS_IFWM) v = xl[j] * fused::conj(xl[j + m]) + yl[j] * fused::conj(yl[j + m]);
            else v = mk<double>(fused::norm2(kind == PASS_IXPM_X ? yl[j] : xl[j]), 0.0);
            dst[line_pos(i, S)] = v;
        }
    };
    const int tb = ctx.tid * kOut;
    cx<double> dx[kOut], dy[kOut];
#pragma unroll
    for (int r = 0; r < kOut; ++r) dx[r] = dy[r] = mk<double>(0.0, 0.0);
    if (p0 < p1) form(p0, 0);
    ctx.sync();
    for (int p = p0; p < p1; ++p) {
        const int buf = (p - p0) & 1;
        const cx<double> *q = line + (size_t)buf * kOut * S, *cq = cl + buf * CW;
        const int *nq = nl + buf * CW;
        if (p + 1 < p1) form(p + 1, buf ^ 1);
        const int kind = a.pass[4 * p], m = a.pass[4 * p + 1], count = a.pass[4 * p + 3];
        cx<double> A[kOut];
#pragma unroll
        for (int r = 0; r < kOut; ++r) A[r] = mk<double>(0.0, 0.0);
        if (DENSE) {
            // coefficient k belongs to n = k - L: output r needs line value tb + r + k.  w holds the kOut values of step k0, cc the
            // coefficients of the steps k0 .. k0 + kOut - 1; what the next kOut steps need is read before these are summed, so
            // no multiply-add waits for a read of its own step.
            cx<double> w[kOut], cc[kOut];
#pragma unroll
            for (int u = 0; u < kOut; ++u) w[u] = q[line_pos(tb + u, S)], cc[u] = cq[u];        // (cq is padded: read, never used)
            int k0 = 0;
            for (; k0 + kOut < count; k0 += kOut) {
                cx<double> nw[kOut], nc[kOut];
#pragma unroll
                for (int u = 0; u < kOut; ++u) nw[u] = q[line_pos(tb + k0 + kOut + u, S)], nc[u] = cq[k0 + kOut + u];
#pragma unroll
                for (int u = 0; u < kOut; ++u)
#pragma unroll
                    for (int r = 0; r < kOut; ++r) cmac(A[r], cc[u], r + u < kOut ? w[(r + u) & (kOut - 1)] : nw[(r + u) & (kOut - 1)]);
#pragma unroll
                for (int u = 0; u < kOut; ++u) w[u] = nw[u], cc[u] = nc[u];
            }
            // the last 1 .. kOut coefficients: step u of them needs the line values up to tb + k0 + u + kOut - 1
            const int rem = count - k0;
            cx<double> nw[kOut];
#pragma unroll
            for (int u = 0; u < kOut; ++u) nw[u] = u + 2 <= rem ? q[line_pos(tb + k0 + kOut + u, S)] : mk<double>(0.0, 0.0);
#pragma unroll
            for (int u = 0; u < kOut; ++u) {
                if (u < rem) {
#pragma unroll
                    for (int r = 0; r < kOut; ++r) cmac(A[r], cc[u], r + u < kOut ? w[(r + u) & (kOut - 1)] : nw[(r + u) & (kOut - 1)]);
                }
            }
        } else {
            cx<double> c = cq[0];
            int n = nq[0];
            for (int k = 0; k < count; ++k) {
                const int o = tb + n + L;
                const cx<double> ck = c;
                cx<double> v[kOut];
#pragma unroll
                for (int r = 0; r < kOut; ++r) v[r] = q[line_pos(o + r, S)];
                c = cq[k + 1], n = nq[k + 1];                                                   // (padded: read, used only if there)
#pragma unroll
                for (int r = 0; r < kOut; ++r) cmac(A[r], ck, v[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < kOut; ++r) {
            const int j = tb + r + 2 * L + m;
            if (kind != PASS_IXPM_Y) dx[r] = dx[r] + xl[j] * A[r];
            if (kind != PASS_IXPM_X) dy[r] = dy[r] + yl[j] * A[r];
        }
        ctx.sync();
    }
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
        const long long t = t0 + tb + r;
        if (t < a.N) {
            a.part[((long long)share * 2 + 0) * a.N + t] = dx[r];
            a.part[((long long)share * 2 + 1) * a.N + t] = dy[r];
        }
    }
}

// ---- the shares in order, the phases, and what the entry point returns
struct FinishArgs {
    const cx<double> *xs;         // 2 x N: the symbols the sums ran on
    const cx<double> *e1;         // 2 x N: perturbationNLIN: the columns after pnorm
    const cx<double> *part;       // split x 2 x N
    const int *phase_m;           // nphase: the m of the centre row's kept coefficients
    const cx<double> *phase_c;
    void *out[4];                 // entry 0: dx, dy (prec), phi_x, phi_y (double); entry 1: nlin, N x 2 (out_c64)
    long long N;
    int split, nphase, ispm_offset, entry, prec_c64, out_c64;
    double ispm_im, peak;
};
SSF_HD double power_at(const cx<double> *v, long long s, long long N) { return s >= 0 && s < N ? fused::norm2(v[s]) : 0.0; }

template <class Ctx> SSF_HD void finish_body(Ctx &ctx, const FinishArgs &a) {
    const cx<double> *x = a.xs, *y = a.xs + a.N;
    for (long long t = (long long)ctx.bid * ctx.nthreads + ctx.tid; t < a.N; t += (long long)ctx.nblocks * ctx.nthreads) {
        cx<double> d[2] = {mk<double>(0.0, 0.0), mk<double>(0.0, 0.0)};
        for (int g = 0; g < a.split; ++g) {
            d[0] = d[0] + a.part[((long long)g * 2 + 0) * a.N + t];
            d[1] = d[1] + a.part[((long long)g * 2 + 1) * a.N + t];
        }
        double ph[2] = {0.0, 0.0};
        for (int k = 0; k < a.nphase; ++k) {
            const long long s = t + a.phase_m[k];
            const double px = power_at(x, s, a.N), py = power_at(y, s, a.N), c = a.phase_c[k].im;
            ph[0] += c * (2.0 * px + py);
            ph[1] += c * (2.0 * py + px);
        }
        const long long so = t + a.ispm_offset;
        const double pw = (power_at(x, so, a.N) + power_at(y, so, a.N)) * a.ispm_im;
        ph[0] += pw, ph[1] += pw;
        if (a.prec_c64) d[0] = round32(d[0]), d[1] = round32(d[1]);
        if (a.entry == 0) {
            store_out(a.out[0], t, a.prec_c64, d[0]);
            store_out(a.out[1], t, a.prec_c64, d[1]);
            ((double *)a.out[2])[t] = ph[0];
            ((double *)a.out[3])[t] = ph[1];
            continue;
        }
        const double root = std::sqrt(a.peak), cube = a.peak * root;
#pragma unroll
        for (int col = 0; col < 2; ++col) {
            double s, c;
            fused::sincos_d(a.peak * ph[col], s, c);
            const cx<double> e = mk<double>(c, s), em1 = mk<double>(c - 1.0, s);
            const cx<double> v = (a.e1[(long long)col * a.N + t] * root) * em1 + (d[col] * cube) * e;
            store_out(a.out[0], 2 * t + col, a.out_c64, v);
        }
    }
}

}  // namespace nlin
}  // namespace ssf
