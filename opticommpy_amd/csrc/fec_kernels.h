// fec_kernels.h -- soft-decision FEC: the per-symbol body of calcLLR and the per-node bodies of LDPC belief propagation (SPA, MSA)
// as host/device-neutral templates on the message precision.  engine_fec.hip wraps them in gfx950 kernels (two engines: the whole
// decode of a codeword in one workgroup with the messages in LDS, or launches over all codewords with the messages in HBM);
// tests/emu/emu_fec.cpp loops the same text over nodes with g++.
// Reference: optic/comm/metrics.py:198-239 (calcLLR), optic/comm/fec.py:347-502 (sumProductAlgorithm), 505-681
// (minSumAlgorithm), 684-758 (decodeLDPC).
//
// Semantics (the reference's, which make parity with it possible):
//   schedule   flooding, per codeword.  V->C messages start at the input LLR (clipped to +-200, punctured rows 0).  An iteration is
//              the check update, the variable update, then the posterior with its hard decision and the parity test.  A codeword
//              stops at the first iteration whose decisions satisfy every check: its output is that iteration's posterior,
//              frameErrors = 0, lastIter = that iteration's index.  A codeword that never does gets the last iteration's posterior,
//              frameErrors = 1 and lastIter = maxIter - 1.
//   edge order the edges of check c are consecutive, in ascending column index (edge id = position in the CSR of H).  A variable
//              sums llr + sum of C->V over its edges in ascending check index, left to right; the outgoing message on an edge is
//              that sum minus the edge's own C->V message; the posterior is the same sum.
//   MSA        adds, compares and a product of signs: val >= 0 -> +1, the first minimum wins (strict <), the edge that gave the
//              minimum gets the second minimum.  No rounding freedom: bit-equal to the reference in the same precision, as long as
//              no multiply-add is contracted (compile with -ffp-contract=off).
//   SPA        tanh(x / 2) once per edge; the leave-one-out products are prefix x suffix products (no division: zeros occur);
//              the product is clipped to +-0.999999, where the message is +-2 atanh(0.999999) evaluated in double as the reference
//              evaluates it in either precision; otherwise 2 atanh(product).  The reference multiplies the d_c - 1 factors in
//              edge order: another rounding, so SPA is held to a tolerance.
//   decision   bit = posterior < 0 (an LLR of exactly 0 decodes to 0).
// One array of E messages serves both directions: a check reads the V->C values of its own edges and overwrites them with C->V, a
// variable reads the C->V values of its own edges and overwrites them with V->C.  `Idx` maps an edge id to its slot (the LDS engine
// pads its array, the global engine interleaves the codewords); it never changes the arithmetic.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FEC_HD __host__ __device__ inline
#else
#define FEC_HD inline
#endif

namespace ssf {
namespace fec {

enum { kSPA = 0, kMSA = 1 };                  // ssf_ldpc_params.alg
enum { kF64 = 0, kF32 = 1 };                  // ssf_ldpc_params.prec / in_dtype
enum { kEngineAuto = 0, kEngineLds = 1, kEngineGlobal = 2 };
constexpr int kMaxDeg = 64;                   // largest check or variable degree (the reference's tables: 30 and 13)
constexpr int kMaxBits = 10;                  // calcLLR: M <= 1024
constexpr double kClipLLR = 200.0;            // decodeLDPC clips its input
constexpr double kClipProd = 0.999999;        // SPA clips the product of tanh
constexpr double kSatMsg = 14.508657238495339;    // 2 atanh(0.999999) in double

struct Plain {
    FEC_HD int operator()(int e) const { return e; }
};
// codeword-minor arrays of the global engine: element e of codeword `off` of `stride`
struct Strided {
    long long stride, off;
    FEC_HD long long operator()(int e) const { return (long long)e * stride + off; }
};
// one unused slot after every 32: lanes that own consecutive checks of degree 8 (stride 8 slots) spread over all 32 banks
struct Padded {
    FEC_HD int operator()(int e) const { return e + (e >> 5); }
    static FEC_HD int slots(int E) { return E + (E >> 5) + 1; }
};

// element (v, cw) of the caller's LLR array: (n_, ncw) row-major, or (ncw, n_) with `transposed`
FEC_HD long long user_index(int v, int cw, int n_, int ncw, int transposed) {
    return transposed ? (long long)cw * n_ + v : (long long)v * ncw + cw;
}

// np.clip(llrs, -200, 200) in the input's type, then astype(prec); rows n_ .. n - 1 are the depuncturing zeros
template <class T>
FEC_HD T load_llr(const void *in, int in_dtype, int v, int cw, int n_, int ncw, int transposed) {
    if (v >= n_) return (T)0;
    const long long i = user_index(v, cw, n_, ncw, transposed);
    if (in_dtype == kF64) {
        double x = ((const double *)in)[i];
        x = x > kClipLLR ? kClipLLR : (x < -kClipLLR ? -kClipLLR : x);
        return (T)x;
    }
    float x = ((const float *)in)[i];
    x = x > (float)kClipLLR ? (float)kClipLLR : (x < -(float)kClipLLR ? -(float)kClipLLR : x);
    return (T)x;
}

template <class T>
FEC_HD T spa_message(T prod) {
    if (prod >= (T)kClipProd) return (T)kSatMsg;          // (the reference's min / max compare in the message type and hand the
    if (prod <= (T)-kClipProd) return (T)-kSatMsg;        //  double constant on at equality)
    return (T)2 * std::atanh(prod);
}

// ---- check update, SPA.  DC > 0: degrees up to DC with the tanh values in a fully unrolled array (registers on the device);
// DC = 0: any degree up to kMaxDeg with a loop.  The same products in the same order either way.
template <class T, int DC, class Idx>
FEC_HD void check_spa(T *msg, int beg, int end, Idx idx) {
    const int d = end - beg;
    if constexpr (DC > 0) {
        T t[DC];
        T run = (T)1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < DC; ++i) {
            if (i < d) {
                const auto s = idx(beg + i);
                t[i] = std::tanh(msg[s] / (T)2);
                msg[s] = run;                 // the product of the factors before this edge
                run *= t[i];
            }
        }
        run = (T)1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = DC - 1; i >= 0; --i) {
            if (i < d) {
                const auto s = idx(beg + i);
                msg[s] = spa_message<T>(msg[s] * run);
                run *= t[i];                  // the product of the factors after the next edge down
            }
        }
    } else {
        T t[kMaxDeg];
        T run = (T)1;
        for (int i = 0; i < d; ++i) {
            const auto s = idx(beg + i);
            t[i] = std::tanh(msg[s] / (T)2);
            msg[s] = run;
            run *= t[i];
        }
        run = (T)1;
        for (int i = d - 1; i >= 0; --i) {
            const auto s = idx(beg + i);
            msg[s] = spa_message<T>(msg[s] * run);
            run *= t[i];
        }
    }
}

// ---- check update, MSA
template <class T, class Idx>
FEC_HD void check_msa(T *msg, int beg, int end, Idx idx) {
    T min1 = (T)INFINITY, min2 = (T)INFINITY;
    int min1_e = -1, sign_prod = 1;
    for (int e = beg; e < end; ++e) {
        const T val = msg[idx(e)];
        const T a = std::fabs(val);
        sign_prod = val >= (T)0 ? sign_prod : -sign_prod;
        if (a < min1) {
            min2 = min1, min1 = a, min1_e = e;
        } else if (a < min2) {
            min2 = a;
        }
    }
    for (int e = beg; e < end; ++e) {
        const auto s = idx(e);
        const int sgn = msg[s] >= (T)0 ? sign_prod : -sign_prod;
        const T mag = e == min1_e ? min2 : min1;
        msg[s] = sgn > 0 ? mag : -mag;
    }
}

// ---- variable update with posterior and hard decision: var_edges[beg .. end) are the variable's edge ids, ascending check
template <class T, class Idx>
FEC_HD void var_update(T *msg, const int *var_edges, int beg, int end, T llr, T &post, unsigned char &bit, Idx idx) {
    T sum = llr;
    for (int k = beg; k < end; ++k) sum += msg[idx(var_edges[k])];
    for (int k = beg; k < end; ++k) {
        const auto s = idx(var_edges[k]);
        msg[s] = sum - msg[s];
    }
    post = sum;
    bit = sum < (T)0 ? 1 : 0;
}

// ---- parity of one check over the hard decisions: edge_var[beg .. end) are the check's variables
template <class Idx>
FEC_HD int check_parity(const unsigned char *bits, const int *edge_var, int beg, int end, Idx idx) {
    int p = 0;
    for (int e = beg; e < end; ++e) p ^= bits[idx(edge_var[e])];
    return p;
}

// one check update of the selected algorithm; MODE: -1 = MSA, 0 = SPA with a loop, 8 / 32 = SPA unrolled to that degree
template <class T, int MODE, class Idx>
FEC_HD void check_update(T *msg, int beg, int end, Idx idx) {
    if constexpr (MODE < 0) check_msa<T, Idx>(msg, beg, end, idx);
    else check_spa<T, MODE, Idx>(msg, beg, end, idx);
}
FEC_HD int spa_mode(int max_check_degree) { return max_check_degree <= 8 ? 8 : (max_check_degree <= 32 ? 32 : 0); }

// ---- calcLLR of one received symbol (re, im): prob_m = exp(-|r - c_m|^2 / sigma2) px_m with |.| as np.abs takes it (hypot);
// per bit position p0 and p1 are the sums of prob_m over m ascending with bit 0 / 1 (zero_mask / one_mask bit j of symbol m);
// llr[j] = log p0 - log p1: +-inf where one of them underflowed, as the reference gives.
FEC_HD void llr_body(double re, double im, double sigma2, int M, int b, const double *tab, const double *px, const unsigned *zero_mask,
                     const unsigned *one_mask, double *llr) {
    double p0[kMaxBits], p1[kMaxBits];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kMaxBits; ++j) p0[j] = p1[j] = 0.0;
    for (int m = 0; m < M; ++m) {
        const double h = std::hypot(re - tab[2 * m], im - tab[2 * m + 1]);
        const double prob = std::exp(-(h * h) / sigma2) * px[m];
        const unsigned z = zero_mask[m], o = one_mask[m];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < kMaxBits; ++j) {
            if ((z >> j) & 1u) p0[j] += prob;
            if ((o >> j) & 1u) p1[j] += prob;
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kMaxBits; ++j)
        if (j < b) llr[j] = std::log(p0[j]) - std::log(p1[j]);
}

// bytes of LDS the one-workgroup engine needs for a graph: padded messages, LLRs, posteriors (of the message type), the parity
// flag (16 bytes) and the bits
constexpr long long kLdsFlag = 16;
FEC_HD long long lds_bytes(long long E, long long n, int prec) {
    const long long w = prec == kF64 ? 8 : 4;
    return ((E + (E >> 5) + 1) + 2 * n) * w + kLdsFlag + ((n + 15) / 16) * 16;
}
constexpr long long kLdsBudget = 160 * 1024;  // per workgroup on gfx950

}  // namespace fec
}  // namespace ssf
