// array_kernels.h -- the general array layer of DeviceArray (opticommpy_amd/device.py): strided copies, take, the element-wise
// arithmetic, the reductions' per-element bodies and freqShift as host/device-neutral inline functions.  engine_array.hip wraps
// them in gfx950 kernels; tests/emu/emu_array.cpp walks the same functions with g++.
// numpy is the definition.  Arithmetic is double: single-precision data are widened on load and rounded once on store, which for
// one +, -, x, / or sqrt is the correctly rounded single-precision result (53 >= 2 24 + 2 bits), so those agree with numpy bit for
// bit.  A real operand beside a complex one is promoted to (re, +0) and goes through the complex formula, as numpy's casts do.
// The translation unit is compiled without contraction of multiply-adds.
// Reference for freq_shift: optic/dsp/core.py:1050-1072 (freqShift).
#pragma once
#include <cmath>
#include <cstdint>

#include "metrics_kernels.h"

namespace ssf {
namespace ak {

constexpr int kBlock = 256;        // lanes per workgroup of every kernel of the engine
constexpr int kMaxBlocks = 4096;   // workgroups of a grid-stride element-wise or movement pass
constexpr int kRedBlocks = 256;    // workgroups of a reduction per column: the number of partials, which fixes the order of the sum
constexpr int kTile = 32;          // the transpose moves kTile x kTile elements per workgroup through LDS (rows padded by one)
constexpr int kMaxDim = 4;

enum { kAdd = 0, kSub = 1, kMul = 2, kDiv = 3 };                                                     // ssf_array_binary_op
enum { kNeg = 0, kConj = 1, kReal = 2, kImag = 3, kAbs = 4, kAbs2 = 5, kAngle = 6, kExp = 7, kSqrt = 8, kConvert = 9 };   // ssf_array_unary_op
enum { kSame = 0, kScalar = 1, kRow = 2, kColumn = 3 };                                              // ssf_array_bcast
enum { kSum = 0, kSumSqDev = 1, kMin = 2, kMax = 3 };                                                // ssf_array_reduce_op

MK_HD bool is_single(int dtype) { return dtype == mk::kC64 || dtype == mk::kF32; }
MK_HD bool is_complex(int dtype) { return dtype == mk::kC128 || dtype == mk::kC64; }
MK_HD bool good_dtype(int dtype) { return dtype >= mk::kC128 && dtype <= mk::kF32; }
MK_HD bool good_itemsize(int s) { return s == 1 || s == 2 || s == 4 || s == 8 || s == 16; }
// elements a lane moves at once so that it writes 16 bytes
MK_HD int vec_width(int out_dtype) { return 16 / (int)mk::elem_size(out_dtype); }

struct C2 {
    double re, im;
};

// ---- movement
struct Desc {
    int ndim;
    long long offset;              // of element (0, 0, ..), in elements
    long long shape[kMaxDim], stride[kMaxDim];       // strides in elements, any sign
};
// element offset of the q-th element in C order
MK_HD long long strided_offset(const Desc &d, long long q) {
    long long off = d.offset;
    for (int a = d.ndim - 1; a >= 0; --a) {
        const long long s = d.shape[a], i = q % s;
        q /= s;
        off += i * d.stride[a];
    }
    return off;
}
MK_HD long long desc_count(const Desc &d) {
    long long c = 1;
    for (int a = 0; a < d.ndim; ++a) c *= d.shape[a];
    return c;
}
// lowest and highest element offset a descriptor reaches (count > 0)
MK_HD void desc_extent(const Desc &d, long long &lo, long long &hi) {
    lo = hi = d.offset;
    for (int a = 0; a < d.ndim; ++a) {
        const long long span = (d.shape[a] - 1) * d.stride[a];
        if (span < 0) lo += span;
        else hi += span;
    }
}
// whether the descriptor walks its elements one after the other in memory
MK_HD bool desc_contiguous(const Desc &d) {
    long long want = 1;
    for (int a = d.ndim - 1; a >= 0; --a) {
        if (d.shape[a] != 1 && d.stride[a] != want) return false;
        want *= d.shape[a];
    }
    return true;
}
// row of the source that output row i of take reads: negative entries wrap, anything still outside is clamped
MK_HD long long take_row(long long idx, long long n_src) {
    if (idx < 0) idx += n_src;
    return idx < 0 ? 0 : idx >= n_src ? n_src - 1 : idx;
}

// ---- element-wise arithmetic
MK_HD void sincos_d(double t, double &s, double &c) {
#if defined(__HIP_DEVICE_COMPILE__)
    ::sincos(t, &s, &c);                  // (full-range argument reduction in double precision)
#else
    s = std::sin(t), c = std::cos(t);
#endif
}

// numpy's complex quotient (Smith's form, loops_arithmetic: @TYPE@_divide)
MK_HD C2 smith_div(C2 a, C2 b) {
    const double br = std::fabs(b.re), bi = std::fabs(b.im);
    if (br >= bi) {
        if (br == 0.0 && bi == 0.0) return C2{a.re / br, a.im / bi};
        const double rat = b.im / b.re, scl = 1.0 / (b.re + b.im * rat);
        return C2{(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const double rat = b.re / b.im, scl = 1.0 / (b.im + b.re * rat);
    return C2{(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

// a op b; cplx: the result type is complex (a real operand then carries im = +0)
MK_HD C2 binary(int op, C2 a, C2 b, bool cplx) {
    if (!cplx) {
        switch (op) {
        case kAdd: return C2{a.re + b.re, 0.0};
        case kSub: return C2{a.re - b.re, 0.0};
        case kMul: return C2{a.re * b.re, 0.0};
        default: return C2{a.re / b.re, 0.0};
        }
    }
    switch (op) {
    case kAdd: return C2{a.re + b.re, a.im + b.im};
    case kSub: return C2{a.re - b.re, a.im - b.im};
    case kMul: return C2{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
    default: return smith_div(a, b);
    }
}

// op(x); cplx: x is complex.  Results of kReal, kImag, kAbs, kAbs2 and kAngle are real (in .re)
MK_HD C2 unary(int op, C2 x, bool cplx) {
    switch (op) {
    case kNeg: return C2{-x.re, cplx ? -x.im : 0.0};
    case kConj: return C2{x.re, cplx ? -x.im : 0.0};
    case kReal: return C2{x.re, 0.0};
    case kImag: return C2{cplx ? x.im : 0.0, 0.0};
    case kAbs: return C2{cplx ? std::hypot(x.re, x.im) : std::fabs(x.re), 0.0};       // hypot: no overflow below the true value's
    case kAbs2: return C2{cplx ? x.re * x.re + x.im * x.im : x.re * x.re, 0.0};
    case kAngle: return C2{std::atan2(cplx ? x.im : 0.0, x.re), 0.0};
    case kExp: {
        if (!cplx) return C2{std::exp(x.re), 0.0};
        double s, c;
        sincos_d(x.im, s, c);
        const double e = std::exp(x.re);
        return C2{e * c, e * s};
    }
    case kSqrt: return C2{std::sqrt(x.re), 0.0};
    default: return C2{x.re, cplx ? x.im : 0.0};                                       // kConvert
    }
}

MK_HD C2 load(int dtype, const void *p, long long q) {
    C2 v;
    mk::load(dtype, p, q, v.re, v.im);
    if (!is_complex(dtype)) v.im = 0.0;
    return v;
}
MK_HD void store(int dtype, void *p, long long q, C2 v) {
    switch (dtype) {
    case mk::kC128: ((mk::Cplx *)p)[q] = mk::Cplx{v.re, v.im}; break;
    case mk::kC64: ((mk::CplxF *)p)[q] = mk::CplxF{(float)v.re, (float)v.im}; break;
    case mk::kF64: ((double *)p)[q] = v.re; break;
    default: ((float *)p)[q] = (float)v.re; break;
    }
}

// the second operand's element for output element q
struct Bcast {
    int kind;
    long long inner;               // kRow: the row's length; kColumn: the elements of a until the column's next value
    C2 scalar;
};
MK_HD long long bcast_index(const Bcast &b, long long q) { return b.kind == kRow ? q % b.inner : b.kind == kColumn ? q / b.inner : q; }

// ---- reductions: per-element terms, and the rule by which one (value, index) candidate beats another
MK_HD C2 reduce_term(int op, C2 x, C2 center) {
    if (op == kSum) return x;
    const double dr = x.re - center.re, di = x.im - center.im;
    return C2{dr * dr + di * di, 0.0};
}
// numpy's argmin / argmax: a NaN wins, the lowest index on a tie (i < 0: no candidate yet)
MK_HD bool extreme_beats(int op, double v2, long long i2, double v, long long i) {
    if (i2 < 0) return false;
    if (i < 0) return true;
    const bool n2 = v2 != v2, n = v != v;
    if (n2 || n) return n2 && (!n || i2 < i);
    if (v2 == v) return i2 < i;
    return op == kMin ? v2 < v : v2 > v;
}

// ---- freqShift: y[k, c] = x[k, c] exp(1j ((2 pi) deltaF) (k (1 / Fs))), the reference's order of operations
MK_HD C2 freq_shift(C2 x, long long k, double w, double Ts) {
    double s, c;
    sincos_d(w * ((double)k * Ts), s, c);
    return C2{x.re * c - x.im * s, x.re * s + x.im * c};
}

}  // namespace ak
}  // namespace ssf
