// engine_siso.hip -- ffe, dfe, volterra and anorm on the device (ssf_siso_eq of include/ssf.h).
//   scales   fixed-order reductions (block_reduce.h) give sqrt(mean |sigIn|^2), sqrt(mean |symbRef|^2) and, for volterra, the
//            maximum of the rounded normalised input.  The kernels below apply them in their loads: no normalised copy of the
//            signal is written.
//   serial   one wavefront walks every symbol that adapts or feeds a later decision, the passes of the pre-convergence included,
//            with R coefficients per lane in registers.  The window samples of a chunk of 64 symbols sit in LDS; the next chunk's
//            are loaded to registers while the current one is consumed and move to LDS at the chunk border.  Each lane forms its
//            regressor entries from LDS (up to three window reads per entry, offsets fixed at launch; for dfe the earlier
//            references come from a second LDS buffer, read once the symbol's reference is known).  One butterfly sum per symbol,
//            the error formed by every lane alike, the decision by wave_argmin.  Lane l keeps the output and |e|^2 of symbol l of
//            the chunk; they leave in one store per chunk.
//   frozen   ffe and volterra in data-aided mode: the symbols of the last pass from nTrain on whose window is a plain slice of
//            the padded input, one per thread, the tile's window samples, the coefficients and the table in LDS.
//   volterra's final pnorm: one fixed-order reduction over sigOut and one scaling pass.
// No communication between waves, no flags, no atomics: every loop's trip count is known at launch and results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "block_reduce.h"
#include "engine_host.h"
#include "siso_kernels.h"

namespace ssf {
namespace {
using namespace sk;
using namespace eng;

constexpr int kBlock = br::kBlock, kMaxBlocks = 1024;

template <bool CX> struct Store;
template <> struct Store<false> {
    using T = double;
    __device__ static T pack(V<false> v) { return v.re; }
    __device__ static V<false> unpack(T s) { return V<false>{s, 0.0}; }
};
template <> struct Store<true> {
    using T = Cplx;
    __device__ static T pack(V<true> v) { return Cplx{v.re, v.im}; }
    __device__ static V<true> unpack(T s) { return V<true>{s.re, s.im}; }
};

// ---- the scales
struct ScaleArgs {
    const void *x;
    int dtype, prec32, slot, nb, divide;      // divide: the maximum is taken of round(x / scal[0])
    long long n;
    double *part, *scal;
};

__global__ __launch_bounds__(kBlock) void k_siso_power(ScaleArgs a) {
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double re, im;
        mk::load(a.dtype, a.x, i, re, im);
        acc += re * re + im * im;
    }
    br::block_sum_store(acc, a.part + blockIdx.x);
}
__global__ __launch_bounds__(64) void k_siso_power_fin(ScaleArgs a) {
    const double s = br::wave_sum_partials(a.part, a.nb, 1);
    if (threadIdx.x == 0) a.scal[a.slot] = sqrt(s / (double)a.n);
}
__global__ __launch_bounds__(kBlock) void k_siso_max(ScaleArgs a) {
    const double sx = a.divide ? a.scal[0] : 1.0;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double re, im;
        mk::load(a.dtype, a.x, i, re, im);
        if (a.divide) re = round_prec(re / sx, a.prec32), im = round_prec(im / sx, a.prec32);
        acc = fmax(acc, im == 0.0 ? fabs(re) : sqrt(re * re + im * im));
    }
    br::block_max_store(acc, a.part + blockIdx.x);
}
__global__ __launch_bounds__(64) void k_siso_max_fin(ScaleArgs a) {
    const double s = br::wave_max_partials(a.part, a.nb);
    if (threadIdx.x == 0) a.scal[a.slot] = s;
}
// y = x / scal[slot]: anorm (any type in, double / complex128 out) and volterra's final pnorm (in place)
__global__ __launch_bounds__(kBlock) void k_siso_scale(ScaleArgs a, void *y) {
    const double s = a.scal[a.slot];
    const bool cx = a.dtype == mk::kC128 || a.dtype == mk::kC64;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double re, im;
        mk::load(a.dtype, a.x, i, re, im);
        if (cx) ((Cplx *)y)[i] = Cplx{re / s, im / s};
        else ((double *)y)[i] = re / s;
    }
}

// ---- the serial walk
struct SerialArgs {
    Geo g;
    const void *x, *ref;
    int xdtype, rdtype, R;
    long long serial_last, nchunks;
    const double *scal, *tab;
    void *coef;                               // ncoef values, in and out
    void *y;
    double *mse;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ int wave_argmin(double d, int i) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double d2 = __shfl_xor(d, o, kWave);
        const int i2 = __shfl_xor(i, o, kWave);
        argmin_merge(d, i, d2, i2);
    }
    return i;
}

// position of a chunk in the walk: pass and first symbol of the chunk inside the pass
struct Pos {
    int pass;
    long long c0;
};

template <int R, bool CX, bool VOL>
__global__ __launch_bounds__(kWave) void k_siso_serial(SerialArgs a) {
    using S = typename Store<CX>::T;
    using T = V<CX>;
    __shared__ S xs[kStageElems];             // the chunk's window samples, normalised
    __shared__ S refs[kChunk];                // its training symbols, normalised
    __shared__ S ds[kMaxFb + kChunk];         // dfe: the references of the kMaxFb symbols before the chunk, then the chunk's
    __shared__ Cplx head[2][kMaxTaps];        // the window a pass starts from after a restart, raw, by parity of the pass
    __shared__ double tabs[2 * kMaxM];
    const Geo &g = a.g;
    const int lane = threadIdx.x, nTaps = g.nTaps, SpS = g.SpS, M = g.M;
    const double sx = a.scal[0], sr = a.scal[1], mx = VOL ? a.scal[2] : 1.0;

    for (int i = lane; i < 2 * M; i += kWave) tabs[i] = a.tab[i];
    for (int i = lane; i < kMaxFb + kChunk; i += kWave) ds[i] = Store<CX>::pack(vzero<CX>());

    T h[R];
    int ent[R];                               // a slot's entry: offsets i0 | i1 << 8 | i2 << 16, degree << 24 (0: none; 4: feedback)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = lane + kWave * r;
        h[r] = vzero<CX>(), ent[r] = 0;
        if (c < g.ncoef) {
            const Entry e = entry_of(g, c);
            ent[r] = e.i0 | e.i1 << 8 | e.i2 << 16 | (e.fb ? 4 : e.deg) << 24;
            h[r] = Store<CX>::unpack(((const S *)a.coef)[c]);
        }
    }
    auto deg = [&](int r) { return ent[r] >> 24; };
    auto off0 = [&](int r) { return ent[r] & 255; };
    const double c0r = lane < M ? a.tab[2 * lane] : 0.0, c0i = lane < M ? a.tab[2 * lane + 1] : 0.0;
    const double mu1 = g.mu, mu2 = g.mu / 2, mu3 = g.mu / 7;

    auto pass_len = [&](int pass) { return pass + 1 < g.passes ? g.nTrain + 1 : a.serial_last; };
    auto advance = [&](Pos p) {
        p.c0 += kChunk;
        if (p.c0 >= pass_len(p.pass)) p.c0 = 0, ++p.pass;
        return p;
    };
    // sample q of a pass's stream, raw
    auto stream_raw = [&](int pass, long long q, double &re, double &im) {
        if (pass > 0 && q < nTaps) {
            const Cplx v = head[pass & 1][q];
            re = v.re, im = v.im;
        } else {
            padded_raw(g, a.xdtype, a.x, q, re, im);
        }
    };

    // the loads of one chunk, raw: window sample e 64 + lane of the chunk and the lane's training symbol
    double pre_re[kPre], pre_im[CX ? kPre : 1], pref_re = 0.0, pref_im = 0.0;
    auto fetch = [&](Pos p) {
        const long long left = pass_len(p.pass) - p.c0;
        const int cnt = left < kChunk ? (int)left : kChunk;
        const int elems = (cnt - 1) * SpS + nTaps;
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const int idx = e * kWave + lane;
            double re = 0.0, im = 0.0;
            if (idx < elems) stream_raw(p.pass, p.c0 * SpS + idx, re, im);
            pre_re[e] = re;
            if constexpr (CX) pre_im[e] = im;
        }
        const long long k = p.c0 + lane;
        pref_re = 0.0, pref_im = 0.0;
        if (lane < cnt && k < g.nTrain) mk::load(a.rdtype, a.ref, k, pref_re, pref_im);
    };
    auto to_lds = [&]() {
        __syncthreads();                      // (one wave: the reads of the chunk before are done)
#pragma unroll
        for (int e = 0; e < kPre; ++e) xs[e * kWave + lane] = Store<CX>::pack(normalise<CX>(g, sx, mx, pre_re[e], pre_im[CX ? e : 0]));
        refs[lane] = Store<CX>::pack(normalise_ref<CX>(g, sr, pref_re, pref_im));
        __syncthreads();
    };
    auto entry = [&](int r, int il) -> T {
        T v = Store<CX>::unpack(xs[il * SpS + off0(r)]);
        if constexpr (VOL) {
            if (deg(r) >= 2) v.re *= Store<CX>::unpack(xs[il * SpS + (ent[r] >> 8 & 255)]).re;
            if (deg(r) >= 3) v.re *= Store<CX>::unpack(xs[il * SpS + (ent[r] >> 16 & 255)]).re;
        }
        return v;
    };

    Pos cur{0, 0};
    if (a.nchunks > 0) {
        fetch(cur);
        to_lds();
    }
    for (long long ci = 0; ci < a.nchunks; ++ci) {
        if (cur.c0 == 0 && cur.pass + 1 < g.passes) {
            // the window the next pass starts from: what this pass's stream holds behind symbol nTrain
            double hr[kMaxTaps / kWave], hi[kMaxTaps / kWave];
#pragma unroll
            for (int j = 0; j < kMaxTaps / kWave; ++j) {
                hr[j] = 0.0, hi[j] = 0.0;
                const int t = j * kWave + lane;
                if (t < nTaps) stream_raw(cur.pass, (g.nTrain + 1) * SpS + t, hr[j], hi[j]);
            }
#pragma unroll
            for (int j = 0; j < kMaxTaps / kWave; ++j) head[(cur.pass + 1) & 1][j * kWave + lane] = Cplx{hr[j], hi[j]};
            __syncthreads();
        }
        const Pos nxt = advance(cur);
        if (ci + 1 < a.nchunks) fetch(nxt);   // in flight while this chunk is consumed
        const long long left = pass_len(cur.pass) - cur.c0;
        const int cnt = left < kChunk ? (int)left : kChunk;

        T xn[R], ybuf = vzero<CX>();
        double ebuf = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xn[r] = vzero<CX>();
            if (deg(r) == 4) xn[r] = Store<CX>::unpack(ds[kMaxFb - 1 - off0(r)]);
            else if (deg(r) > 0) xn[r] = entry(r, 0);
        }
        for (int il = 0; il < cnt; ++il) {
            T phi[R];
#pragma unroll
            for (int r = 0; r < R; ++r) phi[r] = xn[r];
            if (il + 1 < cnt) {               // the next symbol's window entries: issued ahead of this symbol's reduction
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (deg(r) > 0 && deg(r) < 4) xn[r] = entry(r, il + 1);
            }
            T y = lane_output<R, CX>(h, phi);
            y.re = wave_sum(y.re);
            if (CX) y.im = wave_sum(y.im);

            const long long k = cur.c0 + il;
            T rf;
            if (k < g.nTrain) {
                rf = Store<CX>::unpack(refs[il]);
            } else {
                double d = INFINITY;
                int bi = kMaxM;
                if (lane < M) d = dist<CX>(y, c0r, c0i), bi = lane;
                for (int m = lane + kWave; m < M; m += kWave) argmin_merge(d, bi, dist<CX>(y, tabs[2 * m], tabs[2 * m + 1]), m);
                bi = wave_argmin(d, bi);
                bi = bi < M ? bi : M - 1;     // (a NaN output decides nothing: stay inside the table)
                rf = T{tabs[2 * bi], CX ? tabs[2 * bi + 1] : 0.0};
            }
            double esq;
            const T e = error_of<CX>(rf, y, esq);
            if (g.fulltime || k < g.nTrain) {
                const T w1{mu1 * e.re, CX ? mu1 * e.im : 0.0};
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    T w = w1;
                    if (VOL) w.re = deg(r) == 2 ? mu2 * e.re : deg(r) == 3 ? mu3 * e.re : w1.re;
                    vupdate<CX>(h[r], w, phi[r]);
                }
            }
            if (g.nFB > 0) {                  // dfe: this symbol's reference is the newest entry of the next symbol's feedback
                if (lane == 0) ds[kMaxFb + il] = Store<CX>::pack(rf);
                __syncthreads();
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (deg(r) == 4) xn[r] = Store<CX>::unpack(ds[kMaxFb + il - off0(r)]);
            }
            if (lane == il) ybuf = y, ebuf = esq;
        }
        if (lane < cnt) {
            ((S *)a.y)[cur.c0 + lane] = Store<CX>::pack(ybuf);
            a.mse[cur.c0 + lane] = ebuf;
        }
        if (g.nFB > 0) {                      // the last kMaxFb references move ahead of the next chunk
            double kr[kMaxFb / kWave], ki[kMaxFb / kWave];
#pragma unroll
            for (int j = 0; j < kMaxFb / kWave; ++j) {
                const T v = Store<CX>::unpack(ds[cnt + j * kWave + lane]);
                kr[j] = v.re, ki[j] = v.im;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kMaxFb / kWave; ++j) ds[j * kWave + lane] = Store<CX>::pack(T{kr[j], ki[j]});
            __syncthreads();
        }
        if (ci + 1 < a.nchunks) to_lds();
        cur = nxt;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = lane + kWave * r;
        if (c < g.ncoef) ((S *)a.coef)[c] = Store<CX>::pack(h[r]);
    }
}

// ---- the frozen tail
struct FrozenArgs {
    Geo g;
    const void *x;
    int xdtype;
    long long from, count;
    const double *scal, *tab;
    const void *coef;
    void *y;
    double *mse;
};

template <bool CX>
__global__ __launch_bounds__(kTile) void k_siso_frozen(FrozenArgs a) {
    using S = typename Store<CX>::T;
    using T = V<CX>;
    extern __shared__ double lds[];
    const Geo &g = a.g;
    T *w = (T *)lds;                                          // (kTile - 1) SpS + nTaps window samples
    T *coef = w + (kTile - 1) * g.SpS + g.nTaps;              // ncoef coefficients
    double *tab = (double *)(coef + g.ncoef);                 // 2 M
    const long long k0 = a.from + (long long)blockIdx.x * kTile;
    const long long left = a.from + a.count - k0;
    const int cnt = left < kTile ? (int)left : kTile;
    const int elems = (cnt - 1) * g.SpS + g.nTaps;
    const double sx = a.scal[0], mx = g.kind == kVolterra ? a.scal[2] : 1.0;
    for (int i = threadIdx.x; i < elems; i += kTile) {
        double re, im;
        padded_raw(g, a.xdtype, a.x, k0 * g.SpS + i, re, im);
        w[i] = normalise<CX>(g, sx, mx, re, im);
    }
    for (int i = threadIdx.x; i < g.ncoef; i += kTile) coef[i] = Store<CX>::unpack(((const S *)a.coef)[i]);
    for (int i = threadIdx.x; i < 2 * g.M; i += kTile) tab[i] = a.tab[i];
    __syncthreads();
    if ((int)threadIdx.x >= cnt) return;
    const T y = frozen_output<CX>(g, coef, w + threadIdx.x * g.SpS);
    const int bi = nearest<CX>(tab, g.M, y);
    double esq;
    error_of<CX>(T{tab[2 * bi], CX ? tab[2 * bi + 1] : 0.0}, y, esq);
    ((S *)a.y)[k0 + threadIdx.x] = Store<CX>::pack(y);
    a.mse[k0 + threadIdx.x] = esq;
}

// ---- host side
struct Work : WorkBase {
    Buf in, refin, coef, tables, out, mse, part, scal;
    std::vector<double> host_tab;             // kept for its capacity
};
using Call = CallT<Work>;

template <int R, bool CX, bool VOL> void launch_serial(const SerialArgs &a, hipStream_t st) { k_siso_serial<R, CX, VOL><<<1, kWave, 0, st>>>(a); }
// (ffe and dfe have at most kMaxTaps + kMaxFb = 512 coefficients: eight per lane)
template <bool CX, bool VOL> void launch_serial_r(const SerialArgs &a, hipStream_t st) {
    switch (a.R) {
    case 1: return launch_serial<1, CX, VOL>(a, st);
    case 2: return launch_serial<2, CX, VOL>(a, st);
    case 4: return launch_serial<4, CX, VOL>(a, st);
    case 8: return launch_serial<8, CX, VOL>(a, st);
    }
    if constexpr (VOL) {
        if (a.R == 16) return launch_serial<16, CX, VOL>(a, st);
        return launch_serial<24, CX, VOL>(a, st);
    }
}

// a fixed-order reduction of `count` values into scal[slot]: the mean power's root, or the maximum modulus
bool reduce_to(Call &c, const void *xd, int dtype, long long count, int slot, bool maximum, bool divide, int prec32) {
    Work &w = *c.w;
    ScaleArgs s{};
    s.x = xd, s.dtype = dtype, s.prec32 = prec32, s.slot = slot, s.n = count, s.divide = divide;
    s.nb = grid_blocks(count, kBlock, kMaxBlocks), s.part = (double *)w.part.p, s.scal = (double *)w.scal.p;
    if (maximum) {
        k_siso_max<<<s.nb, kBlock, 0, w.st>>>(s);
        k_siso_max_fin<<<1, 64, 0, w.st>>>(s);
    } else {
        k_siso_power<<<s.nb, kBlock, 0, w.st>>>(s);
        k_siso_power_fin<<<1, 64, 0, w.st>>>(s);
    }
    return c.launched();
}

}  // namespace

int siso_run(int device, ssf_siso_params *p, const double *table, void *coef_inout, const void *x, const void *ref, void *sig_out,
             double *mse_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const bool cx = p->dtype == mk::kC128 || p->dtype == mk::kC64;
    const size_t val = cx ? sizeof(Cplx) : sizeof(double);
    if (!c.need(w.part, (size_t)kMaxBlocks * sizeof(double)) || !c.need(w.scal, kScalN * sizeof(double))) return c.rc;

    if (p->kind == kAnorm) {
        const size_t out_bytes = (size_t)p->n * val;
        void *y = c.target(sig_out, w.out, out_bytes);
        if (!y) return c.rc;
        const void *xd = c.input(x, w.in, (size_t)p->n * mk::elem_size(p->dtype));
        if (!xd) return c.rc;
        if (!reduce_to(c, xd, p->dtype, p->n, 2, true, false, 0)) return c.rc;
        ScaleArgs s{};
        s.x = xd, s.dtype = p->dtype, s.slot = 2, s.n = p->n, s.scal = (double *)w.scal.p;
        k_siso_scale<<<grid_blocks(p->n, kBlock, kMaxBlocks), kBlock, 0, w.st>>>(s, y);
        if (!c.launched() || !c.deliver(sig_out, y, out_bytes) || !c.sync()) return c.rc;
        return SSF_OK;
    }

    Geo g{};
    g.n = p->n, g.SpS = p->SpS, g.nTaps = p->nTaps, g.Lpad = p->nTaps / 2, g.L = p->n + 2 * g.Lpad, g.N = p->n / p->SpS;
    g.nTrain = p->nTrain, g.kind = p->kind, g.cx = cx, g.fulltime = p->mode == kFulltime, g.order = p->order;
    g.nFB = p->kind == kDfe ? p->nFB : 0, g.n2 = p->n2, g.n3 = p->n3, g.t2 = (p->nTaps - p->n2) / 2, g.t3 = (p->nTaps - p->n3) / 2;
    g.M = p->M, g.prec32 = p->prec32, g.ncoef = p->ncoef, g.mu = p->mu;
    g.passes = p->nTrain < g.N ? p->preconvIters : 1;
    const Split sp = split_of(g, !p->no_frozen);

    const size_t out_bytes = (size_t)g.N * val, mse_bytes = (size_t)g.N * sizeof(double), coef_bytes = (size_t)p->ncoef * val;
    void *y = c.target(sig_out, w.out, out_bytes);
    double *mse = (double *)c.target(mse_out, w.mse, mse_bytes);
    if (!y || !mse || !c.need(w.coef, coef_bytes)) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)p->n * mk::elem_size(p->dtype));
    if (!xd) return c.rc;
    const void *rd = xd;                      // (never read where there is no training symbol)
    int rdtype = p->dtype;
    if (p->nref > 0) {
        rd = c.input(ref, w.refin, (size_t)p->nref * mk::elem_size(p->ref_dtype));
        if (!rd) return c.rc;
        rdtype = p->ref_dtype;
    }
    if (!c.h2d(w.coef.p, coef_inout, coef_bytes)) return c.rc;
    std::vector<double> &tab = w.host_tab;
    tab.assign(table, table + 2 * (size_t)p->M);
    if (!c.upload(w.tables, tab)) return c.rc;

    if (!reduce_to(c, xd, p->dtype, p->n, 0, false, false, 0)) return c.rc;
    if (p->nref > 0 && !reduce_to(c, rd, rdtype, p->nref, 1, false, false, 0)) return c.rc;
    if (p->kind == kVolterra && !reduce_to(c, xd, p->dtype, p->n, 2, true, true, p->prec32)) return c.rc;

    const int R = slots_for(p->ncoef);
    if (sp.serial_total > 0) {
        SerialArgs a{};
        a.g = g, a.x = xd, a.ref = rd, a.xdtype = p->dtype, a.rdtype = rdtype, a.R = R, a.serial_last = sp.serial_last;
        a.nchunks = (long long)(g.passes - 1) * ((g.nTrain + 1 + kChunk - 1) / kChunk) + (sp.serial_last + kChunk - 1) / kChunk;
        a.scal = (const double *)w.scal.p, a.tab = (const double *)w.tables.p, a.coef = w.coef.p, a.y = y, a.mse = mse;
        if (p->kind == kVolterra) launch_serial_r<false, true>(a, w.st);
        else if (cx) launch_serial_r<true, false>(a, w.st);
        else launch_serial_r<false, false>(a, w.st);
        if (!c.launched()) return c.rc;
    }
    if (sp.frozen_count > 0) {
        FrozenArgs f{};
        f.g = g, f.x = xd, f.xdtype = p->dtype, f.from = sp.frozen_from, f.count = sp.frozen_count;
        f.scal = (const double *)w.scal.p, f.tab = (const double *)w.tables.p, f.coef = w.coef.p, f.y = y, f.mse = mse;
        const size_t lds = ((size_t)(kTile - 1) * g.SpS + g.nTaps + p->ncoef) * sizeof(V<false>) + 2 * (size_t)p->M * sizeof(double);
        const unsigned nb = (unsigned)((sp.frozen_count + kTile - 1) / kTile);
        const void *fn = cx ? (const void *)k_siso_frozen<true> : (const void *)k_siso_frozen<false>;
        if (!c.ok(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute")) return c.rc;
        if (cx) k_siso_frozen<true><<<nb, kTile, lds, w.st>>>(f);
        else k_siso_frozen<false><<<nb, kTile, lds, w.st>>>(f);
        if (!c.launched()) return c.rc;
    }
    if (p->kind == kVolterra) {               // pnorm(sigOut)
        if (!reduce_to(c, y, mk::kF64, g.N, 3, false, false, 0)) return c.rc;
        ScaleArgs s{};
        s.x = y, s.dtype = mk::kF64, s.slot = 3, s.n = g.N, s.scal = (double *)w.scal.p;
        k_siso_scale<<<grid_blocks(g.N, kBlock, kMaxBlocks), kBlock, 0, w.st>>>(s, y);
        if (!c.launched()) return c.rc;
    }
    if (!c.deliver(coef_inout, w.coef.p, coef_bytes) || !c.deliver(sig_out, y, out_bytes) || !c.deliver(mse_out, mse, mse_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    p->serial_symbols = sp.serial_total, p->parallel_symbols = sp.frozen_count, p->R = sp.serial_total > 0 ? R : 0;
    return SSF_OK;
}

}  // namespace ssf
