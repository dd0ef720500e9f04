// engine_eq.hip -- adaptive MIMO equalizer on the device (ssf_mimo_eq of include/ssf.h).
//   serial   one wavefront per output mode holds the nModes nTaps coefficients that make that mode in registers (R per lane) and
//            walks the symbols of a run of consecutive adaptive stages, the numIter replay of stage 0 included, in one launch.
//            Per symbol: one butterfly reduction of the tap products (and of |x|^2 per input mode for NLMS), the error formed by
//            every lane alike, the update in registers.  The padded input of a chunk of symbols sits in LDS; the next chunk's is
//            loaded to registers (coalesced) while the current one is consumed and moves to LDS at the chunk border, so no global
//            load is on the dependent chain.  The next symbol's LDS reads are issued ahead of the current reduction.  Lane l
//            keeps the output and |e|^2 of symbol l of the chunk; they leave in one store per chunk.
//   static   one thread per output symbol and mode, H fixed.
// No communication between waves, no flags, no atomics: every loop's trip count is known at launch and results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "engine_host.h"
#include "eq_kernels.h"

namespace ssf {
namespace {
using namespace eqk;
using namespace eng;

constexpr int kStaticBlock = 256;
constexpr int kMaxSegs = 8;                   // segments of one serial launch: they travel as kernel arguments (scalar loads, no
                                              // vector load behind the prefetch in the wave's in-order memory counter)

struct EqArgs {
    const void *x, *ref;
    int xdtype, rdtype;
    long long n, total;
    int nModes, nTaps, SpS, Lpad, M, nRad, nseg, Cs;
    long long nchunks;
    double Rcma;
    const double *tab, *rad;
    Seg segs[kMaxSegs];
    Cplx *H;                                  // (nModes^2, nTaps)
    Cplx *y;                                  // (total, nModes)
    double *esq;                              // (nModes, total) or NULL
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

// position of a chunk in the walk: segment, repetition, first symbol of the chunk inside the segment
struct Pos {
    int s, rep;
    long long c0;
};
__device__ __forceinline__ Pos advance(Pos p, const Seg *segs, int Cs) {
    p.c0 += Cs;
    if (p.c0 >= segs[p.s].len) {
        p.c0 = 0;
        if (++p.rep >= segs[p.s].reps) p.rep = 0, ++p.s;
    }
    return p;
}

template <int R, typename XT>
__global__ __launch_bounds__(kWave) void k_eq_serial(EqArgs a) {
    __shared__ Cplx xs[kStageElems];
    __shared__ Cplx refs[kChunk];
    __shared__ double tabs[2 * kMaxM];
    __shared__ double rads[kMaxRadii];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int nModes = a.nModes, nTaps = a.nTaps, stride = a.SpS * nModes;

    for (int i = lane; i < 2 * a.M; i += kWave) tabs[i] = a.tab[i];
    for (int i = lane; i < a.nRad; i += kWave) rads[i] = a.rad[i];

    Cplx h[R];
    int off[R], mode[R];
    bool has[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int N, t;
        has[r] = lane_coeff(lane, r, nModes, nTaps, N, t);
        off[r] = t * nModes + N, mode[r] = N;
        h[r] = has[r] ? a.H[(long long)(k + N * nModes) * nTaps + t] : Cplx{0.0, 0.0};
    }
    // the decision point this lane tests first (tables of up to 64 points need no LDS read on the dependent chain)
    const double c0r = lane < a.M ? a.tab[2 * lane] : 0.0, c0i = lane < a.M ? a.tab[2 * lane + 1] : 0.0;
    const double rad0 = lane < a.nRad ? a.rad[lane] : 0.0;

    // the loads of one chunk: its padded input (element e 64 + lane of the chunk, modes interleaved as in memory) and its reference
    // symbol, kept as loaded (XT: complex128 or complex64) so that no load waits for another; they are widened on the way to LDS
    XT pre[kPre];
    double pref0 = 0.0, pref1 = 0.0;          // the reference symbol as loaded: (re, im), or both floats of a complex64 in pref0
    const bool rwide = a.rdtype == mk::kC128;
    auto fetch = [&](Pos p) {
        const Seg sg = a.segs[p.s];
        const long long g0 = sg.start + p.c0;
        const long long left = sg.len - p.c0;
        const int cnt = left < a.Cs ? (int)left : a.Cs;
        const int elems = ((cnt - 1) * a.SpS + nTaps) * nModes;
        const long long first = (g0 * a.SpS - a.Lpad) * nModes;      // element of x the chunk starts at (negative inside the padding)
        const long long count = a.n * nModes;
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const int idx = e * kWave + lane;
            const long long g = first + idx;
            pre[e] = XT{0, 0};
            if (idx < elems && g >= 0 && g < count) pre[e] = ((const XT *)a.x)[g];
        }
        // (the reference is loaded by every lane whatever the rule, from element 0 where the lane has no symbol: its register is
        //  not written again behind the load in flight, which would make the wave wait for the whole prefetch.  The input loads
        //  above are each guarded by their bounds and write registers nothing else touches until to_lds.  a.ref is never NULL
        //  here: ssf::eq_run points it at x when no stage is data-aided)
        const long long ri = (sg.alg == kNlms || sg.alg == kDaRde) && lane < cnt ? (g0 + lane) * nModes + k : 0;
        const double *rp = (const double *)a.ref;
        pref0 = rp[rwide ? 2 * ri : ri], pref1 = rp[rwide ? 2 * ri + 1 : ri];
    };
    auto to_lds = [&]() {
        __syncthreads();                      // (one wave: the reads of the chunk before are done)
#pragma unroll
        for (int e = 0; e < kPre; ++e) xs[e * kWave + lane] = Cplx{(double)pre[e].re, (double)pre[e].im};
        const float r32 = __int_as_float(__double2loint(pref0)), i32 = __int_as_float(__double2hiint(pref0));
        refs[lane] = rwide ? Cplx{pref0, pref1} : Cplx{(double)r32, (double)i32};
        __syncthreads();
    };

    Pos cur{0, 0, 0};
    fetch(cur);
    to_lds();
    for (long long ci = 0; ci < a.nchunks; ++ci) {
        const Pos nxt = advance(cur, a.segs, a.Cs);
        if (ci + 1 < a.nchunks) fetch(nxt);   // in flight while this chunk is consumed
        const Seg sg = a.segs[cur.s];
        const long long g0 = sg.start + cur.c0;
        const long long left = sg.len - cur.c0;
        const int cnt = left < a.Cs ? (int)left : a.Cs;
        const int alg = sg.alg;
        const double mu = sg.mu;

        Cplx xn[R], rn = refs[0], ybuf{0.0, 0.0};
        double ebuf = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) xn[r] = has[r] ? xs[off[r]] : Cplx{0.0, 0.0};
        for (int il = 0; il < cnt; ++il) {
            Cplx x[R];
            const Cplx rf = rn;
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = xn[r];
            if (il + 1 < cnt) {               // the next symbol's window and reference: issued ahead of this symbol's reduction
#pragma unroll
                for (int r = 0; r < R; ++r) xn[r] = has[r] ? xs[(il + 1) * stride + off[r]] : Cplx{0.0, 0.0};
                rn = refs[il + 1];
            }
            double yr, yi;
            lane_output<R>(h, x, yr, yi);
            yr = wave_sum(yr), yi = wave_sum(yi);

            Err e;
            double scl[kMaxModes] = {1.0, 1.0, 1.0, 1.0};
            if (alg == kNlms) {
                double pw[kMaxModes];
                lane_power<R>(x, mode, pw);
#pragma unroll
                for (int m = 0; m < kMaxModes; ++m)
                    if (m < nModes) scl[m] = nlms_scale(wave_sum(pw[m]));
                e = err_linear(rf.re, rf.im, yr, yi);
            } else if (alg == kDdLms) {
                double d = INFINITY;
                int bi = kMaxM;
                if (lane < a.M) d = dist_point(c0r, c0i, yr, yi), bi = lane;
                for (int m = lane + kWave; m < a.M; m += kWave) argmin_merge(d, bi, dist_point(tabs[2 * m], tabs[2 * m + 1], yr, yi), m);
                bi = wave_argmin(d, bi);
                bi = bi < a.M ? bi : a.M - 1;      // (a NaN output decides nothing: stay inside the table)
                e = err_linear(tabs[2 * bi], tabs[2 * bi + 1], yr, yi);
            } else if (alg == kRde) {
                const double ay = sqrt(yr * yr + yi * yi);
                double d = INFINITY;
                int bi = kMaxRadii;
                if (lane < a.nRad) d = dist_radius(rad0, ay), bi = lane;
                for (int m = lane + kWave; m < a.nRad; m += kWave) argmin_merge(d, bi, dist_radius(rads[m], ay), m);
                bi = wave_argmin(d, bi);
                bi = bi < a.nRad ? bi : a.nRad - 1;
                const double Rd = rads[bi];
                e = err_radius(Rd * Rd, yr, yi);
            } else if (alg == kDaRde) {
                e = err_radius(rf.re * rf.re + rf.im * rf.im, yr, yi);
            } else {
                e = err_radius(a.Rcma, yr, yi);
            }
            const double wr = mu * e.gr, wi = mu * e.gi;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double s = 1.0;
                if (alg == kNlms) {
#pragma unroll
                    for (int m = 0; m < kMaxModes; ++m) s = mode[r] == m ? scl[m] : s;
                }
                update(h[r], wr, wi, alg == kNlms ? x[r].re * s : x[r].re, alg == kNlms ? x[r].im * s : x[r].im);
            }
            if (lane == il) ybuf = Cplx{yr, yi}, ebuf = e.esq;
        }
        if (lane < cnt) {
            a.y[(g0 + lane) * nModes + k] = ybuf;
            if (a.esq) a.esq[(long long)k * a.total + g0 + lane] = ebuf;
        }
        if (ci + 1 < a.nchunks) to_lds();
        cur = nxt;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int N, t;
        if (lane_coeff(lane, r, nModes, nTaps, N, t)) a.H[(long long)(k + N * nModes) * nTaps + t] = h[r];
    }
}

struct StaticArgs {
    const void *x;
    int xdtype, nModes, nTaps, SpS, Lpad;
    long long n, start, len;
    const Cplx *H;
    Cplx *y;
};

__global__ __launch_bounds__(kStaticBlock) void k_eq_static(StaticArgs a) {
    const long long count = a.len * a.nModes;
    for (long long q = (long long)blockIdx.x * kStaticBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kStaticBlock) {
        const long long i = a.start + q / a.nModes;
        const int k = (int)(q % a.nModes);
        a.y[i * a.nModes + k] = static_output(a.H, a.xdtype, a.x, a.n, a.nModes, a.nTaps, a.SpS, a.Lpad, i, k);
    }
}

// ---- host side
struct Work : WorkBase {
    Buf in, refin, H, tables, out, esq;
    std::vector<double> host_tab;             // kept for their capacity
    std::vector<Seg> host_segs;
};
using Call = CallT<Work>;

}  // namespace

int eq_run(int device, const ssf_eq_params *p, const ssf_eq_stage *stages, const double *table, const double *radii, void *H_inout,
           const void *x, const void *ref, void *sig_out, double *errsq_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int nModes = p->nModes, nTaps = p->nTaps;
    const size_t out_bytes = (size_t)p->total * nModes * sizeof(Cplx), esq_bytes = (size_t)p->total * nModes * sizeof(double);
    const size_t H_bytes = (size_t)nModes * nModes * nTaps * sizeof(Cplx);
    Cplx *y = (Cplx *)c.target(sig_out, w.out, out_bytes);
    double *esq = errsq_out ? (double *)c.target(errsq_out, w.esq, esq_bytes) : nullptr;
    Cplx *H = (Cplx *)c.target(H_inout, w.H, H_bytes);
    if (!y || !H || (errsq_out && !esq)) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)p->n * nModes * mk::elem_size(p->dtype));
    if (!xd) return c.rc;
    const void *rd = nullptr;
    if (ref) {
        rd = c.input(ref, w.refin, (size_t)p->nref * nModes * mk::elem_size(p->ref_dtype));
        if (!rd) return c.rc;
    }
    if (H != H_inout && !c.h2d(H, H_inout, H_bytes)) return c.rc;
    // symbols no stage reaches stay zero, and so does |e|^2 of a static stage
    if (!c.ok(hipMemsetAsync(y, 0, out_bytes, w.st), "hipMemset")) return c.rc;
    if (esq && !c.ok(hipMemsetAsync(esq, 0, esq_bytes, w.st), "hipMemset")) return c.rc;

    std::vector<double> &tab = w.host_tab;
    tab.assign(table, table + 2 * (size_t)p->M);
    tab.insert(tab.end(), radii, radii + p->nRadii);
    if (!c.upload(w.tables, tab)) return c.rc;

    // runs of consecutive adaptive stages -> one serial launch each (per kMaxSegs stages); a static stage -> one parallel launch
    std::vector<Seg> &segs = w.host_segs;
    segs.clear();
    long long start = 0;
    for (int s = 0; s < p->nStages; ++s) {
        segs.push_back(Seg{start, (long long)stages[s].L, stages[s].alg, s == 0 ? p->numIter : 1, stages[s].mu});
        start += stages[s].L;
    }

    const int Cs = chunk_symbols(nModes, nTaps, p->SpS), R = coeffs_per_lane(nModes, nTaps);
    for (int s = 0; s < p->nStages;) {
        if (segs[s].alg == kStatic) {
            StaticArgs sa{};
            sa.x = xd, sa.xdtype = p->dtype, sa.nModes = nModes, sa.nTaps = nTaps, sa.SpS = p->SpS, sa.Lpad = nTaps / 2;
            sa.n = p->n, sa.start = segs[s].start, sa.len = segs[s].len, sa.H = H, sa.y = y;
            const long long nb = (sa.len * nModes + kStaticBlock - 1) / kStaticBlock;
            k_eq_static<<<(unsigned)(nb < 4096 ? nb : 4096), kStaticBlock, 0, w.st>>>(sa);
            if (!c.launched()) return c.rc;
            ++s;
            continue;
        }
        int e = s;
        long long nchunks = 0;
        for (; e < p->nStages && e - s < kMaxSegs && segs[e].alg != kStatic; ++e) nchunks += (long long)segs[e].reps * ((segs[e].len + Cs - 1) / Cs);
        EqArgs a{};
        a.x = xd, a.ref = rd ? rd : xd, a.xdtype = p->dtype, a.rdtype = rd ? p->ref_dtype : (int)mk::kC64, a.n = p->n, a.total = p->total;
        a.nModes = nModes, a.nTaps = nTaps, a.SpS = p->SpS, a.Lpad = nTaps / 2, a.M = p->M, a.nRad = p->nRadii;
        a.nseg = e - s, a.Cs = Cs, a.nchunks = nchunks, a.Rcma = p->Rcma;
        for (int q = s; q < e; ++q) a.segs[q - s] = segs[q];
        a.tab = (const double *)w.tables.p, a.rad = a.tab + 2 * (size_t)p->M;
        a.H = H, a.y = y, a.esq = esq;
        const bool wide = p->dtype == mk::kC128;
        if (R == 1) wide ? k_eq_serial<1, Cplx><<<nModes, kWave, 0, w.st>>>(a) : k_eq_serial<1, mk::CplxF><<<nModes, kWave, 0, w.st>>>(a);
        else if (R == 2) wide ? k_eq_serial<2, Cplx><<<nModes, kWave, 0, w.st>>>(a) : k_eq_serial<2, mk::CplxF><<<nModes, kWave, 0, w.st>>>(a);
        else wide ? k_eq_serial<4, Cplx><<<nModes, kWave, 0, w.st>>>(a) : k_eq_serial<4, mk::CplxF><<<nModes, kWave, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
        s = e;
    }
    if (!c.deliver(H_inout, H, H_bytes)) return c.rc;
    if (!c.deliver(sig_out, y, out_bytes)) return c.rc;
    if (errsq_out && !c.deliver(errsq_out, esq, esq_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
