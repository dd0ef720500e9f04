// engine_seqdet.hip -- mlse, detector and autocorr on the device (ssf_mlse, ssf_detector, ssf_autocorr of include/ssf.h).
//   forward   one workgroup per column, next state ns on lane ns (64 lanes up to 64 states, whole wavefronts up to 1024 lanes
//             above).  A lane's share of its expected outputs sits in two registers, the M candidate terms h[L] c[j] in registers
//             for M = 2, 4, 8 and in LDS otherwise; the path metrics are double, in LDS, double-buffered: one barrier per step
//             (none with a single wavefront).  y is staged kStageChunk samples at a time, the next chunk's samples
//             waiting in registers while the current one is consumed.  The survivor bytes of kSurvChunk steps are gathered in LDS
//             and leave in 4-byte stores.  The final minimum and its lowest index come from a lane-strided scan and a butterfly
//             over (metric, index).
//   maps      per chunk and column: the chunk's survivor rows in LDS, one lane per end state walks back to the start state.
//   compose   per column: the maps are staged a block at a time by the whole workgroup; one lane follows them from the final
//             state and leaves every chunk's end state.
//   walk      one lane per chunk and column: the chunk's decisions from its end state.
//   detector  one symbol per lane, the table and the log priors in LDS.
//   autocorr  a workgroup owns a run of whole tiles; per tile each wavefront sums the lags k = wave, wave + 4, .. over the tile
//             (lanes stride the samples), the wave's sum is added to the lag's LDS slot in tile order; one wavefront per lag
//             adds the workgroups' partials and divides by N - k.
// No flags, no atomics: every loop's trip count is known at launch and results repeat bit for bit.
// Built with -ffp-contract=off (Makefile): see seqdet_kernels.h.
#include <hip/hip_runtime.h>

#include <vector>

#include "block_reduce.h"
#include "engine_host.h"
#include "seqdet_kernels.h"

namespace ssf {
namespace {
using namespace sq;
using namespace eng;

struct FwdArgs {
    Trellis t;
    const void *y;
    int dtype, cols;
    long long n, colstride;                   // colstride: survivor bytes of one column, a multiple of 16
    const double *h, *c;
    uint8_t *surv;
    double *fin_metric;
    int *fin_state;
};

// ONE: up to 64 states, launched with 64 lanes (a single wavefront: the compiler drops the barriers); otherwise the states rounded
// up to whole wavefronts, 128 .. 1024 lanes.  MT: M where it is 2, 4 or 8 -- the candidate terms then sit in registers and the
// add-compare-select is unrolled (a lone wavefront pays for every instruction it issues) -- and 0 for any other M (terms in LDS).
template <bool CX, bool ONE, int MT>
__global__ __launch_bounds__(ONE ? 64 : 1024) void k_mlse_forward(FwdArgs a) {
    constexpr int kPre = kStageChunk / (ONE ? 64 : 128);      // samples a lane holds in flight: the chunk over the fewest lanes
    const int BLOCK = ONE ? 64 : (int)blockDim.x;
    __shared__ double pm[2][kMaxStates];
    __shared__ double term[2 * kMaxM];
    __shared__ double ys[2 * kStageChunk];
    __shared__ __attribute__((aligned(16))) uint8_t sv[kSurvChunk * kMaxStates];
    const Trellis &t = a.t;
    const int ns = threadIdx.x, col = blockIdx.x;
    const bool live = ns < t.S;

    for (int i = ns; i < 2 * kMaxStates; i += BLOCK) (&pm[0][0])[i] = 0.0;
    for (int i = ns; i < kSurvChunk * kMaxStates / 4; i += BLOCK) ((uint32_t *)sv)[i] = 0u;
    for (int j = ns; j < t.M; j += BLOCK) candidate_term(t, a.h, a.c, j, term[2 * j], term[2 * j + 1]);
    double br = 0.0, bi = 0.0, treg[MT ? 2 * MT : 2] = {};
    if (live) state_base(t, a.h, a.c, ns, br, bi);
    if constexpr (MT > 0) {
#pragma unroll
        for (int j = 0; j < MT; ++j) candidate_term(t, a.h, a.c, j, treg[2 * j], treg[2 * j + 1]);
    }
    const double *terms = MT > 0 ? treg : term;
    uint8_t *surv = a.surv + (long long)col * a.colstride;

    double pre_re[kPre], pre_im[CX ? kPre : 1];
    auto fetch = [&](long long c0) {
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const long long i = c0 + e * BLOCK + ns;
            double re = 0.0, im = 0.0;
            if (e * BLOCK + ns < kStageChunk && i < a.n) mk::load(a.dtype, a.y, i * a.cols + col, re, im);
            pre_re[e] = re;
            if constexpr (CX) pre_im[e] = im;
        }
    };
    auto to_lds = [&]() {
        __syncthreads();                      // the reads of the chunk before are done
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const int i = e * BLOCK + ns;
            if (i < kStageChunk) {
                ys[i] = pre_re[e];
                if constexpr (CX) ys[kStageChunk + i] = pre_im[e];
            }
        }
        __syncthreads();
    };

    int cur = 0;
    fetch(0);
    for (long long c0 = 0; c0 < a.n; c0 += kStageChunk) {
        const long long left = a.n - c0;
        const int cnt = left < kStageChunk ? (int)left : kStageChunk;
        to_lds();
        if (c0 + kStageChunk < a.n) fetch(c0 + kStageChunk);      // in flight while this chunk is consumed
        for (int i = 0; i < cnt; ++i) {
            const int tt = i % kSurvChunk;
            if (live) {
                double best;
                const int j = acs<CX, MT>(t, pm[cur], terms, ns, br, bi, ys[i], CX ? ys[kStageChunk + i] : 0.0, best);
                pm[cur ^ 1][ns] = best;
                sv[tt * t.Sp + ns] = (uint8_t)j;
            }
            cur ^= 1;
            __syncthreads();
            if (tt == kSurvChunk - 1 || i == cnt - 1) {
                const int words = (tt + 1) * t.Sp / 4;
                uint32_t *dst = (uint32_t *)(surv + (c0 + i - tt) * t.Sp);
                for (int w = ns; w < words; w += BLOCK) dst[w] = ((const uint32_t *)sv)[w];
                __syncthreads();              // before the next chunk's first row lands on these bytes
            }
        }
    }
    if (ns < 64) {
        double d = INFINITY;
        int bs = kMaxStates;
        for (int s = ns; s < t.S; s += 64)
            if (pm[cur][s] < d) d = pm[cur][s], bs = s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double d2 = __shfl_xor(d, o, 64);
            const int s2 = __shfl_xor(bs, o, 64);
            argmin_merge(d, bs, d2, s2);
        }
        if (ns == 0) a.fin_metric[col] = d, a.fin_state[col] = bs < t.S ? bs : 0;
    }
}

struct BackArgs {
    Trellis t;
    long long n, colstride, nchunks;
    int cols, cx;
    const uint8_t *surv;
    uint16_t *maps;                           // [col][chunk][end state] -> start state
    int *ends;                                // [col][chunk]: the state the chunk's last step ends in
    const int *fin_state;
    const double *c;
    void *out;
};

__global__ __launch_bounds__(256) void k_mlse_maps(BackArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sv[kSurvChunk * kMaxStates];
    const Trellis &t = a.t;
    const long long ch = blockIdx.x, n0 = ch * kSurvChunk;
    const int col = blockIdx.y;
    const long long left = a.n - n0;
    const int cnt = left < kSurvChunk ? (int)left : kSurvChunk;
    const uint32_t *src = (const uint32_t *)(a.surv + (long long)col * a.colstride + n0 * t.Sp);
    for (int w = threadIdx.x; w < cnt * t.Sp / 4; w += 256) ((uint32_t *)sv)[w] = src[w];
    __syncthreads();
    uint16_t *map = a.maps + ((long long)col * a.nchunks + ch) * t.S;
    for (int e = threadIdx.x; e < t.S; e += 256) {
        int s = e;
        for (int tt = cnt - 1; tt >= 0; --tt) s = step_back(t, sv + tt * t.Sp, s);
        map[e] = (uint16_t)s;
    }
}

__global__ __launch_bounds__(256) void k_mlse_compose(BackArgs a) {
    __shared__ uint16_t buf[kComposeLds];
    const Trellis &t = a.t;
    const int col = blockIdx.x;
    const long long per = kComposeLds / t.S;  // maps staged at a time: at least 16
    const uint16_t *maps = a.maps + (long long)col * a.nchunks * t.S;
    int state = a.fin_state[col];
    for (long long hi = a.nchunks; hi > 0; hi -= per) {
        const long long lo = hi > per ? hi - per : 0;
        const int cnt = (int)(hi - lo) * t.S;
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += 256) buf[i] = maps[lo * t.S + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (long long ch = hi - 1; ch >= lo; --ch) {
                a.ends[(long long)col * a.nchunks + ch] = state;
                state = buf[(ch - lo) * t.S + state];
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_mlse_walk(BackArgs a) {
    const Trellis &t = a.t;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.nchunks * a.cols) return;
    const int col = (int)(g / a.nchunks);
    const long long ch = g % a.nchunks, n0 = ch * kSurvChunk;
    const long long left = a.n - n0;
    const int cnt = left < kSurvChunk ? (int)left : kSurvChunk;
    const uint8_t *rows = a.surv + (long long)col * a.colstride + n0 * t.Sp;
    int s = a.ends[g];
    for (int tt = cnt - 1; tt >= 0; --tt) {
        const int j = rows[tt * t.Sp + s];
        const int k = decided_symbol(t, s, j);
        const long long o = (n0 + tt) * a.cols + col;
        if (a.cx) ((Cplx *)a.out)[o] = Cplx{a.c[2 * k], a.c[2 * k + 1]};
        else ((double *)a.out)[o] = a.c[2 * k];
        s = predecessor(t, s, j);
    }
}

// ---- detector
struct DetArgs {
    long long n;
    int dtype, M, rule;
    double sigma2;
    const double *tab, *logpx;
    const void *r;
    void *decided;
    long long *ind;
};
__global__ __launch_bounds__(kDetBlock) void k_detector(DetArgs a) {
    __shared__ double tab[2 * kMaxM], lp[kMaxM];
    for (int i = threadIdx.x; i < 2 * a.M; i += kDetBlock) tab[i] = a.tab[i];
    for (int i = threadIdx.x; i < a.M; i += kDetBlock) lp[i] = a.logpx[i];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kDetBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kDetBlock) {
        double re, im;
        mk::load(a.dtype, a.r, i, re, im);
        const int m = detect(tab, lp, a.M, a.rule, a.sigma2, re, im);
        if (a.dtype == mk::kC128) ((Cplx *)a.decided)[i] = Cplx{tab[2 * m], tab[2 * m + 1]};
        else ((double *)a.decided)[i] = tab[2 * m];
        a.ind[i] = m;
    }
}

// ---- autocorr
struct AcArgs {
    long long n;
    int nTaps, nb;
    const double *x;
    double *part, *r;
};
__global__ __launch_bounds__(kAcBlock) void k_autocorr(AcArgs a) {
    __shared__ double w[kAcMaxTaps - 1 + kAcTile], acc[kAcMaxTaps];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tpb = ac_tiles_per_block(a.n, a.nb);
    acc[threadIdx.x] = 0.0;
    for (long long ti = 0; ti < tpb; ++ti) {
        const long long t0 = ((long long)blockIdx.x * tpb + ti) * kAcTile;
        if (t0 >= a.n) break;                 // (the same for every lane of the workgroup)
        const long long left = a.n - t0;
        const int cnt = left < kAcTile ? (int)left : kAcTile;
        __syncthreads();
        for (int i = threadIdx.x; i < kAcMaxTaps - 1 + cnt; i += kAcBlock) {
            const long long s = t0 - (kAcMaxTaps - 1) + i;
            w[i] = s >= 0 ? a.x[s] : 0.0;
        }
        __syncthreads();
        for (int k = wave; k < a.nTaps; k += br::kWaves) {
            const double v = br::wave_sum_down(ac_lane_sum(w, k, lane, t0, cnt));
            if (lane == 0) acc[k] += v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.nTaps) a.part[(long long)blockIdx.x * a.nTaps + threadIdx.x] = acc[threadIdx.x];
}
__global__ __launch_bounds__(64) void k_autocorr_fin(AcArgs a) {
    const int k = blockIdx.x;
    const double s = br::wave_sum_partials(a.part + k, a.nb, a.nTaps);
    if (threadIdx.x == 0) a.r[k] = s / (double)(a.n - k);
}

// ---- host side
struct Work : WorkBase {
    Buf in, out, ind, tables, surv, maps, ends, fin, part, res;
    std::vector<double> host_tab;             // kept for its capacity
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};
using Call = CallT<Work>;
static_assert(kAcBlock == br::kBlock && kAcMaxTaps == kAcBlock, "one LDS slot per lane, four waves");

template <bool CX, bool ONE> void launch_forward_m(const FwdArgs &f, int M, int cols, int block, hipStream_t st) {
    switch (M) {
    case 2: return k_mlse_forward<CX, ONE, 2><<<cols, block, 0, st>>>(f);
    case 4: return k_mlse_forward<CX, ONE, 4><<<cols, block, 0, st>>>(f);
    case 8: return k_mlse_forward<CX, ONE, 8><<<cols, block, 0, st>>>(f);
    }
    k_mlse_forward<CX, ONE, 0><<<cols, block, 0, st>>>(f);
}
void launch_forward(const FwdArgs &f, bool cx, bool one, int M, int cols, int block, hipStream_t st) {
    if (cx) one ? launch_forward_m<true, true>(f, M, cols, block, st) : launch_forward_m<true, false>(f, M, cols, block, st);
    else one ? launch_forward_m<false, true>(f, M, cols, block, st) : launch_forward_m<false, false>(f, M, cols, block, st);
}

bool upload_tables(Call &c, const double *a, size_t na, const double *b, size_t nb) {
    Work &w = *c.w;
    w.host_tab.assign(a, a + na);
    if (b) w.host_tab.insert(w.host_tab.end(), b, b + nb);
    else w.host_tab.insert(w.host_tab.end(), nb, 0.0);
    return c.upload(w.tables, w.host_tab);
}

}  // namespace

int64_t mlse_survivor_bytes(int64_t n, int cols, int M, int taps) {
    const Trellis t = trellis_of(M, taps, 0);
    return (int64_t)cols * ((n * t.Sp + 15) / 16 * 16);
}

int mlse_run(int device, ssf_mlse_params *p, const double *h, const double *const_tab, const void *y, void *out, double *final_metric,
             std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const bool cx = p->dtype == mk::kC128;
    const Trellis t = trellis_of(p->M, p->taps, cx);
    const size_t val = cx ? sizeof(Cplx) : sizeof(double), io_bytes = (size_t)p->n * p->cols * val;
    const long long nchunks = (p->n + kSurvChunk - 1) / kSurvChunk;
    const long long colstride = (p->n * t.Sp + 15) / 16 * 16;
    const size_t fin_bytes = (size_t)p->cols * (sizeof(double) + sizeof(int));

    void *o = c.target(out, w.out, io_bytes);
    if (!o) return c.rc;
    const void *yd = c.input(y, w.in, io_bytes);
    if (!yd) return c.rc;
    if (!c.need(w.surv, (size_t)colstride * p->cols) || !c.need(w.maps, (size_t)p->cols * nchunks * t.S * sizeof(uint16_t)) ||
        !c.need(w.ends, (size_t)p->cols * nchunks * sizeof(int)) || !c.need(w.fin, fin_bytes))
        return c.rc;
    if (!upload_tables(c, h, 2 * (size_t)p->taps, const_tab, 2 * (size_t)p->M)) return c.rc;
    if (p->timing)
        for (hipEvent_t &e : w.ev)
            if (!e && !c.ok(hipEventCreate(&e), "hipEventCreate")) return c.rc;

    FwdArgs f{};
    f.t = t, f.y = yd, f.dtype = p->dtype, f.cols = p->cols, f.n = p->n, f.colstride = colstride;
    f.h = (const double *)w.tables.p, f.c = f.h + 2 * p->taps, f.surv = (uint8_t *)w.surv.p;
    f.fin_metric = (double *)w.fin.p, f.fin_state = (int *)(f.fin_metric + p->cols);
    const bool one = t.S <= 64;
    if (p->timing && !c.ok(hipEventRecord(w.ev[0], w.st), "hipEventRecord")) return c.rc;
    const int block = one ? 64 : (t.S + 63) / 64 * 64;
    launch_forward(f, cx, one, p->M, p->cols, block, w.st);
    if (!c.launched()) return c.rc;
    if (p->timing && !c.ok(hipEventRecord(w.ev[1], w.st), "hipEventRecord")) return c.rc;

    BackArgs b{};
    b.t = t, b.n = p->n, b.colstride = colstride, b.nchunks = nchunks, b.cols = p->cols, b.cx = cx, b.surv = f.surv;
    b.maps = (uint16_t *)w.maps.p, b.ends = (int *)w.ends.p, b.fin_state = f.fin_state, b.c = f.c, b.out = o;
    k_mlse_maps<<<dim3((unsigned)nchunks, (unsigned)p->cols), 256, 0, w.st>>>(b);
    k_mlse_compose<<<p->cols, 256, 0, w.st>>>(b);
    k_mlse_walk<<<(unsigned)((nchunks * p->cols + 255) / 256), 256, 0, w.st>>>(b);
    if (!c.launched()) return c.rc;
    if (p->timing && !c.ok(hipEventRecord(w.ev[2], w.st), "hipEventRecord")) return c.rc;
    if (!c.deliver(final_metric, f.fin_metric, (size_t)p->cols * sizeof(double)) || !c.deliver(out, o, io_bytes) || !c.sync()) return c.rc;
    p->fwd_ms = p->tb_ms = 0.0;
    if (p->timing) {
        float a = 0.f, d = 0.f;
        if (!c.ok(hipEventElapsedTime(&a, w.ev[0], w.ev[1]), "hipEventElapsedTime") || !c.ok(hipEventElapsedTime(&d, w.ev[1], w.ev[2]), "hipEventElapsedTime"))
            return c.rc;
        p->fwd_ms = a, p->tb_ms = d;
    }
    p->states = t.S, p->kernel = one ? 0 : 1, p->chunk = kSurvChunk, p->survivor_bytes = (int64_t)colstride * p->cols;
    return SSF_OK;
}

int detector_run(int device, int64_t n, int dtype, int M, int rule, double sigma2, const double *const_tab, const double *logpx, const void *r,
                 void *decided, int64_t *ind, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t val = mk::elem_size(dtype), io_bytes = (size_t)n * val, ind_bytes = (size_t)n * sizeof(int64_t);
    void *o = c.target(decided, w.out, io_bytes);
    long long *id = (long long *)c.target(ind, w.ind, ind_bytes);
    if (!o || !id) return c.rc;
    const void *rd = c.input(r, w.in, io_bytes);
    if (!rd) return c.rc;
    if (!upload_tables(c, const_tab, 2 * (size_t)M, logpx, (size_t)M)) return c.rc;
    DetArgs a{};
    a.n = n, a.dtype = dtype, a.M = M, a.rule = rule, a.sigma2 = sigma2, a.tab = (const double *)w.tables.p, a.logpx = a.tab + 2 * M;
    a.r = rd, a.decided = o, a.ind = id;
    k_detector<<<grid_blocks(n, kDetBlock, 1 << 16), kDetBlock, 0, w.st>>>(a);
    if (!c.launched() || !c.deliver(decided, o, io_bytes) || !c.deliver(ind, id, ind_bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int autocorr_run(int device, int64_t n, int nTaps, const void *x, double *r_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    AcArgs a{};
    a.n = n, a.nTaps = nTaps, a.nb = ac_blocks(n);
    if (!c.need(w.part, (size_t)a.nb * nTaps * sizeof(double)) || !c.need(w.res, (size_t)nTaps * sizeof(double))) return c.rc;
    a.x = (const double *)c.input(x, w.in, (size_t)n * sizeof(double));
    if (!a.x) return c.rc;
    a.part = (double *)w.part.p, a.r = (double *)w.res.p;
    k_autocorr<<<a.nb, kAcBlock, 0, w.st>>>(a);
    k_autocorr_fin<<<nTaps, 64, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    if (!c.deliver(r_out, a.r, (size_t)nTaps * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
