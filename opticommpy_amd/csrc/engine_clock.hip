// engine_clock.hip -- the sampling clock on the device (ssf_clock_interp, ssf_quantize, ssf_clip, ssf_minmax, ssf_clock_scale_add,
// ssf_gardner, ssf_clock_drift of include/ssf.h).
//   element-wise   grid-stride passes over the elements in memory order (samples, columns): neighbouring lanes hold neighbouring
//                  columns of one output time and then the next time, so the two input samples an interpolated output reads sit in
//                  the lines its neighbours read.  adc's interpolate -> clip -> quantise is ONE pass (ck::chain_element).
//   min / max      one partial pair per workgroup, a second launch folds the partials; exact in any order.
//   gardner        one wavefront per column walks the recursion (a feedback delay of one detector update, nothing to run side by
//                  side): the column's input sits in LDS a chunk of kChunk samples at a time, the next chunk's loads are in flight
//                  in registers (all lanes, coalesced) while the chunk in hand is consumed and move to LDS at the chunk border; the
//                  outputs and timing values collect in an LDS ring and leave kFlush at a time, one per lane.  The recursion is
//                  evaluated by every lane alike; the input window x[m-2 .. m+2] is kept in registers, so the one LDS read of the
//                  next sample is issued an iteration ahead of its use.
//   clock drift    a sum per column, then per column one workgroup that counts the peaks and keeps the first and the last.
// No atomics and no communication between workgroups: results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "block_reduce.h"
#include "clock_kernels.h"
#include "engine_host.h"

namespace ssf {
namespace {
using namespace ck;
using namespace eng;

static_assert(kBlock == br::kBlock, "the reductions are written for block_reduce.h's workgroup");

// ---- element-wise passes
__device__ __forceinline__ void store_element(int dtype, bool as_double, void *out, long long q, double re, double im) {
    if (is_complex(dtype)) {
        if (as_double || dtype == mk::kC128) ((Cplx *)out)[q] = Cplx{re, im};
        else ((CplxF *)out)[q] = CplxF{(float)re, (float)im};
    } else {
        if (as_double || dtype == mk::kF64) ((double *)out)[q] = re;
        else ((float *)out)[q] = (float)re;
    }
}

__global__ __launch_bounds__(kBlock) void k_clock_chain(Chain c, const void *x, const double *t_re, const double *t_im, void *out) {
    const long long count = c.n_out * c.ncols;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kBlock) {
        double re, im;
        chain_element(c, x, t_re, t_im, q, re, im);
        store_element(c.dtype, c.quantize != 0, out, q, re, im);
    }
}

// real value q stride of a flat array of doubles or floats -> float64
__global__ __launch_bounds__(kBlock) void k_clock_quantize(long long count, int single, int stride, double qmin, double qdelta,
                                                           long long levels, const void *x, double *out) {
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kBlock) {
        const double v = single ? (double)((const float *)x)[q * stride] : ((const double *)x)[q * stride];
        out[q] = quantize(v, qmin, qdelta, levels);
    }
}

__global__ __launch_bounds__(kBlock) void k_clock_clip(long long count, int dtype, double lo, double hi, const void *x, void *out) {
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kBlock) {
        double re, im;
        mk::load(dtype, x, q, re, im);
        if (is_complex(dtype)) clip_complex(re, im, lo, hi);
        else re = clip_real(re, lo, hi);
        store_element(dtype, false, out, q, re, im);
    }
}

// out = (x + noise) scale over `count` doubles (noise may be NULL)
__global__ __launch_bounds__(kBlock) void k_clock_scale_add(long long count, double scale, int has_scale, const double *x,
                                                            const double *noise, double *out) {
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kBlock) {
        double v = x[q];
        if (noise) v = v + noise[q];
        out[q] = has_scale ? v * scale : v;
    }
}

// ---- min and max over a flat array of reals
__device__ void block_minmax_store(double mn, double mx, double *out) {
    __shared__ double sh[2][br::kWaves];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_down(mn, o, 64), b = __shfl_down(mx, o, 64);
        mn = a < mn ? a : mn, mx = b > mx ? b : mx;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = mn, sh[1][threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < br::kWaves; ++w) {
            mn = sh[0][w] < mn ? sh[0][w] : mn;
            mx = sh[1][w] > mx ? sh[1][w] : mx;
        }
        out[0] = mn, out[1] = mx;
    }
}
__global__ __launch_bounds__(kBlock) void k_clock_minmax(long long count, int single, const void *x, double *part) {
    double mn = INFINITY, mx = -INFINITY;
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < count; q += (long long)gridDim.x * kBlock) {
        const double v = single ? (double)((const float *)x)[q] : ((const double *)x)[q];
        mn = v < mn ? v : mn, mx = v > mx ? v : mx;
    }
    block_minmax_store(mn, mx, part + 2 * blockIdx.x);
}
__global__ __launch_bounds__(kBlock) void k_clock_minmax_fold(int nb, const double *part, double *out) {
    double mn = INFINITY, mx = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += kBlock) {
        mn = part[2 * b] < mn ? part[2 * b] : mn;
        mx = part[2 * b + 1] > mx ? part[2 * b + 1] : mx;
    }
    block_minmax_store(mn, mx, out);
}

// ---- clock recovery
struct GardnerArgs {
    const void *x;
    long long n, nSamples, Ln;
    int nModes, nyquist;
    double kp, ki;
    CplxF *out;                   // (Ln, nModes), zeroed
    double *tv;                   // (Ln, nModes), zeroed
    long long *last_n;            // nModes
    int *status;                  // nModes
};

template <typename XT>
__global__ __launch_bounds__(kWave) void k_gardner(GardnerArgs a) {
    __shared__ Cplx xs[kWin];
    __shared__ CplxF ring[kRing];
    __shared__ double tring[kRing];
    const int col = blockIdx.x, lane = threadIdx.x;
    const int nModes = a.nModes;
    constexpr long long kMask = kRing - 1;

    for (int i = lane; i < kRing; i += kWave) ring[i] = CplxF{0.0f, 0.0f}, tring[i] = 0.0;

    // the loads of one chunk: samples chunk kChunk .. + kWin - 1 of the column (zeros from sample n on: the padding), kept as
    // loaded so that no load waits for another; they are widened on the way to LDS
    XT pre[kPre];
    auto fetch = [&](long long chunk) {
        const long long base = chunk * kChunk;
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const int idx = e * kWave + lane;
            const long long p = base + idx;
            pre[e] = XT{0, 0};
            if (idx < kWin && p < a.n) pre[e] = ((const XT *)a.x)[p * nModes + col];
        }
    };
    auto to_lds = [&]() {
        __syncthreads();                      // (one wave: the reads of the chunk before are done)
#pragma unroll
        for (int e = 0; e < kPre; ++e) {
            const int idx = e * kWave + lane;
            if (idx < kWin) xs[idx] = Cplx{(double)pre[e].re, (double)pre[e].im};
        }
        __syncthreads();
    };
    // outputs [f, f + kFlush) leave, one per lane, and their ring places are cleared for the outputs kRing further on
    auto flush = [&](long long f) {
        __syncthreads();
        const long long q = f + lane;
        if (q < a.Ln) {
            a.out[q * nModes + col] = ring[q & kMask];
            a.tv[q * nModes + col] = tring[q & kMask];
        }
        ring[q & kMask] = CplxF{0.0f, 0.0f}, tring[q & kMask] = 0.0;
        __syncthreads();
    };

    double t_nco = 0.0, intPart = 0.0;
    long long n = 2, m = 2, chunk = 0, f = 0;
    int status = kGardnerOk;
    fetch(0);
    to_lds();
    fetch(1);                                 // in flight while chunk 0 is consumed
    Cplx w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = xs[i];

    while (loop_runs(n, m, a.Ln, a.nSamples)) {
        const CplxF pa = ring[(n - 2) & kMask], pb = ring[(n - 1) & kMask];
        const CplxF y = interpolate(w, t_nco);
        if (lane == 0) ring[n & kMask] = y;
        if ((n & 1) == 0) loop_filter(t_nco, intPart, a.nyquist ? ted_nyquist(pa, pb, y) : ted_gardner(pa, pb, y), a.kp, a.ki);
        const int step = nco_gap(t_nco);
        n += step;
        if (f > 0 && n < f + 2) {             // the loop fell back behind what has left LDS
            status = kGardnerBackrun;
            break;
        }
        if (lane == 0 && n < a.Ln) tring[n & kMask] = t_nco;            // (n == Ln: the write the reference makes out of bounds)
        if (step > 0) {
            ++m;
            if (m >= 2 + (chunk + 1) * kChunk) {
                ++chunk;
                to_lds();
                fetch(chunk + 1);
#pragma unroll
                for (int i = 0; i < 5; ++i) w[i] = xs[i];
            } else {
                w[0] = w[1], w[1] = w[2], w[2] = w[3], w[3] = w[4];
                w[4] = xs[(int)(m + 2 - chunk * kChunk)];
            }
        }
        while (n >= f + kLag) flush(f), f += kFlush;
        __syncthreads();                      // lane 0's ring writes, before the next output's reads
    }
    for (int r = 0; r < kRing / kFlush; ++r) flush(f + r * kFlush);
    if (lane == 0) a.last_n[col] = n, a.status[col] = status;
}

// ---- clock drift
__global__ __launch_bounds__(kBlock) void k_drift_sum(long long n, int ncols, const double *t, double *sums) {
    const int col = blockIdx.x;
    double acc = 0.0;
    for (long long r = threadIdx.x; r < n; r += kBlock) acc += t[r * ncols + col];
    br::block_sum_store(acc, sums + col);
}

__global__ __launch_bounds__(kBlock) void k_drift_peaks(long long n, int ncols, int per_column, const double *t, const double *sums,
                                                        double *ppm) {
    __shared__ long long sh[3][br::kWaves];
    const int col = blockIdx.x;
    double total = 0.0;
    for (int k = 0; k < ncols; ++k) total += sums[k];
    const double mean = per_column ? sums[col] / (double)n : total / (double)(n * ncols);
    long long count = 0, first = n, last = -1;
    for (long long i = 1 + threadIdx.x; i + 1 < n - 1; i += kBlock) {
        long long at;
        if (drift_peak(t, n, ncols, col, mean, i, at)) ++count, first = at < first ? at : first, last = at > last ? at : last;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long c2 = __shfl_down(count, o, 64), f2 = __shfl_down(first, o, 64), l2 = __shfl_down(last, o, 64);
        count += c2, first = f2 < first ? f2 : first, last = l2 > last ? l2 : last;
    }
    if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = count, sh[1][threadIdx.x >> 6] = first, sh[2][threadIdx.x >> 6] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < br::kWaves; ++w) {
            count += sh[0][w];
            first = sh[1][w] < first ? sh[1][w] : first;
            last = sh[2][w] > last ? sh[2][w] : last;
        }
        ppm[col] = drift_ppm(count, first, last, mean);
    }
}

// ---- host side
struct Work : WorkBase {
    Buf in, tre, tim, out, noise, part, res, sig, tv, last, status;
};
using Call = CallT<Work>;

inline unsigned blocks_for(long long count) { return (unsigned)grid_blocks(count, kBlock, kMaxBlocks, 1); }

}  // namespace

int clock_interp(int device, const ssf_clock_params *p, const void *x, const double *t_re, const double *t_im, void *out,
                 std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    Chain ch{p->n_in, p->n_out, p->ncols, p->dtype, p->form, p->clip, p->quantize, p->inTs, p->outTs, p->lo, p->hi, p->qmin, p->qdelta,
             p->qlevels, 1.0 / p->inTs};
    const long long count = p->n_out * p->ncols;
    const size_t esz = p->quantize ? (is_complex(p->dtype) ? 16 : 8) : mk::elem_size(p->dtype);
    void *o = c.target(out, w.out, (size_t)count * esz);
    if (!o) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)p->n_in * p->ncols * mk::elem_size(p->dtype));
    if (!xd) return c.rc;
    const double *tr = nullptr, *ti = nullptr;
    if (t_re && !(tr = (const double *)c.input(t_re, w.tre, (size_t)p->n_out * sizeof(double)))) return c.rc;
    if (t_im && !(ti = (const double *)c.input(t_im, w.tim, (size_t)p->n_out * sizeof(double)))) return c.rc;
    k_clock_chain<<<blocks_for(count), kBlock, 0, w.st>>>(ch, xd, tr, ti, o);
    if (!c.launched() || !c.deliver(out, o, (size_t)count * esz) || !c.sync()) return c.rc;
    return SSF_OK;
}

int clock_quantize(int device, int64_t count, int dtype, double qmin, double qdelta, int64_t levels, const void *x, double *out,
                   std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    double *o = (double *)c.target(out, w.out, (size_t)count * sizeof(double));
    if (!o) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)count * mk::elem_size(dtype));
    if (!xd) return c.rc;
    k_clock_quantize<<<blocks_for(count), kBlock, 0, w.st>>>(count, is_single(dtype), is_complex(dtype) ? 2 : 1, qmin, qdelta, levels, xd, o);
    if (!c.launched() || !c.deliver(out, o, (size_t)count * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

int clock_clip(int device, int64_t count, int dtype, double lo, double hi, const void *x, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t bytes = (size_t)count * mk::elem_size(dtype);
    void *o = c.target(out, w.out, bytes);
    if (!o) return c.rc;
    const void *xd = c.input(x, w.in, bytes);
    if (!xd) return c.rc;
    k_clock_clip<<<blocks_for(count), kBlock, 0, w.st>>>(count, dtype, lo, hi, xd, o);
    if (!c.launched() || !c.deliver(out, o, bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int clock_minmax(int device, int64_t count, int dtype, const void *x, double *out2, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long reals = count * (is_complex(dtype) ? 2 : 1);
    const unsigned nb = blocks_for(reals);
    if (!c.need(w.part, (size_t)nb * 2 * sizeof(double)) || !c.need(w.res, 2 * sizeof(double))) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)count * mk::elem_size(dtype));
    if (!xd) return c.rc;
    k_clock_minmax<<<nb, kBlock, 0, w.st>>>(reals, is_single(dtype), xd, (double *)w.part.p);
    if (!c.launched()) return c.rc;
    k_clock_minmax_fold<<<1, kBlock, 0, w.st>>>((int)nb, (const double *)w.part.p, (double *)w.res.p);
    if (!c.launched()) return c.rc;
    if (!c.deliver(out2, w.res.p, 2 * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

int clock_scale_add(int device, int64_t count, double scale, int has_scale, const double *x, const double *noise, double *out,
                    std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t bytes = (size_t)count * sizeof(double);
    double *o = (double *)c.target(out, w.out, bytes);
    if (!o) return c.rc;
    const double *xd = (const double *)c.input(x, w.in, bytes);
    if (!xd) return c.rc;
    const double *nd = nullptr;
    if (noise && !(nd = (const double *)c.input(noise, w.noise, bytes))) return c.rc;
    k_clock_scale_add<<<blocks_for(count), kBlock, 0, w.st>>>(count, scale, has_scale, xd, nd, o);
    if (!c.launched() || !c.deliver(out, o, bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int clock_gardner(int device, const ssf_gardner_params *p, const void *x, void *sig_out, double *t_out, int64_t *last_n,
                  std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int nModes = p->nModes;
    const size_t sig_bytes = (size_t)p->Ln * nModes * sizeof(CplxF), t_bytes = (size_t)p->Ln * nModes * sizeof(double);
    CplxF *sig = (CplxF *)c.target(sig_out, w.sig, sig_bytes);
    double *tv = (double *)c.target(t_out, w.tv, t_bytes);
    if (!sig || !tv) return c.rc;
    if (!c.need(w.last, (size_t)nModes * sizeof(long long)) || !c.need(w.status, (size_t)nModes * sizeof(int))) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)p->n * nModes * mk::elem_size(p->dtype));
    if (!xd) return c.rc;
    // outputs the loop never reaches stay zero
    if (!c.ok(hipMemsetAsync(sig, 0, sig_bytes, w.st), "hipMemset") || !c.ok(hipMemsetAsync(tv, 0, t_bytes, w.st), "hipMemset")) return c.rc;
    GardnerArgs a{};
    a.x = xd, a.n = p->n, a.nSamples = p->n + p->lpad, a.Ln = p->Ln, a.nModes = nModes, a.nyquist = p->nyquist, a.kp = p->kp, a.ki = p->ki;
    a.out = sig, a.tv = tv, a.last_n = (long long *)w.last.p, a.status = (int *)w.status.p;
    if (p->dtype == mk::kC128) k_gardner<Cplx><<<nModes, kWave, 0, w.st>>>(a);
    else k_gardner<CplxF><<<nModes, kWave, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    std::vector<int> status(nModes);
    std::vector<long long> last(nModes);
    if (!c.deliver(last.data(), w.last.p, (size_t)nModes * sizeof(long long)) || !c.deliver(status.data(), w.status.p, (size_t)nModes * sizeof(int))) return c.rc;
    if (!c.deliver(sig_out, sig, sig_bytes) || !c.deliver(t_out, tv, t_bytes) || !c.sync()) return c.rc;
    for (int k = 0; k < nModes; ++k) {
        last_n[k] = last[k];
        if (status[k] != kGardnerOk) {
            *err = "the loop of mode " + std::to_string(k) + " fell back more than " + std::to_string(kLag - kFlush - 2) +
                   " outputs behind the furthest one it had reached: the loop gains are far outside a working range";
            return SSF_ERR_UNSUPPORTED;
        }
    }
    return SSF_OK;
}

int clock_drift(int device, int64_t n, int ncols, int per_column, const double *t, double *ppm_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    if (!c.need(w.part, (size_t)ncols * sizeof(double)) || !c.need(w.res, (size_t)ncols * sizeof(double))) return c.rc;
    const double *td = (const double *)c.input(t, w.in, (size_t)n * ncols * sizeof(double));
    if (!td) return c.rc;
    k_drift_sum<<<ncols, kBlock, 0, w.st>>>(n, ncols, td, (double *)w.part.p);
    if (!c.launched()) return c.rc;
    k_drift_peaks<<<ncols, kBlock, 0, w.st>>>(n, ncols, per_column, td, (const double *)w.part.p, (double *)w.res.p);
    if (!c.launched()) return c.rc;
    if (!c.deliver(ppm_out, w.res.p, (size_t)ncols * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
