// engine_sync.hip -- sequence synchronisation on the device (ssf_symbol_sync, ssf_finddelay of include/ssf.h).
//   prepare   one lane per row of the (n, nModes) arrays: |x| or Re / Im into the zero-padded transform buffers (the transmitted
//             sequences n_rx - 1 places in), column sums for the mean as one partial per workgroup, added in a fixed order;
//             a complex64 sequence keeps the reference's float32 arithmetic, its mean is numpy's pairwise sum
//   forward   rocFFT, all sequences in one batch, once; every pair reuses them
//   product   A_m conj(B_n) (two received modes per transform in 'amp') -> rocFFT inverse, all pairs in one batch
//   peaks     per correlation and part max |c|, its lowest index and the signed value: grid-stride, wave shuffle, LDS, one
//             candidate per workgroup, a second launch merges the candidates -- the merge is order-independent
//   decide    one lane: corrMatrix, swap, rot, and in 'real' after a second round of nModes correlations delay and conj
//   gather    out[i, k] = f(tx[(i + delay[k]) mod n_tx, swap[k]]); swap, rot, conj, delay are read from device memory
// No host decision between the launches; the record is copied once at the end.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "engine_host.h"
#include "sync_kernels.h"

namespace ssf {
namespace {
using namespace sk;
using namespace eng;

static_assert(kBlock == br::kBlock, "block_reduce.h is written for this workgroup");
constexpr int kWaves = br::kWaves;
constexpr int kPwDepth = 16;                  // frames of the pairwise recursion inside one chunk of 8192 (it needs 7)

struct SyncArgs {
    int mode, round, nModes, dtype, f32, side;   // side 0: transmitted (x), 1: received (y)
    long long n, off, L, lags, n_tx;
    const void *x;                            // (n, nModes) of dtype
    Cplx *F, *G;                              // (sequences, L), (slots, L)
    double *part;                             // (2 sides, kMaxBlocks, kMaxModes) column sums
    double *mean;                             // (2 sides, kMaxModes)
    const long long *leaf_start;              // numpy's pairwise leaves of a sequence of n elements
    float *leaf_sum;                          // (kMaxModes, nleaf)
    long long nleaf;
    int nb, nslots, peak_base;
    double scale;
    Peak *cand, *peak;                        // (slots, 2, nb); (first-round slots + nModes, 2)
    Record *rec;
    void *out;
};

// one lane per row: consecutive lanes read consecutive rows of nModes elements each
__global__ __launch_bounds__(kBlock) void k_prepare(SyncArgs a) {
    double acc[kMaxModes];
#pragma unroll
    for (int m = 0; m < kMaxModes; ++m) acc[m] = 0.0;
    const int base = a.side ? a.nModes : 0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
#pragma unroll
        for (int m = 0; m < kMaxModes; ++m) {
            if (m >= a.nModes) break;
            double re, im;
            load(a.dtype, a.x, i * a.nModes + m, re, im);
            Cplx v;
            if (a.mode == kAmp) {
                v.re = amp_value(re, im, a.f32), v.im = 0.0;
                acc[m] += v.re;
            } else if (a.mode == kReal && a.side) {
                v.re = re, v.im = 0.0;
                Cplx w;
                w.re = im, w.im = 0.0;
                a.F[(long long)(2 * a.nModes + m) * a.L + i] = w;
            } else {
                v.re = re, v.im = im;
            }
            a.F[(long long)(base + m) * a.L + a.off + i] = v;
        }
    }
    if (a.mode != kAmp) return;
    for (int m = 0; m < a.nModes; ++m)
        br::block_sum_store(acc[m], a.part + ((long long)a.side * kMaxBlocks + blockIdx.x) * kMaxModes + m);
}

__global__ __launch_bounds__(kBlock) void k_pw_leaf(SyncArgs a) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int m = blockIdx.y, base = a.side ? a.nModes : 0;
    if (t >= a.nleaf) return;
    const long long first = a.leaf_start[t], len = a.leaf_start[t + 1] - first;
    a.leaf_sum[(long long)m * a.nleaf + t] = pw_leaf_re(a.F + (long long)(base + m) * a.L + a.off + first, len);
}

// the column means of one side: lane m adds the partials of column m in order
__global__ __launch_bounds__(64) void k_means(SyncArgs a) {
    __shared__ mk::PwFrame stk[kMaxModes][kPwDepth];
    const int m = threadIdx.x;
    if (m >= a.nModes) return;
    double mean;
    if (a.f32) {
        mean = mean_f32(mk::pw_combine(a.leaf_sum + (long long)m * a.nleaf, a.n, stk[m]), a.n);
    } else {
        double s = 0.0;
        for (int b = 0; b < a.nb; ++b) s += a.part[((long long)a.side * kMaxBlocks + b) * kMaxModes + m];
        mean = s / (double)a.n;
    }
    a.mean[a.side * kMaxModes + m] = mean;
}

__global__ __launch_bounds__(kBlock) void k_center(SyncArgs a) {
    const int m = blockIdx.y, base = a.side ? a.nModes : 0;
    const double mean = a.mean[a.side * kMaxModes + m];
    Cplx *f = a.F + (long long)(base + m) * a.L + a.off;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock)
        f[i].re = center_value(f[i].re, mean, a.f32);
}

__global__ __launch_bounds__(kBlock) void k_product(SyncArgs a) {
    int sa, sb, sb2;
    slot_sequences(a.mode, a.round, a.nModes, blockIdx.y, a.rec->swap, sa, sb, sb2);
    const Cplx *A = a.F + (long long)sa * a.L, *B = a.F + (long long)sb * a.L, *B2 = a.F + (long long)(sb2 < 0 ? sb : sb2) * a.L;
    Cplx *g = a.G + (long long)blockIdx.y * a.L;
    for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < a.L; j += (long long)gridDim.x * kBlock)
        g[j] = sb2 < 0 ? spectral_product(A[j], B[j], a.scale) : spectral_pair(A[j], B[j], B2[j], a.scale);
}

__device__ void block_peak(Peak &p, Peak *sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Peak q;
        q.mag = __shfl_down(p.mag, o, 64), q.idx = __shfl_down(p.idx, o, 64), q.val = __shfl_down(p.val, o, 64);
        peak_merge(p, q);
    }
    __syncthreads();
    if (lane == 0) sh[wave] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kWaves; ++w) peak_merge(p, sh[w]);
}

__global__ __launch_bounds__(kBlock) void k_peaks(SyncArgs a) {
    __shared__ Peak sh[kWaves];
    const int slot = blockIdx.y;
    const Cplx *g = a.G + (long long)slot * a.L;
    Peak p0 = peak_none(a.lags), p1 = peak_none(a.lags);
    for (long long j = (long long)blockIdx.x * kBlock + threadIdx.x; j < a.lags; j += (long long)gridDim.x * kBlock)
        peak_channels(a.mode, g[j], j, p0, p1);
    block_peak(p0, sh);
    block_peak(p1, sh);
    if (threadIdx.x == 0) {
        a.cand[((long long)slot * 2) * a.nb + blockIdx.x] = p0;
        a.cand[((long long)slot * 2 + 1) * a.nb + blockIdx.x] = p1;
    }
}

// the candidates of one (slot, part) -> its peak
__global__ __launch_bounds__(kBlock) void k_peaks_fin(SyncArgs a) {
    __shared__ Peak sh[kWaves];
    const int sc = blockIdx.x;
    Peak p = peak_none(a.lags);
    for (int b = threadIdx.x; b < a.nb; b += kBlock) peak_merge(p, a.cand[(long long)sc * a.nb + b]);
    block_peak(p, sh);
    if (threadIdx.x == 0) a.peak[a.peak_base + sc] = p;
}

__global__ void k_decide(SyncArgs a) {
    if (threadIdx.x || blockIdx.x) return;
    Record &r = *a.rec;
    const int first = 2 * n_slots(a.mode, a.nModes);
    if (a.mode == kAmp) decide_amp(a.nModes, a.n_tx, a.peak, r);
    else if (a.mode == kReal && a.round == 1) decide_real_rot(a.nModes, a.peak, r);
    else if (a.mode == kReal) decide_real_delay(a.nModes, a.n_tx, a.peak, a.peak + first, r);
    else r.peak_index[0] = a.peak[0].idx, r.delay[0] = a.peak[0].idx - (a.n_tx - 1);
}

// flat over (n_tx, nModes): stores are contiguous, loads contiguous along the modes that keep their column
template <class T> __global__ __launch_bounds__(kBlock) void k_gather(SyncArgs a) {
    const T *tx = (const T *)a.x;
    T *out = (T *)a.out;
    const Record &r = *a.rec;
    const long long total = a.n * a.nModes;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long long)gridDim.x * kBlock) {
        const long long i = e / a.nModes;
        const int k = (int)(e - i * a.nModes);
        int s = r.swap[k];
        s = s < 0 ? 0 : s >= a.nModes ? a.nModes - 1 : s;
        T v = tx[roll_source(i, r.delay[k], a.n) * a.nModes + s];
        rotate_conj(v.re, v.im, r.rot[k], r.conj[k]);
        out[e] = v;
    }
}

__global__ __launch_bounds__(kBlock) void k_widen(const CplxF *x, Cplx *y, long long count) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += (long long)gridDim.x * kBlock) {
        const CplxF v = x[i];
        Cplx w;
        w.re = (double)v.re, w.im = (double)v.im;
        y[i] = w;
    }
}

// ---- host side
struct Work : WorkBase {
    Buf in_x, in_y, wide, dec, F, G, part, mean, leaf_sum, cand, peak, rec, out;
    FftPlans plans;
    PwLeaves leaves;
};
using Call = CallT<Work>;

// one side into the transform buffers, centred in 'amp'
bool prepare(Call &c, SyncArgs a, int side, const void *x, int dtype, bool f32, long long n, long long off) {
    Work &w = *c.w;
    a.side = side, a.x = x, a.dtype = dtype, a.f32 = f32, a.n = n, a.off = off;
    a.nb = grid_blocks(n, kBlock, kMaxBlocks, 1);
    k_prepare<<<a.nb, kBlock, 0, w.st>>>(a);
    if (a.mode == kAmp) {
        if (f32) {
            if (!pairwise_leaves(c, w.leaves, n, a.nleaf, a.leaf_start)) return false;
            if (!c.need(w.leaf_sum, (size_t)kMaxModes * a.nleaf * sizeof(float))) return false;
            a.leaf_sum = (float *)w.leaf_sum.p;
            k_pw_leaf<<<dim3((unsigned)((a.nleaf + kBlock - 1) / kBlock), a.nModes), kBlock, 0, w.st>>>(a);
        }
        k_means<<<1, 64, 0, w.st>>>(a);
        k_center<<<dim3(a.nb, a.nModes), kBlock, 0, w.st>>>(a);
    }
    return c.launched();
}

// product -> inverse transforms -> peaks of `nslots` correlations, left at a.peak[peak_base ...]
bool correlate(Call &c, SyncArgs a, int round, int nslots, int peak_base) {
    Work &w = *c.w;
    a.round = round, a.nslots = nslots, a.peak_base = peak_base;
    k_product<<<dim3(grid_blocks(a.L, kBlock, kMaxBlocks, 1), nslots), kBlock, 0, w.st>>>(a);
    if (!c.launched()) return false;
    if (!transform(c, a.G, a.L, nslots, true)) return false;
    a.nb = grid_blocks(a.lags, kBlock, kMaxBlocks, 1);
    k_peaks<<<dim3(a.nb, nslots), kBlock, 0, w.st>>>(a);
    k_peaks_fin<<<2 * nslots, kBlock, 0, w.st>>>(a);
    k_decide<<<1, 64, 0, w.st>>>(a);
    return c.launched();
}

// everything up to the record in device memory; x, y: device pointers
bool run(Call &c, int mode, int nModes, const void *x, int x_dtype, bool x_f32, long long n_x, const void *y, int y_dtype, bool y_f32,
         long long n_y) {
    Work &w = *c.w;
    SyncArgs a{};
    a.mode = mode, a.nModes = nModes, a.n_tx = n_x;
    a.lags = n_x + n_y - 1;
    a.L = 4;
    while (a.L < a.lags) a.L <<= 1;
    a.scale = 1.0 / (double)a.L;
    const int nseq = n_sequences(mode, nModes), nslots = n_slots(mode, nModes);
    const size_t seq_bytes = (size_t)a.L * sizeof(Cplx);
    if (!c.need(w.F, nseq * seq_bytes) || !c.need(w.G, nslots * seq_bytes)) return false;
    if (!c.need(w.part, 2 * (size_t)kMaxBlocks * kMaxModes * sizeof(double)) || !c.need(w.mean, 2 * kMaxModes * sizeof(double))) return false;
    if (!c.need(w.cand, 2 * (size_t)nslots * kMaxBlocks * sizeof(Peak)) || !c.need(w.peak, 2 * (size_t)(nslots + nModes) * sizeof(Peak))) return false;
    if (!c.need(w.rec, sizeof(Record))) return false;
    a.F = (Cplx *)w.F.p, a.G = (Cplx *)w.G.p, a.part = (double *)w.part.p, a.mean = (double *)w.mean.p;
    a.cand = (Peak *)w.cand.p, a.peak = (Peak *)w.peak.p, a.rec = (Record *)w.rec.p;
    if (!c.ok(hipMemsetAsync(w.F.p, 0, nseq * seq_bytes, w.st), "hipMemset")) return false;
    if (!c.ok(hipMemsetAsync(w.rec.p, 0, sizeof(Record), w.st), "hipMemset")) return false;
    if (!prepare(c, a, 0, x, x_dtype, x_f32, n_x, n_y - 1)) return false;
    if (!prepare(c, a, 1, y, y_dtype, y_f32, n_y, 0)) return false;
    if (!transform(c, a.F, a.L, nseq, false)) return false;
    if (!correlate(c, a, 1, nslots, 0)) return false;
    if (mode == kReal && !correlate(c, a, 2, nModes, 2 * nslots)) return false;
    return true;
}

bool fetch_record(Call &c, Record &r, int cols, long long lags) {
    if (!c.deliver(&r, c.w->rec.p, sizeof(Record)) || !c.sync()) return false;
    for (int k = 0; k < cols; ++k)
        if (r.peak_index[k] < 0 || r.peak_index[k] >= lags) return c.reject(SSF_ERR_BAD_ARG, "no correlation peak (the input is not finite)");
    return true;
}

}  // namespace

int sync_run(int device, const ssf_sync_params *p, const void *rx, const void *tx, void *out, ssf_sync_result *res, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int nModes = p->nModes;
    const size_t tx_bytes = (size_t)p->n_tx * nModes * mk::elem_size(p->tx_dtype), rx_count = (size_t)p->n_rx * nModes;
    void *o = c.target(out, w.out, tx_bytes);
    if (!o) return c.rc;
    const void *txd = c.input(tx, w.in_x, tx_bytes);
    if (!txd) return c.rc;
    const void *rxd = nullptr;
    int rx_dtype = p->rx_dtype;
    long long n_rx = p->n_rx;
    if (p->SpS > 1) {
        // the received signal to one sample per symbol with decimate's own kernels (complex128 in, complex128 out)
        const void *in = rx;
        if (rx_dtype == mk::kC64) {
            const void *r32 = c.input(rx, w.in_y, rx_count * sizeof(CplxF));
            if (!r32 || !c.need(w.wide, rx_count * sizeof(Cplx))) return c.rc;
            k_widen<<<grid_blocks((long long)rx_count, kBlock, kMaxBlocks, 1), kBlock, 0, w.st>>>((const CplxF *)r32, (Cplx *)w.wide.p, (long long)rx_count);
            if (!c.launched() || !c.sync()) return c.rc;
            in = w.wide.p;
        }
        n_rx = p->n_rx / p->SpS;
        if (!c.need(w.dec, (size_t)n_rx * nModes * sizeof(Cplx))) return c.rc;
        if (int rc = rx_decimate(device, p->n_rx, nModes, p->SpS, p->SpS, in, w.dec.p, nullptr, err)) return rc;
        if (!c.ok(hipSetDevice(device), "hipSetDevice")) return c.rc;
        rxd = w.dec.p, rx_dtype = mk::kC128;
    } else {
        rxd = c.input(rx, w.in_y, rx_count * mk::elem_size(rx_dtype));
        if (!rxd) return c.rc;
    }
    if (!run(c, p->mode, nModes, txd, p->tx_dtype, p->tx_dtype == mk::kC64, p->n_tx, rxd, rx_dtype, p->rx_dtype == mk::kC64, n_rx)) return c.rc;
    SyncArgs g{};
    g.x = txd, g.out = o, g.n = p->n_tx, g.nModes = nModes, g.rec = (Record *)w.rec.p;
    const int nb = grid_blocks(p->n_tx * nModes, kBlock, kMaxBlocks, 1);
    if (p->tx_dtype == mk::kC64) k_gather<CplxF><<<nb, kBlock, 0, w.st>>>(g);
    else k_gather<Cplx><<<nb, kBlock, 0, w.st>>>(g);
    if (!c.launched()) return c.rc;
    if (!c.deliver(out, o, tx_bytes)) return c.rc;
    Record r;
    if (!fetch_record(c, r, nModes, p->n_tx + n_rx - 1)) return c.rc;
    if (res) {
        *res = ssf_sync_result{};
        for (int k = 0; k < nModes; ++k) res->delay[k] = r.delay[k], res->swap[k] = r.swap[k], res->rot[k] = r.rot[k], res->conj[k] = r.conj[k];
        for (int i = 0; i < nModes * nModes; ++i) res->corrMatrix[i] = r.corr[i];
    }
    return SSF_OK;
}

int sync_finddelay(int device, int64_t nx, int64_t ny, int x_dtype, int y_dtype, const void *x, const void *y, int64_t *delay_out,
                   std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const void *xd = c.input(x, w.in_x, (size_t)nx * mk::elem_size(x_dtype));
    const void *yd = xd ? c.input(y, w.in_y, (size_t)ny * mk::elem_size(y_dtype)) : nullptr;
    if (!xd || !yd) return c.rc;
    if (!run(c, kDelay, 1, xd, x_dtype, false, nx, yd, y_dtype, false, ny)) return c.rc;
    Record r;
    if (!fetch_record(c, r, 1, nx + ny - 1)) return c.rc;
    *delay_out = r.delay[0];
    return SSF_OK;
}

// the call's transforms alone, on the engine's own buffers and plans: seconds per round of (forward x nseq, inverse x nslots,
// inverse x nslots2), from device events around `reps` rounds (tools/bench_sync.py: the floor the kernels add to)
int sync_transform_time(int device, int64_t L, int nseq, int nslots, int nslots2, int reps, double *seconds_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t seq_bytes = (size_t)L * sizeof(Cplx);
    if (!c.need(w.F, nseq * seq_bytes) || !c.need(w.G, nslots * seq_bytes)) return c.rc;
    if (!c.ok(hipMemsetAsync(w.F.p, 0, nseq * seq_bytes, w.st), "hipMemset")) return c.rc;
    if (!c.ok(hipMemsetAsync(w.G.p, 0, nslots * seq_bytes, w.st), "hipMemset")) return c.rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!c.ok(hipEventCreate(&e0), "hipEventCreate") || !c.ok(hipEventCreate(&e1), "hipEventCreate")) return c.rc;
    bool good = true;
    for (int r = -1; r < reps && good; ++r) {                      // round -1 warms the plans up
        if (r == 0) good = c.ok(hipEventRecord(e0, w.st), "hipEventRecord");
        good = good && transform(c, w.F.p, L, nseq, false) && transform(c, w.G.p, L, nslots, true);
        if (good && nslots2) good = transform(c, w.G.p, L, nslots2, true);
    }
    float ms = 0.f;
    good = good && c.ok(hipEventRecord(e1, w.st), "hipEventRecord") && c.sync() && c.ok(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!good) return c.rc;
    *seconds_out = (double)ms * 1e-3 / (double)reps;
    return SSF_OK;
}

}  // namespace ssf
