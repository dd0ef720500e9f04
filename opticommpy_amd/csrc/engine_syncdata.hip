// engine_syncdata.hip -- the glue of syncDataSequences, movingAverage and bert on the device (ssf_sync_tile, ssf_sync_extract,
// ssf_real_part, ssf_copy_columns, ssf_moving_average, ssf_bert of include/ssf.h).
//   columns   one lane per element of a block of columns copied between two row-major arrays (decimate takes six columns at 41
//             samples per symbol: 'signal' mode splits seven or eight and merges the results).
//   tile      one lane per element of the padded length: the tiled (and zero-stuffed) transmitted sequence and the zero-padded
//             received one, both complex128.
//   extract   count (a workgroup per kSpan rows and column: kept samples and their power, the power through block_reduce.h) ->
//             offsets (a workgroup per column: exclusive scan of the counts, lane-chunked, and the column's norm from the partial
//             powers in a fixed order) -> scatter (the count's flags again, a wave scan of the lanes' counts by __shfl_up, the
//             waves' totals through LDS, then every lane writes its kept samples at its rank, divided by the norm).
//   average   a workgroup per kMaTile rows and column: tile and halo into LDS (zeros loaded, never stored), each lane sums the
//             windows of its outputs (lane, lane + 256, ..: neighbouring lanes read neighbouring LDS words) from the lowest row up.
//   bert      grid-stride passes with block_reduce.h's sums; a single wave combines the partials and leaves the scalars.
// No atomics: for a given shape every result repeats bit for bit.
#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "engine_host.h"
#include "syncdata_kernels.h"

namespace ssf {
namespace {
using namespace sd;
using namespace eng;
static_assert(kBlock == br::kBlock, "the sums are written for this workgroup");

// ---- tile
struct TileArgs {
    long long nRx, nTx, nPad;
    int modes, SpS, rx_dtype, tx_dtype;
    const void *rx, *tx;
    Cplx *rx_out, *tx_out;
};
__global__ __launch_bounds__(kBlock) void k_tile(TileArgs a) {
    const long long total = a.nPad * a.modes;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < total; g += (long long)gridDim.x * kBlock) {
        const long long i = g / a.modes;
        const int m = (int)(g % a.modes);
        a.tx_out[g] = tile_tx(a.tx_dtype, a.tx, i, m, a.modes, a.nTx, a.SpS);
        a.rx_out[g] = pad_rx(a.rx_dtype, a.rx, i, m, a.modes, a.nRx);
    }
}

__global__ __launch_bounds__(kBlock) void k_real_part(const Cplx *x, double *out, long long count) {
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < count; g += (long long)gridDim.x * kBlock) out[g] = x[g].re;
}

struct ColArgs {
    long long n;
    int width, src_cols, src_first, dst_cols, dst_first;
    const Cplx *src;
    Cplx *dst;
};
__global__ __launch_bounds__(kBlock) void k_copy_columns(ColArgs a) {
    const long long total = a.n * a.width;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < total; g += (long long)gridDim.x * kBlock) {
        long long from, to;
        column_block_index(g, a.width, a.src_cols, a.src_first, a.dst_cols, a.dst_first, from, to);
        a.dst[to] = a.src[from];
    }
}

// ---- extraction
struct ExtArgs {
    long long n, nb, nOut;
    int modes, cx_out, normalize;
    const Cplx *x;
    void *out;
    int *cnt;                                 // [col][workgroup]: kept samples
    long long *off;                           // [col][workgroup]: kept before the workgroup; the column's total at [modes * nb + col]
    double *pw;                               // [col][workgroup]: power of the kept samples
    double *norm;                             // [col]
};

// the kept samples of the lanes before this one in the workgroup; total: the workgroup's (scan_step / rank_before of
// syncdata_kernels.h, the shuffles and the LDS slots here)
__device__ int block_rank(int c, int &total) {
    __shared__ int wtot[br::kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) inc = scan_step(inc, __shfl_up(inc, o, 64), lane, o);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    return rank_before(wtot, br::kWaves, wave, inc, c, total);
}

__global__ __launch_bounds__(kBlock) void k_ext_count(ExtArgs a) {
    const int col = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * kSpan + (long long)threadIdx.x * kItems;
    double pw;
    const int f = lane_flags(a.x, a.n, a.modes, col, row0, pw);
    int total;
    block_rank(popcount4(f), total);
    const long long slot = (long long)col * a.nb + blockIdx.x;
    if (threadIdx.x == 0) a.cnt[slot] = total;
    br::block_sum_store(pw, a.pw + slot);
}

__global__ __launch_bounds__(kBlock) void k_ext_offsets(ExtArgs a) {
    __shared__ long long chunk[kBlock];
    const int col = blockIdx.x;
    const int *cnt = a.cnt + (long long)col * a.nb;
    long long *off = a.off + (long long)col * a.nb;
    long long lo, hi, s = 0;
    offsets_chunk(a.nb, threadIdx.x, lo, hi);
    for (long long b = lo; b < hi; ++b) s += cnt[b];
    chunk[threadIdx.x] = s;
    __syncthreads();
    long long before = 0, total = 0;
    for (int l = 0; l < kBlock; ++l) {
        if (l < (int)threadIdx.x) before += chunk[l];
        total += chunk[l];
    }
    for (long long b = lo; b < hi; ++b) off[b] = before, before += cnt[b];
    if (threadIdx.x < 64) {
        const double p = br::wave_sum_partials(a.pw + (long long)col * a.nb, (int)a.nb, 1);
        if (threadIdx.x == 0) {
            a.off[(long long)a.modes * a.nb + col] = total;
            a.norm[col] = a.normalize ? column_norm(p, total) : 1.0;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_ext_scatter(ExtArgs a) {
    const int col = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * kSpan + (long long)threadIdx.x * kItems;
    double pw;
    const int f = lane_flags(a.x, a.n, a.modes, col, row0, pw);
    int total;
    const int before = block_rank(popcount4(f), total);
    const long long at = a.off[(long long)col * a.nb + blockIdx.x] + before;
    lane_scatter(a.x, a.modes, col, row0, f, at, a.norm[col], a.cx_out != 0, a.out, a.nOut);
}

// ---- windowed mean
struct MaArgs {
    long long n;
    int cols, N, dtype;
    const void *x;
    void *out;
};
template <bool CX> __global__ __launch_bounds__(kBlock) void k_moving_average(MaArgs a) {
    __shared__ __attribute__((aligned(16))) double w[(kMaTile + kMaMaxN - 1) * (CX ? 2 : 1)];
    const int col = blockIdx.y;
    const long long t0 = (long long)blockIdx.x * kMaTile;
    const long long left = a.n - t0;
    const int cnt = left < kMaTile ? (int)left : kMaTile;
    const int have = cnt + a.N - 1;           // rows t0 - N / 2 .. t0 + cnt - 1 + (N - 1) / 2
    for (int j = threadIdx.x; j < have; j += kBlock) {
        const long long r = t0 - a.N / 2 + j;
        double re = 0.0, im = 0.0;
        if (r >= 0 && r < a.n) mk::load(a.dtype, a.x, r * a.cols + col, re, im);
        if constexpr (CX) w[2 * j] = re, w[2 * j + 1] = im;
        else w[j] = re;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < cnt; o += kBlock) {
        double re, im;
        window_mean<CX>(w, o, a.N, re, im);
        const long long g = (t0 + o) * a.cols + col;
        if constexpr (CX) ((Cplx *)a.out)[g] = Cplx{re, im};
        else ((double *)a.out)[g] = re;
    }
}

// ---- bert
struct BertArgs {
    long long n;
    int nb;
    const double *x;
    const uint8_t *bits;
    double *part;                             // [workgroup][3]
    double *scal;                             // kBertScal
};
__global__ __launch_bounds__(kBlock) void k_bert_stats(BertArgs a) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) bert_stats(acc, a.x[i], a.bits[i] == 1);
    br::block_sum_store<3>(acc, a.part + 3LL * blockIdx.x);
}
__global__ __launch_bounds__(kBlock) void k_bert_dev(BertArgs a) {
    const double I1 = a.scal[2], I0 = a.scal[3];
    double acc[2] = {0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock)
        bert_dev(acc, a.x[i], a.bits[i] == 1, I1, I0);
    br::block_sum_store<2>(acc, a.part + 3LL * blockIdx.x);
}
__global__ __launch_bounds__(kBlock) void k_bert_errors(BertArgs a) {
    const double Id = a.scal[6];
    double e = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) e += bert_error(a.x[i], a.bits[i] == 1, Id);
    br::block_sum_store(e, a.part + 3LL * blockIdx.x);
}
// one wave: the totals of pass `pass` and the scalars that follow from them
__global__ __launch_bounds__(64) void k_bert_fin(BertArgs a, int pass) {
    double tot[3];
    for (int k = 0; k < 3; ++k) tot[k] = br::wave_sum_partials(a.part + k, a.nb, 3);
    if (threadIdx.x != 0) return;
    if (pass == 0) bert_means(tot, a.n, a.scal);
    else if (pass == 1) bert_threshold(tot, a.scal);
    else a.scal[8] = tot[0], a.scal[9] = 0.0;
}

// ---- host side
struct Work : WorkBase {
    Buf in, in2, out, out2, cnt, off, pw, norm, part, scal;
};
using Call = CallT<Work>;

}  // namespace

int syncdata_tile(int device, const ssf_sync_tile_params *p, const void *rx, const void *tx, void *rx_out, void *tx_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t out_bytes = (size_t)p->n_pad * p->nModes * sizeof(Cplx);
    TileArgs a{};
    a.nRx = p->n_rx, a.nTx = p->n_tx, a.nPad = p->n_pad, a.modes = p->nModes, a.SpS = p->SpS, a.rx_dtype = p->rx_dtype, a.tx_dtype = p->tx_dtype;
    a.rx_out = (Cplx *)c.target(rx_out, w.out, out_bytes);
    a.tx_out = (Cplx *)c.target(tx_out, w.out2, out_bytes);
    if (!a.rx_out || !a.tx_out) return c.rc;
    if (!(a.rx = c.input(rx, w.in, (size_t)p->n_rx * p->nModes * mk::elem_size(p->rx_dtype)))) return c.rc;
    if (!(a.tx = c.input(tx, w.in2, (size_t)p->n_tx * p->nModes * mk::elem_size(p->tx_dtype)))) return c.rc;
    k_tile<<<grid_blocks(a.nPad * a.modes, kBlock, kElemMaxBlocks), kBlock, 0, w.st>>>(a);
    if (!c.launched() || !c.deliver(rx_out, a.rx_out, out_bytes) || !c.deliver(tx_out, a.tx_out, out_bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int syncdata_real_part(int device, int64_t count, const void *x, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    double *o = (double *)c.target(out, w.out, (size_t)count * sizeof(double));
    if (!o) return c.rc;
    const Cplx *xd = (const Cplx *)c.input(x, w.in, (size_t)count * sizeof(Cplx));
    if (!xd) return c.rc;
    k_real_part<<<grid_blocks(count, kBlock, kElemMaxBlocks), kBlock, 0, w.st>>>(xd, o, count);
    if (!c.launched() || !c.deliver(out, o, (size_t)count * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

int syncdata_copy_columns(int device, int64_t n, int width, int src_cols, int src_first, int dst_cols, int dst_first, const void *src, void *dst,
                          std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    ColArgs a{};
    a.n = n, a.width = width, a.src_cols = src_cols, a.src_first = src_first, a.dst_cols = dst_cols, a.dst_first = dst_first;
    a.src = (const Cplx *)src, a.dst = (Cplx *)dst;
    k_copy_columns<<<grid_blocks(n * width, kBlock, kElemMaxBlocks), kBlock, 0, c.w->st>>>(a);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int syncdata_extract(int device, int64_t n, int modes, int64_t n_out, int out_dtype, int normalize, const void *x, void *out, int64_t *kept,
                     std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const bool cx = out_dtype == mk::kC128;
    const size_t out_bytes = (size_t)n_out * modes * (cx ? sizeof(Cplx) : sizeof(double));
    ExtArgs a{};
    a.n = n, a.nb = ext_blocks(n), a.nOut = n_out, a.modes = modes, a.cx_out = cx, a.normalize = normalize;
    a.out = c.target(out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.x = (const Cplx *)c.input(x, w.in, (size_t)n * modes * sizeof(Cplx));
    if (!a.x) return c.rc;
    const size_t slots = (size_t)modes * a.nb;
    if (!c.need(w.cnt, slots * sizeof(int)) || !c.need(w.off, (slots + modes) * sizeof(long long)) || !c.need(w.pw, slots * sizeof(double)) ||
        !c.need(w.norm, (size_t)modes * sizeof(double)))
        return c.rc;
    a.cnt = (int *)w.cnt.p, a.off = (long long *)w.off.p, a.pw = (double *)w.pw.p, a.norm = (double *)w.norm.p;
    if (!c.ok(hipMemsetAsync(a.out, 0, out_bytes, w.st), "hipMemset")) return c.rc;
    const dim3 grid((unsigned)a.nb, (unsigned)modes);
    k_ext_count<<<grid, kBlock, 0, w.st>>>(a);
    k_ext_offsets<<<modes, kBlock, 0, w.st>>>(a);
    k_ext_scatter<<<grid, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    if (!c.deliver(kept, a.off + slots, (size_t)modes * sizeof(int64_t)) || !c.deliver(out, a.out, out_bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int syncdata_moving_average(int device, int64_t n, int cols, int N, int dtype, const void *x, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const bool cx = dtype != mk::kF64;
    const size_t out_bytes = (size_t)n * cols * (cx ? sizeof(Cplx) : sizeof(double));
    MaArgs a{};
    a.n = n, a.cols = cols, a.N = N, a.dtype = dtype;
    a.out = c.target(out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.x = c.input(x, w.in, (size_t)n * cols * mk::elem_size(dtype));
    if (!a.x) return c.rc;
    const dim3 grid((unsigned)((n + kMaTile - 1) / kMaTile), (unsigned)cols);
    if (cx) k_moving_average<true><<<grid, kBlock, 0, w.st>>>(a);
    else k_moving_average<false><<<grid, kBlock, 0, w.st>>>(a);
    if (!c.launched() || !c.deliver(out, a.out, out_bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

int syncdata_bert(int device, int64_t n, const void *irx, const void *bits, double *scal_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    BertArgs a{};
    a.n = n, a.nb = grid_blocks(n, kBlock, kBertMaxBlocks);
    if (!c.need(w.part, (size_t)a.nb * 3 * sizeof(double)) || !c.need(w.scal, kBertScal * sizeof(double))) return c.rc;
    if (!(a.x = (const double *)c.input(irx, w.in, (size_t)n * sizeof(double)))) return c.rc;
    if (!(a.bits = (const uint8_t *)c.input(bits, w.in2, (size_t)n))) return c.rc;
    a.part = (double *)w.part.p, a.scal = (double *)w.scal.p;
    k_bert_stats<<<a.nb, kBlock, 0, w.st>>>(a);
    k_bert_fin<<<1, 64, 0, w.st>>>(a, 0);
    k_bert_dev<<<a.nb, kBlock, 0, w.st>>>(a);
    k_bert_fin<<<1, 64, 0, w.st>>>(a, 1);
    k_bert_errors<<<a.nb, kBlock, 0, w.st>>>(a);
    k_bert_fin<<<1, 64, 0, w.st>>>(a, 2);
    if (!c.launched()) return c.rc;
    if (!c.deliver(scal_out, a.scal, kBertScal * sizeof(double)) || !c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
