// engine_metrics.hip -- link metrics on the device (ssf_metrics, ssf_pnorm, ssf_signal_power, ssf_demodulate of include/ssf.h).
// Three passes over the symbols, each followed by a one-wave combine kernel; the rotation, the norms and sigma^2 stay in device
// memory between them (no host wait before the results are copied back).  Every sum is wave shuffle -> LDS -> one partial per
// workgroup, and the partials are added in a fixed order: no floating-point atomics, results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "block_reduce.h"
#include "engine_host.h"
#include "metrics_kernels.h"

namespace ssf {
namespace {
using namespace mk;
using namespace eng;

constexpr int kBlock = br::kBlock, kMaxBlocks = 512;
constexpr int kPwDepth = 16;              // frames of the pairwise recursion inside one chunk of 8192 (it needs 7)

struct KArgs {
    const void *rx, *tx;
    long long n0, n, sn, sm;              // first evaluated row, evaluated rows, element strides of a row / a mode
    int nModes, M, bits, dtype, rotate, has_tx, want, nb;
    double sqrtEs, H;
    const double *raw, *cn, *px, *log2px; // device tables
    const float *w32;
    double *part, *scal, *res;
    int32_t *idx;
    const long long *leaf_start;
    float *leaf_sum;
    long long nleaf;
};

// one wave: tot[mode * K + v] = sum over the nb partials of that mode
template <int K> __device__ void sum_partials(const double *part, int nb, int nModes, double *tot) {
    for (int q = 0; q < nModes * K; ++q) {
        const int k = q / K, v = q - k * K;
        const double a = br::wave_sum_partials(part + (long long)k * nb * K + v, nb, K);
        if (threadIdx.x == 0) tot[q] = a;
    }
    __syncthreads();
}

__device__ __forceinline__ void load_tables(double *dst, const double *src, int count) {
    for (int i = threadIdx.x; i < count; i += kBlock) dst[i] = src[i];
}

__global__ __launch_bounds__(kBlock) void k_stats(KArgs a) {
    const int k = blockIdx.y;
    double acc[kStatN] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        const long long off = (a.n0 + i) * a.sn + k * a.sm;
        double rr, ri, tr = 0.0, ti = 0.0;
        load(a.dtype, a.rx, off, rr, ri);
        if (a.has_tx) load(a.dtype, a.tx, off, tr, ti);
        stats_body(acc, a.rotate != 0, a.has_tx != 0, rr, ri, tr, ti);
    }
    br::block_sum_store<kStatN>(acc, a.part + ((long long)k * gridDim.x + blockIdx.x) * kStatN);
}

__global__ __launch_bounds__(64) void k_stats_fin(KArgs a) {
    __shared__ double tot[kMaxModes * kStatN];
    sum_partials<kStatN>(a.part, a.nb, a.nModes, tot);
    if (threadIdx.x == 0) {
        stats_combine(tot, a.nModes, a.n, a.rotate != 0, a.has_tx != 0, a.scal);
        for (int k = 0; k < a.nModes; ++k) a.scal[k * kScalN + 9] = tot[k * kStatN + 2], a.scal[k * kScalN + 10] = tot[k * kStatN + 3];
    }
}

__global__ __launch_bounds__(kBlock) void k_decide(KArgs a) {
    extern __shared__ double lds[];
    const int k = blockIdx.y;
    load_tables(lds, a.raw, 2 * a.M);
    double s[kScalN];
#pragma unroll
    for (int j = 0; j < kScalN; ++j) s[j] = a.scal[k * kScalN + j];
    __syncthreads();
    double acc[kDecN] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        const long long off = (a.n0 + i) * a.sn + k * a.sm;
        double rr, ri, tr, ti;
        load(a.dtype, a.rx, off, rr, ri);
        load(a.dtype, a.tx, off, tr, ti);
        decide_body(acc, s, lds, a.M, a.sqrtEs, a.want, rr, ri, tr, ti);
    }
    br::block_sum_store<kDecN>(acc, a.part + ((long long)k * gridDim.x + blockIdx.x) * kDecN);
}

__global__ __launch_bounds__(64) void k_decide_fin(KArgs a) {
    __shared__ double tot[kMaxModes * kDecN];
    sum_partials<kDecN>(a.part, a.nb, a.nModes, tot);
    const int k = threadIdx.x;
    if (k < a.nModes) decide_combine(tot + k * kDecN, a.n, a.bits, a.scal + k * kScalN, a.res + k * kResN);
}

__global__ __launch_bounds__(kBlock) void k_soft(KArgs a) {
    extern __shared__ double lds[];
    const int k = blockIdx.y, M = a.M;
    double *raw = lds, *cn = lds + 2 * M, *px = lds + 4 * M, *l2 = lds + 5 * M;
    load_tables(raw, a.raw, 2 * M);
    load_tables(cn, a.cn, 2 * M);
    load_tables(px, a.px, M);
    load_tables(l2, a.log2px, M);
    double s[kScalN];
#pragma unroll
    for (int j = 0; j < kScalN; ++j) s[j] = a.scal[k * kScalN + j];
    __syncthreads();
    double acc[kSoftN] = {0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        const long long off = (a.n0 + i) * a.sn + k * a.sm;
        double rr, ri, tr, ti;
        load(a.dtype, a.rx, off, rr, ri);
        load(a.dtype, a.tx, off, tr, ti);
        SoftDispatch<1>::run(a.bits, acc, s, raw, cn, px, l2, M, a.sqrtEs, rr, ri, tr, ti);
    }
    br::block_sum_store<kSoftN>(acc, a.part + ((long long)k * gridDim.x + blockIdx.x) * kSoftN);
}

__global__ __launch_bounds__(64) void k_soft_fin(KArgs a) {
    __shared__ double tot[kMaxModes * kSoftN];
    sum_partials<kSoftN>(a.part, a.nb, a.nModes, tot);
    const int k = threadIdx.x;
    if (k < a.nModes) soft_combine(tot + k * kSoftN, a.n, a.H, a.res + k * kResN);
}

// blind EVM: decisions against the single-precision pnorm(table) in a.cn; decided indices to idx[mode][row]
__global__ __launch_bounds__(kBlock) void k_blind(KArgs a) {
    extern __shared__ double lds[];
    const int k = blockIdx.y;
    load_tables(lds, a.cn, 2 * a.M);
    const double jrx = a.scal[k * kScalN + 6];
    __syncthreads();
    double acc[1] = {0.0};
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double rr, ri;
        load(a.dtype, a.rx, (a.n0 + i) * a.sn + k * a.sm, rr, ri);
        a.idx[(long long)k * a.n + i] = blind_body(acc, jrx, lds, a.M, rr, ri);
    }
    br::block_sum_store<1>(acc, a.part + ((long long)k * gridDim.x + blockIdx.x));
}

__global__ __launch_bounds__(kBlock) void k_pw_leaf(KArgs a) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    const int k = blockIdx.y;
    if (t >= a.nleaf) return;
    const long long first = a.leaf_start[t], len = a.leaf_start[t + 1] - first;
    a.leaf_sum[(long long)k * a.nleaf + t] = pw_leaf(a.w32, a.idx + (long long)k * a.n + first, len);
}

__global__ __launch_bounds__(64) void k_blind_fin(KArgs a) {
    __shared__ double tot[kMaxModes];
    __shared__ PwFrame stk[kMaxModes][kPwDepth];
    sum_partials<1>(a.part, a.nb, a.nModes, tot);
    const int k = threadIdx.x;
    if (k < a.nModes) {
        const float s32 = pw_combine(a.leaf_sum + (long long)k * a.nleaf, a.n, stk[k]);
        const float mean32 = (float)((double)s32 / (double)a.n);           // np.mean of float32: float32(float64(sum) / n)
        double *res = a.res + k * kResN;
        res[6] = (tot[k] / (double)a.n) / (double)mean32;
        res[9] = (double)a.n;
    }
}

// hard decisions of `n` symbols -> log2(M) bits each, most significant first
__global__ __launch_bounds__(kBlock) void k_demod(KArgs a, int32_t *bits) {
    extern __shared__ double lds[];
    load_tables(lds, a.raw, 2 * a.M);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double rr, ri;
        load(a.dtype, a.rx, i, rr, ri);
        const int m = nearest(lds, a.M, rr, ri);
        for (int j = 0; j < a.bits; ++j) bits[i * a.bits + j] = (m >> (a.bits - 1 - j)) & 1;
    }
}

// y = x / sqrt(mean |x|^2) in double precision
__global__ __launch_bounds__(kBlock) void k_scale(KArgs a, void *y) {
    const double s = a.scal[6];
    const bool cplx = a.dtype == kC128 || a.dtype == kC64;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double rr, ri;
        load(a.dtype, a.rx, i, rr, ri);
        if (cplx) {
            Cplx v;
            v.re = rr / s, v.im = ri / s;
            ((Cplx *)y)[i] = v;
        } else {
            ((double *)y)[i] = rr / s;
        }
    }
}

// ---- host side
struct Work : WorkBase {
    Buf tables, part, scal, res, idx, leaf_sum, in_rx, in_tx, out;
    PwLeaves leaves;
    std::vector<double> host_tab;             // kept for their capacity
    std::vector<float> host_w32;
};
using Call = CallT<Work>;

}  // namespace

int metrics_run(int device, const ssf_metrics_params *p, const void *rx, const void *tx, const double *const_raw,
                const double *const_norm, const double *px, const float *evm_w32, ssf_metrics_result *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int M = p->M, nModes = p->nModes;
    const bool blind = (p->want & kWantEvmBlind) != 0;
    int bits = 0;
    while ((1 << bits) < M) ++bits;

    KArgs a{};
    a.n0 = p->discard, a.n = p->n - 2 * p->discard;
    a.sn = p->transposed ? 1 : nModes, a.sm = p->transposed ? p->n : 1;
    a.nModes = nModes, a.M = M, a.bits = bits, a.dtype = p->dtype, a.rotate = p->rotate, a.has_tx = tx != nullptr, a.want = p->want;
    a.nb = grid_blocks(a.n, kBlock, kMaxBlocks);
    a.sqrtEs = std::sqrt(p->Es), a.H = p->H;

    // tables: raw (2M) | normalised (2M) | px (M) | log2 px (M) doubles, then M float weights
    std::vector<double> &tab = w.host_tab;
    std::vector<float> &w32 = w.host_w32;
    tab.assign(6 * (size_t)M, 0.0);
    w32.assign(M, 0.f);
    for (int m = 0; m < 2 * M; ++m) tab[m] = const_raw ? const_raw[m] : 0.0, tab[2 * M + m] = const_norm[m];
    for (int m = 0; m < M; ++m) {
        tab[4 * M + m] = px ? px[m] : 1.0 / M;
        tab[5 * M + m] = std::log2(tab[4 * M + m]);
        if (evm_w32) w32[m] = evm_w32[m];
    }
    const size_t tab_bytes = tab.size() * sizeof(double);
    if (!c.need(w.tables, tab_bytes + M * sizeof(float))) return c.rc;
    if (!c.need(w.part, (size_t)nModes * kMaxBlocks * kDecN * sizeof(double))) return c.rc;
    if (!c.need(w.scal, (size_t)kMaxModes * kScalN * sizeof(double))) return c.rc;
    if (!c.need(w.res, (size_t)kMaxModes * kResN * sizeof(double))) return c.rc;
    const size_t in_bytes = (size_t)p->n * nModes * elem_size(p->dtype);
    if (!(a.rx = c.input(rx, w.in_rx, in_bytes))) return c.rc;
    if (tx && !(a.tx = c.input(tx, w.in_tx, in_bytes))) return c.rc;
    if (!c.h2d(w.tables.p, tab.data(), tab_bytes) || !c.h2d((char *)w.tables.p + tab_bytes, w32.data(), M * sizeof(float))) return c.rc;
    a.raw = (const double *)w.tables.p, a.cn = a.raw + 2 * M, a.px = a.raw + 4 * M, a.log2px = a.raw + 5 * M;
    a.w32 = (const float *)((char *)w.tables.p + tab_bytes);
    a.part = (double *)w.part.p, a.scal = (double *)w.scal.p, a.res = (double *)w.res.p;
    if (!c.ok(hipMemsetAsync(w.res.p, 0, (size_t)kMaxModes * kResN * sizeof(double), w.st), "hipMemset")) return c.rc;

    if (blind) {
        if (!pairwise_leaves(c, w.leaves, a.n, a.nleaf, a.leaf_start)) return c.rc;
        if (!c.need(w.idx, (size_t)a.n * nModes * sizeof(int32_t))) return c.rc;
        if (!c.need(w.leaf_sum, (size_t)a.nleaf * nModes * sizeof(float))) return c.rc;
        a.idx = (int32_t *)w.idx.p, a.leaf_sum = (float *)w.leaf_sum.p;
    }

    const dim3 grid(a.nb, nModes), block(kBlock);
    k_stats<<<grid, block, 0, w.st>>>(a);
    k_stats_fin<<<1, 64, 0, w.st>>>(a);
    if (blind) {
        k_blind<<<grid, block, 2 * M * sizeof(double), w.st>>>(a);
        k_pw_leaf<<<dim3((unsigned)((a.nleaf + kBlock - 1) / kBlock), nModes), block, 0, w.st>>>(a);
        k_blind_fin<<<1, 64, 0, w.st>>>(a);
    } else {
        k_decide<<<grid, block, 2 * M * sizeof(double), w.st>>>(a);
        k_decide_fin<<<1, 64, 0, w.st>>>(a);
        if (p->want & (kWantGmi | kWantMi)) {
            k_soft<<<grid, block, 6 * M * sizeof(double), w.st>>>(a);
            k_soft_fin<<<1, 64, 0, w.st>>>(a);
        }
    }
    if (!c.launched()) return c.rc;
    std::vector<double> res((size_t)nModes * kResN);
    if (!c.deliver(res.data(), w.res.p, res.size() * sizeof(double))) return c.rc;
    if (!c.sync()) return c.rc;
    for (int k = 0; k < nModes; ++k) {
        const double *r = res.data() + (size_t)k * kResN;
        ssf_metrics_result &o = out[k];
        o.BER = r[0], o.SER = r[1], o.SNR = r[2], o.GMI = r[3], o.NGMI = r[4], o.MI = r[5], o.EVM = r[6];
        o.bit_errors = (int64_t)r[7], o.symbol_errors = (int64_t)r[8], o.n = (int64_t)r[9];
    }
    return SSF_OK;
}

// power statistics of `count` values taken as one column: scal[6] = sqrt(mean |x|^2), scal[9] = sum |x|^2
static bool flat_stats(Call &c, KArgs &a, int64_t count, int dtype, const void *x) {
    Work &w = *c.w;
    if (!c.need(w.part, (size_t)kMaxBlocks * kDecN * sizeof(double))) return false;
    if (!c.need(w.scal, (size_t)kMaxModes * kScalN * sizeof(double))) return false;
    if (!(a.rx = c.input(x, w.in_rx, (size_t)count * elem_size(dtype)))) return false;
    a.n0 = 0, a.n = count, a.sn = 1, a.sm = 0, a.nModes = 1, a.dtype = dtype, a.nb = grid_blocks(count, kBlock, kMaxBlocks);
    a.part = (double *)w.part.p, a.scal = (double *)w.scal.p;
    k_stats<<<dim3(a.nb, 1), kBlock, 0, w.st>>>(a);
    k_stats_fin<<<1, 64, 0, w.st>>>(a);
    return c.launched();
}

int metrics_pnorm(int device, int64_t count, int dtype, const void *x, void *y, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    KArgs a{};
    const size_t out_bytes = (size_t)count * ((dtype == kC128 || dtype == kC64) ? 16 : 8);
    void *yd = c.target(y, w.out, out_bytes);
    if (!yd) return c.rc;
    if (!flat_stats(c, a, count, dtype, x)) return c.rc;
    k_scale<<<a.nb, kBlock, 0, w.st>>>(a, yd);
    if (!c.launched()) return c.rc;
    if (!c.deliver(y, yd, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int metrics_power(int device, int64_t count, int64_t rows, int dtype, const void *x, double *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    KArgs a{};
    if (!flat_stats(c, a, count, dtype, x)) return c.rc;
    double total = 0.0;
    if (!c.deliver(&total, a.scal + 9, sizeof(double))) return c.rc;
    if (!c.sync()) return c.rc;
    *out = total / (double)rows;                                            // sum over the columns of mean |x|^2
    return SSF_OK;
}

int metrics_demod(int device, int64_t count, int dtype, int M, const double *const_raw, const void *symb, int32_t *bits_out,
                  std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    KArgs a{};
    int bits = 0;
    while ((1 << bits) < M) ++bits;
    const size_t out_bytes = (size_t)count * bits * sizeof(int32_t);
    if (!c.upload(w.tables, const_raw, 2 * (size_t)M * sizeof(double))) return c.rc;
    int32_t *od = (int32_t *)c.target(bits_out, w.out, out_bytes);
    if (!od) return c.rc;
    if (!(a.rx = c.input(symb, w.in_rx, (size_t)count * elem_size(dtype)))) return c.rc;
    a.n = count, a.M = M, a.bits = bits, a.dtype = dtype, a.raw = (const double *)w.tables.p;
    k_demod<<<grid_blocks(count, kBlock, kMaxBlocks), kBlock, 2 * M * sizeof(double), w.st>>>(a, od);
    if (!c.launched()) return c.rc;
    if (!c.deliver(bits_out, od, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
