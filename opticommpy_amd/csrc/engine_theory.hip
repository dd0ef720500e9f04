// engine_theory.hip -- mutual information on the device: the quadrature of theoryMI (ssf_theory_mi) and the Monte-Carlo calcMI
// (ssf_calc_mi) of include/ssf.h.  k_theory_mi: one workgroup per (node tile, point i, SNR), one lane per node; the point's row
// (three doubles per j) sits in LDS and every lane reads it at the same address (a broadcast).  Each workgroup stores its partial
// sums; k_theory_fin adds the tiles, then the points, in a fixed order.  No floating-point atomics: results repeat bit for bit.
// The host waits for its results once, at the end of a call (and at its start for whatever an earlier, failed call left on the stream).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "block_reduce.h"
#include "engine_host.h"
#include "theory_kernels.h"

namespace ssf {
namespace {
using namespace tk;
using namespace eng;

constexpr int kBlock = br::kBlock, kMaxBlocks = 512;
static_assert(kBlock == kTile, "one node per lane");
constexpr int kRowsPerLaunch = 16384;          // (point, SNR) pairs per launch: bounds the partial sums (17 MiB) and a launch's run time

struct TArgs {
    const double *tab, *px, *sigma;            // device: M (re, im) pairs, M probabilities, nS deviations
    double *part, *res;                        // [SNR of the launch][point][tile][2]; res[nS]
    int M;
};

__global__ __launch_bounds__(kBlock) void k_theory_mi(TArgs a, int s0) {
    extern __shared__ double row[];
    const int i = blockIdx.y;
    const double sigma = a.sigma[s0 + blockIdx.z];
    for (int j = threadIdx.x; j < a.M; j += kBlock) row_entry(a.tab, a.px, i, j, sigma, row + kRow * j);
    __syncthreads();
    double acc[2] = {0.0, 0.0};
    const int q = blockIdx.x * kTile + threadIdx.x;
    if (q < kNodes) node_body(acc, row, a.M, q);
    br::block_sum_store<2>(acc, a.part + (((long long)blockIdx.z * a.M + i) * kTiles + blockIdx.x) * 2);
}

// one workgroup per SNR of the launch: lane-strided over the points, then the workgroup's tree
__global__ __launch_bounds__(kBlock) void k_theory_fin(TArgs a, int s0) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.M; i += kBlock) acc += point_term(a.part + ((long long)blockIdx.x * a.M + i) * kTiles * 2, a.px[i]);
    br::block_sum_store(acc, a.res + s0 + blockIdx.x);
}

struct CArgs {
    const void *rx, *tx;
    const double *tab, *px, *log2px;
    double *part, *res;
    long long n;
    int M, dtype, nb;
    double ninv, H;
};

__global__ __launch_bounds__(kBlock) void k_calc_mi(CArgs a) {
    extern __shared__ double lds[];
    double *tab = lds, *px = lds + 2 * a.M, *l2 = lds + 3 * a.M;
    for (int m = threadIdx.x; m < a.M; m += kBlock) tab[2 * m] = a.tab[2 * m], tab[2 * m + 1] = a.tab[2 * m + 1], px[m] = a.px[m], l2[m] = a.log2px[m];
    __syncthreads();
    double acc[1] = {0.0};
    for (long long k = (long long)blockIdx.x * kBlock + threadIdx.x; k < a.n; k += (long long)gridDim.x * kBlock) {
        double rr, ri, tr, ti;
        mk::load(a.dtype, a.rx, k, rr, ri);
        mk::load(a.dtype, a.tx, k, tr, ti);
        calc_body(acc, tab, px, l2, a.M, a.ninv, rr, ri, tr, ti);
    }
    br::block_sum_store<1>(acc, a.part + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_calc_fin(CArgs a) {
    const double tot = br::wave_sum_partials(a.part, a.nb, 1);
    if (threadIdx.x == 0) a.res[0] = calc_combine(tot, a.n, a.H);
}

struct Work : WorkBase {
    Buf tables, part, res, in_rx, in_tx;
    std::vector<double> host_tab;              // kept for its capacity
};
using Call = CallT<Work>;

}  // namespace

int theory_mi(int device, int M, int nS, const double *const_tab, const double *px, const double *sigma, double *mi_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    std::vector<double> &tab = w.host_tab;
    tab.assign(const_tab, const_tab + 2 * (size_t)M);
    tab.insert(tab.end(), px, px + M);
    tab.insert(tab.end(), sigma, sigma + nS);
    const int chunk = std::max(1, std::min(nS, kRowsPerLaunch / M));
    if (!c.upload(w.tables, tab)) return c.rc;
    if (!c.need(w.part, (size_t)chunk * M * kTiles * 2 * sizeof(double))) return c.rc;
    if (!c.need(w.res, (size_t)nS * sizeof(double))) return c.rc;
    TArgs a{};
    a.tab = (const double *)w.tables.p, a.px = a.tab + 2 * M, a.sigma = a.px + M;
    a.part = (double *)w.part.p, a.res = (double *)w.res.p, a.M = M;
    for (int s0 = 0; s0 < nS; s0 += chunk) {   // launches on one stream: the partial sums are reused in order
        const int ns = std::min(chunk, nS - s0);
        k_theory_mi<<<dim3(kTiles, M, ns), kBlock, (size_t)kRow * M * sizeof(double), w.st>>>(a, s0);
        k_theory_fin<<<ns, kBlock, 0, w.st>>>(a, s0);
    }
    if (!c.launched()) return c.rc;
    std::vector<double> res(nS);
    if (!c.deliver(res.data(), w.res.p, res.size() * sizeof(double))) return c.rc;
    if (!c.sync()) return c.rc;
    const double H = entropy(px, M);
    for (int s = 0; s < nS; ++s) mi_out[s] = H - res[s];
    return SSF_OK;
}

int theory_calc_mi(int device, int64_t n, int dtype, int M, double sigma2, const double *const_tab, const double *px, const void *rx,
                   const void *tx, double *mi_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    std::vector<double> &tab = w.host_tab;     // table (2M) | px (M) | log2 px (M)
    tab.assign(const_tab, const_tab + 2 * (size_t)M);
    tab.insert(tab.end(), px, px + M);
    for (int m = 0; m < M; ++m) tab.push_back(std::log2(px[m]));
    CArgs a{};
    a.n = n, a.M = M, a.dtype = dtype, a.nb = grid_blocks(n, kBlock, kMaxBlocks);
    a.ninv = -(1.0 / sigma2), a.H = entropy(px, M);
    if (!c.upload(w.tables, tab)) return c.rc;
    if (!c.need(w.part, (size_t)kMaxBlocks * sizeof(double))) return c.rc;
    if (!c.need(w.res, sizeof(double))) return c.rc;
    const size_t in_bytes = (size_t)n * mk::elem_size(dtype);
    if (!(a.rx = c.input(rx, w.in_rx, in_bytes))) return c.rc;
    if (!(a.tx = c.input(tx, w.in_tx, in_bytes))) return c.rc;
    a.tab = (const double *)w.tables.p, a.px = a.tab + 2 * M, a.log2px = a.tab + 3 * M;
    a.part = (double *)w.part.p, a.res = (double *)w.res.p;
    k_calc_mi<<<a.nb, kBlock, 4 * (size_t)M * sizeof(double), w.st>>>(a);
    k_calc_fin<<<1, 64, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    if (!c.deliver(mi_out, w.res.p, sizeof(double))) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
