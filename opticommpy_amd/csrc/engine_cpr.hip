// engine_cpr.hip -- carrier phase recovery on the device (ssf_cpr, ssf_bps, ssf_foe of include/ssf.h).
//   search   a workgroup owns 256 output symbols plus a halo of 2 Nh; it walks the test phases in chunks, writes each chunk's
//            minimum distances to LDS (they never reach HBM), turns every row into prefix sums in a fixed order, takes the window
//            of every symbol as the difference of two of them and keeps the running (minimum, index) of its symbol in registers
//   unwrap   np.unwrap(4 phi) / 4 as a fixed-order block scan: per-block scan, scan of the block sums, apply
//   apply    x e^{j phi}, then the joint norm over all modes (one partial per workgroup, partials summed in a fixed order)
//   FOE      x ** P -> rocFFT (plans cached per device, length and mode count) -> first maximum in fftshift order -> derotation
// No floating-point atomics anywhere: results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "block_reduce.h"
#include "cpr_kernels.h"
#include "engine_host.h"

namespace ssf {
namespace {
using namespace ck;
using namespace eng;

constexpr int kBlock = br::kBlock, kWaves = br::kWaves, kMaxBlocks = 1024;
constexpr int kSegs = 16;                     // segments a row of minimum distances is cut into for its prefix sums
constexpr int kMaxChunk = kBlock / kSegs;     // test phases per LDS chunk: one lane per row and segment
constexpr size_t kLdsBudget = 60 * 1024;      // dynamic LDS of the search per workgroup (64 KiB with the static part: no opt-in needed)

struct BpsArgs {
    const void *x;
    int dtype, nModes, Nh, B, M, Bc, W, sep, nr, ni, ntab;
    long long n;
    const double *tab, *rot, *testph, *lre, *lim;
    double *phase;                            // (n, nModes): the raw test phase of every symbol
};

__global__ __launch_bounds__(kBlock) void k_bps(BpsArgs a) {
    extern __shared__ double lds[];
    __shared__ double segtot[kBlock];
    double *tab = lds, *d = lds + a.ntab;
    const int mode = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * kTile;
    if (a.sep) {
        for (int i = tid; i < a.nr; i += kBlock) tab[i] = a.lre[i];
        for (int i = tid; i < a.ni; i += kBlock) tab[a.nr + i] = a.lim[i];
    } else {
        for (int i = tid; i < 2 * a.M; i += kBlock) tab[i] = a.tab[i];
    }
    double best = INFINITY;
    int bi = 0;
    const long long k = t0 + tid;
    // the prefix sums of a chunk: lane -> (row of the chunk, one of kSegs segments of that row)
    const int row = tid / kSegs, seg = tid - row * kSegs, seglen = (a.W + kSegs - 1) / kSegs;
    const int j0 = seg * seglen, j1 = j0 + seglen < a.W ? j0 + seglen : a.W;
    for (int b0 = 0; b0 < a.B; b0 += a.Bc) {
        const int nb = a.B - b0 < a.Bc ? a.B - b0 : a.Bc;
        __syncthreads();                      // tables loaded; the previous chunk's sums are done
        for (int j = tid; j < a.W; j += kBlock) {
            const long long g = t0 - a.Nh + j;
            double xr = 0.0, xi = 0.0;        // the reference pads with zeros on both sides
            if (g >= 0 && g < a.n) load(a.dtype, a.x, g * a.nModes + mode, xr, xi);
            for (int bl = 0; bl < nb; ++bl) {
                const double c = a.rot[2 * (b0 + bl)], s = a.rot[2 * (b0 + bl) + 1];
                d[bl * a.W + j] = a.sep ? dmin_sep(tab, a.nr, tab + a.nr, a.ni, xr, xi, c, s) : dmin_full(tab, a.M, xr, xi, c, s);
            }
        }
        __syncthreads();
        // every row of the chunk -> its inclusive prefix sums, in place: segments in order, then the segments before them
        double *r = d + row * a.W;
        double run = 0.0;
        if (row < nb)
            for (int j = j0; j < j1; ++j) run += r[j], r[j] = run;
        segtot[tid] = run;
        __syncthreads();
        if (row < nb && seg) {
            double off = 0.0;
            for (int q = 0; q < seg; ++q) off += segtot[row * kSegs + q];
            for (int j = j0; j < j1; ++j) r[j] = off + r[j];
        }
        __syncthreads();
        if (k < a.n) {
            for (int bl = 0; bl < nb; ++bl) {
                const double sum = window_from_prefix(d + bl * a.W, tid, a.Nh);
                if (sum < best) best = sum, bi = b0 + bl;       // strict: the lowest index wins a tie
            }
        }
    }
    if (k < a.n) a.phase[k * a.nModes + mode] = a.testph[bi];
}

// ---- unwrap
struct UnwrapArgs {
    long long n, nblk;
    int nModes;
    const double *phi;                        // (n, nModes) raw
    double *loc, *bsum;                       // (nModes, n) scan inside a block; (nModes, nblk) block sums -> offsets
};

// inclusive scan of one value per lane over the workgroup, fixed order; returns the exclusive prefix, sh[kBlock - 1] = total
__device__ double block_scan(double v, double *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const double x = t >= o ? sh[t - o] : 0.0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    return t ? sh[t - 1] : 0.0;
}

__global__ __launch_bounds__(kBlock) void k_unwrap_local(UnwrapArgs a) {
    __shared__ double sh[kBlock];
    const int m = blockIdx.y, t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * kScanBlock + (long long)t * kScanPer;
    double v[kScanPer], run = 0.0;
#pragma unroll
    for (int e = 0; e < kScanPer; ++e) {
        const long long k = k0 + e;
        if (k >= 1 && k < a.n) run += unwrap_corr(4.0 * a.phi[(k - 1) * a.nModes + m], 4.0 * a.phi[k * a.nModes + m]);
        v[e] = run;
    }
    const double excl = block_scan(run, sh);
#pragma unroll
    for (int e = 0; e < kScanPer; ++e)
        if (k0 + e < a.n) a.loc[(long long)m * a.n + k0 + e] = excl + v[e];
    if (t == kBlock - 1) a.bsum[(long long)m * a.nblk + blockIdx.x] = sh[kBlock - 1];
}

// block sums of one mode -> exclusive offsets, in place
__global__ __launch_bounds__(kBlock) void k_unwrap_offsets(UnwrapArgs a) {
    __shared__ double sh[kBlock];
    const int m = blockIdx.x, t = threadIdx.x;
    double *b = a.bsum + (long long)m * a.nblk;
    const long long span = (a.nblk + kBlock - 1) / kBlock, j0 = t * span;
    double run = 0.0;
    for (long long j = j0; j < j0 + span && j < a.nblk; ++j) run += b[j];
    run = block_scan(run, sh);
    for (long long j = j0; j < j0 + span && j < a.nblk; ++j) {
        const double v = b[j];
        b[j] = run;
        run += v;
    }
}

struct ApplyArgs {
    const void *x;
    int dtype, nModes;
    long long n, nblk;
    const double *phi, *loc, *boff;
    double *phase_out;                        // (n, nModes) unwrapped
    Cplx *y;
    double *part;
};

// phase = (4 phi + cumulative correction) / 4;  y = x e^{j phase};  partial sums of |y|^2
__global__ __launch_bounds__(kBlock) void k_apply(ApplyArgs a) {
    const long long total = a.n * a.nModes;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const long long k = i / a.nModes;
        const int m = (int)(i - k * a.nModes);
        const double cum = a.boff[(long long)m * a.nblk + k / kScanBlock] + a.loc[(long long)m * a.n + k];
        const double ph = (4.0 * a.phi[i] + cum) / 4.0;
        a.phase_out[i] = ph;
        double xr, xi, s, c;
        load(a.dtype, a.x, i, xr, xi);
        sincos_d(ph, s, c);
        Cplx y;
        rotate(xr, xi, c, s, y.re, y.im);
        a.y[i] = y;
        acc += y.re * y.re + y.im * y.im;
    }
    br::block_sum_store(acc, a.part + blockIdx.x);
}

// scal[0] = sqrt(mean |y|^2) over all `count` values, from the nb partial sums: one wave
__global__ __launch_bounds__(64) void k_norm_fin(const double *part, int nb, long long count, double *scal) {
    const double s = br::wave_sum_partials(part, nb, 1);
    if (threadIdx.x == 0) scal[0] = sqrt(s / (double)count);
}

__global__ __launch_bounds__(kBlock) void k_scale(Cplx *y, long long count, const double *scal) {
    const double s = scal[0];
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < count; i += (long long)gridDim.x * kBlock) {
        Cplx v = y[i];
        v.re = v.re / s, v.im = v.im / s;
        y[i] = v;
    }
}

// ---- frequency offset estimation
struct FoeArgs {
    const void *x;
    int dtype, nModes, P, nb;
    long long n;
    double Fs;
    Cplx *f;                                  // (nModes, n): x ** P, then its transform
    double *cand_m;                           // (nModes, nb) candidates of the maximum search
    long long *cand_i, *peak;                 // ... and peak[nModes]: position of the maximum in fftshift order
    const double *slope;                      // nModes
    Cplx *y;
    double *part;
};

__global__ __launch_bounds__(kBlock) void k_foe_pow(FoeArgs a) {
    const long long total = a.n * a.nModes;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const long long k = i / a.nModes;
        const int m = (int)(i - k * a.nModes);
        double xr, xi;
        load(a.dtype, a.x, i, xr, xi);
        Cplx v;
        cpow_int(xr, xi, a.P, v.re, v.im);
        a.f[(long long)m * a.n + k] = v;
    }
}

__device__ void block_argmax(double &mag, long long &pos) {
    __shared__ double shm[kWaves];
    __shared__ long long shi[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_down(mag, o, 64);
        const long long i2 = __shfl_down(pos, o, 64);
        argmax_merge(mag, pos, m2, i2);
    }
    if (lane == 0) shm[wave] = mag, shi[wave] = pos;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kWaves; ++w) argmax_merge(mag, pos, shm[w], shi[w]);
}

__global__ __launch_bounds__(kBlock) void k_foe_argmax(FoeArgs a) {
    const int m = blockIdx.y;
    double mag = -1.0;
    long long pos = a.n;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        const Cplx v = a.f[(long long)m * a.n + shifted_bin(i, a.n)];
        argmax_merge(mag, pos, v.re * v.re + v.im * v.im, i);
    }
    block_argmax(mag, pos);
    if (threadIdx.x == 0) a.cand_m[m * a.nb + blockIdx.x] = mag, a.cand_i[m * a.nb + blockIdx.x] = pos;
}

__global__ __launch_bounds__(kBlock) void k_foe_argmax_fin(FoeArgs a) {
    const int m = blockIdx.x;
    double mag = -1.0;
    long long pos = a.n;
    for (int b = threadIdx.x; b < a.nb; b += kBlock) argmax_merge(mag, pos, a.cand_m[m * a.nb + b], a.cand_i[m * a.nb + b]);
    block_argmax(mag, pos);
    if (threadIdx.x == 0) a.peak[m] = pos;
}

__global__ __launch_bounds__(kBlock) void k_foe_derotate(FoeArgs a) {
    const long long total = a.n * a.nModes;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const long long k = i / a.nModes;
        const int m = (int)(i - k * a.nModes);
        double xr, xi;
        load(a.dtype, a.x, i, xr, xi);
        Cplx y;
        derotate(xr, xi, a.slope[m], k, a.Fs, y.re, y.im);
        a.y[i] = y;
        acc += y.re * y.re + y.im * y.im;
    }
    br::block_sum_store(acc, a.part + blockIdx.x);
}

// ---- host side
struct Work : WorkBase {
    Buf tables, in, xw, f, phi, phase, loc, bsum, part, scal, cand_m, cand_i, peak, slope, out;
    FftPlans plans;
    std::vector<double> host_tab, host_slope;     // kept for their capacity
};
using Call = CallT<Work>;

// the table as the product of its real and imaginary levels, if it is one (square QAM): 2 sqrt(M) comparisons per distance
bool separable(const double *tab, int M, std::vector<double> &lre, std::vector<double> &lim) {
    lre.clear(), lim.clear();
    auto add = [](std::vector<double> &v, double x) {
        for (double y : v)
            if (y == x) return;
        v.push_back(x);
    };
    for (int m = 0; m < M; ++m) {
        add(lre, tab[2 * m]), add(lim, tab[2 * m + 1]);
        if (lre.size() * lim.size() > (size_t)M) return false;
    }
    if (lre.size() * lim.size() != (size_t)M) return false;
    for (int m = 0; m < M; ++m)                                  // M distinct points on an M-point grid fill it
        for (int q = 0; q < m; ++q)
            if (tab[2 * m] == tab[2 * q] && tab[2 * m + 1] == tab[2 * q + 1]) return false;
    return true;
}

// tables of the search to the device and the launch; x: device, (n, nModes) of `dtype`; phase: device (n, nModes)
bool run_bps(Call &c, const void *x, int dtype, long long n, int nModes, int Nh, int B, int M, const double *table, double *phase) {
    Work &w = *c.w;
    std::vector<double> lre, lim;
    const bool sep = separable(table, M, lre, lim);
    std::vector<double> &host = w.host_tab;
    host.assign(2 * (size_t)M + 3 * (size_t)B, 0.0);
    for (int m = 0; m < 2 * M; ++m) host[m] = table[m];
    double *rot = host.data() + 2 * M, *testph = rot + 2 * B;
    for (int b = 0; b < B; ++b) {
        testph[b] = (double)b * (kPiD / 2.0) / (double)B;         // np.arange(0, B) * (np.pi / 2) / B
        rot[2 * b] = std::cos(testph[b]), rot[2 * b + 1] = std::sin(testph[b]);
    }
    if (sep) host.insert(host.end(), lre.begin(), lre.end()), host.insert(host.end(), lim.begin(), lim.end());
    if (!c.upload(w.tables, host)) return false;
    BpsArgs a{};
    a.x = x, a.dtype = dtype, a.nModes = nModes, a.Nh = Nh, a.B = B, a.M = M, a.n = n;
    a.W = kTile + 2 * Nh;
    a.sep = sep, a.nr = sep ? (int)lre.size() : 0, a.ni = sep ? (int)lim.size() : 0;
    a.ntab = sep ? a.nr + a.ni : 2 * M;
    const size_t per_phase = (size_t)a.W * sizeof(double), room = kLdsBudget - (size_t)a.ntab * sizeof(double);
    a.Bc = (int)(room / per_phase);
    if (a.Bc > kMaxChunk) a.Bc = kMaxChunk;
    if (a.Bc > B) a.Bc = B;
    a.tab = (const double *)w.tables.p, a.rot = a.tab + 2 * M, a.testph = a.rot + 2 * B;
    a.lre = a.testph + B, a.lim = a.lre + a.nr;
    a.phase = phase;
    const size_t lds = (size_t)a.ntab * sizeof(double) + (size_t)a.Bc * per_phase;
    k_bps<<<dim3((unsigned)((n + kTile - 1) / kTile), nModes), kBlock, lds, w.st>>>(a);
    return c.launched();
}

// x (device) -> y = x exp(-j 2 pi fo k / Fs) (device, may not alias x), fo[nModes] to the host; partial sums of |y|^2 in w.part
bool run_foe(Call &c, const void *x, int dtype, long long n, int nModes, int P, double Fs, Cplx *y, double *fo, int *nb_out) {
    Work &w = *c.w;
    FoeArgs a{};
    a.x = x, a.dtype = dtype, a.nModes = nModes, a.P = P, a.n = n, a.Fs = Fs;
    a.nb = grid_blocks(n, kBlock, kMaxBlocks);
    const int nbf = grid_blocks(n * nModes, kBlock, kMaxBlocks);
    if (!c.need(w.f, (size_t)n * nModes * sizeof(Cplx))) return false;
    if (!c.need(w.cand_m, (size_t)nModes * a.nb * sizeof(double)) || !c.need(w.cand_i, (size_t)nModes * a.nb * sizeof(long long))) return false;
    if (!c.need(w.peak, nModes * sizeof(long long)) || !c.need(w.slope, nModes * sizeof(double))) return false;
    if (!c.need(w.part, kMaxBlocks * sizeof(double))) return false;
    a.f = (Cplx *)w.f.p, a.cand_m = (double *)w.cand_m.p, a.cand_i = (long long *)w.cand_i.p, a.peak = (long long *)w.peak.p;
    a.slope = (const double *)w.slope.p, a.y = y, a.part = (double *)w.part.p;
    k_foe_pow<<<nbf, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return false;
    if (!transform(c, w.f.p, n, nModes, false)) return false;
    k_foe_argmax<<<dim3(a.nb, nModes), kBlock, 0, w.st>>>(a);
    k_foe_argmax_fin<<<nModes, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return false;
    std::vector<long long> peak(nModes);
    std::vector<double> &slope = w.host_slope;
    slope.assign(nModes, 0.0);
    if (!c.deliver(peak.data(), w.peak.p, nModes * sizeof(long long)) || !c.sync()) return false;
    for (int m = 0; m < nModes; ++m) {
        if (peak[m] < 0 || peak[m] >= n) return c.reject(SSF_ERR_BAD_ARG, "no spectral maximum (the input is not finite)");
        fo[m] = foe_frequency(peak[m], n, Fs, P);
        slope[m] = foe_slope(fo[m]);
    }
    if (!c.h2d(w.slope.p, slope.data(), nModes * sizeof(double))) return false;
    k_foe_derotate<<<nbf, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return false;
    *nb_out = nbf;
    return true;
}

// y /= sqrt(mean |y|^2) from the nb partial sums in w.part
bool run_norm(Call &c, Cplx *y, long long count, int nb) {
    Work &w = *c.w;
    if (!c.need(w.scal, sizeof(double))) return false;
    k_norm_fin<<<1, 64, 0, w.st>>>((const double *)w.part.p, nb, count, (double *)w.scal.p);
    k_scale<<<grid_blocks(count, kBlock, kMaxBlocks), kBlock, 0, w.st>>>(y, count, (const double *)w.scal.p);
    return c.launched();
}

}  // namespace

int cpr_bps(int device, int64_t n, int nModes, int dtype, int Nh, int B, int M, const double *table, const void *x, double *phase_out,
            std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t ph_bytes = (size_t)n * nModes * sizeof(double);
    double *phase = (double *)c.target(phase_out, w.phase, ph_bytes);
    if (!phase) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)n * nModes * mk::elem_size(dtype));
    if (!xd) return c.rc;
    if (!run_bps(c, xd, dtype, n, nModes, Nh, B, M, table, phase)) return c.rc;
    if (!c.deliver(phase_out, phase, ph_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int cpr_foe(int device, int64_t n, int nModes, int dtype, int P, double Fs, const void *x, void *sig_out, double *fo_out,
            std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const size_t out_bytes = (size_t)n * nModes * sizeof(Cplx);
    Cplx *y = (Cplx *)c.target(sig_out, w.out, out_bytes);
    if (!y) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)n * nModes * mk::elem_size(dtype));
    if (!xd) return c.rc;
    int nb = 0;
    if (!run_foe(c, xd, dtype, n, nModes, P, Fs, y, fo_out, &nb)) return c.rc;
    if (!c.deliver(sig_out, y, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int cpr_run(int device, const ssf_cpr_params *p, const double *table, const void *x, void *sig_out, double *phase_out, double *fo_out,
            std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long n = p->n, count = n * p->nModes;
    const int nModes = p->nModes;
    const size_t out_bytes = (size_t)count * sizeof(Cplx), ph_bytes = (size_t)count * sizeof(double);
    UnwrapArgs u{};
    u.n = n, u.nModes = nModes, u.nblk = (n + kScanBlock - 1) / kScanBlock;
    Cplx *y = (Cplx *)c.target(sig_out, w.out, out_bytes);
    double *phase = (double *)c.target(phase_out, w.phase, ph_bytes);
    if (!y || !phase) return c.rc;
    if (!c.need(w.phi, ph_bytes) || !c.need(w.loc, ph_bytes) || !c.need(w.bsum, (size_t)nModes * u.nblk * sizeof(double))) return c.rc;
    if (!c.need(w.part, kMaxBlocks * sizeof(double))) return c.rc;
    if (p->runFOE && !c.need(w.xw, out_bytes)) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)count * mk::elem_size(p->dtype));
    if (!xd) return c.rc;
    int dtype = p->dtype;
    if (p->runFOE) {
        std::vector<double> fo(nModes);
        int nb = 0;
        if (!run_foe(c, xd, dtype, n, nModes, p->P, p->Fs, (Cplx *)w.xw.p, fo.data(), &nb)) return c.rc;
        if (!run_norm(c, (Cplx *)w.xw.p, count, nb)) return c.rc;
        if (fo_out)
            for (int m = 0; m < nModes; ++m) fo_out[m] = fo[m];
        xd = w.xw.p, dtype = mk::kC128;
    }
    if (!run_bps(c, xd, dtype, n, nModes, p->Nh, p->B, p->M, table, (double *)w.phi.p)) return c.rc;
    u.phi = (const double *)w.phi.p, u.loc = (double *)w.loc.p, u.bsum = (double *)w.bsum.p;
    k_unwrap_local<<<dim3((unsigned)u.nblk, nModes), kBlock, 0, w.st>>>(u);
    k_unwrap_offsets<<<nModes, kBlock, 0, w.st>>>(u);
    ApplyArgs a{};
    a.x = xd, a.dtype = dtype, a.nModes = nModes, a.n = n, a.nblk = u.nblk;
    a.phi = u.phi, a.loc = u.loc, a.boff = u.bsum, a.phase_out = phase, a.y = y, a.part = (double *)w.part.p;
    const int nb = grid_blocks(count, kBlock, kMaxBlocks);
    k_apply<<<nb, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    if (!run_norm(c, y, count, nb)) return c.rc;
    if (!c.deliver(sig_out, y, out_bytes)) return c.rc;
    if (phase_out && !c.deliver(phase_out, phase, ph_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
