// engine_array.hip -- the general array layer of DeviceArray on the device (ssf_array_copy, ssf_array_take, ssf_array_transpose,
// ssf_array_binary, ssf_array_unary, ssf_array_fill, ssf_array_reduce, ssf_freq_shift of include/ssf.h).
//   movement       a strided copy walks the elements in the destination's C order, one element per lane, 64-bit offsets on both
//                  sides; where both sides are contiguous and 16-byte aligned the bytes move 16 per lane.  take gathers whole rows.
//                  The transpose goes through a padded LDS tile: the global reads and the global writes both run along a row.
//   element-wise   a lane takes as many consecutive elements as fill 16 bytes of the result (4 float32, 2 float64 / complex64,
//                  1 complex128); every array is a whole allocation, so the packs are aligned.  A row or column operand and the
//                  last, partial pack go element by element.
//   reductions     per column up to kRedBlocks workgroups, each lane four running doubles over a grid-stride walk, the workgroup's
//                  partial by block_reduce.h, then ONE lane adds the partials in index order.  No atomics: a result repeats bit for
//                  bit, and the cap kRedBlocks belongs to it.
// Every entry point synchronises its stream before it returns: a result may be handed to any other engine's stream.
#include <hip/hip_runtime.h>

#include <vector>

#include "array_kernels.h"
#include "block_reduce.h"
#include "engine_host.h"

namespace ssf {
namespace {
using namespace ak;
using namespace eng;

static_assert(kBlock == br::kBlock, "the reductions are written for block_reduce.h's workgroup");

struct alignas(16) B16 {
    unsigned long long a, b;
};
template <int S> struct ItemOf;
template <> struct ItemOf<1> { using type = unsigned char; };
template <> struct ItemOf<2> { using type = unsigned short; };
template <> struct ItemOf<4> { using type = unsigned int; };
template <> struct ItemOf<8> { using type = unsigned long long; };
template <> struct ItemOf<16> { using type = B16; };

#define GRID_STRIDE(q, count) \
    for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < (count); q += (long long)gridDim.x * kBlock)

// ---- movement
template <typename T> __global__ __launch_bounds__(kBlock) void k_strided_copy(Desc sd, Desc dd, long long count, const T *src, T *dst) {
    GRID_STRIDE(q, count) dst[strided_offset(dd, q)] = src[strided_offset(sd, q)];
}
// `vecs` packs of 16 bytes, then `tail` single bytes
__global__ __launch_bounds__(kBlock) void k_flat_copy(long long vecs, int tail, const B16 *src, B16 *dst) {
    GRID_STRIDE(q, vecs) dst[q] = src[q];
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) ((unsigned char *)(dst + vecs))[threadIdx.x] = ((const unsigned char *)(src + vecs))[threadIdx.x];
}
template <typename T, typename I>
__global__ __launch_bounds__(kBlock) void k_take(long long n_src, long long n_idx, long long inner, const I *idx, const T *src, T *dst) {
    GRID_STRIDE(q, n_idx * inner) {
        const long long i = q / inner, j = q - i * inner;
        dst[q] = src[take_row((long long)idx[i], n_src) * inner + j];
    }
}
// dst (cols, rows) = src (rows, cols)^T; workgroup (bx, by) of 32 x 8 lanes moves the tile at (by kTile, bx kTile)
template <typename T> __global__ __launch_bounds__(kBlock) void k_transpose(long long rows, long long cols, long long tiles_x, const T *src, T *dst) {
    __shared__ T tile[kTile][kTile + 1];
    const long long by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    for (int r = ty; r < kTile; r += kBlock / kTile) {
        const long long row = by * kTile + r, col = bx * kTile + tx;
        if (row < rows && col < cols) tile[r][tx] = src[row * cols + col];
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += kBlock / kTile) {
        const long long orow = bx * kTile + r, ocol = by * kTile + tx;            // of dst: orow < cols, ocol < rows
        if (orow < cols && ocol < rows) dst[orow * rows + ocol] = tile[tx][r];
    }
}
template <typename T> __global__ __launch_bounds__(kBlock) void k_fill(long long count, T value, T *dst) {
    GRID_STRIDE(q, count) dst[q] = value;
}

// ---- element-wise: V consecutive elements of one array, as one aligned pack where the dtype allows
template <typename T, int V> struct alignas(sizeof(T) * V > 16 ? 16 : sizeof(T) * V) Pack {
    T v[V];
};
template <int V> __device__ __forceinline__ void load_pack(int dtype, const void *p, long long q0, C2 (&out)[V]) {
    switch (dtype) {
    case mk::kC128: {
        const auto pk = *(const Pack<mk::Cplx, V> *)((const mk::Cplx *)p + q0);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = C2{pk.v[e].re, pk.v[e].im};
        break;
    }
    case mk::kC64: {
        const auto pk = *(const Pack<mk::CplxF, V> *)((const mk::CplxF *)p + q0);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = C2{(double)pk.v[e].re, (double)pk.v[e].im};
        break;
    }
    case mk::kF64: {
        const auto pk = *(const Pack<double, V> *)((const double *)p + q0);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = C2{pk.v[e], 0.0};
        break;
    }
    default: {
        const auto pk = *(const Pack<float, V> *)((const float *)p + q0);
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = C2{(double)pk.v[e], 0.0};
        break;
    }
    }
}
template <int V> __device__ __forceinline__ void store_pack(int dtype, void *p, long long q0, const C2 (&in)[V]) {
    switch (dtype) {
    case mk::kC128: {
        Pack<mk::Cplx, V> pk;
#pragma unroll
        for (int e = 0; e < V; ++e) pk.v[e] = mk::Cplx{in[e].re, in[e].im};
        *(Pack<mk::Cplx, V> *)((mk::Cplx *)p + q0) = pk;
        break;
    }
    case mk::kC64: {
        Pack<mk::CplxF, V> pk;
#pragma unroll
        for (int e = 0; e < V; ++e) pk.v[e] = mk::CplxF{(float)in[e].re, (float)in[e].im};
        *(Pack<mk::CplxF, V> *)((mk::CplxF *)p + q0) = pk;
        break;
    }
    case mk::kF64: {
        Pack<double, V> pk;
#pragma unroll
        for (int e = 0; e < V; ++e) pk.v[e] = in[e].re;
        *(Pack<double, V> *)((double *)p + q0) = pk;
        break;
    }
    default: {
        Pack<float, V> pk;
#pragma unroll
        for (int e = 0; e < V; ++e) pk.v[e] = (float)in[e].re;
        *(Pack<float, V> *)((float *)p + q0) = pk;
        break;
    }
    }
}

struct BinArgs {
    int op, swap, a_dtype, b_dtype, out_dtype;
    long long count;
    Bcast bc;
    const void *a, *b;
    void *out;
};
__device__ __forceinline__ C2 bin_element(const BinArgs &g, C2 a, C2 b) {
    return g.swap ? binary(g.op, b, a, is_complex(g.out_dtype)) : binary(g.op, a, b, is_complex(g.out_dtype));
}
template <int V> __global__ __launch_bounds__(kBlock) void k_binary(BinArgs g) {
    const long long packs = (g.count + V - 1) / V;
    GRID_STRIDE(pq, packs) {
        const long long q0 = pq * V;
        if (q0 + V <= g.count) {
            C2 a[V], b[V], o[V];
            load_pack<V>(g.a_dtype, g.a, q0, a);
            if (g.bc.kind == kSame) load_pack<V>(g.b_dtype, g.b, q0, b);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (g.bc.kind == kScalar) b[e] = g.bc.scalar;
                else if (g.bc.kind != kSame) b[e] = load(g.b_dtype, g.b, bcast_index(g.bc, q0 + e));
                o[e] = bin_element(g, a[e], b[e]);
            }
            store_pack<V>(g.out_dtype, g.out, q0, o);
        } else {
            for (long long q = q0; q < g.count; ++q) {
                const C2 b = g.bc.kind == kScalar ? g.bc.scalar : load(g.b_dtype, g.b, bcast_index(g.bc, q));
                store(g.out_dtype, g.out, q, bin_element(g, load(g.a_dtype, g.a, q), b));
            }
        }
    }
}
template <int V> __global__ __launch_bounds__(kBlock) void k_unary(int op, int in_dtype, int out_dtype, long long count, const void *x, void *out) {
    const long long packs = (count + V - 1) / V;
    const bool cplx = is_complex(in_dtype);
    GRID_STRIDE(pq, packs) {
        const long long q0 = pq * V;
        if (q0 + V <= count) {
            C2 a[V];
            load_pack<V>(in_dtype, x, q0, a);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = unary(op, a[e], cplx);
            store_pack<V>(out_dtype, out, q0, a);
        } else {
            for (long long q = q0; q < count; ++q) store(out_dtype, out, q, unary(op, load(in_dtype, x, q), cplx));
        }
    }
}
__global__ __launch_bounds__(kBlock) void k_freq_shift(long long n, int ncols, int dtype, double w, double Ts, const void *x, mk::Cplx *out) {
    GRID_STRIDE(q, n * ncols) {
        const C2 y = freq_shift(load(dtype, x, q), q / ncols, w, Ts);
        out[q] = mk::Cplx{y.re, y.im};
    }
}

constexpr int kLoads = 4;
// ---- reductions over the rows of (rows, cols): blockIdx.y is the column, gridDim.x the partials per column
// part: (cols, gridDim.x, 2) doubles
__global__ __launch_bounds__(kBlock) void k_reduce_sum(int op, int dtype, long long rows, int cols, const double *center, const void *x, double *part) {
    const int col = blockIdx.y;
    const C2 c = center ? C2{center[2 * col], center[2 * col + 1]} : C2{0.0, 0.0};
    // kLoads running sums per lane, so that as many loads are in flight; they are joined in a fixed order
    double a[kLoads][2] = {};
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long r0 = (long long)blockIdx.x * kBlock + threadIdx.x; r0 < rows; r0 += kLoads * stride) {
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
            const long long r = r0 + k * stride;
            if (r < rows) {
                const C2 t = reduce_term(op, load(dtype, x, r * cols + col), c);
                a[k][0] += t.re, a[k][1] += t.im;
            }
        }
    }
    const double acc[2] = {(a[0][0] + a[1][0]) + (a[2][0] + a[3][0]), (a[0][1] + a[1][1]) + (a[2][1] + a[3][1])};
    br::block_sum_store<2>(acc, part + 2 * ((long long)col * gridDim.x + blockIdx.x));
}
__global__ void k_reduce_sum_fold(int nb, int cols, const double *part, double *out) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    double re = 0.0, im = 0.0;
    for (int b = 0; b < nb; ++b) re += part[2 * ((long long)col * nb + b)], im += part[2 * ((long long)col * nb + b) + 1];
    out[2 * col] = re, out[2 * col + 1] = im;
}
// the extreme of a workgroup's candidates -> (val[0], arg[0])
__device__ void block_extreme_store(int op, double v, long long i, double *val, long long *arg) {
    __shared__ double shv[br::kWaves];
    __shared__ long long shi[br::kWaves];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_down(v, o, 64);
        const long long i2 = __shfl_down(i, o, 64);
        if (extreme_beats(op, v2, i2, v, i)) v = v2, i = i2;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) shv[threadIdx.x >> 6] = v, shi[threadIdx.x >> 6] = i;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < br::kWaves; ++w)
            if (extreme_beats(op, shv[w], shi[w], v, i)) v = shv[w], i = shi[w];
        *val = v, *arg = i;
    }
}
__global__ __launch_bounds__(kBlock) void k_reduce_extreme(int op, int dtype, long long rows, int cols, const void *x, double *pval, long long *parg) {
    const int col = blockIdx.y;
    double v = 0.0;
    long long i = -1;
    GRID_STRIDE(r, rows) {
        const double v2 = load(dtype, x, r * cols + col).re;
        if (extreme_beats(op, v2, r, v, i)) v = v2, i = r;
    }
    const long long slot = (long long)col * gridDim.x + blockIdx.x;
    block_extreme_store(op, v, i, pval + slot, parg + slot);
}
__global__ void k_reduce_extreme_fold(int op, int nb, int cols, const double *pval, const long long *parg, double *val, long long *arg) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    double v = 0.0;
    long long i = -1;
    for (int b = 0; b < nb; ++b)
        if (extreme_beats(op, pval[(long long)col * nb + b], parg[(long long)col * nb + b], v, i)) v = pval[(long long)col * nb + b], i = parg[(long long)col * nb + b];
    val[col] = v, arg[col] = i;
}

// ---- host side
struct Work : WorkBase {
    Buf idx, row, in, out, center, part, parg, res, rarg;
};
using Call = CallT<Work>;

inline unsigned blocks_for(long long count) { return (unsigned)grid_blocks(count, kBlock, kMaxBlocks, 1); }

Desc to_desc(const ssf_array_desc *d) {
    Desc r{};
    r.ndim = d->ndim, r.offset = d->offset;
    for (int a = 0; a < d->ndim; ++a) r.shape[a] = d->shape[a], r.stride[a] = d->stride[a];
    return r;
}

template <template <typename> class F, typename... A> bool by_itemsize(int itemsize, A &&...a) {
    switch (itemsize) {
    case 1: F<unsigned char>::run(a...); return true;
    case 2: F<unsigned short>::run(a...); return true;
    case 4: F<unsigned int>::run(a...); return true;
    case 8: F<unsigned long long>::run(a...); return true;
    case 16: F<B16>::run(a...); return true;
    }
    return false;
}
template <typename T> struct RunCopy {
    static void run(hipStream_t st, const Desc &sd, const Desc &dd, long long count, const void *src, void *dst) {
        k_strided_copy<T><<<blocks_for(count), kBlock, 0, st>>>(sd, dd, count, (const T *)src, (T *)dst);
    }
};
template <typename T> struct RunTake {
    static void run(hipStream_t st, long long n_src, long long n_idx, long long inner, int idx_itemsize, const void *idx, const void *src, void *dst) {
        if (idx_itemsize == 8) k_take<T, long long><<<blocks_for(n_idx * inner), kBlock, 0, st>>>(n_src, n_idx, inner, (const long long *)idx, (const T *)src, (T *)dst);
        else k_take<T, int><<<blocks_for(n_idx * inner), kBlock, 0, st>>>(n_src, n_idx, inner, (const int *)idx, (const T *)src, (T *)dst);
    }
};
template <typename T> struct RunTranspose {
    static void run(hipStream_t st, long long rows, long long cols, const void *src, void *dst) {
        const long long tx = (cols + kTile - 1) / kTile, ty = (rows + kTile - 1) / kTile;
        k_transpose<T><<<(unsigned)(tx * ty), kBlock, 0, st>>>(rows, cols, tx, (const T *)src, (T *)dst);
    }
};
template <typename T> struct RunFill {
    static void run(hipStream_t st, long long count, const void *value, void *dst) {
        T v;
        memcpy(&v, value, sizeof(T));
        k_fill<T><<<blocks_for(count), kBlock, 0, st>>>(count, v, (T *)dst);
    }
};

bool all_device(Call &c, std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (!on_device(p)) return c.reject(SSF_ERR_BAD_ARG, "array data must be device memory");
    return true;
}

}  // namespace

int array_copy(int device, const ssf_array_desc *sdesc, const void *src, const ssf_array_desc *ddesc, void *dst, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {src, dst})) return c.rc;
    const Desc sd = to_desc(sdesc), dd = to_desc(ddesc);
    const long long count = desc_count(dd);
    const int isz = sdesc->itemsize;
    const long long bytes = count * isz;
    const bool flat = desc_contiguous(sd) && desc_contiguous(dd) && (sd.offset * isz) % 16 == 0 && (dd.offset * isz) % 16 == 0;
    if (flat) {
        const long long vecs = bytes / 16;
        k_flat_copy<<<blocks_for(vecs), kBlock, 0, c.w->st>>>(vecs, (int)(bytes - vecs * 16), (const B16 *)((const char *)src + sd.offset * isz),
                                                             (B16 *)((char *)dst + dd.offset * isz));
    } else {
        by_itemsize<RunCopy>(isz, c.w->st, sd, dd, count, src, dst);
    }
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_take(int device, int64_t n_src, int64_t n_idx, int64_t inner, int itemsize, int idx_itemsize, const void *idx, const void *src,
               void *dst, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {src, dst})) return c.rc;
    const void *id = c.input(idx, c.w->idx, (size_t)n_idx * idx_itemsize);
    if (!id) return c.rc;
    by_itemsize<RunTake>(itemsize, c.w->st, (long long)n_src, (long long)n_idx, (long long)inner, idx_itemsize, id, src, dst);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_transpose(int device, int64_t rows, int64_t cols, int itemsize, const void *src, void *dst, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {src, dst})) return c.rc;
    by_itemsize<RunTranspose>(itemsize, c.w->st, (long long)rows, (long long)cols, src, dst);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_fill(int device, int64_t count, int itemsize, const void *value, void *dst, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {dst})) return c.rc;
    by_itemsize<RunFill>(itemsize, c.w->st, (long long)count, value, dst);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_binary(int device, const ssf_array_binary_params *p, const void *a, const void *b, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {a, out})) return c.rc;
    BinArgs g{};
    g.op = p->op, g.swap = p->swap, g.a_dtype = p->a_dtype, g.b_dtype = p->b_dtype, g.out_dtype = p->out_dtype, g.count = p->count;
    g.bc.kind = p->kind, g.bc.inner = p->inner, g.bc.scalar = C2{p->scalar_re, p->scalar_im};
    g.a = a, g.out = out;
    if (p->kind == kSame || p->kind == kColumn) {
        if (!all_device(c, {b})) return c.rc;
        g.b = b;
    } else if (p->kind == kRow) {
        if (!(g.b = c.input(b, c.w->row, (size_t)p->inner * mk::elem_size(p->b_dtype)))) return c.rc;
    }
    const int V = vec_width(p->out_dtype);
    const unsigned nb = blocks_for((p->count + V - 1) / V);
    if (V == 4) k_binary<4><<<nb, kBlock, 0, c.w->st>>>(g);
    else if (V == 2) k_binary<2><<<nb, kBlock, 0, c.w->st>>>(g);
    else k_binary<1><<<nb, kBlock, 0, c.w->st>>>(g);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_unary(int device, int op, int in_dtype, int out_dtype, int64_t count, const void *x, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {x, out})) return c.rc;
    const int V = vec_width(out_dtype);
    const unsigned nb = blocks_for((count + V - 1) / V);
    if (V == 4) k_unary<4><<<nb, kBlock, 0, c.w->st>>>(op, in_dtype, out_dtype, (long long)count, x, out);
    else if (V == 2) k_unary<2><<<nb, kBlock, 0, c.w->st>>>(op, in_dtype, out_dtype, (long long)count, x, out);
    else k_unary<1><<<nb, kBlock, 0, c.w->st>>>(op, in_dtype, out_dtype, (long long)count, x, out);
    if (!c.launched() || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_reduce(int device, int op, int dtype, int64_t rows, int cols, const double *center, const void *x, double *out, int64_t *arg_out,
                 std::string *err) {
    Call c(device, err);
    if (c.rc || !all_device(c, {x})) return c.rc;
    Work &w = *c.w;
    const int nb = grid_blocks(rows, kBlock, kRedBlocks, 1);
    const dim3 grid((unsigned)nb, (unsigned)cols);
    const unsigned fold_blocks = (unsigned)((cols + 63) / 64);
    if (!c.need(w.part, (size_t)cols * nb * 2 * sizeof(double)) || !c.need(w.res, (size_t)cols * 2 * sizeof(double))) return c.rc;
    if (op == kSum || op == kSumSqDev) {
        const double *cd = nullptr;
        if (center && !(cd = (const double *)c.input(center, w.center, (size_t)cols * 2 * sizeof(double)))) return c.rc;
        k_reduce_sum<<<grid, kBlock, 0, w.st>>>(op, dtype, (long long)rows, cols, cd, x, (double *)w.part.p);
        if (!c.launched()) return c.rc;
        k_reduce_sum_fold<<<fold_blocks, 64, 0, w.st>>>(nb, cols, (const double *)w.part.p, (double *)w.res.p);
        if (!c.launched()) return c.rc;
        if (!c.deliver(out, w.res.p, (size_t)cols * 2 * sizeof(double)) || !c.sync()) return c.rc;
        return SSF_OK;
    }
    if (!c.need(w.parg, (size_t)cols * nb * sizeof(long long)) || !c.need(w.rarg, (size_t)cols * sizeof(long long))) return c.rc;
    k_reduce_extreme<<<grid, kBlock, 0, w.st>>>(op, dtype, (long long)rows, cols, x, (double *)w.part.p, (long long *)w.parg.p);
    if (!c.launched()) return c.rc;
    k_reduce_extreme_fold<<<fold_blocks, 64, 0, w.st>>>(op, nb, cols, (const double *)w.part.p, (const long long *)w.parg.p, (double *)w.res.p,
                                                         (long long *)w.rarg.p);
    if (!c.launched()) return c.rc;
    if (!c.deliver(out, w.res.p, (size_t)cols * sizeof(double)) || !c.deliver(arg_out, w.rarg.p, (size_t)cols * sizeof(long long)) || !c.sync()) return c.rc;
    return SSF_OK;
}

int array_freq_shift(int device, int64_t n, int ncols, int dtype, double deltaF, double Fs, const void *x, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long count = (long long)n * ncols;
    const size_t out_bytes = (size_t)count * sizeof(mk::Cplx);
    void *o = c.target(out, w.out, out_bytes);
    if (!o) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)count * mk::elem_size(dtype));
    if (!xd) return c.rc;
    k_freq_shift<<<blocks_for(count), kBlock, 0, w.st>>>((long long)n, ncols, dtype, (2.0 * M_PI) * deltaF, 1.0 / Fs, xd, (mk::Cplx *)o);
    if (!c.launched() || !c.deliver(out, o, out_bytes) || !c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
