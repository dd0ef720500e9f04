// emu_array.cpp -- the array layer's kernels walked on the host: includes opticommpy_amd/csrc/array_kernels.h, the bodies the
// gfx950 kernels of engine_array.hip call, and runs them over the device's grids with g++ (tests/test_array_emu.py).  The
// reductions follow the device's order: per lane four running sums over the grid-stride walk, the wave's shuffle tree, the four
// waves, then the partials in index order.
// Usage: emu_array in.bin out.bin.  in.bin: 32 int64 of header (mode first), then the arrays of the mode, as raw bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "array_kernels.h"

using namespace ssf;
using namespace ssf::ak;

static std::vector<char> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> b((size_t)n);
    if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
    fclose(f);
    return b;
}

// the lanes of one launch, in order: f(block, lane)
template <class F> static void for_lanes(long long count, int max_blocks, F f) {
    long long nb = (count + kBlock - 1) / kBlock;
    nb = nb < 1 ? 1 : nb > max_blocks ? max_blocks : nb;
    for (long long b = 0; b < nb; ++b)
        for (int l = 0; l < kBlock; ++l) f(b, l, nb);
}
template <class F> static void grid_stride(long long count, F f) {
    for_lanes(count, kMaxBlocks, [&](long long b, int l, long long nb) {
        for (long long q = b * kBlock + l; q < count; q += nb * kBlock) f(q);
    });
}

// block_reduce.h: __shfl_down over 64 lanes (a lane past the end reads itself), lane 0 holds the wave's sum
static double wave_sum_down(const double *v64) {
    double v[64], n[64];
    memcpy(v, v64, sizeof v);
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < 64; ++l) n[l] = v[l] + (l + o < 64 ? v[l + o] : v[l]);
        memcpy(v, n, sizeof v);
    }
    return v[0];
}
static double block_sum(const double *v256) {
    double w[4];
    for (int k = 0; k < 4; ++k) w[k] = wave_sum_down(v256 + 64 * k);
    return ((w[0] + w[1]) + w[2]) + w[3];
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<char> in = read_file(argv[1]);
    const long long *h = (const long long *)in.data();
    const char *body = in.data() + 32 * sizeof(long long);
    std::vector<char> out;
    const int mode = (int)h[0];
    if (mode == 0) {                       // strided copy: itemsize, ndim, soff, doff, dst elements, shape[4], sstride[4], dstride[4]
        const int isz = (int)h[1];
        Desc sd{}, dd{};
        sd.ndim = dd.ndim = (int)h[2], sd.offset = h[3], dd.offset = h[4];
        out.assign((size_t)h[5] * isz, (char)0xee);
        for (int a = 0; a < kMaxDim; ++a) sd.shape[a] = dd.shape[a] = h[6 + a], sd.stride[a] = h[10 + a], dd.stride[a] = h[14 + a];
        const long long count = desc_count(dd);
        grid_stride(count, [&](long long q) { memcpy(out.data() + strided_offset(dd, q) * isz, body + strided_offset(sd, q) * isz, (size_t)isz); });
    } else if (mode == 1) {                // take: itemsize, n_src, n_idx, inner; idx (int64), src
        const int isz = (int)h[1];
        const long long n_src = h[2], n_idx = h[3], inner = h[4];
        const long long *idx = (const long long *)body;
        const char *src = body + n_idx * 8;
        out.resize((size_t)(n_idx * inner) * isz);
        grid_stride(n_idx * inner, [&](long long q) {
            const long long i = q / inner, j = q - i * inner;
            memcpy(out.data() + q * isz, src + (take_row(idx[i], n_src) * inner + j) * isz, (size_t)isz);
        });
    } else if (mode == 2) {                // binary: op, swap, a_dtype, b_dtype, out_dtype, kind, count, inner, nb; scalar (2 doubles), a, b
        const int op = (int)h[1], swap = (int)h[2], adt = (int)h[3], bdt = (int)h[4], odt = (int)h[5];
        Bcast bc;
        bc.kind = (int)h[6], bc.inner = h[8];
        const long long count = h[7];
        const double *sc = (const double *)body;
        bc.scalar = C2{sc[0], sc[1]};
        const char *a = body + 16;
        const std::vector<char> bcopy(a + count * mk::elem_size(adt), in.data() + in.size());      // (its own allocation: aligned)
        const char *b = bcopy.data();
        out.resize((size_t)count * mk::elem_size(odt));
        const int V = vec_width(odt);
        grid_stride((count + V - 1) / V, [&](long long pq) {
            for (long long q = pq * V; q < pq * V + V && q < count; ++q) {
                const C2 bv = bc.kind == kScalar ? bc.scalar : load(bdt, b, bcast_index(bc, q));
                const C2 av = load(adt, a, q);
                store(odt, out.data(), q, swap ? binary(op, bv, av, is_complex(odt)) : binary(op, av, bv, is_complex(odt)));
            }
        });
    } else if (mode == 3) {                // unary: op, in_dtype, out_dtype, count; x
        const int op = (int)h[1], idt = (int)h[2], odt = (int)h[3];
        const long long count = h[4];
        out.resize((size_t)count * mk::elem_size(odt));
        const int V = vec_width(odt);
        grid_stride((count + V - 1) / V, [&](long long pq) {
            for (long long q = pq * V; q < pq * V + V && q < count; ++q) store(odt, out.data(), q, unary(op, load(idt, body, q), is_complex(idt)));
        });
    } else if (mode == 4) {                // reduce: op, dtype, rows, cols; centre (cols, 2), x -> (cols, 2) doubles + cols int64
        const int op = (int)h[1], dt = (int)h[2];
        const long long rows = h[3], cols = h[4];
        const double *center = (const double *)body;
        const char *x = body + cols * 16;
        out.resize((size_t)cols * 24);
        double *res = (double *)out.data();
        long long *arg = (long long *)(out.data() + cols * 16);
        long long nb = (rows + kBlock - 1) / kBlock;
        nb = nb < 1 ? 1 : nb > kRedBlocks ? kRedBlocks : nb;
        const long long stride = nb * kBlock;
        for (long long col = 0; col < cols; ++col) {
            const C2 c{center[2 * col], center[2 * col + 1]};
            double tre = 0.0, tim = 0.0, best = 0.0;
            long long besti = -1;
            for (long long b = 0; b < nb; ++b) {
                if (op == kSum || op == kSumSqDev) {
                    double lre[kBlock], lim[kBlock];
                    for (int l = 0; l < kBlock; ++l) {
                        double a[4][2] = {};
                        for (long long r0 = b * kBlock + l; r0 < rows; r0 += 4 * stride)
                            for (int k = 0; k < 4; ++k) {
                                const long long r = r0 + k * stride;
                                if (r < rows) {
                                    const C2 t = reduce_term(op, load(dt, x, r * cols + col), c);
                                    a[k][0] += t.re, a[k][1] += t.im;
                                }
                            }
                        lre[l] = (a[0][0] + a[1][0]) + (a[2][0] + a[3][0]), lim[l] = (a[0][1] + a[1][1]) + (a[2][1] + a[3][1]);
                    }
                    tre += block_sum(lre), tim += block_sum(lim);
                } else {
                    // (a candidate list merged in any order gives the same extreme: extreme_beats is a total order)
                    for (int l = 0; l < kBlock; ++l)
                        for (long long r = b * kBlock + l; r < rows; r += stride) {
                            const double v2 = load(dt, x, r * cols + col).re;
                            if (extreme_beats(op, v2, r, best, besti)) best = v2, besti = r;
                        }
                }
            }
            res[2 * col] = (op == kSum || op == kSumSqDev) ? tre : best, res[2 * col + 1] = tim, arg[col] = besti;
        }
    } else if (mode == 5) {                // freq shift: dtype, n, ncols; (deltaF, Fs), x
        const int dt = (int)h[1];
        const long long n = h[2], ncols = h[3];
        const double *prm = (const double *)body;
        const double w = (2.0 * M_PI) * prm[0], Ts = 1.0 / prm[1];
        out.resize((size_t)(n * ncols) * 16);
        grid_stride(n * ncols, [&](long long q) { store(mk::kC128, out.data(), q, freq_shift(load(dt, body + 16, q), q / ncols, w, Ts)); });
    } else if (mode == 6) {                // transpose: itemsize, rows, cols; src
        const int isz = (int)h[1];
        const long long rows = h[2], cols = h[3];
        out.assign((size_t)(rows * cols) * isz, (char)0xee);
        const long long tiles_x = (cols + kTile - 1) / kTile, tiles_y = (rows + kTile - 1) / kTile;
        std::vector<char> tile((size_t)kTile * (kTile + 1) * isz);
        for (long long blk = 0; blk < tiles_x * tiles_y; ++blk) {
            const long long by = blk / tiles_x, bx = blk - by * tiles_x;
            for (int t = 0; t < kBlock; ++t) {
                const int tx = t & (kTile - 1), ty = t / kTile;
                for (int r = ty; r < kTile; r += kBlock / kTile) {
                    const long long row = by * kTile + r, col = bx * kTile + tx;
                    if (row < rows && col < cols) memcpy(&tile[(size_t)(r * (kTile + 1) + tx) * isz], body + (row * cols + col) * isz, (size_t)isz);
                }
            }
            for (int t = 0; t < kBlock; ++t) {
                const int tx = t & (kTile - 1), ty = t / kTile;
                for (int r = ty; r < kTile; r += kBlock / kTile) {
                    const long long orow = bx * kTile + r, ocol = by * kTile + tx;
                    if (orow < cols && ocol < rows) memcpy(out.data() + (orow * rows + ocol) * isz, &tile[(size_t)(tx * (kTile + 1) + r) * isz], (size_t)isz);
                }
            }
        }
    } else {
        return 2;
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    fclose(f);
    return 0;
}
