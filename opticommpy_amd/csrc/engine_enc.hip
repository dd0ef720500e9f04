// engine_enc.hip -- LDPC encoding and Gray mapping on the device (ssf_ldpc_encoder_create / destroy, ssf_ldpc_encode, ssf_modulate
// of include/ssf.h).  The per-lane bodies are enc_kernels.h; here are the three kernels that walk them, one launch per call each.
//   k_dense    workgroup (x, y): parity rows 256 x .. 256 x + 255 of the codewords 16 y .. 16 y + 15.  It packs the tile's messages
//              into LDS (one ballot per word), then every lane takes one row of P through all 16 messages: a row is read once per
//              tile.  Consecutive lanes hold consecutive rows, so the byte stores of the codeword-major layout are contiguous.
//              The workgroups x = 0 also copy the systematic part, out of the packed words.
//   k_accum    one workgroup per codeword: packs the message into LDS, then takes the parities of the rows of A 256 at a time with no
//              barrier in between (the ballot of every 64 goes to LDS), then wave 0 scans the ballots' totals, 64 at a time with
//              the same ballot trick, into a carry per ballot, then every lane writes its checks: the XOR prefix inside the
//              ballot plus the ballot's carry.  Three barriers per codeword, whatever the number of checks.
//   k_modulate one symbol per lane, the table in LDS.
// The (k, N) orientation is the same kernels with strided loads and stores (enc::user_index); nothing is transposed in memory.
#include <hip/hip_runtime.h>

#include <vector>

#include "enc_kernels.h"
#include "engine_host.h"

namespace ssf {
namespace {
using namespace enc;
using namespace eng;

struct EncArgs {
    const uint64_t *P;                        // dense: (rows, W) words
    const int *ptr, *idx;                     // sparse: CSR of A
    int k, rows, W, copy;                     // copy: the message is the first k rows of the codeword
    const unsigned char *in;
    unsigned char *out;
    int N, n, transposed;                     // n: rows stored per codeword
};

// 64 lanes, one bit each -> one word; every lane of the wave gets it
__device__ __forceinline__ uint64_t ballot_bit(unsigned bit) { return (uint64_t)__ballot((int)bit); }

__global__ __launch_bounds__(kBlock) void k_dense(EncArgs a) {
    extern __shared__ __align__(16) uint64_t s_msg[];     // (kTile, W)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int c0 = blockIdx.y * kTile;
    for (int p = wave; p < kTile * a.W; p += kBlock / kWave) {
        const int t = p / a.W, w = p - t * a.W;
        const uint64_t word = ballot_bit(load_bit(a.in, w * kWave + lane, c0 + t, a.k, a.N, a.transposed));
        if (lane == 0) s_msg[p] = word;
    }
    __syncthreads();
    const int nt = a.N - c0 < kTile ? a.N - c0 : kTile;
    if (a.copy && blockIdx.x == 0)
        for (int j = tid; j < a.k && j < a.n; j += kBlock)
            for (int t = 0; t < nt; ++t)
                a.out[user_index(j, c0 + t, a.n, a.N, a.transposed)] = (unsigned char)word_bit(s_msg + (size_t)t * a.W, j);
    const int i = blockIdx.x * kRows + tid;
    const int row = (a.copy ? a.k : 0) + i;   // where parity i stands in the codeword
    if (i >= a.rows || row >= a.n) return;
    uint64_t acc[kTile];
    dense_row(a.P + (size_t)i * a.W, s_msg, a.W, acc);
#pragma unroll
    for (int t = 0; t < kTile; ++t)
        if (t < nt) a.out[user_index(row, c0 + t, a.n, a.N, a.transposed)] = (unsigned char)parity64(acc[t]);
}

__global__ __launch_bounds__(kBlock) void k_accum(EncArgs a) {
    extern __shared__ __align__(16) uint64_t s_msg[];     // W words, then the ballots of the parities, then a carry per ballot
    const int Wm = (a.rows + kWave - 1) / kWave;
    uint64_t *s_par = s_msg + a.W;
    unsigned char *s_cin = (unsigned char *)(s_par + Wm);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int c = blockIdx.x;
    for (int w = wave; w < a.W; w += kBlock / kWave) {
        const uint64_t word = ballot_bit(load_bit(a.in, w * kWave + lane, c, a.k, a.N, a.transposed));
        if (lane == 0) s_msg[w] = word;
    }
    __syncthreads();
    for (int j = tid; j < a.k && j < a.n; j += kBlock) a.out[user_index(j, c, a.n, a.N, a.transposed)] = (unsigned char)word_bit(s_msg, j);
    // the parities of all rows, a span of 256 at a time with no barrier in between: the loads of one span overlap the next
#pragma unroll 2
    for (int base = 0; base < a.rows; base += kSpan) {
        const int i = base + tid;
        const unsigned p = i < a.rows ? row_parity(s_msg, a.idx, a.ptr[i], a.ptr[i + 1]) : 0u;
        const uint64_t word = ballot_bit(p);
        if (lane == 0 && base + wave * kWave < a.rows) s_par[base / kWave + wave] = word;
    }
    __syncthreads();
    // the carry into every ballot: wave 0 scans the ballots' totals, 64 at a time, with the same ballot trick
    if (wave == 0) {
        unsigned carry = 0;                   // the same value in every lane
        for (int s = 0; s < Wm; s += kWave) {
            const int j = s + lane;
            const unsigned t = j < Wm ? scan_total(s_par[j]) : 0u;
            const uint64_t word = ballot_bit(t);
            if (j < Wm) s_cin[j] = (unsigned char)(scan_lane(word, lane) ^ t ^ carry);      // exclusive: without the ballot's own total
            carry ^= scan_total(word);
        }
    }
    __syncthreads();
    for (int i = tid; i < a.rows && a.k + i < a.n; i += kBlock)
        a.out[user_index(a.k + i, c, a.n, a.N, a.transposed)] = (unsigned char)(scan_lane(s_par[i / kWave], i & (kWave - 1)) ^ s_cin[i / kWave]);
}

struct ModArgs {
    const double *tab;                        // M (re, im) pairs
    const unsigned char *bits;
    double2 *out;
    long long n;
    int M, b;
};

__global__ __launch_bounds__(kBlock) void k_modulate(ModArgs a) {
    __shared__ double2 s_tab[kModMaxM];
    for (int i = threadIdx.x; i < a.M; i += kBlock) s_tab[i] = make_double2(a.tab[2 * i], a.tab[2 * i + 1]);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock)
        a.out[i] = s_tab[symbol_index(a.bits, i, a.b)];
}

struct Work : WorkBase {
    Buf in, out, tab;
    std::vector<double> host_tab;             // kept for its capacity
};
using Call = CallT<Work>;

}  // namespace

int enc_create(int device, const ssf_ldpc_encoder_desc *d, const uint64_t *block1, const uint64_t *block2, const int32_t *indptr,
               const int32_t *indices, ssf_ldpc_encoder **out, std::string *err) {
    Call c(device, err, false);
    if (c.rc) return c.rc;
    ssf_ldpc_encoder *e = new ssf_ldpc_encoder();
    e->device = device, e->form = d->form, e->k = d->k, e->systematic = d->systematic, e->W = (d->k + kWave - 1) / kWave;
    bool ok;
    if (d->form == kDense) {
        e->rows = d->m1 + d->m2;
        const size_t b1 = (size_t)d->m1 * e->W * sizeof(uint64_t), b2 = (size_t)d->m2 * e->W * sizeof(uint64_t);
        ok = c.ok(hipMalloc((void **)&e->d_P, b1 + b2), "hipMalloc") && c.ok(hipMemcpy(e->d_P, block1, b1, hipMemcpyHostToDevice), "hipMemcpy") &&
             (!b2 || c.ok(hipMemcpy(e->d_P + (size_t)d->m1 * e->W, block2, b2, hipMemcpyHostToDevice), "hipMemcpy"));
    } else {
        e->rows = d->m1;
        const size_t np = (size_t)d->m1 + 1, ni = (size_t)d->nnz;
        ok = c.ok(hipMalloc((void **)&e->d_ptr, (np + ni + 1) * sizeof(int)), "hipMalloc") &&
             c.ok(hipMemcpy(e->d_ptr, indptr, np * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") &&
             (!ni || c.ok(hipMemcpy(e->d_ptr + np, indices, ni * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy"));
        e->d_idx = e->d_ptr ? e->d_ptr + np : nullptr;
    }
    if (!ok) {
        (void)hipFree(e->d_P);
        (void)hipFree(e->d_ptr);
        delete e;
        return c.rc;
    }
    *out = e;
    return SSF_OK;
}

int enc_destroy(ssf_ldpc_encoder *e, std::string *err) {
    Call c(e->device, err, false);
    if (!c.rc) {
        if (e->d_P) c.ok(hipFree(e->d_P), "hipFree");
        if (e->d_ptr) c.ok(hipFree(e->d_ptr), "hipFree");
    }
    delete e;
    return c.rc;
}

int enc_encode(int device, const ssf_ldpc_encoder *e, const ssf_ldpc_encode_params *p, const void *bits_in, void *cw_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int N = p->numCodewords;
    const size_t out_bytes = (size_t)p->n * N;
    EncArgs a{};
    a.P = e->d_P, a.ptr = e->d_ptr, a.idx = e->d_idx, a.k = e->k, a.rows = e->rows, a.W = e->W;
    a.copy = e->form == kSparse || e->systematic, a.N = N, a.n = p->n, a.transposed = p->transposed;
    a.out = (unsigned char *)c.target(cw_out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.in = (const unsigned char *)c.input(bits_in, w.in, (size_t)e->k * N);
    if (!a.in) return c.rc;
    if (e->form == kDense) {
        const dim3 grid((unsigned)((e->rows + kRows - 1) / kRows), (unsigned)((N + kTile - 1) / kTile));
        k_dense<<<grid, kBlock, (size_t)kTile * e->W * sizeof(uint64_t), w.st>>>(a);
    } else {
        const size_t Wm = (size_t)(e->rows + kWave - 1) / kWave;          // [message words | ballots | carries, rounded up to words]
        k_accum<<<N, kBlock, ((size_t)e->W + Wm + (Wm + 7) / 8) * sizeof(uint64_t), w.st>>>(a);
    }
    if (!c.launched()) return c.rc;
    if (!c.deliver(cw_out, a.out, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int enc_modulate(int device, int64_t nsymb, int M, const double *table, const void *bits, void *symb_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    int b = 0;
    while ((1 << b) < M) ++b;
    const size_t out_bytes = (size_t)nsymb * 2 * sizeof(double);
    ModArgs a{};
    a.out = (double2 *)c.target(symb_out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.bits = (const unsigned char *)c.input(bits, w.in, (size_t)nsymb * b);
    if (!a.bits) return c.rc;
    w.host_tab.assign(table, table + 2 * (size_t)M);
    if (!c.upload(w.tab, w.host_tab)) return c.rc;
    a.tab = (const double *)w.tab.p, a.n = nsymb, a.M = M, a.b = b;
    k_modulate<<<grid_blocks(nsymb, kBlock, 8192), kBlock, 0, w.st>>>(a);
    if (!c.launched()) return c.rc;
    if (!c.deliver(symb_out, a.out, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
