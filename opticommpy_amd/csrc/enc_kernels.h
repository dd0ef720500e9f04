// enc_kernels.h -- LDPC encoding and Gray mapping: the per-lane bodies of the three kernels of engine_enc.hip as host/device-neutral
// functions.  engine_enc.hip wraps them in gfx950 kernels; tests/emu/emu_enc.cpp walks the same text with g++ in the same tiling.
// Reference: optic/comm/fec.py:153-344 (encodeLDPC, encodeDVBS2, encoder), 1019-1072 (encodeTriang),
// optic/comm/modulation.py:334-366 (modulateGray).
//
// Everything is GF(2) or a table lookup: no rounding, no order that matters -- the results are the reference's bits.
//   pack       64 message bits of one codeword become one 64-bit word, bit l of word w is message bit 64 w + l; bits beyond k are 0
//              (one lane per bit, the word is the wave's ballot).  An input byte counts as b & 1.
//   dense      parity row i of a codeword is the parity of popcount(XOR_w P[i][w] & msg[w]): one lane per row, the packed messages
//              of a tile of codewords in LDS, the row's words read once for the whole tile.
//   sparse     the DVB-S2 accumulator: p[i] = XOR of the message bits in row i of A, cw[k + i] = p[i] ^ cw[k + i - 1].  The XOR
//              prefix scan of 64 consecutive checks is a ballot and a popcount below the lane; the carry into a ballot is the
//              XOR of the parities of the ballots before it, scanned the same way, 64 ballots at a time.
//   modulate   symbol i is table[sum_j bit[i b + j] << (b - 1 - j)]: the first bit of a symbol is the most significant.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ENC_HD __host__ __device__ inline
#else
#define ENC_HD inline
#endif

namespace ssf {
namespace enc {

enum { kDense = 0, kSparse = 1 };             // ssf_ldpc_encoder_desc.form
constexpr int kBlock = 256;                   // lanes of a workgroup, every kernel
constexpr int kWave = 64;                     // checks one ballot scans: a wave's span
constexpr int kTile = 16;                     // dense: codewords whose packed messages share a workgroup's LDS
constexpr int kRows = kBlock;                 // dense: parity rows per workgroup, one per lane
constexpr int kSpan = kBlock;                 // sparse: checks whose parities a workgroup takes in one pass, four ballots
constexpr int kMaxWordsDense = 512;           // dense: kTile * words * 8 bytes of LDS <= 64 KiB  (k <= 32 768)
constexpr int kMaxWordsSparse = 2048;         // sparse: words * 8 bytes of LDS for the message  (k <= 131 072)
constexpr int kMaxChecksSparse = 262144;      // sparse: 9 bytes of LDS per 64 checks: their ballot and its carry
constexpr int kModMaxM = 1024;

// element (i, c) of a caller's array of `len` bits per codeword: (len, N) row-major, or (N, len) with `transposed`
ENC_HD long long user_index(int i, int c, int len, int N, int transposed) {
    return transposed ? (long long)c * len + i : (long long)i * N + c;
}

// message bit j of codeword c as 0 / 1; 0 beyond the message or the batch (the lanes of the last word, the rows of the last tile)
ENC_HD unsigned load_bit(const unsigned char *in, int j, int c, int k, int N, int transposed) {
    return (j < k && c < N) ? (unsigned)(in[user_index(j, c, k, N, transposed)] & 1) : 0u;
}

ENC_HD unsigned word_bit(const uint64_t *words, int j) { return (unsigned)((words[j >> 6] >> (j & 63)) & 1u); }

ENC_HD unsigned parity64(uint64_t x) { return (unsigned)(__builtin_popcountll(x) & 1); }

// dense: acc[t] ^= P[i][w] & msg[t][w] over the words of row i, for the `kTile` messages of the tile (msg: kTile rows of W words)
ENC_HD void dense_row(const uint64_t *prow, const uint64_t *msg, int W, uint64_t acc[kTile]) {
    for (int t = 0; t < kTile; ++t) acc[t] = 0;
    for (int w = 0; w < W; ++w) {
        const uint64_t p = prow[w];
        for (int t = 0; t < kTile; ++t) acc[t] ^= p & msg[(long long)t * W + w];
    }
}

// sparse: parity of the message bits named by cols[start .. end)
ENC_HD unsigned row_parity(const uint64_t *msg, const int *cols, int start, int end) {
    unsigned p = 0;
    for (int e = start; e < end; ++e) p ^= word_bit(msg, cols[e]);
    return p;
}

// inclusive XOR prefix of lane `lane` from the ballot of the wave's 64 parities, and the wave's total
ENC_HD unsigned scan_lane(uint64_t ballot, int lane) { return parity64(ballot & (~0ull >> (63 - lane))); }
ENC_HD unsigned scan_total(uint64_t ballot) { return parity64(ballot); }

// modulate: the table index of symbol i of b bits, most significant first
ENC_HD int symbol_index(const unsigned char *bits, long long i, int b) {
    int idx = 0;
    for (int j = 0; j < b; ++j) idx = (idx << 1) | (bits[i * b + j] & 1);
    return idx;
}

}  // namespace enc
}  // namespace ssf
