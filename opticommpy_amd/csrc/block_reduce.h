// block_reduce.h -- the fixed-order sums of the DSP engines' kernels (device side, HIP only: no *_kernels.h includes it).
// A sum over the elements of a launch is: a grid-stride running value per lane -> the wave's lanes by __shfl_down 32, 16 .. 1 ->
// one value per wave in LDS -> ((w0 + w1) + w2) + w3 as the workgroup's partial -> one wave adds the partials, lane-strided,
// then the same shuffle tree.  No atomics and nothing left to the scheduler: for a given grid a result repeats bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace ssf {
namespace br {

constexpr int kBlock = 256, kWaves = kBlock / 64;     // the workgroup these sums are written for

// sum over the 64 lanes of a wave; lane 0 holds it
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// K running sums of this workgroup of kBlock lanes -> out[0 .. K).  The leading barrier makes a second call in the same kernel
// safe: no wave writes the LDS slots while another still reads them for the call before.
template <int K> __device__ void block_sum_store(const double (&acc)[K], double *out) {
    __shared__ double sh[kWaves][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_down(acc[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sh[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        out[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
    }
}
__device__ inline void block_sum_store(double v, double *out) {
    const double acc[1] = {v};
    block_sum_store<1>(acc, out);
}

// one wave: the sum of part[0], part[stride], .. (nb values), lane-strided then the shuffle tree; lane 0 holds it
__device__ __forceinline__ double wave_sum_partials(const double *part, int nb, long long stride) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) a += part[b * stride];
    return wave_sum_down(a);
}

// ---- the maximum of non-negative values over a launch, by the same route as the sums (a maximum does not depend on the order;
// the route is fixed all the same)
__device__ __forceinline__ double wave_max_down(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}
__device__ inline void block_max_store(double v, double *out) {
    __shared__ double sh[kWaves];
    v = wave_max_down(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *out = fmax(fmax(fmax(sh[0], sh[1]), sh[2]), sh[3]);
}
__device__ __forceinline__ double wave_max_partials(const double *part, int nb) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) a = fmax(a, part[b]);
    return wave_max_down(a);
}

}  // namespace br
}  // namespace ssf
