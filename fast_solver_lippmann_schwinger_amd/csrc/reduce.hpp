// The two-stage fixed-order reduction shared by the Krylov kernels (pointwise.hip: GMRES BLAS-1; bicgstab.hip).
// Each block accumulates a grid-stride slice, reduces across its four waves (shuffle, then LDS), and writes one
// partial; a single wave sums the partials in index order -- in a finisher kernel, or inside the consuming kernel.
// RED_BLOCKS is fixed so results do not depend on N beyond the slice boundaries -> run-to-run bitwise reproducible.
#pragma once
#include "common.hpp"

namespace lsfc {

static constexpr int RED_BLOCKS = 1024;
static constexpr int RED_THREADS = 256;
// blocks actually launched for a vector of n entries: at least ~4 entries per thread (a 48^3 grid gets 108 blocks, not 1024
// blocks of mostly idle threads); a function of n only, so results stay run-to-run reproducible
static inline int red_blocks(int64_t n) {
    const int64_t b = (n + (int64_t)RED_THREADS * 4 - 1) / ((int64_t)RED_THREADS * 4);
    return (int)(b < 1 ? 1 : (b > RED_BLOCKS ? RED_BLOCKS : b));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ cplx block_sum(cplx acc, cplx* sh) {
    acc.x = wave_sum(acc.x); acc.y = wave_sum(acc.y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    cplx r = make_double2(0.0, 0.0);
    if (threadIdx.x == 0) { for (int w = 0; w < RED_THREADS / 64; ++w) { r.x += sh[w].x; r.y += sh[w].y; } }
    return r;   // valid in thread 0
}

// sum of partial[0..count) in the order k_finish uses, in all 64 lanes of one wave
__device__ __forceinline__ cplx finish_in_wave(const cplx* __restrict__ partial, int count) {
    cplx acc = make_double2(0.0, 0.0);
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < count; i += 64) { acc.x += partial[i].x; acc.y += partial[i].y; }
    acc.x = wave_sum(acc.x); acc.y = wave_sum(acc.y);
    return make_double2(__shfl(acc.x, 0, 64), __shfl(acc.y, 0, 64));
}

} // namespace lsfc
