// What the Krylov kernels share on the device (krylov_blas.hip: the BLAS-1 layer of GMRES; bicgstab.hip): the two-stage
// fixed-order reduction, the complex multiply-adds, and the loops both files run.  The bits of every residual history
// depend on the order of summation and on the spelling of the multiply-adds: each is written here, once.
// Each block accumulates a grid-stride slice, reduces across its four waves (shuffle, then LDS), and writes one
// partial; a single wave sums the partials in index order (finish_in_wave) -- in the finisher kernel, or inside the
// consuming kernel.
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
// blocks of an element-wise kernel over `count` entries
static inline unsigned grid_for(int64_t count, int block = 256, int cap = 256 * 16) {
    int64_t g = (count + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// acc += conj(u) v
__device__ __forceinline__ void cdot_acc(cplx& acc, cplx u, cplx v) {
    acc.x = fma(u.x, v.x, fma(u.y, v.y, acc.x));
    acc.y = fma(u.x, v.y, fma(-u.y, v.x, acc.y));
}
// acc.x += |x|^2
__device__ __forceinline__ void cnorm_acc(cplx& acc, cplx x) { acc.x = fma(x.x, x.x, fma(x.y, x.y, acc.x)); }
// a - c * b
__device__ __forceinline__ cplx csubmul(cplx a, cplx c, cplx b) {
    return make_double2(a.x - fma(c.x, b.x, -c.y * b.y), a.y - fma(c.x, b.y, c.y * b.x));
}
// a + c * b
__device__ __forceinline__ cplx caddmul(cplx a, cplx c, cplx b) {
    return make_double2(a.x + fma(c.x, b.x, -c.y * b.y), a.y + fma(c.x, b.y, c.y * b.x));
}
// a * b (born.hip: the pointwise products of the linearised scattering kernels)
__device__ __forceinline__ cplx cprod(cplx a, cplx b) {
    return make_double2(fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x));
}
// acc += c * q, the product rounded before it is added (the gemv loops)
__device__ __forceinline__ void cmul_acc(cplx& acc, cplx c, cplx q) {
    acc.x += fma(c.x, q.x, -c.y * q.y);
    acc.y += fma(c.x, q.y, c.y * q.x);
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

// sum of partial[0..count) in all 64 lanes of one wave: THE order of the second stage
__device__ __forceinline__ cplx finish_in_wave(const cplx* __restrict__ partial, int count) {
    cplx acc = make_double2(0.0, 0.0);
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < count; i += 64) { acc.x += partial[i].x; acc.y += partial[i].y; }
    acc.x = wave_sum(acc.x); acc.y = wave_sum(acc.y);
    return make_double2(__shfl(acc.x, 0, 64), __shfl(acc.y, 0, 64));
}

// this block's slice of sum_i conj(a[i]) b[i], valid in thread 0 (sh: RED_THREADS / 64 entries of LDS)
__device__ __forceinline__ cplx dot_slice(const cplx* __restrict__ a, const cplx* __restrict__ b, int64_t n, cplx* sh) {
    cplx acc = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) cdot_acc(acc, a[i], b[i]);
    return block_sum(acc, sh);
}
// this block's slice of y = a - b; y may be a or b (no __restrict__)
__device__ __forceinline__ void sub_slice(cplx* y, const cplx* a, const cplx* b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx u = a[i], v = b[i]; y[i] = make_double2(u.x - v.x, u.y - v.y);
    }
}

} // namespace lsfc
