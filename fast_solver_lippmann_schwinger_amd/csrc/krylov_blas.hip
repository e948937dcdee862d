// The BLAS-1 layer of the Krylov solvers (gfx950): GMRES calls it through krylov_blas.hpp, BiCGStab(l) shares its
// device pieces through reduce.hpp.  All kernels are HBM-bound: 16 B per lane accesses, grid-stride loops, and the
// two-stage fixed-order reduction of reduce.hpp (bitwise reproducible, no float atomics).  An operation with a fused
// and an unfused form has ONE device body and two kernel heads that differ in where its scalar comes from: a device
// scalar (a finisher, perhaps an all-reduce, ran in between), or the producer's block partials, summed by the consumer.
#include "common.hpp"
#include "krylov_blas.hpp"
#include "reduce.hpp"

namespace lsfc {

// ---- reductions ----------------------------------------------------------------------------------------------------

// partial[b] = sum_i conj(a[i]) * b[i]   (Julia dot(a, b))
__global__ __launch_bounds__(RED_THREADS) void k_dot_partial(const cplx* __restrict__ a, const cplx* __restrict__ b, cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    const cplx r = dot_slice(a, b, n, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// The finisher, one block per slot (RED_BLOCKS entries apart): out[s] = sum of the slot's first `count` partials (mode 0),
// or sqrt(re sum) in out[s].x (mode 1)
__global__ __launch_bounds__(64) void k_finish(const cplx* __restrict__ partial, int count, cplx* __restrict__ out, int mode) {
    cplx acc = finish_in_wave(partial + (int64_t)blockIdx.x * RED_BLOCKS, count);
    if (threadIdx.x == 0) { if (mode == 1) acc = make_double2(sqrt(acc.x), 0.0); out[blockIdx.x] = acc; }
}

// multi-dot for classical Gram-Schmidt: partial[j*RED_BLOCKS + b] = sum conj(V_j) * w for NC columns at once, so w is
// read once per group of NC columns instead of once per column
template <int NC>
__global__ __launch_bounds__(RED_THREADS) void k_multidot_partial(const cplx* __restrict__ V, int64_t ldv, int k, const cplx* __restrict__ w,
                                                                   cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    cplx acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx v = w[i];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            if (j < k) cdot_acc(acc[j], V[(int64_t)j * ldv + i], v);
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (j < k) {
            const cplx r = block_sum(acc[j], sh);
            if (threadIdx.x == 0) partial[(int64_t)j * RED_BLOCKS + blockIdx.x] = r;
            __syncthreads();
        }
    }
}

// ---- axpy + dot: one step of modified Gram-Schmidt -------------------------------------------------------------------
// On one device no all-reduce sits between a reduction and its consumer, so the finisher launches disappear: every block
// of the CONSUMING kernel sums the producer's block partials itself (<= 1024 values from L2, by finish_in_wave as the
// finisher does, so every block -- and the host -- sees bit-identical scalars), and block 0 publishes the scalar for the
// host.  A modified Gram-Schmidt sweep over k vectors is then k + 2 launches instead of 2k + 4, a classical one 3.

// w -= c * v, then partial[b] = sum conj(vnext) * w  (one pass over w), or of |w|^2 when vnext == NULL (the last step: the norm)
__device__ __forceinline__ void axpy_dot_body(cplx* __restrict__ w, const cplx* __restrict__ v, cplx c, const cplx* __restrict__ vnext,
                                              cplx* __restrict__ partial, int64_t n, cplx* sh) {
    cplx acc = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx q = v[i], x = csubmul(w[i], c, q);
        w[i] = x;
        if (vnext) cdot_acc(acc, vnext[i], x);
        else cnorm_acc(acc, x);
    }
    const cplx r = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// c = h[0], a device scalar
__global__ __launch_bounds__(RED_THREADS) void k_axpy_dot_partial(cplx* __restrict__ w, const cplx* __restrict__ v, const cplx* __restrict__ h,
                                                                   const cplx* __restrict__ vnext, cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    axpy_dot_body(w, v, *h, vnext, partial, n, sh);
}
// c = sum(hpartial[0..nb)); block 0: *hout = c
__global__ __launch_bounds__(RED_THREADS) void k_axpy_dot_fused(cplx* __restrict__ w, const cplx* __restrict__ v, const cplx* __restrict__ hpartial, int nb,
                                                                 cplx* __restrict__ hout, const cplx* __restrict__ vnext, cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    __shared__ cplx hs;
    if (threadIdx.x < 64) { const cplx h = finish_in_wave(hpartial, nb); if (threadIdx.x == 0) { hs = h; if (blockIdx.x == 0) *hout = h; } }
    __syncthreads();
    axpy_dot_body(w, v, hs, vnext, partial, n, sh);
}

// ---- gemv: classical Gram-Schmidt update, x += V y -----------------------------------------------------------------

// sum_j cs[j] * V_j[i], j < k (cs in LDS)
__device__ __forceinline__ cplx gemv_at(const cplx* __restrict__ V, int64_t ldv, int k, const cplx* cs, int64_t i) {
    cplx acc = make_double2(0.0, 0.0);
    for (int j = 0; j < k; ++j) cmul_acc(acc, cs[j], V[(int64_t)j * ldv + i]);
    return acc;
}

// y += sign * sum_j c[j] * V_j   (k <= 64 columns; coefficients in device memory)
__global__ void k_gemv_acc(cplx* __restrict__ y, const cplx* __restrict__ V, int64_t ldv, int k, const cplx* __restrict__ c, double sign, int64_t n) {
    __shared__ cplx cs[64];
    if (threadIdx.x < k) cs[threadIdx.x] = c[threadIdx.x];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx acc = gemv_at(V, ldv, k, cs, i);
        cplx v = y[i]; v.x = fma(sign, acc.x, v.x); v.y = fma(sign, acc.y, v.y); y[i] = v;
    }
}

// w -= V h with h_j = sum(hpartial[j*RED_BLOCKS + 0..nb)), j < k <= 64; partial[b] = |w|^2 slice; block 0: hout[j] = h_j
__global__ __launch_bounds__(RED_THREADS) void k_cgs_update_fused(cplx* __restrict__ w, const cplx* __restrict__ V, int64_t ldv, int k,
                                                                   const cplx* __restrict__ hpartial, int nb, cplx* __restrict__ hout,
                                                                   cplx* __restrict__ partial, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    __shared__ cplx cs[64];
    for (int j = threadIdx.x >> 6; j < k; j += RED_THREADS / 64) {
        const cplx h = finish_in_wave(hpartial + (int64_t)j * RED_BLOCKS, nb);
        if ((threadIdx.x & 63) == 0) { cs[j] = h; if (blockIdx.x == 0) hout[j] = h; }
    }
    __syncthreads();
    cplx nrm = make_double2(0.0, 0.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const cplx acc = gemv_at(V, ldv, k, cs, i);
        cplx x = w[i]; x.x -= acc.x; x.y -= acc.y; w[i] = x;
        cnorm_acc(nrm, x);
    }
    const cplx r = block_sum(nrm, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// ---- element-wise ------------------------------------------------------------------------------------------------------

// y = a - b
__global__ void k_sub(cplx* __restrict__ y, const cplx* __restrict__ a, const cplx* __restrict__ b, int64_t n) { sub_slice(y, a, b, n); }

// a *= inv
__device__ __forceinline__ void scale_body(cplx* __restrict__ a, double inv, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        cplx v = a[i]; a[i] = make_double2(v.x * inv, v.y * inv);
    }
}
// a *= 1 / s[0].x   (s on the device: no host round trip between the norm and the scaling)
__global__ void k_scale_inv_dev(cplx* __restrict__ a, const cplx* __restrict__ s, int64_t n) { scale_body(a, 1.0 / s->x, n); }
// a *= 1 / sqrt(sum(npartial[0..nb)).x); block 0: *nout = (norm, 0)
__global__ __launch_bounds__(RED_THREADS) void k_scale_inv_fused(cplx* __restrict__ a, const cplx* __restrict__ npartial, int nb, cplx* __restrict__ nout, int64_t n) {
    __shared__ double ns;
    if (threadIdx.x < 64) { const cplx s2 = finish_in_wave(npartial, nb); if (threadIdx.x == 0) { ns = sqrt(s2.x); if (blockIdx.x == 0) *nout = make_double2(ns, 0.0); } }
    __syncthreads();
    scale_body(a, 1.0 / ns, n);
}

__global__ void k_sqrt_dev(cplx* s) { if (threadIdx.x == 0) *s = make_double2(sqrt(s->x), 0.0); }

// ---- blocked modified Gram-Schmidt -----------------------------------------------------------------------------------
// Modified Gram-Schmidt in blocks of MB basis vectors (large vectors: the sweep is pure HBM traffic).  Strict MGS takes the
// inner product with v_{i+1} only after w has been updated with v_i: four passes over N-vectors per basis vector (read w, v_i,
// v_{i+1}, write w).  But  <v_j, w - sum_{l<j} h_l v_l> = <v_j, w> - sum_{l<j} h_l <v_j, v_l>,  so ONE pass over w and the MB
// vectors of a block yields the MB inner products with the not-yet-updated w plus the MB (MB - 1) / 2 inner products of the
// block's vectors with each other (they cost no memory traffic: the vectors are in registers anyway), from which every
// workgroup of the next kernel recovers the MGS coefficients h_0 .. h_{MB-1} by the recurrence above -- the same numbers
// modified Gram-Schmidt produces, up to the order of rounding.  That kernel updates w with the whole block and, in the same
// pass, takes the inner products with the NEXT block (or |w|^2 after the last).  Passes per basis vector: 2 + 2 / MB (MB = 4:
// 2.5 instead of 4).  Partials: slot base + j (j < MB) = <v_j, w>, base + MB + pair(j, l) = <v_j, v_l> for l < j.
constexpr int MB = 4, MGS_PAIRS = MB * (MB - 1) / 2, MGS_SLOTS = MB + MGS_PAIRS;
__device__ __forceinline__ constexpr int mgs_pair(int j, int l) { return j * (j - 1) / 2 + l; }     // l < j
__global__ __launch_bounds__(RED_THREADS) void k_mgs_block(cplx* __restrict__ w, const cplx* __restrict__ Vp, int mp, const cplx* __restrict__ ppartial, int nb,
                                                            cplx* __restrict__ hout, const cplx* __restrict__ Vn, int mn, cplx* __restrict__ npartial,
                                                            int64_t ldv, int64_t n) {
    __shared__ cplx sh[RED_THREADS / 64];
    __shared__ cplx fin[MGS_SLOTS];
    __shared__ cplx hs[MB];
    if (mp > 0) {
        // (slots of a short block are numbered as those of a full one: pair(j, l) does not depend on mp)
        for (int q = threadIdx.x >> 6; q < MGS_SLOTS; q += RED_THREADS / 64) {
            const bool used = q < mp || (q >= MB && q - MB < mp * (mp - 1) / 2);
            if (used) { const cplx v = finish_in_wave(ppartial + (int64_t)q * RED_BLOCKS, nb); if ((threadIdx.x & 63) == 0) fin[q] = v; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            cplx h[MB];
            for (int j = 0; j < mp; ++j) {
                cplx a = fin[j];
                for (int l = 0; l < j; ++l) a = csubmul(a, h[l], fin[MB + mgs_pair(j, l)]);      // a -= h_l * <v_j, v_l>
                h[j] = a; hs[j] = a;
                if (blockIdx.x == 0) hout[j] = a;
            }
        }
        __syncthreads();
    }
    cplx c[MB];
#pragma unroll
    for (int j = 0; j < MB; ++j) c[j] = j < mp ? hs[j] : make_double2(0.0, 0.0);
    cplx ad[MB], ag[MGS_PAIRS];
#pragma unroll
    for (int j = 0; j < MB; ++j) ad[j] = make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < MGS_PAIRS; ++j) ag[j] = make_double2(0.0, 0.0);
    // two elements per thread and trip (i and i + stride): twice the loads in flight per wave
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    auto element = [&](int64_t i) {
        cplx x = w[i];
        if (mp > 0) {
#pragma unroll
            for (int j = 0; j < MB; ++j) {
                if (j < mp) x = csubmul(x, c[j], Vp[(int64_t)j * ldv + i]);
            }
            w[i] = x;
        }
        if (mn > 0) {
            cplx u[MB];
#pragma unroll
            for (int j = 0; j < MB; ++j) {
                if (j < mn) {
                    u[j] = Vn[(int64_t)j * ldv + i];
                    cdot_acc(ad[j], u[j], x);
#pragma unroll
                    for (int l = 0; l < j; ++l) cdot_acc(ag[mgs_pair(j, l)], u[j], u[l]);        // <v_j, v_l> = sum conj(v_j) v_l
                }
            }
        } else {
            cnorm_acc(ad[0], x);                                     // after the last block: |w|^2
        }
    };
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += 2 * stride) {
        element(i);
        if (i + stride < n) element(i + stride);
    }
#pragma unroll
    for (int q = 0; q < MGS_SLOTS; ++q) {
        const bool used = mn > 0 ? (q < mn || (q >= MB && q - MB < mn * (mn - 1) / 2)) : q == 0;
        if (used) {
            const cplx r = block_sum(q < MB ? ad[q] : ag[q - MB], sh);
            if (threadIdx.x == 0) npartial[(int64_t)q * RED_BLOCKS + blockIdx.x] = r;
            __syncthreads();
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

int blas_red_blocks(int64_t n) { return red_blocks(n); }
int blas_partial_slot() { return RED_BLOCKS; }
int blas_partial_count() { return RED_BLOCKS * 66; }   // 64 slots of a multidot + two more (norm partials, alternating slots of the fused sweeps)

// out[s] = the sum of slot s of `partial` (sqrt_re: its real part's square root), s < slots, for vectors of n entries
static void finish(const cplx* partial, int slots, cplx* out, int64_t n, bool sqrt_re, hipStream_t st) {
    hipLaunchKernelGGL(k_finish, dim3(slots), dim3(64), 0, st, partial, red_blocks(n), out, sqrt_re ? 1 : 0);
    LSFC_HIP(hipGetLastError());
}
// out.x = sqrt(sum partial[0..nb).x): the norm from its block partials (the DGKS test needs it on the host before scaling)
void blas_finish_norm(const cplx* partial, cplx* out, int64_t n, hipStream_t st) { finish(partial, 1, out, n, true, st); }

void blas_dot_partial(const cplx* a, const cplx* b, cplx* partial, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_dot_partial, dim3(red_blocks(n)), dim3(RED_THREADS), 0, st, a, b, partial, n);
    LSFC_HIP(hipGetLastError());
}
void blas_dot(const cplx* a, const cplx* b, cplx* partial, cplx* out, int64_t n, hipStream_t st) {
    blas_dot_partial(a, b, partial, n, st);
    finish(partial, 1, out, n, false, st);
}
void blas_nrm2(const cplx* a, cplx* partial, cplx* out, int64_t n, hipStream_t st, bool defer_sqrt) {
    blas_dot_partial(a, a, partial, n, st);
    finish(partial, 1, out, n, !defer_sqrt, st);
}
void blas_sqrt_dev(cplx* s, hipStream_t st) {
    hipLaunchKernelGGL(k_sqrt_dev, dim3(1), dim3(64), 0, st, s);
    LSFC_HIP(hipGetLastError());
}

void blas_axpy_dot(cplx* w, const cplx* v, const cplx* h, const cplx* vnext, cplx* partial, cplx* out, int64_t n, hipStream_t st, bool defer_sqrt) {
    hipLaunchKernelGGL(k_axpy_dot_partial, dim3(red_blocks(n)), dim3(RED_THREADS), 0, st, w, v, h, vnext, partial, n);
    finish(partial, 1, out, n, !(vnext || defer_sqrt), st);
}
void blas_axpy_dot_fused(cplx* w, const cplx* v, const cplx* hpartial, cplx* hout, const cplx* vnext, cplx* partial, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_axpy_dot_fused, dim3(red_blocks(n)), dim3(RED_THREADS), 0, st, w, v, hpartial, red_blocks(n), hout, vnext, partial, n);
    LSFC_HIP(hipGetLastError());
}

void blas_multidot_partial(const cplx* V, int64_t ldv, int k, const cplx* w, cplx* partial, int64_t n, hipStream_t st) {
    constexpr int NC = 8;
    const int nb = red_blocks(n);
    for (int j0 = 0; j0 < k; j0 += NC) {
        const int kc = k - j0 < NC ? k - j0 : NC;
        hipLaunchKernelGGL(k_multidot_partial<NC>, dim3(nb), dim3(RED_THREADS), 0, st, V + (int64_t)j0 * ldv, ldv, kc, w, partial + (int64_t)j0 * RED_BLOCKS, n);
    }
    LSFC_HIP(hipGetLastError());
}
void blas_multidot(const cplx* V, int64_t ldv, int k, const cplx* w, cplx* partial, cplx* out, int64_t n, hipStream_t st) {
    blas_multidot_partial(V, ldv, k, w, partial, n, st);
    finish(partial, k, out, n, false, st);
}

void blas_gemv_acc(cplx* y, const cplx* V, int64_t ldv, int k, const cplx* c, double sign, int64_t n, hipStream_t st) {
    LSFC_REQUIRE(k <= 64, "gemv_acc: at most 64 columns");
    hipLaunchKernelGGL(k_gemv_acc, dim3(grid_for(n)), dim3(256), 0, st, y, V, ldv, k, c, sign, n);
    LSFC_HIP(hipGetLastError());
}
void blas_cgs_update_fused(cplx* w, const cplx* V, int64_t ldv, int k, const cplx* hpartial, cplx* hout, cplx* npartial, int64_t n, hipStream_t st) {
    LSFC_REQUIRE(k <= 64, "cgs_update: at most 64 columns");
    hipLaunchKernelGGL(k_cgs_update_fused, dim3(red_blocks(n)), dim3(RED_THREADS), 0, st, w, V, ldv, k, hpartial, red_blocks(n), hout, npartial, n);
    LSFC_HIP(hipGetLastError());
}

void blas_sub(cplx* y, const cplx* a, const cplx* b, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_sub, dim3(grid_for(n)), dim3(256), 0, st, y, a, b, n);
    LSFC_HIP(hipGetLastError());
}
void blas_scale_inv_dev(cplx* a, const cplx* s, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_scale_inv_dev, dim3(grid_for(n)), dim3(256), 0, st, a, s, n);
    LSFC_HIP(hipGetLastError());
}
void blas_scale_inv_fused(cplx* a, const cplx* npartial, cplx* nout, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_scale_inv_fused, dim3(grid_for(n)), dim3(RED_THREADS), 0, st, a, npartial, red_blocks(n), nout, n);
    LSFC_HIP(hipGetLastError());
}

// one kernel of the blocked sweep: w -= Vp h (h from the partials `ppartial` of the previous kernel, published in hout; mp = 0:
// nothing to subtract, w is only read), then the partials of the inner products with the mn <= MB vectors Vn (mn = 0: of |w|^2,
// slot 0) into `npartial`; both partial areas hold blas_mgs_slots() slots
int blas_mgs_block_size() { return MB; }
int blas_mgs_slots() { return MGS_SLOTS; }
void blas_mgs_block(cplx* w, const cplx* Vp, int mp, const cplx* ppartial, cplx* hout, const cplx* Vn, int mn, cplx* npartial, int64_t ldv, int64_t n, hipStream_t st) {
    LSFC_REQUIRE(mp >= 0 && mp <= MB && mn >= 0 && mn <= MB, "mgs block: at most %d vectors per block", MB);
    hipLaunchKernelGGL(k_mgs_block, dim3(red_blocks(n)), dim3(RED_THREADS), 0, st, w, Vp, mp, ppartial, red_blocks(n), hout, Vn, mn, npartial, ldv, n);
    LSFC_HIP(hipGetLastError());
}

// loads this translation unit's code object on the current device (pruned.hip: pruned_warmup -- every code object of the library is
// resident before the first transfer or pass of a process exists; DESIGN 3, "The round-2 first-apply GPU fault")
__global__ void k_warmup_krylov_blas(int* p) { if (p) *p = 0; }
void warmup_krylov_blas() {
    hipLaunchKernelGGL(k_warmup_krylov_blas, dim3(1), dim3(64), 0, 0, (int*)nullptr);
    LSFC_HIP(hipGetLastError());
}

} // namespace lsfc
