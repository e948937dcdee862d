// Host-side interface of krylov_blas.hip: the BLAS-1 layer of the Krylov solvers.  Results land in device scalars;
// `partial` is scratch of blas_partial_count() entries, in slots of blas_partial_slot() entries.
#pragma once
#include "common.hpp"

namespace lsfc {

int  blas_partial_count();
void blas_dot(const cplx* a, const cplx* b, cplx* partial, cplx* out, int64_t n, hipStream_t);          // out = a' * b
// defer_sqrt: leave the sum of squares (to be all-reduced across ranks, then blas_sqrt_dev)
void blas_nrm2(const cplx* a, cplx* partial, cplx* out, int64_t n, hipStream_t, bool defer_sqrt = false);  // out.x = ||a||
void blas_sqrt_dev(cplx* s, hipStream_t);
// w -= h[0]*v ; then out = vnext' * w (vnext != NULL) or out.x = ||w|| (vnext == NULL)
void blas_axpy_dot(cplx* w, const cplx* v, const cplx* h, const cplx* vnext, cplx* partial, cplx* out, int64_t n, hipStream_t, bool defer_sqrt = false);
void blas_multidot(const cplx* V, int64_t ldv, int k, const cplx* w, cplx* partial, cplx* out, int64_t n, hipStream_t); // out[j] = V_j' * w
void blas_gemv_acc(cplx* y, const cplx* V, int64_t ldv, int k, const cplx* c, double sign, int64_t n, hipStream_t);      // y += sign * V c
void blas_sub(cplx* y, const cplx* a, const cplx* b, int64_t n, hipStream_t);
void blas_scale_inv_dev(cplx* a, const cplx* s, int64_t n, hipStream_t);                                   // a /= s[0].x
// fused single-device Gram-Schmidt steps: the consumer of a reduction sums the producer's block partials itself (no finisher
// launches); `partial` slots are blas_partial_slot() entries apart; block 0 publishes the scalars in hout / nout
int  blas_red_blocks(int64_t n);
int  blas_partial_slot();                       // entries between two slots of `partial`
void blas_finish_norm(const cplx* partial, cplx* out, int64_t n, hipStream_t);
void blas_dot_partial(const cplx* a, const cplx* b, cplx* partial, int64_t n, hipStream_t);
void blas_axpy_dot_fused(cplx* w, const cplx* v, const cplx* hpartial, cplx* hout, const cplx* vnext, cplx* partial, int64_t n, hipStream_t);
void blas_multidot_partial(const cplx* V, int64_t ldv, int k, const cplx* w, cplx* partial, int64_t n, hipStream_t);
void blas_cgs_update_fused(cplx* w, const cplx* V, int64_t ldv, int k, const cplx* hpartial, cplx* hout, cplx* npartial, int64_t n, hipStream_t);
void blas_scale_inv_fused(cplx* a, const cplx* npartial, cplx* nout, int64_t n, hipStream_t);
// modified Gram-Schmidt in blocks of blas_mgs_block_size() basis vectors (krylov_blas.hip: k_mgs_block): 2 + 2 / MB passes over
// N-vectors per basis vector instead of 4
int  blas_mgs_block_size();
int  blas_mgs_slots();                          // partial slots one kernel of the blocked sweep writes / reads
void blas_mgs_block(cplx* w, const cplx* Vp, int mp, const cplx* ppartial, cplx* hout, const cplx* Vn, int mn, cplx* npartial, int64_t ldv, int64_t n, hipStream_t);

} // namespace lsfc
