// Host-side interface of the level-scheduled sparse triangular solve (trisolve.hip), used by precond.hip.
#pragma once
#include "common.hpp"

namespace lsfc {

// One lane's share of a CSR row: (sx, sy) += sum of val[e] x[col[e]] over e = e0, e0 + stride, ... < e1, in that order.
// The one row sum of the library's sparse kernels (the solves of trisolve.hip, the SpMV of precond.hip); UNROLL = 1 where
// rows are short and many are in flight (a few lanes per row), 4 where a workgroup streams one long row.
template <int UNROLL>
__device__ __forceinline__ void csr_row_sum(int64_t e0, int64_t e1, int stride, const int* __restrict__ col, const cplx* __restrict__ val,
                                            const cplx* x, double& sx, double& sy) {
#pragma unroll UNROLL
    for (int64_t e = e0; e < e1; e += stride) {
        const cplx a = val[e], v = x[col[e]];
        sx += a.x * v.x - a.y * v.y; sy += a.x * v.y + a.y * v.x;
    }
}

struct TriFactor;      // one triangular factor on the device, rows in level order, with its launch schedule

// From HOST CSR (0-based, N rows, the diagonal stored, every other entry below it for `lower`, above it otherwise).
// Synchronous; LSFC_EINVAL on an entry on the wrong side, a column out of range or a zero or missing diagonal.
TriFactor* trisolve_build(int64_t N, const int64_t* rowptr, const int64_t* col, const double* val, bool lower);
void trisolve_destroy(TriFactor*);
// x <- F^{-1} b (device vectors of N, b != x), enqueued on st as a single chain of trisolve_launches(F) launches
void trisolve_enqueue(const TriFactor*, const cplx* b, cplx* x, hipStream_t st);
int trisolve_levels(const TriFactor*);               // depth of the dependency graph
int trisolve_launches(const TriFactor*);
const int64_t* trisolve_schedule(const TriFactor*);  // the ten counts of lsfc_precond_schedule (include/lsfc.h)
void warmup_trisolve();

} // namespace lsfc
