// What the two halves of the block-tridiagonal preconditioner share: the object that blocktri_factor.hip builds and
// blocktri_sweep.hip applies.  Included by those two files only; everyone else sees blocktri.hpp.
#pragma once
#include "blocktri.hpp"

namespace lsfc {

typedef float2 cplx32;             // a stored entry of S_k^{-1} at float storage

__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ void cfma(cplx& s, cplx a, cplx b) { s.x += a.x * b.x - a.y * b.y; s.y += a.x * b.y + a.y * b.x; }

static inline unsigned nblk(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct BtApply {                   // what the sweep kernels read
    int64_t b; int K;
    const int64_t* rowptr; const int64_t* rlo; const int64_t* rhi; const int* col; const cplx* val;
};

struct BlockTri {
    int64_t N = 0, K = 0, b = 0, nnz = 0;
    DevBuf<int64_t> rowptr, rlo, rhi; DevBuf<int> col; DevBuf<cplx> val;     // private CSR of Msp, split at the block boundaries
    int prec = BLOCKTRI_INV_F64;
    DevBuf<cplx> S;                                                          // S_k^{-1}, k = 0 .. K-1 (fp64 storage) ...
    DevBuf<cplx32> S32;                                                      // ... or the same blocks rounded to float pairs
    int64_t factor_us = 0; double min_ratio = 0.0;
    bool pivoted = false; DevBuf<int> perm;                                  // partial pivoting: perm[k b + i] = row of S_k that became pivot row i
    DevBuf<cplx> bt_t, bt_part; int batch_cap = 0;                           // group apply: stencil products (b x R), partial sums (ranges x R x b)
    // the transposed apply (blocktri_transpose_tables, on first use): CSR of Msp^T split at the block boundaries as the one
    // above is, and the values of As^T on the same pattern
    DevBuf<int64_t> t_rowptr, t_rlo, t_rhi; DevBuf<int> t_col; DevBuf<cplx> t_val, t_as; bool has_t = false;
    BtApply tables(bool transposed) const {
        if (transposed) return BtApply{b, (int)K, t_rowptr.p, t_rlo.p, t_rhi.p, t_col.p, t_val.p};
        return BtApply{b, (int)K, rowptr.p, rlo.p, rhi.p, col.p, val.p};
    }
};

int blocktri_sweep_launches(const BlockTri*);      // launches of one apply (blocktri_sweep.hip: it knows the walk threshold)
// one empty kernel of each unit: warmup_blocktri (blocktri_factor.hip) loads both code objects
void warmup_blocktri_factor();
void warmup_blocktri_sweep();

} // namespace lsfc
