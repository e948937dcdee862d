// Host-side interface of the block-tridiagonal factorisation of Msp and the apply of Msp^{-1} from it, used by precond.hip.
//
// As, AG and Msp of the sparsifying preconditioner (src/preconditioner.jl:27-58; examples/example3D.jl:57-68) carry the
// full 9-point / 27-point stencil of an n x m (x l) grid, x fastest.  With the slowest axis as block index Msp is
// block tridiagonal: K blocks of b = N / K rows, diagonal blocks D_k, couplings L_k (block k to k-1), U_k (k to k+1).
// Exact block elimination
//     S_0 = D_0,   S_k = D_k - L_k S_{k-1}^{-1} U_{k-1}
//     forward   z_k = S_k^{-1} (w_k - L_k z_{k-1})
//     backward  x_{K-1} = z_{K-1},   x_k = z_k - S_k^{-1} (U_k x_{k+1})
// with the explicit inverses S_k^{-1} stored dense (column-major, K b^2 16 B).  The reference has UMFPACK's lu(Msp) here.
//
// blocktri_factor.hip computes the inverses, once per object; blocktri_sweep.hip runs the two sweeps, 2 K - 1 steps per
// apply; blocktri_object.hpp is the object the two share.
#pragma once
#include "common.hpp"

namespace lsfc {

struct BlockTri;       // K explicit inverses S_k^{-1} (b x b, column-major) and a private copy of the CSR of Msp

// how the inverses are stored (LSFC_PRECOND_INV_F64 / _F32 of include/lsfc.h): complex double, or interleaved float pairs
// rounded once from the fp64 block; the elimination itself is fp64 either way
static constexpr int BLOCKTRI_INV_F64 = 0, BLOCKTRI_INV_F32 = 1;

// pivoting inside the Schur blocks (LSFC_PRECOND_PIVOT_* of include/lsfc.h): none; partial row pivoting in every block;
// without first and, if that breaks down, the whole factorisation again with partial pivoting
static constexpr int BLOCKTRI_PIVOT_NONE = 0, BLOCKTRI_PIVOT_PARTIAL = 1, BLOCKTRI_PIVOT_AUTO = 2;

struct BlockTriInfo {
    int64_t K, b, factor_bytes, launches, factor_us;
    int pivoting;
    double min_pivot_ratio;
};

// |pivot| / max|S_k| below which the inversion of a Schur block is refused, with or without pivoting (include/lsfc.h)
static constexpr double BLOCKTRI_PIVOT_MIN = 1e-8;

// LSFC_ENOMEM unless K b^2 16 B (8 B at float storage) of factors plus the work space fit into the free memory of the
// current device; `extra` = bytes the caller is about to allocate besides.  From the dimensions, the precision and the
// pivoting mode alone: nothing is allocated or read.  blocktri_memory_need is the arithmetic of it.
struct BlockTriNeed { double inverse_bytes, work_bytes; };
BlockTriNeed blocktri_memory_need(int64_t N, int64_t K, int prec, int pivoting = BLOCKTRI_PIVOT_NONE);
void blocktri_require_memory(int64_t N, int64_t K, double extra, const char* who, int prec, int pivoting = BLOCKTRI_PIVOT_NONE);
// Factorise: rowptr / col / msp are DEVICE arrays (CSR, 0-based, columns ascending, N rows).  Synchronous.
BlockTri* blocktri_factor(int64_t N, int64_t K, const int64_t* rowptr, const int64_t* col, const cplx* msp, int prec, int pivoting = BLOCKTRI_PIVOT_NONE);
int blocktri_precision(const BlockTri*);
void blocktri_destroy(BlockTri*);
const int* blocktri_col32(const BlockTri*);          // the columns as 32-bit integers (device), nnz of them
int64_t blocktri_nnz(const BlockTri*);
// The tables of the transposed apply: the CSR of Msp^T split at the block boundaries (kept inside), and for the caller's
// SpMV its row pointers and columns with the values of As^T on that pattern (as_val: As on the pattern of Msp, device).
// Built on the first call (synchronous, allocates: not inside a stream capture), returned as they are from then on.
struct BlockTriT { const int64_t* rowptr; const int* col; const cplx* as_val; int64_t bytes; };
BlockTriT blocktri_transpose_tables(BlockTri*, const cplx* as_val);
// x <- Msp^{-1} w (device vectors of N, w != x), enqueued on st as a single chain of launches; `transposed`: x <- Msp^{-T} w
// from the same inverses (after blocktri_transpose_tables)
void blocktri_enqueue(const BlockTri*, const cplx* w, cplx* x, hipStream_t st, bool transposed = false);
// The same for a group of R <= 8 right-hand sides, member r at w + r N and x + r N: every S_k^{-1} is read once per group.
// The bits of a member's result do not depend on R or on r.  blocktri_batch_reserve(bt, R) first (it allocates: not
// inside a stream capture); it returns the bytes of the group work space.
int64_t blocktri_batch_reserve(BlockTri*, int R);
void blocktri_enqueue_batch(const BlockTri*, int R, const cplx* w, cplx* x, hipStream_t st, bool transposed = false);
BlockTriInfo blocktri_info(const BlockTri*);
void blocktri_get_block(const BlockTri*, int64_t k, cplx* host_out);  // the stored block, widened to double at float storage
// perm[i] = row of S_k that became pivot row i, b entries to the host (the identity on an object factorised without pivoting)
void blocktri_get_pivots(const BlockTri*, int64_t k, int64_t* host_out);
void warmup_blocktri();

} // namespace lsfc
