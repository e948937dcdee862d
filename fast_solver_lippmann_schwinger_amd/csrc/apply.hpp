// What the drivers outside apply.hip need from it: the passes of the pruned pipeline on a slab of planes (host_apply.hip), the
// fused pass on a chunk of the x' range (dist.hip), the groups of a batch, and the way in for host vectors.  Include plan.hpp first.
#pragma once
#include "pruned.hpp"
#include <algorithm>

struct lsfc_plan;

namespace lsfc {

struct ConvOp;

// The passes of the single-device pruned pipeline: xfwd -> yfwd -> fused z -> yinv -> xinv in 3D, xfwd -> fused y -> xinv
// in 2D (natural rows, or tiles: lsfc_plan::tile2d).  Every driver -- device vectors, batches, the chunked host-vector
// pipeline, the per-stage profile -- issues these and nothing else.  A one-member launch gets the batch strides a1_elems /
// a2_elems like any other (the kernels only multiply them by the member index).
struct Slab { int z0, nz; };            // z planes [z0, z0 + nz) of the grid: the x and y passes work plane by plane
void pass_xfwd(lsfc_plan* p, const VecBatch& vb, int nrhs, const ConvOp& op, Slab s, hipStream_t st);
void pass_yfwd(lsfc_plan* p, int nrhs, Slab s, hipStream_t st);         // 3D only
void pass_fused(lsfc_plan* p, int nrhs, hipStream_t st);                // needs every plane
void pass_yinv(lsfc_plan* p, int nrhs, Slab s, hipStream_t st);         // 3D only
void pass_xinv(lsfc_plan* p, const VecBatch& vb, int nrhs, const ConvOp& op, Slab s, hipStream_t st);

// The fused z pass of the 3D tiled layout on `Wc` x' storage indices, starting at the tile that the offsets into A2 and
// the symbol point to (the whole range on one device; dist.hip: one chunk of the owned range)
void plan_zfused_3d(lsfc_plan* p, int Wc, int64_t a2_off, int64_t sym_off, int nrhs, hipStream_t st);

// cnt <= LSFC_MAX_BATCH vectors of N complex back to back
inline VecBatch vec_batch(const cplx* x, cplx* y, int64_t N, int cnt) {
    VecBatch vb{};
    for (int j = 0; j < cnt; ++j) { vb.x[j] = x + j * N; vb.y[j] = y + j * N; }
    return vb;
}
// nrhs vectors in groups of at most LSFC_MAX_BATCH, which share one pass of the pipeline (one symbol read per group):
// f(index of the group's first vector, its members, their vectors).  The vectors back to back ...
template <class F> void for_each_group(int64_t nrhs, const cplx* x, cplx* y, int64_t N, F&& f) {
    for (int64_t j0 = 0; j0 < nrhs; j0 += LSFC_MAX_BATCH) {
        const int cnt = (int)std::min<int64_t>(LSFC_MAX_BATCH, nrhs - j0);
        f(j0, cnt, vec_batch(x + j0 * N, y + j0 * N, N, cnt));
    }
}
// ... or as pointer lists
template <class F> void for_each_group(int64_t nrhs, const cplx* const* in, cplx* const* out, F&& f) {
    for (int64_t j0 = 0; j0 < nrhs; j0 += LSFC_MAX_BATCH) {
        const int cnt = (int)std::min<int64_t>(LSFC_MAX_BATCH, nrhs - j0);
        VecBatch vb{};
        for (int j = 0; j < cnt; ++j) { vb.x[j] = in[j0 + j]; vb.y[j] = out[j0 + j]; }
        f(j0, cnt, vb);
    }
}

// nrhs HOST vectors back to back through the plan, synchronous (host_apply.hip): the chunked pipeline for large 3D vectors,
// one staged copy each way otherwise, scatter / gather over the ranks of a multi-device plan
void host_convolve(lsfc_plan* p, const cplx* x, cplx* y, int64_t nrhs, const ConvOp& op);

} // namespace lsfc
