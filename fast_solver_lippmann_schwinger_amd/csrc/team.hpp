// A team of slabs: what the Krylov solvers, the host-vector apply and the per-stage profile share when a vector lives in pieces.
// An ordinary plan (or one rank of a multi-process plan) is a team of one slab, the whole vector; a single-process
// multi-device plan is its P z slabs, one per rank, all driven from the calling thread.  (dist.hip)
#pragma once
#include "plan.hpp"
#include <vector>

namespace lsfc {

// (RankSlab: apply.hpp has a Slab already, the z planes of one pass)
struct RankSlab {
    lsfc_plan* p; int device, rank;         // the plan or sub-plan that owns the slab; rank = its position in the team
    int64_t n, off;                         // entries of the slab and its place in the whole vector
    hipStream_t st() const { return p->stream; }
};

struct SlabTeam {
    lsfc_plan* root;
    std::vector<RankSlab> slabs;
    bool multi;                             // P slabs on their own devices: `each` makes the slab's device current
    explicit SlabTeam(lsfc_plan* root);
    int size() const { return (int)slabs.size(); }

    template <class F> void each(F&& f) const {
        for (const RankSlab& s : slabs) { if (multi) LSFC_HIP(hipSetDevice(s.device)); f(s); }
    }
    void sync() const { each([](const RankSlab& s) { LSFC_HIP(hipStreamSynchronize(s.st())); }); }
    // the operator (plan_operator) on one device vector per slab, stream-ordered
    void apply(const cplx* const* in, cplx* const* out) const;
    // The slabs of host vectors into the staging buffers of their plans (plan_ensure_staging): x -> xs, and b -> ys unless NULL.
    // Stream-ordered copies; gather copies the slabs of xs (or of ys) back.  Neither synchronises.
    void scatter(const cplx* x, const cplx* b) const;
    void gather(cplx* x, bool from_ys = false) const;
    // A host preconditioner callback, in place on the whole vector (the two-argument ldiv!): the slabs v(slab) gathered into
    // the pinned vector, every stream synchronised, the call, its return code checked, the slabs scattered back
    template <class V> void host_precond(const Precond& pc, cplx* pinned, V&& v) const {
        each([&](const RankSlab& s) { LSFC_HIP(hipMemcpyAsync(pinned + s.off, v(s), (size_t)s.n * sizeof(cplx), hipMemcpyDeviceToHost, s.st())); });
        sync();
        const int rc = pc.fn(pc.user, (double*)pinned, root->N);
        if (rc != 0) fail(LSFC_EINVAL, "preconditioner callback returned %d", rc);
        each([&](const RankSlab& s) { LSFC_HIP(hipMemcpyAsync(v(s), pinned + s.off, (size_t)s.n * sizeof(cplx), hipMemcpyHostToDevice, s.st())); });
    }
};

} // namespace lsfc
