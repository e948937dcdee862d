"""Timing of the device assembly of the sparsifying matrices (lsfc_sparsify_build) and of the routes around it.

For every case: the device build into device memory (kernels only, median of --reps after one warm build that also
creates the plan's spatial kernel), the build into host memory (kernels + download of the CSR arrays), the singular
value spread of the classes; where it fits, the route a Python user had before (rows through lsfc_sample_sources,
one numpy SVD per class); at 3D 48^3 the host LU of Msp (scipy splu, in a child process under a time limit).
One JSON line per measurement on stdout and appended to --out.

    python tools/bench_sparsify.py --out profiles/sparsify_timing.jsonl

--factor: the preconditioner factorised on the device instead (SparsifyingPreconditioner.from_operator: assembly plus
block-tridiagonal factorisation, csrc/blocktri_factor.hip) -- set-up time, time per apply beside its byte floor
2 K b^2 16 B / 6.29 TB/s, and, where scipy's splu of the same Msp is affordable (2D, 3D up to 24^3), the host-LU route
with its level-scheduled apply on the same pair.

    python tools/bench_sparsify.py --factor --out profiles/precond_blocktri.jsonl

--nrhs R[,R...]: the device-factorised preconditioner applied to R right-hand sides at once (ldiv_batch_: one group sweep
that reads every S_k^{-1} once) against R single applies of the same object in the same process, with the rate the
batched time implies on the byte model 2 K b^2 16 B per group.  --gmres adds, for the largest R, a preconditioned
gmres_batch_ of R incident directions against R back-to-back gmres_ calls with the same object.

    python tools/bench_sparsify.py --nrhs 1,2,4,8 --gmres --out profiles/precond_batch.jsonl

--inverse-dtype complex128[,complex64] (with --nrhs): the same rows once per storage of the inverses, both objects timed
in one process; the byte model is 2 K b^2 times the bytes of a stored entry, and every row also has the factorisation
time of its object and the spread (min, max) of the timed single applies.

    python tools/bench_sparsify.py --inverse-dtype complex128,complex64 --nrhs 1,8 --out profiles/precond_f32.jsonl

--pivoting none,partial: the factorisation (from_operator, fp64 storage) once per pivoting mode in one process: after a
warm-up object per mode, --reps objects each; median, minimum and maximum of the factorisation time the library reports
(factor_us: pattern, Schur updates and inversions, no assembly) and of the apply time of the last object.

    python tools/bench_sparsify.py --pivoting none,partial --out profiles/precond_pivot.jsonl"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def operator(ndim, n):
    import fast_solver_lippmann_schwinger_amd as pkg
    if ndim == 2:                                          # examples/example.jl: h = 1/(n-1), k = 1/h, trapezoidal
        h = 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        nu = lambda X, Y: 0.3 * np.exp(-40 * (X ** 2 + Y ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48)   # noqa: E731
        return pkg.buildFastConvolution(x, x, h, 1.0 / h, nu, quadRule="trapezoidal")
    h = 1.0 / n                                            # examples/example3D.jl: h = 1/n, k = 1/h, Greengard-Vico
    x = -0.5 + h * np.arange(n)
    X, Y, Z = (a.reshape(-1, order="F") for a in np.meshgrid(x, x, x, indexing="ij"))
    nu = 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48)
    return pkg.buildFastConvolution3D(x, x, x, None, None, None, h, 1.0 / h, nu)


def device_build(M, nnz, N, nclass, reps):
    import ctypes as C
    import torch
    import fast_solver_lippmann_schwinger_amd._lib as L
    t = [torch.empty(N + 1, dtype=torch.int64, device="cuda"), torch.empty(nnz, dtype=torch.int64, device="cuda"),
         torch.empty(nnz, dtype=torch.complex128, device="cuda"), torch.empty(nnz, dtype=torch.complex128, device="cuda"),
         torch.empty(nnz, dtype=torch.complex128, device="cuda"), torch.empty(nclass * 3, dtype=torch.float64, device="cuda")]
    p = [C.c_void_p(v.data_ptr()) for v in t]
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(L.load().lsfc_sparsify_build(M._plan, *p, L.LSFC_MEM_DEVICE))
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    del t
    torch.cuda.empty_cache()
    return ms


def host_build(M, reps, values):
    import fast_solver_lippmann_schwinger_amd as pkg
    ms, a = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        a = pkg.sparsify_arrays(M, values)
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, a


def user_route(M, ndim, n):
    """rows via lsfc_sample_sources, then one numpy SVD per class (the assembly a user could write before)"""
    import fast_solver_lippmann_schwinger_amd as pkg
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sparsify_ref as ref
    dims = (n, n, 1) if ndim == 2 else (n, n, n)
    N = int(np.prod(dims))
    t0 = time.perf_counter()
    for sA, _, _, _ in ref.classes(*dims):
        S = np.asarray(sA) - 1
        R = pkg.sampleG3D(0, None, None, None, S, M) if ndim == 3 else _rows2d(M, S)
        comp = np.ones(N, bool)
        comp[S] = False
        np.linalg.svd(R[:, comp], full_matrices=False)
    return 1e3 * (time.perf_counter() - t0)


def _rows2d(M, S):
    import ctypes as C
    import fast_solver_lippmann_schwinger_amd._lib as L
    out = np.empty((len(S), M.N), dtype=np.complex128)
    src = np.ascontiguousarray(S, dtype=np.int64)
    L.check(L.load().lsfc_sample_sources(M._plan, src.ctypes.data_as(C.c_void_p), len(S), out.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
    return out


SPLU_CHILD = r"""
import sys, time, numpy as np, scipy.sparse as sp, scipy.sparse.linalg as spla
d = np.load(sys.argv[1])
N = d["rowptr"].size - 1
A = sp.csr_matrix((d["val"], d["col"], d["rowptr"]), shape=(N, N)).tocsc()
t0 = time.perf_counter()
lu = spla.splu(A)
print((time.perf_counter() - t0) * 1e3, lu.L.nnz + lu.U.nnz)
"""


def splu_time(a, limit, tmpdir):
    path = os.path.join(tmpdir, "msp_csr.npz")
    np.savez(path, rowptr=a["rowptr"], col=a["col"], val=a["Msp"])
    try:
        r = subprocess.run([sys.executable, "-c", SPLU_CHILD, path], capture_output=True, text=True, timeout=limit)
        ms, fill = r.stdout.split()
        return {"splu_ms": float(ms), "lu_nnz": int(fill)}
    except subprocess.TimeoutExpired:
        return {"splu_ms": None, "note": f"splu did not finish within {limit} s"}
    finally:
        os.remove(path)


def apply_ms(P, N, reps=20):
    import torch
    v = torch.from_numpy(np.random.default_rng(0).standard_normal(N) + 0j).cuda()
    P.ldiv_(v)                                             # captures the graph
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        P.ldiv_(v)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def factor_mode(args):
    import scipy.sparse.linalg as spla
    import torch
    import fast_solver_lippmann_schwinger_amd as pkg
    for spec in args.cases.split(","):
        ndim, n = (int(v) for v in spec.split(":"))
        N = n ** ndim
        M = operator(ndim, n)
        pkg.sparsify_arrays(M, ("As",))                    # warm: the plan's spatial kernel
        t0 = time.perf_counter()
        P = pkg.SparsifyingPreconditioner.from_operator(M)
        setup = time.perf_counter() - t0
        st = P.stats()
        floor_ms = 1e3 * 2 * st["factor_bytes"] / 6.29e12
        rec = {"case": f"{ndim}D n={n}", "N": N, "blocks": st["blocks"], "block_size": st["block_size"],
               "factor_GB": round(st["factor_bytes"] / 1e9, 3), "assembly_plus_factor_s": round(setup, 4),
               "factor_s": round(st["factor_us"] / 1e6, 4), "min_pivot_ratio": round(st["min_pivot_ratio"], 4),
               "launches": st["launches"], "apply_ms": round(apply_ms(P, N), 4), "apply_floor_ms": round(floor_ms, 4)}
        if ndim == 2 or n <= 24:
            Msp, As = pkg.sparsifying_pair(M)
            t0 = time.perf_counter()
            lu = spla.splu(Msp)
            rec["host_splu_s"] = round(time.perf_counter() - t0, 3)
            Ph = pkg.SparsifyingPreconditioner(Msp, As, lu=lu)
            rec["host_route_apply_ms"] = round(apply_ms(Ph, N), 4)
            rec["host_route_launches"] = Ph.stats()["launches"]
            b = np.random.default_rng(1).standard_normal(N) + 1j * np.random.default_rng(2).standard_normal(N)
            xh = Ph.solve(b)
            rec["rel_diff_to_host_route"] = float(np.linalg.norm(P.solve(b) - xh) / np.linalg.norm(xh))
            Ph.close()
        emit(args.out, rec)
        P.close()
        del M
        torch.cuda.empty_cache()


def pivoting_mode(args):
    import torch
    import fast_solver_lippmann_schwinger_amd as pkg
    modes = args.pivoting.split(",")
    for spec in args.cases.split(","):
        ndim, n = (int(v) for v in spec.split(":"))
        N = n ** ndim
        M = operator(ndim, n)
        pkg.sparsify_arrays(M, ("As",))                    # warm: the plan's spatial kernel
        for mode in modes:                                 # warm-up: one object per mode
            pkg.SparsifyingPreconditioner.from_operator(M, pivoting=mode).close()
        for mode in modes:
            factor_s, P = [], None
            for _ in range(args.reps):
                if P is not None:
                    P.close()
                P = pkg.SparsifyingPreconditioner.from_operator(M, pivoting=mode)
                factor_s.append(P.stats()["factor_us"] / 1e6)
            st = P.stats()
            applies = [apply_ms(P, N) for _ in range(args.reps)]
            emit(args.out, {"case": f"{ndim}D n={n}", "N": N, "blocks": st["blocks"], "block_size": st["block_size"], "pivoting": mode,
                            "pivoted": st["pivoting"], "reps": args.reps, "factor_s_median": round(float(np.median(factor_s)), 4),
                            "factor_s_min_max": [round(min(factor_s), 4), round(max(factor_s), 4)],
                            "apply_ms_median": round(float(np.median(applies)), 4),
                            "apply_ms_min_max": [round(min(applies), 4), round(max(applies), 4)],
                            "min_pivot_ratio": round(st["min_pivot_ratio"], 4)})
            P.close()
        del M
        torch.cuda.empty_cache()


def timed_ms(fn, reps):
    import torch
    fn()                                                   # warm-up (captures the graph, allocates work buffers)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def median_ms(fn, reps):
    return float(np.median(timed_ms(fn, reps)))


def nrhs_rows(args, pkg, M, B, groups, name, inverse_dtype):
    """one row per group size for an object of the given storage; returns (object, its stats)"""
    N = B.shape[1]
    P = pkg.SparsifyingPreconditioner.from_operator(M, inverse_dtype=inverse_dtype)
    st = P.stats()
    single = timed_ms(lambda: P.ldiv_(B[0].clone()), args.reps)
    for R in groups:
        def singles():
            W = B[:R].clone()
            for j in range(R):
                P.ldiv_(W[j])
        batched_ms = median_ms(lambda: P.ldiv_batch_(B[:R].clone()), args.reps)
        singles_ms = median_ms(singles, args.reps)
        groups_of_8 = (R + 7) // 8
        emit(args.out, {"case": name, "N": N, "blocks": st["blocks"], "block_size": st["block_size"], "inverse_dtype": inverse_dtype,
                        "factor_GB": round(st["factor_bytes"] / 1e9, 3), "factor_s": round(st["factor_us"] / 1e6, 4), "nrhs": R,
                        "batched_ms": round(batched_ms, 4), "singles_ms": round(singles_ms, 4),
                        "single_apply_ms": round(float(np.median(single)), 4),
                        "single_apply_ms_min_max": [round(min(single), 4), round(max(single), 4)],
                        "single_apply_TBps": round(2 * st["factor_bytes"] / (float(np.median(single)) * 1e-3) / 1e12, 3),
                        "per_vector_ms": round(batched_ms / R, 4), "ratio_batched_over_singles": round(batched_ms / singles_ms, 4),
                        "model_GB": round(groups_of_8 * 2 * st["factor_bytes"] / 1e9, 3),
                        "implied_TBps": round(groups_of_8 * 2 * st["factor_bytes"] / (batched_ms * 1e-3) / 1e12, 3)})
    return P, st


def nrhs_mode(args):
    import torch
    import fast_solver_lippmann_schwinger_amd as pkg
    groups = [int(v) for v in args.nrhs.split(",")]
    for spec in args.cases.split(","):
        ndim, n = (int(v) for v in spec.split(":"))
        N = n ** ndim
        M = operator(ndim, n)
        rng = np.random.default_rng(0)
        B = torch.from_numpy(rng.standard_normal((max(groups), N)) + 1j * rng.standard_normal((max(groups), N))).cuda()
        for inverse_dtype in args.inverse_dtype.split(",")[:-1]:            # all but the last storage: apply rows only
            nrhs_rows(args, pkg, M, B, groups, f"{ndim}D n={n}", inverse_dtype)[0].close()
        P, st = nrhs_rows(args, pkg, M, B, groups, f"{ndim}D n={n}", args.inverse_dtype.split(",")[-1])
        if args.gmres:
            R = max(groups)
            h = 1.0 / (n - 1) if ndim == 2 else 1.0 / n
            k = 1.0 / h
            x = -0.5 + h * np.arange(n)
            grids = np.meshgrid(*(ndim * [x]), indexing="ij")
            X = [g.reshape(-1, order="F") for g in grids]
            rng = np.random.default_rng(1)
            RHS = []
            for _ in range(R):                             # R incident plane waves, random directions
                d = rng.standard_normal(ndim)
                d /= np.linalg.norm(d)
                u_inc = np.exp(1j * k * sum(di * Xi for di, Xi in zip(d, X)))
                RHS.append(-(M * u_inc - u_inc))
            RHS = np.ascontiguousarray(np.stack(RHS))
            t0 = time.perf_counter()
            _, hb = pkg.gmres_batch_(np.zeros_like(RHS), M, RHS, Pl=P, reltol=1e-6, log=True)
            tb = time.perf_counter() - t0
            t0 = time.perf_counter()
            hs = [pkg.gmres_(np.zeros(N, dtype=np.complex128), M, RHS[j], Pl=P, reltol=1e-6, log=True)[1] for j in range(R)]
            ts = time.perf_counter() - t0
            steps_b, steps_s = max(h.iters for h in hb), sum(h.iters for h in hs)
            emit(args.out, {"case": f"{ndim}D n={n}", "gmres_nrhs": R, "batch_s": round(tb, 4), "back_to_back_s": round(ts, 4),
                            "batch_iters": [h.iters for h in hb], "single_iters": [h.iters for h in hs],
                            "batch_ms_per_lockstep_step": round(1e3 * tb / steps_b, 3),
                            "single_ms_per_step": round(1e3 * ts / steps_s, 3), "batch_info": P.batch_info()})
        P.close()
        del M, B
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="2:201,3:48,3:128,3:256")
    ap.add_argument("--splu-limit", type=float, default=240.0)
    ap.add_argument("--device-only", action="store_true", help="only the device builds (for a kernel trace)")
    ap.add_argument("--factor", action="store_true", help="time the device-factorised preconditioner (see the module docstring)")
    ap.add_argument("--nrhs", default="", help="group sizes, e.g. 1,2,4,8: batched apply against single applies (see the module docstring)")
    ap.add_argument("--inverse-dtype", default="complex128", help="with --nrhs: storages of the inverses to time in one process, "
                    "complex128 and / or complex64, comma separated")
    ap.add_argument("--gmres", action="store_true", help="with --nrhs: also a preconditioned gmres_batch_ against back-to-back gmres_")
    ap.add_argument("--pivoting", default="", help="pivoting modes to time in one process, e.g. none,partial (see the module docstring)")
    args = ap.parse_args()
    if args.pivoting:
        if args.cases == ap.get_default("cases"):
            args.cases = "2:513,3:24,3:48"
        return pivoting_mode(args)
    if args.nrhs:
        if args.cases == ap.get_default("cases"):
            args.cases = "2:513,3:24,3:48,3:64"
        return nrhs_mode(args)
    if args.factor:
        if args.cases == ap.get_default("cases"):
            args.cases = "2:201,2:257,2:513,3:24,3:48,3:64"
        return factor_mode(args)
    import torch
    import fast_solver_lippmann_schwinger_amd as pkg
    for spec in args.cases.split(","):
        ndim, n = (int(v) for v in spec.split(":"))
        dims = (n, n, 1) if ndim == 2 else (n, n, n)
        N = int(np.prod(dims))
        nclass = 9 if ndim == 2 else 27
        M = operator(ndim, n)
        nnz = int(pkg.sparsify_pattern(*dims)[1].size) if N <= 200 ** 3 else (3 * n - 2) ** ndim
        first = device_build(M, nnz, N, nclass, 1)[0]               # includes the spatial kernel (one convolution)
        ms = device_build(M, nnz, N, nclass, args.reps)
        rec = {"case": f"{ndim}D n={n}", "N": N, "nnz": nnz, "first_build_ms": round(first, 3),
               "device_build_ms_median": round(float(np.median(ms)), 3), "device_build_ms_min": round(min(ms), 3)}
        csr_bytes = (N + 1) * 8 + nnz * 8 + 2 * nnz * 16
        if args.device_only:
            emit(args.out, rec)
            continue
        if csr_bytes < 40e9:
            hms, a = host_build(M, args.reps if N <= 128 ** 3 else 2, ("As", "Msp"))
            sig = a["sigma"]
            rec.update({"host_build_ms_median": round(float(np.median(hms)), 3), "host_csr_MB": round(csr_bytes / 1e6, 1),
                        "sigma_min_over_max": [float((sig[:, 2] / sig[:, 0]).min()), float((sig[:, 2] / sig[:, 0]).max())],
                        "sigma_gap_min": float((sig[:, 1] / sig[:, 2]).min())})
        else:
            a = None
        emit(args.out, rec)
        if N * 27 * 16 <= 4e9:
            emit(args.out, {"case": rec["case"], "user_route_sample_sources_numpy_svd_ms": round(user_route(M, ndim, n), 1)})
        if ndim == 3 and n == 48 and a is not None:
            emit(args.out, {"case": rec["case"], **splu_time(a, args.splu_limit, os.path.dirname(os.path.abspath(args.out or ".")))})
        del a, M
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
