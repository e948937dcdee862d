"""The transposed and the adjoint operator (M.T, M.H) against M on one MI355X, appended to profiles/adjoint_apply.jsonl
(one JSON line per measurement).

  apply [SIZE ...]   device tensors, HIP-event time of `reps` applies through time_apply.  Every shape is warmed up first; then
                     N, T and H are measured alternated, three rounds; each gets its best time and its spread (max / min - 1).
                     The N-to-N spread of the same run is the yardstick the T/N and H/N ratios are read against.  One
                     profile_apply per op (per-stage ms and algorithmic bytes) goes into the same record.
                     SIZE: 48, 256, 512 (3D cubes, buildFastConvolution3D) or 2d1024 (2D, Greengard-Vico); default all four.
  gmres [N]          GMRES(30) to reltol 1e-6 on M and on M.H at N^3 (default 256), plane-wave right-hand side, same process,
                     alternated over three repetitions after a one-step solve of each.
usage: python tools/bench_adjoint.py apply 48 256 512 2d1024 | gmres 256"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402
from tools.bench_configs import bump  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "adjoint_apply.jsonl")
ROUNDS = 3


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def operator(size):
    """-> (M, number of points, reps of one timing)"""
    if size == "2d1024":
        n = 1024
        h = 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        return lsfc.buildFastConvolution(x, x, h, 1.0 / h, lambda X, Y: bump(X, Y), quadRule="Greengard_Vico"), n * n, 200
    n = int(size)
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    nu = (bump(x)[None, None, :] / 0.3 * bump(x)[None, :, None] / 0.3 * bump(x)[:, None, None]).ravel()   # separable: no N-sized temporaries
    return lsfc.buildFastConvolution3D(x, x, x, None, None, None, h, 1.0 / h, nu), n ** 3, {48: 500, 256: 40}.get(n, 20)


def views(M):
    return {"N": M, "T": M.T, "H": M.H}


def apply(size):
    M, N, reps = operator(size)
    xb = torch.randn(N, dtype=torch.complex128, device="cuda")
    yb = torch.empty_like(xb)
    V = views(M)
    defect = M.symmetry_defect()
    for v in V.values():                                   # warm-up of every shape (code objects, clocks, the probe of the check)
        lsfc.time_apply(v, xb, yb, max(2, reps // 4))
    ms = {w: [] for w in V}
    for _ in range(ROUNDS):                                # alternated
        for w, v in V.items():
            ms[w].append(lsfc.time_apply(v, xb, yb, reps) / reps)
    best = {w: min(t) for w, t in ms.items()}
    stages = {w: [(name, round(t, 4), b) for name, t, b in lsfc.profile_apply(v, xb, yb, 5)] for w, v in V.items()}
    emit({"mode": "apply", "size": size, "N": N, "pipeline": M.pipeline, "reps": reps, "rounds": ROUNDS, "symmetry_defect": defect,
          "ms_per_apply": ms, "best_ms": best, "spread": {w: max(t) / min(t) - 1 for w, t in ms.items()},
          "T_over_N": best["T"] / best["N"], "H_over_N": best["H"] / best["N"],
          "Gpts_per_s": {w: N / best[w] / 1e6 for w in best}, "stages": stages})
    M.close()


def gmres(n, restart=30, reltol=1e-6):
    M, N, _ = operator(str(n))
    k = float(n)
    x = -0.5 + np.arange(n) / n
    u_inc = torch.exp(1j * k * torch.from_numpy(x).cuda()).repeat(n * n)        # exp(i k X), x fastest
    rhs = M * u_inc
    rhs.sub_(u_inc).neg_()
    del u_inc
    V = {"N": M, "H": M.H}
    for v in V.values():                                   # the Krylov workspace is allocated on first use and kept
        lsfc.gmres_(torch.zeros_like(rhs), v, rhs, restart=restart, maxiter=1, reltol=reltol)
    sec, info = {w: [] for w in V}, {}
    for _ in range(ROUNDS):
        for w, v in V.items():
            torch.cuda.synchronize()
            t0 = time.time()
            u, h = lsfc.gmres_(torch.zeros_like(rhs), v, rhs, restart=restart, reltol=reltol, log=True)
            torch.cuda.synchronize()
            sec[w].append(time.time() - t0)
            res = float(torch.linalg.norm(v * u - rhs) / torch.linalg.norm(rhs))
            info[w] = {"iters": h.iters, "mvps": h.mvps, "converged": h.isconverged, "true_relres": res}
    emit({"mode": "gmres", "n": n, "N": N, "restart": restart, "reltol": reltol, "seconds": sec, "best_seconds": {w: min(t) for w, t in sec.items()},
          "spread": {w: max(t) / min(t) - 1 for w, t in sec.items()}, "solve": info,
          "ms_per_mvp": {w: 1e3 * min(sec[w]) / info[w]["mvps"] for w in V}})
    M.close()


if __name__ == "__main__":
    mode, args = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "apply":
        for s in args or ["48", "256", "512", "2d1024"]:
            apply(s)
            torch.cuda.empty_cache()
    elif mode == "gmres":
        gmres(int(args[0]) if args else 256)
    else:
        sys.exit(__doc__)
