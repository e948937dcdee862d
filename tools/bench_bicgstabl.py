"""BiCGStab(l) against GMRES on one MI355X, appended to profiles/bicgstabl.jsonl (one JSON line per measurement).

  solve N [N ...]    the problem of BASELINE.json configs[2] (3D cube of N points per axis, plane-wave right-hand side,
                     examples/example3D.jl:71-78) to reltol 1e-6: mvps, cycles, wall time and peak device memory of
                     bicgstabl_ at l = 1, 2, 4 and of GMRES(30) in the same process
  largest [N ...]    cubes in ascending order (default 512 640 768 1024): one capped solve (8 operator applications) of
                     lsfc_bicgstabl(l = 1) and of GMRES(20) where each passes its memory check; stops at the first size where
                     neither fits.  GMRES has no check of its own for a single solve, so the tool applies its rule
                     ((restart + 2) vectors against the free memory) and does not call it otherwise: nothing is run into an
                     out-of-memory failure.
  batch N [NRHS ...] plane waves of NRHS different directions (default 1 2 4 8) on the cube of N at l = 2, device tensors,
                     reltol 1e-6: one bicgstabl_batch_ call against back-to-back bicgstabl_ calls on the same right-hand sides,
                     alternated over three repetitions after a warm-up of both; without a preconditioner, and with
                     SparsifyingPreconditioner.from_operator where its dense blocks fit (N <= 64).  Appended to
                     profiles/bicgstabl_batch.jsonl: wall times, cycles and mvps per member, batch_info of the
                     preconditioner, peak device memory
  kernels N L [L ...] three cycles of bicgstabl_ at each l on the cube of N, nothing recorded: the target of
                     `rocprofv3 --kernel-trace --stats -- python3 tools/bench_bicgstabl.py kernels 512 4 8`
                     (profiles/bicgstabl_kernel_stats.csv; the template argument in a kernel's name is its vector count)
usage: python tools/bench_bicgstabl.py solve 256 512 | largest | batch 48 1 2 4 8 | kernels 512 4 8"""
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402
from tools.bench_configs import bump  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "bicgstabl.jsonl")
OUT_BATCH = os.path.join(ROOT, "profiles", "bicgstabl_batch.jsonl")


def emit(rec, out=OUT):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def problem(n):
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    k = 1.0 / h
    nu = (bump(x)[None, None, :] / 0.3 * bump(x)[None, :, None] / 0.3 * bump(x)[:, None, None]).ravel()   # separable: no N-sized temporaries
    M = lsfc.buildFastConvolution3D(x, x, x, None, None, None, h, k, nu)
    u_inc = torch.exp(1j * k * torch.from_numpy(x).cuda()).repeat(n * n)        # exp(i k X), x fastest
    rhs = M * u_inc
    rhs.sub_(u_inc).neg_()
    del u_inc
    return M, rhs


class PeakMemory:
    """smallest free device memory seen while a solve runs (the call releases the GIL), as used GB"""

    def __enter__(self):
        self.free0, self.total = torch.cuda.mem_get_info()
        self.low, self.stop = self.free0, False
        self.t = threading.Thread(target=self._poll)
        self.t.start()
        return self

    def _poll(self):
        while not self.stop:
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.005)

    def __exit__(self, *a):
        self.stop = True
        self.t.join()
        self.peak_used_GB = (self.total - self.low) / 1e9
        self.before_GB = (self.total - self.free0) / 1e9


def timed(fn):
    torch.cuda.synchronize()
    with PeakMemory() as pm:
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        t = time.time() - t0
    return out, t, pm


def solve(n, reltol=1e-6):
    M, rhs = problem(n)
    base = {"mode": "solve", "n": n, "N": n ** 3, "reltol": reltol, "vector_GB": n ** 3 * 16 / 1e9}
    for l in (1, 2, 4):
        try:
            (u, h), t, pm = timed(lambda: lsfc.bicgstabl_(torch.zeros_like(rhs), M, rhs, l=l, reltol=reltol, log=True))
        except lsfc.LsfcError as e:
            emit(dict(base, solver=f"bicgstabl(l={l})", error=str(e)))
            continue
        res = float(torch.linalg.norm(M * u - rhs) / torch.linalg.norm(rhs))
        emit(dict(base, solver=f"bicgstabl(l={l})", mvps=h.mvps, cycles=h.iters, converged=h.isconverged, seconds=t,
                  true_relres=res, peak_used_GB=pm.peak_used_GB, used_before_GB=pm.before_GB))
        del u
    free = torch.cuda.mem_get_info()[0]
    if 32 * n ** 3 * 16 > free:
        emit(dict(base, solver="gmres(30)", error=f"32 vectors need {32 * n ** 3 * 16 / 1e9:.1f} GB, {free / 1e9:.1f} GB are free: not run"))
    else:
        # (a one-step solve first, as tools/bench_configs.py does: the Krylov workspace is allocated on first use and kept)
        lsfc.gmres_(torch.zeros_like(rhs), M, rhs, restart=30, maxiter=1, reltol=reltol, log=True)
        (u, h), t, pm = timed(lambda: lsfc.gmres_(torch.zeros_like(rhs), M, rhs, restart=30, reltol=reltol, log=True))
        res = float(torch.linalg.norm(M * u - rhs) / torch.linalg.norm(rhs))
        emit(dict(base, solver="gmres(30)", mvps=h.mvps, iters=h.iters, converged=h.isconverged, seconds=t, true_relres=res,
                  peak_used_GB=pm.peak_used_GB, used_before_GB=pm.before_GB,
                  note="workspace allocated by a one-step solve beforehand; used_before_GB includes it"))
    M.close()


def largest(sizes):
    for n in sizes:
        base = {"mode": "largest", "n": n, "N": n ** 3, "vector_GB": n ** 3 * 16 / 1e9}
        try:
            M, rhs = problem(n)
        except (lsfc.LsfcError, torch.OutOfMemoryError) as e:
            emit(dict(base, solver="plan", error=str(e)[:300]))
            break
        fits = 0
        try:
            (u, h), t, pm = timed(lambda: lsfc.bicgstabl_(torch.zeros_like(rhs), M, rhs, l=1, max_mv_products=8, log=True))
            emit(dict(base, solver="bicgstabl(l=1)", fits=True, mvps=h.mvps, cycles=h.iters, seconds=t, resnorm=[float(v) for v in h["resnorm"]],
                      peak_used_GB=pm.peak_used_GB, used_before_GB=pm.before_GB))
            fits += 1
            del u
        except lsfc.LsfcError as e:
            emit(dict(base, solver="bicgstabl(l=1)", fits=False, code=e.code, error=str(e)))
        free = torch.cuda.mem_get_info()[0]
        need = 22 * n ** 3 * 16
        if need > free:
            emit(dict(base, solver="gmres(20)", fits=False, error=f"22 vectors need {need / 1e9:.1f} GB, {free / 1e9:.1f} GB are free: not run"))
        else:
            try:
                (u, h), t, pm = timed(lambda: lsfc.gmres_(torch.zeros_like(rhs), M, rhs, restart=20, maxiter=8, log=True))
                emit(dict(base, solver="gmres(20)", fits=True, mvps=h.mvps, iters=h.iters, seconds=t, peak_used_GB=pm.peak_used_GB,
                          used_before_GB=pm.before_GB))
                fits += 1
                del u
            except (lsfc.LsfcError, torch.OutOfMemoryError) as e:
                emit(dict(base, solver="gmres(20)", fits=False, error=str(e)[:300]))
        M.close()
        del M, rhs
        torch.cuda.empty_cache()
        if not fits:
            break


# incident directions of the batch measurement (unit vectors; tests/plasma_example.jl:160-176 uses two)
DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, -1, 0)]


def batch_problem(n, nrhs):
    M, _ = problem(n)
    k = float(n)
    x = torch.from_numpy(-0.5 + np.arange(n) / n).cuda()
    rhs = torch.empty((nrhs, n ** 3), dtype=torch.complex128, device="cuda")
    for j in range(nrhs):
        d = np.array(DIRECTIONS[j % len(DIRECTIONS)], dtype=float)
        d /= np.linalg.norm(d) * (1 + j // len(DIRECTIONS))
        ex, ey, ez = (torch.exp(1j * k * c * x) for c in d)                        # separable: exp(i k d . r), x fastest
        u_inc = (ez[:, None, None] * ey[None, :, None] * ex[None, None, :]).reshape(-1)
        rhs[j] = M * u_inc
        rhs[j].sub_(u_inc).neg_()
    return M, rhs


def batch(n, counts, reltol=1e-6, reps=3):
    for precond in (False, True):
        if precond and n > 64:
            emit({"mode": "batch", "n": n, "preconditioner": "blocktri", "error": f"not run: {n} dense blocks of {n * n}^2 complex do not fit"}, OUT_BATCH)
            continue
        for nrhs in counts:
            M, rhs = batch_problem(n, nrhs)
            P = lsfc.SparsifyingPreconditioner.from_operator(M) if precond else None
            kw = dict(l=2, Pl=P, reltol=reltol, log=True)
            one_by_one = lambda: [lsfc.bicgstabl_(torch.zeros_like(rhs[j]), M, rhs[j], **kw) for j in range(nrhs)]   # noqa: E731
            together = lambda: lsfc.bicgstabl_batch_(torch.zeros_like(rhs), M, rhs, **kw)                            # noqa: E731
            one_by_one(), together()                                                 # warm-up of every shape both use
            t_single, t_batch, peak = [], [], 0.0
            for _ in range(reps):                                                    # alternated
                singles, t, _pm = timed(one_by_one)
                t_single.append(t)
                (X, hs), t, pm = timed(together)
                t_batch.append(t)
                peak = max(peak, pm.peak_used_GB)
            diff = max(float(torch.linalg.norm(X[j] - singles[j][0]) / torch.linalg.norm(singles[j][0])) for j in range(nrhs))
            emit({"mode": "batch", "n": n, "N": n ** 3, "nrhs": nrhs, "l": 2, "reltol": reltol, "preconditioner": "blocktri" if precond else None,
                  "seconds_batch": t_batch, "seconds_one_by_one": t_single, "ratio_one_by_one_over_batch": min(t_single) / min(t_batch),
                  "cycles": [h.iters for h in hs], "mvps": [h.mvps for h in hs], "converged": [h.isconverged for h in hs],
                  "cycles_single": [h.iters for _, h in singles], "max_rel_diff_to_single": diff,
                  "batch_info": P.batch_info() if precond else None, "peak_used_GB": peak}, OUT_BATCH)
            if P is not None:
                P.close()
            M.close()
            del M, rhs, X, singles
            torch.cuda.empty_cache()


def kernels(n, ls):
    M, rhs = problem(n)
    for l in ls:
        _, h = lsfc.bicgstabl_(torch.zeros_like(rhs), M, rhs, l=l, max_mv_products=6 * l, reltol=1e-14, log=True)
        print(f"n={n} l={l}: {h.iters} cycles, {h.mvps} mvps", flush=True)
    torch.cuda.synchronize()
    M.close()


if __name__ == "__main__":
    mode, sizes = (sys.argv[1] if len(sys.argv) > 1 else "solve"), [int(v) for v in sys.argv[2:]]
    if mode == "solve":
        for n in sizes or [256, 512]:
            solve(n)
    elif mode == "largest":
        largest(sizes or [512, 640, 768, 1024])
    elif mode == "batch" and sizes:
        batch(sizes[0], sizes[1:] or [1, 2, 4, 8])
    elif mode == "kernels" and len(sizes) > 1:
        kernels(sizes[0], sizes[1:])
    else:
        sys.exit(__doc__)
