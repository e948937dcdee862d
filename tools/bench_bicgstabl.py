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
  multi N DEVICES [L] the same problem on a single-process multi-device plan (MultiDeviceFastM3D, bicgstabl_multi_, host vectors) at l = L (default 2),
                     DEVICES a comma-separated list such as 0,1,2,3: one solve to reltol 1e-6, then the time of a cycle (capped
                     solves of 2 and 10 cycles, best of three, the difference over 8) beside 2 l times the plan's measured apply
                     (MultiDeviceFastM3D.bench) plus the vector-kernel time of a cycle on one device (its cycle minus 2 l of its
                     applies).  Appended to profiles/bicgstabl_multi.jsonl.  A device listed more than once makes logical ranks
                     on one GPU: the record then says that it is a rehearsal, which measures enqueue order and copy overhead, not scaling
usage: python tools/bench_bicgstabl.py solve 256 512 | largest | batch 48 1 2 4 8 | kernels 512 4 8 | multi 256 0,0"""
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
OUT_MULTI = os.path.join(ROOT, "profiles", "bicgstabl_multi.jsonl")


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


def _cycle_seconds(solve_capped, l, reset=lambda: None):
    """time of one cycle: capped solves of 2 and 10 cycles (after a warm-up), best of three each, the difference over 8 -- what
    both share (staging of host vectors, the initial residual) cancels; reset() runs outside the timed window"""
    cap = lambda c: 1 + 2 * l * c                                                   # noqa: E731
    reset()
    solve_capped(cap(2))
    t, done = {}, {}
    for c in (2, 10) * 3:
        reset()
        (_, h), sec, _pm = timed(lambda: solve_capped(cap(c)))
        t[c], done[c] = min(t.get(c, sec), sec), h.iters
    if done[10] <= done[2]:
        sys.exit(f"the solve stops after {done[10]} cycles: too few to time one")
    return (t[10] - t[2]) / (done[10] - done[2])


def multi(n, devices, l=2, reltol=1e-6):
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    N, P = n ** 3, len(devices)
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    k = 1.0 / h
    nu = (bump(x)[None, None, :] / 0.3 * bump(x)[None, :, None] / 0.3 * bump(x)[:, None, None]).ravel()
    M = MultiDeviceFastM3D(n, h, k, nu, devices=devices)
    u_inc = np.tile(np.exp(1j * k * x), n * n)
    rhs = -(M * u_inc - u_inc)
    del u_inc
    rehearsal = len(set(devices)) < P
    on_one = max(devices.count(d) for d in set(devices))
    rec = {"mode": "multi", "n": n, "N": N, "l": l, "reltol": reltol, "devices": devices, "ranks": P, "transport": M.transport,
           "rehearsal_on_one_gpu": rehearsal, "vector_GB": N * 16 / 1e9,
           "work_GB_per_device_by_the_rule": on_one * (2 * l + 3 + 2) * (N // P) * 16 / 1e9}
    if rehearsal:
        rec["note"] = ("rehearsal: a device is listed more than once, so logical ranks share one GPU -- this measures enqueue order and "
                       "copy overhead, not scaling")
    (u, hist), sec, pm = timed(lambda: lsfc.bicgstabl_multi_(np.zeros(N, complex), M, rhs, l=l, reltol=reltol, log=True))
    rec["solve"] = {"mvps": hist.mvps, "cycles": hist.iters, "converged": hist.isconverged, "seconds": sec, "peak_used_GB": pm.peak_used_GB,
                    "true_relres": float(np.linalg.norm(M * u - rhs) / np.linalg.norm(rhs))}
    del u
    x0 = np.zeros(N, complex)                              # (one buffer, zeroed outside the timed window: no page faults inside it)
    rec["cycle_s"] = _cycle_seconds(lambda mv: lsfc.bicgstabl_multi_(x0, M, rhs, l=l, reltol=1e-14, max_mv_products=mv, log=True), l,
                                    reset=lambda: x0.fill(0))
    del x0
    steps = 10
    rec["apply_s"] = M.bench(steps, 2)["elapsed_s"] / steps
    M.close()
    del M, rhs
    torch.cuda.empty_cache()
    # one device: the vector kernels of a cycle = its cycle minus 2 l of its applies
    M1, rhs1 = problem(n)
    cyc1 = _cycle_seconds(lambda mv: lsfc.bicgstabl_(torch.zeros_like(rhs1), M1, rhs1, l=l, reltol=1e-14, max_mv_products=mv, log=True), l)
    y = M1 * rhs1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        y = M1 * rhs1
    torch.cuda.synchronize()
    app1 = (time.perf_counter() - t0) / steps
    M1.close()
    rec.update(single_device_cycle_s=cyc1, single_device_apply_s=app1, single_device_vector_kernels_s=cyc1 - 2 * l * app1,
               expected_cycle_s=2 * l * rec["apply_s"] + (cyc1 - 2 * l * app1))
    rec["cycle_over_expected"] = rec["cycle_s"] / rec["expected_cycle_s"]
    emit(rec, OUT_MULTI)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "multi":
        multi(int(sys.argv[2]), [int(d) for d in sys.argv[3].split(",")], *[int(v) for v in sys.argv[4:5]])
        sys.exit(0)
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
