"""The transposed and the adjoint preconditioner (P.T, P.H) against P on one MI355X, appended to
profiles/precond_transpose.jsonl (one JSON line per measurement).

  apply [SIZE ...]   a `from_operator` object at SIZE^3 (default 32 and 48; 48: b = 2304, K = 48) at both storages of the
                     inverses; device tensors, HIP-event time of `reps` applies.  Single apply and group apply of 8, under N,
                     T and H, alternated, best of three rounds, with the spread (max / min - 1) of each.  The N-to-N spread
                     of the same run is the yardstick the T/N and H/N ratios are read against.
  gmres [N]          GMRES to reltol 1e-6 on M.H at N^3 (default 48) with Pl = P.H and without: steps and seconds.
usage: python tools/bench_precond_transpose.py apply 32 48 | gmres 48"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402
from tools.bench_adjoint import operator  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "precond_transpose.jsonl")
ROUNDS = 3
GROUP = 8


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def event_ms(fn, reps):
    """HIP-event time of `reps` calls of fn, per call"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def apply(size):
    M, N, _ = operator(size)
    n = int(size)
    reps = 50 if n <= 32 else 10
    for dt in ("complex128", "complex64"):
        P = lsfc.SparsifyingPreconditioner.from_operator(M, inverse_dtype=dt)
        views = {"N": P, "T": P.T, "H": P.H}
        v = torch.randn(N, dtype=torch.complex128, device="cuda")
        V = torch.randn(GROUP, N, dtype=torch.complex128, device="cuda")
        forms = {"single": lambda p: p.ldiv_(v), "group8": lambda p: p.ldiv_batch_(V)}
        for f in forms.values():                           # warm-up: tables, graphs, group work space, clocks
            for p in views.values():
                event_ms(lambda: f(p), 2)
                v.normal_()
                V.normal_()
        ms = {form: {w: [] for w in views} for form in forms}
        for _ in range(ROUNDS):                            # alternated
            for form, f in forms.items():
                for w, p in views.items():
                    v.normal_()                            # (in place applies: keep the entries of order one)
                    V.normal_()
                    ms[form][w].append(event_ms(lambda: f(p), reps))
        best = {form: {w: min(t) for w, t in per.items()} for form, per in ms.items()}
        info = P.blocktri_info()
        emit({"mode": "apply", "size": size, "N": N, "inverse_dtype": dt, "blocks": info["blocks"], "block_size": info["block_size"],
              "factor_bytes": info["factor_bytes"], "reps": reps, "rounds": ROUNDS, "ms": ms, "best_ms": best,
              "spread": {form: {w: max(t) / min(t) - 1 for w, t in per.items()} for form, per in ms.items()},
              "T_over_N": {form: best[form]["T"] / best[form]["N"] for form in forms},
              "H_over_N": {form: best[form]["H"] / best[form]["N"] for form in forms},
              "group8_over_8_singles": {w: best["group8"][w] / (GROUP * best["single"][w]) for w in views}})
        P.close()
        del P
        torch.cuda.empty_cache()
    M.close()


def gmres(n, reltol=1e-6):
    M, N, _ = operator(str(n))
    k = float(n)
    x = -0.5 + np.arange(n) / n
    u_inc = torch.exp(1j * k * torch.from_numpy(x).cuda()).repeat(n * n)        # exp(i k X), x fastest
    rhs = M * u_inc
    rhs.sub_(u_inc).neg_()
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    A = M.H
    runs = {"with_P.H": {"Pl": P.H}, "plain": {"maxiter": 400}}
    for kw in runs.values():                               # work space, tables and graphs exist before the clock runs
        lsfc.gmres_(torch.zeros_like(rhs), A, rhs, reltol=reltol, **{**kw, "maxiter": 1})
    sec, info = {w: [] for w in runs}, {}
    for _ in range(ROUNDS):
        for w, kw in runs.items():
            torch.cuda.synchronize()
            t0 = time.time()
            u, h = lsfc.gmres_(torch.zeros_like(rhs), A, rhs, reltol=reltol, log=True, **kw)
            torch.cuda.synchronize()
            sec[w].append(time.time() - t0)
            res = float(torch.linalg.norm(A * u - rhs) / torch.linalg.norm(rhs))
            info[w] = {"iters": h.iters, "mvps": h.mvps, "converged": h.isconverged, "true_relres": res}
    emit({"mode": "gmres", "n": n, "N": N, "op": "H", "reltol": reltol, "seconds": sec, "best_seconds": {w: min(t) for w, t in sec.items()},
          "solve": info})
    P.close()
    M.close()


if __name__ == "__main__":
    mode, args = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "apply":
        for s in args or ["32", "48"]:
            apply(s)
            torch.cuda.empty_cache()
    elif mode == "gmres":
        gmres(int(args[0]) if args else 48)
    else:
        sys.exit(__doc__)
