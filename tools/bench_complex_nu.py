"""A complex nu (an absorbing medium, lsfc_plan_set_nu_complex) against the real nu ON THE SAME PLAN on one MI355X, appended to
profiles/complex_nu.jsonl (one JSON line per size).

  [SIZE ...]   device tensors, HIP-event time of `reps` applies through time_apply.  Every shape is warmed up first with both
               kinds of nu; then, three rounds: the plan takes the real nu and N, T, H are measured, it takes the complex nu
               (nu (1 - 0.5i), from a device tensor) and N, T, H are measured again.  Each of the six gets its best time and
               its spread (max / min - 1).  The N-to-N spread of the real nu in the same run is the yardstick the complex / real
               ratios are read against; the byte model says 1 + 8 / 568 in 3D (8 more bytes per point in the one x pass that
               multiplies).  One profile_apply per kind and op (per-stage ms and algorithmic bytes) goes into the same record.
               SIZE: 48, 256, 512 (3D cubes, buildFastConvolution3D) or 2d1024 (2D, Greengard-Vico); default all four.
  real [--tree DIR] SIZE ...
               the real-nu apply alone, N and T, best of three, of the package in the checkout DIR (default: this one): run once
               on the parent commit's checkout built next to this one and once on this one, it tells whether the real path of a
               size costs what it did (records of mode "real_nu_apply"; "tree" is the name of DIR, or "this").  SIZE: any n (an n^3 cube) or 2dN.
               This mode uses nothing but calls the parent commit has too.
usage: python tools/bench_complex_nu.py 48 256 512 2d1024 | real --tree ../parent 80 300 2d1000"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = len(sys.argv) > 1 and sys.argv[1] == "real"
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if REAL and "--tree" in sys.argv else ROOT
sys.path.insert(0, ROOT)
sys.path.insert(0, TREE)                                   # the package of the checkout under measurement
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402
assert os.path.dirname(os.path.dirname(os.path.abspath(lsfc.__file__))) == TREE, lsfc.__file__
if not REAL:
    from tools.bench_adjoint import operator, views  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "complex_nu.jsonl")
ROUNDS = 3
OPS = ("N", "T", "H")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def run(size):
    M, N, reps = operator(size)
    nu = {"real": torch.from_numpy(M.nu).cuda()}
    nu["complex"] = nu["real"] * (1 - 0.5j)
    xb = torch.randn(N, dtype=torch.complex128, device="cuda")
    yb = torch.empty_like(xb)
    V = views(M)
    for kind in ("real", "complex"):                       # warm-up of every shape and of both paths
        M.set_nu(nu[kind])
        assert M.nu_is_complex == (kind == "complex")
        for v in V.values():
            lsfc.time_apply(v, xb, yb, max(2, reps // 4))
    ms = {kind: {w: [] for w in OPS} for kind in nu}
    for _ in range(ROUNDS):                                # alternated
        for kind in ("real", "complex"):
            M.set_nu(nu[kind])
            for w in OPS:
                ms[kind][w].append(lsfc.time_apply(V[w], xb, yb, reps) / reps)
    stages = {}
    for kind in ("real", "complex"):
        M.set_nu(nu[kind])
        stages[kind] = {w: [(name, round(t, 4), b) for name, t, b in lsfc.profile_apply(V[w], xb, yb, 5)] for w in OPS}
    best = {kind: {w: min(t) for w, t in ms[kind].items()} for kind in ms}
    model = {w: sum(b for _, _, b in stages["complex"][w]) / sum(b for _, _, b in stages["real"][w]) for w in OPS}
    emit({"mode": "complex_nu", "size": size, "N": N, "pipeline": M.pipeline, "reps": reps, "rounds": ROUNDS, "ms_per_apply": ms, "best_ms": best,
          "spread": {kind: {w: max(t) / min(t) - 1 for w, t in ms[kind].items()} for kind in ms},
          "N_to_N_spread": max(ms["real"]["N"]) / min(ms["real"]["N"]) - 1,
          "complex_over_real": {w: best["complex"][w] / best["real"][w] for w in OPS}, "byte_model_ratio": model, "stages": stages})
    M.close()


def bump(x):
    return 0.3 * np.exp(-40 * x ** 2)


def real(size, tree_as_given):
    if size.startswith("2d"):
        n = int(size[2:])
        h = 1.0 / n
        x = -0.5 + h * np.arange(n)
        M, N, reps = lsfc.buildFastConvolution(x, x, h, 40.0, lambda X, Y: bump(X) * bump(Y) / 0.3, quadRule="Greengard_Vico"), n * n, 200
    else:
        n = int(size)
        h = 1.0 / n
        x = -0.5 + h * np.arange(n)
        nu = (bump(x)[None, None, :] / 0.3 * bump(x)[None, :, None] / 0.3 * bump(x)[:, None, None]).ravel()
        M, N, reps = lsfc.buildFastConvolution3D(x, x, x, None, None, None, h, 1.0 / h, nu), n ** 3, 200 if n <= 100 else 30
    xb = torch.randn(N, dtype=torch.complex128, device="cuda")
    yb = torch.empty_like(xb)
    ms = {}
    for w, V in (("N", M), ("T", M.T)):
        lsfc.time_apply(V, xb, yb, max(2, reps // 4))
        ms[w] = [lsfc.time_apply(V, xb, yb, reps) / reps for _ in range(ROUNDS)]
    passes = [ln for ln in M.describe_passes().split("\n") if ln.startswith("x")]
    emit({"mode": "real_nu_apply", "tree": tree_as_given, "size": size, "N": N, "reps": reps, "passes": passes, "ms_per_apply": ms,
          "best_ms": {w: min(t) for w, t in ms.items()}, "spread": {w: max(t) / min(t) - 1 for w, t in ms.items()}})
    M.close()


if __name__ == "__main__":
    if any(a in ("-h", "--help") for a in sys.argv[1:]):
        sys.exit(__doc__)
    if REAL:
        args = sys.argv[2:]
        given = "this"
        if "--tree" in args:
            i = args.index("--tree")
            given = os.path.basename(os.path.normpath(args[i + 1]))      # the directory's name, not where it lies
            del args[i:i + 2]
        for s in args:
            real(s, given)
        sys.exit(0)
    for s in sys.argv[1:] or ["48", "256", "512", "2d1024"]:
        run(s)
        torch.cuda.empty_cache()
