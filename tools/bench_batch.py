"""Multi-right-hand-side apply: ms per right-hand side and bytes model for R = 1, 2, 4, 8 (lsfc_apply_batch, one fused pass per
group) against R single applies.  usage: python tools/bench_batch.py [n ...]   (3D cubes; default 48 128 256)

gmres-batch mode: wall time of gmres_batch_ (host arrays in, host arrays out) for two or more builds of the library, each
build in child processes of its own that alternate -- per build `--rounds` children, each with one warm-up call and
`--reps` timed calls per configuration.  One JSON line per (build, configuration): the repetitions, their median and
the spread (max - min) / median.  Configurations (operator and incident plane waves of tools/bench_sparsify.py):
    a   48^3, 8 right-hand sides, no preconditioner, default restart
    b   48^3, 1, 2, 4 and 8 right-hand sides, the device block-tridiagonal preconditioner, reltol 1e-6
    c   48^3, 8 right-hand sides, a host Python callback that does nothing
    d   256^3, 4 right-hand sides, restart 20, 60 iterations (24 GB of Krylov vectors)

    python tools/bench_batch.py gmres-batch --libs parent=/path/to/liblsfc.so,this= --out profiles/gmres_batch_lockstep.jsonl
(an empty path is the library of this tree)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402


def run(n):
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    g = np.exp(-40 * x ** 2)
    nu = (0.3 * g[:, None, None] * g[None, :, None] * g[None, None, :]).reshape(-1)
    M = lsfc.buildFastConvolution3D(x, x, x, None, None, None, h, 1.0 / h, nu)
    N = n ** 3
    M.set_tuning(batch_fuse=1)            # measure the fused pass at every size (auto falls back to member-by-member above 256^3 padded points)
    out = []
    for R in (1, 2, 4, 8):
        B = torch.randn(R, N, dtype=torch.complex128, device="cuda")
        reps = max(3, min(200, int(2e9 / (N * R * 600))))
        for fused in (True, False):
            def once():
                if fused:
                    lsfc.apply_batch(M, B, 0)
                else:
                    for j in range(R):
                        M * B[j]
            once(); M.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                once()
            M.synchronize(); torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / reps * 1e3 / R
            model = ((35 - 8 + 8.0 / R) * 16 + 8) if fused else 568.0
            out.append({"n": n, "R": R, "fused_batch": fused, "ms_per_rhs": ms, "bytes_per_point_model": model,
                        "algorithmic_GBps_of_568": 568.0 * N / (ms * 1e-3) / 1e9})
            print(json.dumps(out[-1]), flush=True)
    M.close()


def gmres_batch_child(configs, reps):
    """one build (the library this process loaded): {configuration: [seconds]} as one JSON line"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_sparsify import operator
    out = {}
    for n, names in ((48, "abc"), (256, "d")):
        if not set(names) & set(configs):
            continue
        M = operator(3, n)
        h = 1.0 / n
        x = -0.5 + h * np.arange(n)
        X = [g.reshape(-1, order="F") for g in np.meshgrid(x, x, x, indexing="ij")]
        rng = np.random.default_rng(1)
        RHS = []
        for _ in range(8 if n == 48 else 4):                   # incident plane waves, random directions
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            u_inc = np.exp(1j * (1.0 / h) * sum(di * Xi for di, Xi in zip(d, X)))
            RHS.append(-(M * u_inc - u_inc))
        RHS = np.ascontiguousarray(np.stack(RHS))
        runs = []
        if "a" in configs and n == 48:
            runs.append(("a", 8, {}))
        if "b" in configs and n == 48:
            P = lsfc.SparsifyingPreconditioner.from_operator(M)
            runs += [(f"b R={R}", R, dict(Pl=P, reltol=1e-6)) for R in (1, 2, 4, 8)]
        if "c" in configs and n == 48:
            runs.append(("c", 8, dict(Pl=lambda v: None)))
        if "d" in configs and n == 256:
            runs.append(("d", 4, dict(restart=20, maxiter=60)))
        for name, R, kw in runs:
            s = []
            for i in range(reps + 1):
                t0 = time.perf_counter()
                lsfc.gmres_batch_(np.zeros_like(RHS[:R]), M, RHS[:R], **kw)
                if i:                                          # (the first call is the warm-up)
                    s.append(time.perf_counter() - t0)
            out[name] = s
        M.close()
        torch.cuda.empty_cache()
    print("GMRES_BATCH " + json.dumps(out), flush=True)


def gmres_batch_mode(argv):
    ap = argparse.ArgumentParser(prog="bench_batch.py gmres-batch")
    ap.add_argument("--libs", required=True, help="name=path[,name=path ...]; an empty path: the library of this tree")
    ap.add_argument("--configs", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args(argv)
    configs = args.configs.split(",")
    if args.child:
        return gmres_batch_child(configs, args.reps)
    libs = [spec.split("=", 1) for spec in args.libs.split(",")]
    times = {}
    for _ in range(args.rounds):
        for build, path in libs:                               # the builds alternate, one fresh process each
            env = dict(os.environ)
            if path:
                env["LSFC_LIBRARY"] = os.path.abspath(path)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "gmres-batch", "--child", "--libs", "-", "--configs", args.configs,
                                "--reps", str(args.reps)], env=env, capture_output=True, text=True, check=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("GMRES_BATCH ")][-1]
            print(f"# {build}: {line}", file=sys.stderr, flush=True)
            for name, s in json.loads(line[len("GMRES_BATCH "):]).items():
                times.setdefault((build, name), []).extend(s)
    for (build, name), s in times.items():
        med = float(np.median(s))
        rec = {"build": build, "config": name, "reps_s": [round(v, 5) for v in s], "median_s": round(med, 5), "spread": round((max(s) - min(s)) / med, 4)}
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["gmres-batch"]:
        sys.exit(gmres_batch_mode(sys.argv[2:]))
    for n in ([int(a) for a in sys.argv[1:]] or [48, 128, 256]):
        run(n)
