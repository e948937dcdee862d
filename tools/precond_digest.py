"""SHA-256 of the result of a fixed list of device preconditioner applies: the bitwise fingerprint of csrc/precond.hip,
csrc/trisolve.hip and of the sweeps of csrc/blocktri_sweep.hip as the preconditioner object drives them, and SHA-256 of what
csrc/blocktri_factor.hip stored.  Two builds of the library that print the same lines sum in the same order, schedule the
triangular solves alike and factorise alike.

  LU route       every entry of RECIPES in tests/test_gpu_precond.py (through its _Precond, _synthetic and _rhs) and the real
                 pairs ("2d", 33) and ("gv3", 16); each line also holds the twenty schedule counts (lsfc_precond_schedule, L then U)
  block-tridiagonal route
                 b = 17, 97, 98, 129, 257, 1025, 2049 of tests/blocktri_cases.SHAPES at both storages of the inverses:
                 solve, and solve_batch with 1, 3 and 8 right-hand sides, under op N, T and H; one 16^3 object made from a
                 plan with pivoting="partial"; the planted-pivot pair of tests/blocktri_pivot_ref.py (b = 70, K = 3, eps = 1e-9)
                 with pivoting="auto", whose pass without pivoting breaks down.  Every object also gives a line on its
                 factorisation: SHA-256 of every stored block and of every block's pivots, min_pivot_ratio as float.hex

    python tools/precond_digest.py                                  one JSON line per case, this tree's library
    python tools/precond_digest.py --libs parent=/path/to/liblsfc.so,this= [--out profiles/precond_split_refactor.jsonl]
                                                                    one fresh child process per build (LSFC_LIBRARY; an empty
                                                                    path is the library of this tree), one line per case
                                                                    with both digests and "equal"; exit status 1 if any differ"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BLOCK_SIZES = (17, 97, 98, 129, 257, 1025, 2049)
GROUPS = (1, 3, 8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(label, x, schedule=None, **more):
    rec = {"case": label, "x": sha(x), **more}
    if schedule is not None:
        rec["schedule"] = [int(v) for v in schedule]
    print("DIGEST " + json.dumps(rec), flush=True)


def child():
    import scipy.sparse.linalg as spla
    import fast_solver_lippmann_schwinger_amd as lsfc
    import blocktri_cases as bc
    import blocktri_pivot_ref as pv
    import test_gpu_precond as gp
    from test_gpu_sparsify import case

    for name in gp.RECIPES:
        P = gp._Precond(lsfc, *gp._synthetic(name))
        emit(f"lu {name} N={P.N}", P.apply(gp._rhs(P.N)), P.schedule(0) + P.schedule(1))
        P.close()
    for kind, n in (("2d", 33), ("gv3", 16)):
        Msp, As = gp._real_pair(kind, n)
        P = lsfc.SparsifyingPreconditioner(Msp, As, lu=spla.splu(Msp.tocsc()))
        st = P.stats()
        emit(f"lu {kind} n={n}", P.solve(gp._rhs(P.N)), list(st["schedule_L"].values()) + list(st["schedule_U"].values()))
        P.close()

    def every_op(label, P):
        K = P.blocktri_info()["blocks"]                    # the factorisation: x is the digest of all stored blocks together
        blocks = [sha(P.blocktri_block(k)) for k in range(K)]
        emit(f"{label} factorisation", "".join(blocks).encode(), blocks=blocks, pivots=[sha(P.blocktri_pivots(k)) for k in range(K)],
             min_pivot_ratio=float(P.blocktri_info()["min_pivot_ratio"]).hex())
        B = bc.right_hand_sides(P.N, max(GROUPS))
        for op, view in (("N", P), ("T", P.T), ("H", P.H)):
            emit(f"{label} {op} solve", view.solve(B[0]))
            for R in GROUPS:
                emit(f"{label} {op} solve_batch R={R}", view.solve_batch(B[:R]))

    for b, K, pattern in (s for s in bc.SHAPES if s[0] in BLOCK_SIZES):
        Msp, As = bc.synth(b, K, pattern, seed=b)
        for dt in ("complex128", "complex64"):
            P = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K, inverse_dtype=dt)
            every_op(f"blocktri {bc.shape_id((b, K, pattern))} {dt}", P)
            P.close()
    M = case("gv3", (16, 16, 16))[0]
    P = lsfc.SparsifyingPreconditioner.from_operator(M, pivoting="partial")
    every_op("blocktri from a 16^3 plan, partial pivoting", P)
    P.close()
    M.close()
    Msp, As = pv.planted(1e-9)
    P = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=pv.PLANT_K, pivoting="auto")
    assert P.blocktri_info()["pivoting"] == 1              # the pass without pivoting broke down
    every_op("blocktri planted pivot b=70 K=3, auto pivoting", P)
    P.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--libs", default="", help="name=path,name=path: compare two builds, a fresh child process each; an empty path: this tree's library")
    ap.add_argument("--out", default="", help="append the comparison lines to this file")
    args = ap.parse_args()
    if not args.libs:
        return child()
    (na, pa), (nb, pb) = [spec.split("=", 1) for spec in args.libs.split(",")]
    got = {}
    for name, path in ((na, pa), (nb, pb)):
        env = dict(os.environ)
        env.pop("LSFC_LIBRARY", None)
        if path:
            env["LSFC_LIBRARY"] = os.path.abspath(path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:                              # (nothing more is started on the device after a child that failed)
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        got[name] = [json.loads(ln[len("DIGEST "):]) for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    a, b = got[na], got[nb]
    if [d["case"] for d in a] != [d["case"] for d in b]:
        sys.exit("the two builds ran different lists of cases")
    bad = 0
    for da, db in zip(a, b):
        equal = da == db
        bad += not equal
        rec = {"check": "digest", "case": da["case"], f"x_sha256_{na}": da["x"], f"x_sha256_{nb}": db["x"], "equal": equal}
        for key in ("schedule", "blocks", "pivots", "min_pivot_ratio"):
            if key in da:
                rec.update({f"{key}_{na}": da[key], f"{key}_{nb}": db.get(key)})
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    print(f"# {len(a)} cases, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
