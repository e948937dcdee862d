"""SHA-256 of x and of the residual history for a fixed list of Krylov solves: the bitwise fingerprint of the BLAS-1 layer
(csrc/krylov_blas.hip, csrc/bicgstab.hip, csrc/reduce.hpp).  Two builds of the library that print the same lines sum and
multiply in the same order.

The operator is that of tests/test_gpu_gmres_kernels.py (helpers of tests/krylov_common.py and tests/gmres_ref.py): an
identity plan and the preconditioner diag(lambda), so only the reductions see the order of summation.  The solves:
  gmres_            N = 1, 65, 1025, 4097, 65538, restart 30: strict MGS, blocked MGS, CGS, DGKS
  gmres_            N = 1025, restart 5, 64, 65, 100: blocked MGS, CGS (block remainders, the 64-column boundary of the
                    fused CGS sweep, the chunked x += V y)
  gmres_            four ranks on one device (MultiDeviceFastM3D 16 x 22 x 36, restart 65): MGS, CGS, DGKS, unfused and all-reduced
  bicgstabl_multi_  the same four ranks, l = 1, 2, with and without the host callback (the rank sums and the gather / scatter)
  gmres_batch_      the three right-hand sides of test_batch_equals_single_solves_bitwise: MGS, CGS, DGKS
  bicgstabl_        N = 4097, l = 1, 2, 4, 8;  bicgstabl_batch_ with three members at l = 2
  symmetry_defect   a 16^3 plan (blas_dot / blas_nrm2 called directly)

    python tools/krylov_digest.py                                   one JSON line per solve, this tree's library
    python tools/krylov_digest.py --libs parent=/path/to/liblsfc.so,this= [--out profiles/krylov_blas_refactor.jsonl]
                                                                    one fresh child process per build (LSFC_LIBRARY; an empty
                                                                    path is the library of this tree), one line per solve
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

ORTH = {"MGS": "ModifiedGramSchmidt", "CGS": "ClassicalGramSchmidt", "DGKS": "DGKS"}
PATHS = [("MGS", "0"), ("MGS", "1"), ("CGS", None), ("DGKS", None)]        # (orth, LSFC_MGS_BLOCK)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emit(label, x, hists):
    r = np.concatenate([np.asarray(h["resnorm"], dtype=np.float64) for h in hists])
    print("DIGEST " + json.dumps({"solve": label, "iters": [int(h.iters) for h in hists], "x": sha(x), "history": sha(r)}), flush=True)


def child():
    import fast_solver_lippmann_schwinger_amd as lsfc
    import bicgstabl_batch_cases as bc
    import bicgstabl_ref as br
    import gmres_ref as gr
    import krylov_common as kc

    plans = {}

    def plan(N):                                       # the identity plan of krylov_common.plan
        if N not in plans:
            n, m = kc._shape(N)
            plans[N] = lsfc.FastM(np.ones((2 * n, 2 * m), complex), np.zeros(N), 2 * n, 2 * m, n, m, 1.0,
                                  quadRule="Greengard_Vico", flags=lsfc._lib.LSFC_FLAG_FORCE_ROCFFT)
        return plans[N]

    def gmres(M, P, b, orth, mb, **kw):
        os.environ.pop("LSFC_GMRES_LOOKAHEAD", None)
        if mb is None:
            os.environ.pop("LSFC_MGS_BLOCK", None)
        else:
            os.environ["LSFC_MGS_BLOCK"] = mb
        return lsfc.gmres_(np.zeros(M.N, complex), M, b, Pl=P, log=True, orth_meth=ORTH[orth], **kw)

    for N, restarts, paths in [(N, (30,), PATHS) for N in (1, 65, 1025, 4097, 65538)] + [(1025, (5, 64, 65, 100), [PATHS[1], PATHS[2]])]:
        lam, b = gr.disc_spectrum(N, 0.9, seed=N), gr.random_rhs(N, seed=N + 1)
        P = kc._diag_precond(lsfc, lam)
        for restart in restarts:
            for orth, mb in paths:
                x, h = gmres(plan(N), P, b, orth, mb, restart=restart, maxiter=100 if restart < 100 else 130)
                emit(f"gmres N={N} restart={restart} {orth} block={mb}", x, [h])
        P.close()
    os.environ.pop("LSFC_MGS_BLOCK", None)

    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n, m, l = 16, 22, 36
    N = n * m * l
    M = MultiDeviceFastM3D(n, 1.0 / n, 3.0, np.zeros(N), devices=[0] * 4, m=m, l=l)
    lam, b = gr.disc_spectrum(N, 0.9, seed=10), gr.random_rhs(N, seed=11)

    def scale(v, lam=lam):
        v *= lam

    for orth in ORTH:
        x, h = lsfc.gmres_(np.zeros(N, complex), M, b, Pl=scale, restart=65, maxiter=100, log=True, orth_meth=ORTH[orth])
        emit(f"gmres four ranks on one device restart=65 {orth}", x, [h])
    for l_ in (1, 2):
        for name, Pl in (("no callback", None), ("host callback", scale)):
            x, h = lsfc.bicgstabl_multi_(np.zeros(N, complex), M, b, l=l_, Pl=Pl, max_mv_products=60, log=True)
            emit(f"bicgstabl_multi four ranks on one device l={l_} {name}", x, [h])
    M.close()

    N = 4097
    lam = gr.disc_spectrum(N, 0.6, seed=5)
    B = np.zeros((3, N), complex)
    B[0] = gr.random_rhs(N, seed=6)
    B[1, :12] = gr.random_rhs(12, seed=7)
    B[2, 100:140] = gr.random_rhs(40, seed=8)
    def scale3(v, lam=lam):
        v *= lam

    for orth in ORTH:
        X, hs = lsfc.gmres_batch_(np.zeros((3, N), complex), plan(N), B, Pl=scale3, restart=20, log=True, orth_meth=ORTH[orth])
        emit(f"gmres_batch N={N} nrhs=3 {orth}", X, hs)

    lam, b = br.length_problem(N)
    P = kc._diag_precond(lsfc, lam)
    for l in (1, 2, 4, 8):
        x, h = lsfc.bicgstabl_(np.zeros(N, complex), plan(N), b, l=l, Pl=P, max_mv_products=100, log=True)
        emit(f"bicgstabl N={N} l={l}", x, [h])
    members = bc.length_members(N, 2)
    X, hs = lsfc.bicgstabl_batch_(bc.stack(members, "x0", N), plan(N), bc.stack(members, "b", N), l=2, Pl=P,
                                  max_mv_products=members[0]["max_mv_products"], log=True)
    emit(f"bicgstabl_batch N={N} nrhs=3 l=2", X, hs)
    P.close()
    for M in plans.values():
        M.close()

    n = 16
    x = -0.5 + np.arange(n) / n
    g = np.exp(-40 * x ** 2)
    M = lsfc.buildFastConvolution3D(x, x, x, None, None, None, 1.0 / n, float(n), (0.3 * g[:, None, None] * g[None, :, None] * g[None, None, :]).reshape(-1))
    d = np.array([M.symmetry_defect()])
    print("DIGEST " + json.dumps({"solve": f"symmetry_defect {n}^3", "value": float(d[0]), "x": sha(d), "history": sha(d)}), flush=True)
    M.close()


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
    if [d["solve"] for d in a] != [d["solve"] for d in b]:
        sys.exit("the two builds ran different lists of solves")
    bad = 0
    for da, db in zip(a, b):
        equal = (da["x"], da["history"]) == (db["x"], db["history"])
        bad += not equal
        rec = {"check": "digest", "solve": da["solve"], "iters": da.get("iters"), f"x_sha256_{na}": da["x"], f"x_sha256_{nb}": db["x"],
               f"history_sha256_{na}": da["history"], f"history_sha256_{nb}": db["history"], "equal": equal}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    print(f"# {len(a)} solves, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
