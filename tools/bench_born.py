"""Linearised scattering (BornOperator, lsfc_born_*) on one MI355X, appended to profiles/born.jsonl (one JSON line per case).
HIP events around `reps` calls; every shape is warmed up first, reps is chosen so that a timed window holds at least 0.2 s of
work, and the best of three windows is reported with the spread (max / min - 1).

  object    128^3, 16 far-field sources (plane waves), 64 far-field directions, GMRES(30) at reltol 1e-8, chunk 16: the background,
            J dnu and J^H r; beside each the time of its batched solve alone (gmres_batch_ on the same right-hand sides, the
            operator or its transpose) and of its receivers apply alone, so that the glue -- lsfc_born_scale / _image, the
            conjugation, the zeroing of x0, the copies of the small vectors -- is what is left.
  image     lsfc_born_image at 256^3 with 8 and 32 members against its byte model (2 S + 1) N 16 B and the project's measured copy
            ceiling (6.29 TB/s); lsfc_born_scale with 8 members against (2 * 8 + 1 or 0.5) N 16 B.  Reported, not gated.

  reciprocal  the object shape again in reciprocal mode (lsfc_born_set_mode): the receiver-field set-up (the switch from the
            adjoint-state mode with a background present: nrecv solves on M) and its operator applications; J dnu and J^H r beside
            the adjoint-state calls of the same build and object, and the number of applies after which the set-up has paid.
  contract  lsfc_born_contract N and H at 256^3 with 8 x 8 and 16 x 64 members against its byte model (U is read once
            per 16 receivers, V once per 16 sources, in / out once), the copy ceiling, and the 8-flop-per-pair count.

usage: python tools/bench_born.py [--out FILE] [--quick] [--reciprocal]
       (--quick: 32^3 / 64^3, for a rehearsal of the tool itself; --reciprocal: the last two sections only)"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402
import fast_solver_lippmann_schwinger_amd._lib as L  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "born.jsonl")
COPY_CEILING = 6.29e12          # bytes/s, VERDICT.md
ROUNDS, WINDOW_S = 3, 0.2


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(fns):
    """fns: name -> callable; alternated over ROUNDS; -> name -> (best ms, spread, reps)"""
    reps = {}
    for k, f in fns.items():
        f()                                                 # warm-up of the shape
        torch.cuda.synchronize()
        reps[k] = max(1, math.ceil(WINDOW_S * 1e3 / max(timed(f, 1), 1e-3)))
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            ms[k].append(timed(f, reps[k]))
    return {k: {"ms": min(v), "spread": max(v) / min(v) - 1, "reps": reps[k]} for k, v in ms.items()}


def sphere(count, seed):
    v = np.random.default_rng(seed).standard_normal((count, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def grid(n):
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    Xg, Yg, Zg = np.meshgrid(x, x, x, indexing="ij")
    return x, h, [A.reshape(-1, order="F") for A in (Xg, Yg, Zg)]


def object_cases(n, nsrc, nrecv):
    x, h, (X, Y, Z) = grid(n)
    k = 1.0 / h / 4.0                                       # k h = 0.25
    nu = 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2))
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu)
    R = lsfc.Receivers(x, x, x, k=k, directions=sphere(nrecv, 1))
    S = lsfc.Receivers(x, x, x, k=k, directions=sphere(nsrc, 2))
    N = n ** 3
    U_inc = torch.empty(nsrc, N, dtype=torch.complex128, device="cuda")
    for s in range(nsrc):                                   # one plane wave per source
        e = np.zeros(nsrc, dtype=np.complex128)
        e[s] = 1.0
        U_inc[s] = torch.from_numpy(S.plane_waves(e)).cuda()
    opts = dict(reltol=1e-8, restart=30)
    B = lsfc.BornOperator(M, R, U_inc, chunk=nsrc, **opts)
    dnu = torch.randn(N, dtype=torch.float64, device="cuda")
    r = torch.randn(nsrc * nrecv, dtype=torch.complex128, device="cuda")
    # the same right-hand sides for the solves alone
    rhs_n = B.fields * dnu * (-k * k)
    rhs_h = R.apply_batch(torch.conj_physical(r).reshape(nsrc, nrecv), op="T")
    X0 = torch.zeros_like(U_inc)

    def solve(A, rhs):
        X0.zero_()
        lsfc.gmres_batch_(X0, A, rhs, initially_zero=True, **opts)

    res = measure({
        "background": lambda: B.set_background(U_inc),
        "background_solve_alone": lambda: solve(M, U_inc),
        "background_receivers_alone": lambda: R.apply_batch(B.fields, op="N", M=M),
        "J": lambda: B.apply(dnu),
        "J_solve_alone": lambda: solve(M.T, rhs_n),
        "J_receivers_alone": lambda: R.apply_batch(X0, op="N"),
        "JH": lambda: B.adjoint(r),
        "JH_solve_alone": lambda: solve(M, rhs_h),
        "JH_receivers_alone": lambda: R.apply_batch(r.reshape(nsrc, nrecv), op="T"),
    })
    for name in ("background", "J", "JH"):
        glue = res[name]["ms"] - res[name + "_solve_alone"]["ms"] - res[name + "_receivers_alone"]["ms"]
        emit({"case": f"3d{n}_src{nsrc}_recv{nrecv}_{name}", "N": N, "nsrc": nsrc, "nrecv": nrecv, "chunk": B.info()["chunk"], **res[name],
              "solve_alone": res[name + "_solve_alone"], "receivers_alone": res[name + "_receivers_alone"], "glue_ms": glue,
              "mvps": B.info()["mvps"] if name == "JH" else None})
    B.close(), R.close(), S.close(), M.close()
    torch.cuda.empty_cache()


PARENT_MS = {"J": 56.7, "JH": 62.7}                     # README, the adjoint-state figures of the commit before reciprocal mode


def reciprocal_cases(n, nsrc, nrecv):
    x, h, (X, Y, Z) = grid(n)
    k = 1.0 / h / 4.0
    nu = 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2))
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu)
    R = lsfc.Receivers(x, x, x, k=k, directions=sphere(nrecv, 1))
    S = lsfc.Receivers(x, x, x, k=k, directions=sphere(nsrc, 2))
    N = n ** 3
    U_inc = torch.empty(nsrc, N, dtype=torch.complex128, device="cuda")
    for s in range(nsrc):
        e = np.zeros(nsrc, dtype=np.complex128)
        e[s] = 1.0
        U_inc[s] = torch.from_numpy(S.plane_waves(e)).cuda()
    B = lsfc.BornOperator(M, R, U_inc, chunk=nsrc, reltol=1e-8, restart=30)
    dnu = torch.randn(N, dtype=torch.float64, device="cuda")
    r = torch.randn(nsrc * nrecv, dtype=torch.complex128, device="cuda")
    calls = {"J": lambda: B.apply(dnu), "JH": lambda: B.adjoint(r)}
    adjoint_state = measure(calls)
    adjoint_mvps = {}
    for name, f in calls.items():
        f()
        adjoint_mvps[name] = B.info()["mvps"]
    # the set-up: one warm-up switch, then three timed ones (one call each: it is seconds, not a 0.2 s window)
    setup = []
    for i in range(ROUNDS + 1):
        B.set_mode("adjoint-state")
        torch.cuda.synchronize()
        setup.append(timed(lambda: B.set_mode("reciprocal"), 1))
        assert B.converged, B.message
    setup = setup[1:]
    info = B.receiver_info()
    emit({"case": f"3d{n}_src{nsrc}_recv{nrecv}_reciprocal_setup", "N": N, "nsrc": nsrc, "nrecv": nrecv, "chunk": B.info()["chunk"], "ms": min(setup),
          "spread": max(setup) / min(setup) - 1, "reps": 1, "solves": info["solves"], "mvps": info["mvps"],
          "receiver_field_bytes": info["receiver_field_bytes"]})
    reciprocal = measure(calls)
    for name in calls:
        gain = adjoint_state[name]["ms"] - reciprocal[name]["ms"]
        emit({"case": f"3d{n}_src{nsrc}_recv{nrecv}_reciprocal_{name}", "N": N, "nsrc": nsrc, "nrecv": nrecv, **reciprocal[name],
              "mvps": B.info()["mvps"], "adjoint_state_same_build": adjoint_state[name], "adjoint_state_mvps": adjoint_mvps[name],
              "adjoint_state_parent_ms": PARENT_MS[name] if (n, nsrc, nrecv) == (128, 16, 64) else None,
              "speedup": adjoint_state[name]["ms"] / reciprocal[name]["ms"],
              "applies_to_pay_for_setup": min(setup) / gain if gain > 0 else None,
              "stream_bytes": (nsrc + nrecv) * N * 16})
    B.close(), R.close(), S.close(), M.close()
    torch.cuda.empty_cache()


def contract_cases(n):
    N = n ** 3
    x = -0.5 + np.arange(n) / n
    M = lsfc.buildFastConvolution3D(x, x, x, None, None, None, 1.0 / n, 2.0, np.zeros(N))      # N, device and stream for the entry
    for nsrc, nrecv in ((8, 8), (16, 64)):
        U = torch.randn(nsrc, N, dtype=torch.complex128, device="cuda")
        V = torch.randn(nrecv, N, dtype=torch.complex128, device="cuda")
        dnu = torch.randn(N, dtype=torch.float64, device="cuda")
        r = torch.randn(nsrc * nrecv, dtype=torch.complex128, device="cuda")
        res = measure({"N": lambda: lsfc.born_contract(M, U, V, dnu, op="N", scale=-4.0),
                       "H": lambda: lsfc.born_contract(M, U, V, r, op="H", scale=-4.0)})
        ts, tr = -(-nsrc // 16), -(-nrecv // 16)
        model = {"N": (nsrc * tr + nrecv * ts) * N * 16 + N * 8, "H": (nsrc + nrecv * ts) * N * 16 + (2 * ts - 1) * N * 16}
        for op in ("N", "H"):
            sec = res[op]["ms"] * 1e-3
            emit({"case": f"contract_{op}_3d{n}_src{nsrc}_recv{nrecv}", "N": N, "nsrc": nsrc, "nrecv": nrecv, **res[op], "model_bytes": model[op],
                  "floor_bytes": (nsrc + nrecv) * N * 16 + (N * 8 if op == "N" else N * 16), "model_bytes_per_s": model[op] / sec,
                  "share_of_copy_ceiling": model[op] / sec / COPY_CEILING, "tflops_8_per_pair": 8.0 * nsrc * nrecv * N / sec / 1e12})
        del U, V
        torch.cuda.empty_cache()
    M.close()


def kernel_cases(n):
    N = n ** 3
    x = -0.5 + np.arange(n) / n
    M = lsfc.buildFastConvolution3D(x, x, x, None, None, None, 1.0 / n, 2.0, np.zeros(N))      # N, device and stream for the entries
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.lsfc_plan_set_stream(M._plan, stream))
    p = lambda t: C.c_void_p(t.data_ptr())                 # noqa: E731
    g = torch.empty(N, dtype=torch.complex128, device="cuda")
    for S in (8, 32):
        U = torch.randn(S, N, dtype=torch.complex128, device="cuda")
        P = torch.randn(S, N, dtype=torch.complex128, device="cuda")
        res = measure({"image": lambda: L.check(lib.lsfc_born_image(M._plan, p(U), p(P), S, -4.0, 0.0, 0, p(g), L.LSFC_MEM_DEVICE))})["image"]
        by = (2 * S + 1) * N * 16
        emit({"case": f"image_3d{n}_members{S}", "N": N, "members": S, **res, "model_bytes": by, "model_bytes_per_s": by / (res["ms"] * 1e-3),
              "share_of_copy_ceiling": by / (res["ms"] * 1e-3) / COPY_CEILING})
        if S == 8:
            for cplx in (False, True):
                d = torch.randn(N, dtype=torch.complex128 if cplx else torch.float64, device="cuda")
                res = measure({"scale": lambda: L.check(lib.lsfc_born_scale(M._plan, p(d), int(cplx), p(U), p(P), S, L.LSFC_MEM_DEVICE))})["scale"]
                by = (2 * S + (1.0 if cplx else 0.5)) * N * 16
                emit({"case": f"scale_3d{n}_members{S}_{'complex' if cplx else 'real'}_dnu", "N": N, "members": S, **res, "model_bytes": by,
                      "model_bytes_per_s": by / (res["ms"] * 1e-3), "share_of_copy_ceiling": by / (res["ms"] * 1e-3) / COPY_CEILING})
        del U, P
        torch.cuda.empty_cache()
    M.close()


if __name__ == "__main__":
    if any(a in ("-h", "--help") for a in sys.argv[1:]):
        sys.exit(__doc__)
    if "--out" in sys.argv:
        OUT = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    quick = "--quick" in sys.argv
    if "--reciprocal" not in sys.argv:
        object_cases(32 if quick else 128, 16, 64)
        kernel_cases(64 if quick else 256)
    reciprocal_cases(32 if quick else 128, 16, 64)
    contract_cases(64 if quick else 256)
