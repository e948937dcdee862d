"""The off-grid sampling operator (Receivers, lsfc_receivers_apply) on one MI355X, appended to profiles/receivers.jsonl (one JSON
line per case).  Device tensors, HIP events around `reps` applies; every shape is warmed up first, reps is chosen so that a timed
window holds at least 0.2 s of work, and the best of three windows is reported with the spread (max / min - 1).

  cases     3D 256^3: 256 and 1024 point receivers (N, H, and N fused with the medium of a plan); 256 far-field directions (N);
            2D 1024^2: 360 point receivers (N, H); a group of 8 members against eight single applies of the same object,
            alternated (3D, 256 points and 256 directions).
  reported  ms per apply, pairs/s (grid points x receivers x members), and
            far field:  bytes/s of the byte model N * 16 B * ceil(nrecv / directions per pass) per member against the project's
                        measured copy ceiling (6.29 TB/s), the operations/s of the model below against the fp64 vector
                        peak, and which of the two bounds is the nearer one;
            points:     the share of the fp64 vector peak (78.6 TFLOP/s, datasheet) on the operation model below.
  operation model (FMA = 2; kept here, not measured): per (point, receiver)
            3D points   14 for the distance, 1 / r and the amplitude, 60 for one fp64 sincos on its small-argument path
                        (range reduction and two polynomials), 8 per member for the complex multiply-add
            2D points   8 for the distance, 300 for j0 and y0 together (each a rational or asymptotic form with its own
                        sqrt / sincos), 8 per member
            far field   6 for Eyz * Ex, 8 per member (Ey * Ez, once per line and direction, is left out)
  launches  the far-field forward reads q once per pass of RT directions: passes = ceil(nrecv / RT) block rows of one launch per
            256 directions -- counted from lsfc_receivers_info and the launch geometry of csrc/receivers.hip, not timed.

usage: python tools/bench_receivers.py [--out FILE] [--quick]      (--quick: 64^3 / 128^2, for a rehearsal of the tool itself)"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fast_solver_lippmann_schwinger_amd as lsfc  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "receivers.jsonl")
COPY_CEILING = 6.29e12          # bytes/s, VERDICT.md
FP64_PEAK = 78.6e12             # FLOP/s, vector, datasheet
ROUNDS, WINDOW_S = 3, 0.2
FLOPS = {("points", 3): (14 + 60, 8), ("points", 2): (8 + 300, 8), ("far", 3): (6, 8), ("far", 2): (6, 8)}   # (per pair, per pair and member)


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


def reps_for(fn):
    fn()                                                    # warm-up of the shape (work buffers, code object)
    torch.cuda.synchronize()
    one = max(timed(fn, 1), 1e-3)
    return max(1, math.ceil(WINDOW_S * 1e3 / one))


def measure(fns):
    """fns: name -> callable; alternated over ROUNDS; -> name -> (best ms, spread, reps)"""
    reps = {k: reps_for(f) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            ms[k].append(timed(f, reps[k]))
    return {k: {"ms": min(v), "spread": max(v) / min(v) - 1, "reps": reps[k]} for k, v in ms.items()}


def rates(kind, ndim, N, nrecv, nrhs, ms, rt):
    per_pair, per_member = FLOPS[(kind, ndim)]
    pairs = N * nrecv * nrhs
    flops = N * nrecv * (per_pair + per_member * nrhs)
    out = {"pairs_per_s": pairs / (ms * 1e-3), "model_flops_per_s": flops / (ms * 1e-3), "share_of_fp64_peak": flops / (ms * 1e-3) / FP64_PEAK}
    if kind == "far":
        passes = -(-nrecv // rt)
        by = N * 16 * passes * nrhs
        out.update({"passes_over_q": passes, "model_bytes_per_s": by / (ms * 1e-3), "share_of_copy_ceiling": by / (ms * 1e-3) / COPY_CEILING})
        out["nearer_bound"] = "bandwidth" if out["share_of_copy_ceiling"] >= out["share_of_fp64_peak"] else "fp64 vector"
    return out


def sphere(count, ndim, radius, seed=1):
    v = np.random.default_rng(seed).standard_normal((count, ndim))
    return radius * v / np.linalg.norm(v, axis=1)[:, None]


def main(quick):
    n3, n2 = (64, 128) if quick else (256, 1024)
    h3 = 1.0 / n3
    x3 = -0.5 + h3 * np.arange(n3)
    k3 = 0.25 / h3                                          # k h = 0.25: k r stays below 200 at radius 2
    nu = np.random.default_rng(0).uniform(0.0, 0.3, n3 ** 3)
    M = lsfc.buildFastConvolution3D(x3, x3, x3, None, None, None, h3, k3, nu)
    N3 = n3 ** 3
    q = torch.randn(N3, dtype=torch.complex128, device="cuda")
    for nrecv in (256, 1024):
        R = lsfc.Receivers(x3, x3, x3, k=k3, points=sphere(nrecv, 3, 2.0))
        rt = R.info()["receivers_per_thread"]
        w = torch.randn(nrecv, dtype=torch.complex128, device="cuda")
        res = measure({"N": lambda: R * q, "H": lambda: R.H * w, "N_fused": lambda: R.scattered_field(M, q)})
        for name, r in res.items():
            emit({"case": f"3d{n3}_points{nrecv}_{name}", "kind": "points", "ndim": 3, "N": N3, "nrecv": nrecv, "nrhs": 1, **r,
                  **rates("points", 3, N3, nrecv, 1, r["ms"], rt)})
        if nrecv == 256:
            Q8 = torch.randn(8, N3, dtype=torch.complex128, device="cuda")
            res = measure({"group_of_8": lambda: R.apply_batch(Q8), "eight_singles": lambda: [R * Q8[j] for j in range(8)]})
            emit({"case": f"3d{n3}_points256_nrhs8", "kind": "points", "ndim": 3, "N": N3, "nrecv": nrecv, "nrhs": 8, **{k: v for k, v in res.items()},
                  "group_over_singles": res["group_of_8"]["ms"] / res["eight_singles"]["ms"], **rates("points", 3, N3, nrecv, 8, res["group_of_8"]["ms"], rt)})
            del Q8
        R.close()
    Rf = lsfc.Receivers(x3, x3, x3, k=k3, directions=sphere(256, 3, 1.0))
    info = Rf.info()
    rt = info["receivers_per_thread"]
    res = measure({"N": lambda: Rf * q})
    emit({"case": f"3d{n3}_far256_N", "kind": "far", "ndim": 3, "N": N3, "nrecv": 256, "nrhs": 1, "table_bytes": info["table_bytes"], **res["N"],
          **rates("far", 3, N3, 256, 1, res["N"]["ms"], rt), "forward_launches_per_group": -(-256 // 256), "block_rows_per_launch": -(-256 // rt)})
    Q8 = torch.randn(8, N3, dtype=torch.complex128, device="cuda")
    res = measure({"group_of_8": lambda: Rf.apply_batch(Q8), "eight_singles": lambda: [Rf * Q8[j] for j in range(8)]})
    emit({"case": f"3d{n3}_far256_nrhs8", "kind": "far", "ndim": 3, "N": N3, "nrecv": 256, "nrhs": 8, **{k: v for k, v in res.items()},
          "group_over_singles": res["group_of_8"]["ms"] / res["eight_singles"]["ms"], **rates("far", 3, N3, 256, 8, res["group_of_8"]["ms"], rt)})
    del Q8, q
    Rf.close()
    M.close()
    torch.cuda.empty_cache()
    h2 = 1.0 / n2
    x2 = -0.5 + h2 * np.arange(n2)
    k2 = 40.0
    R2 = lsfc.Receivers(x2, x2, k=k2, points=sphere(360, 2, 2.0))
    q2 = torch.randn(n2 * n2, dtype=torch.complex128, device="cuda")
    w2 = torch.randn(360, dtype=torch.complex128, device="cuda")
    res = measure({"N": lambda: R2 * q2, "H": lambda: R2.H * w2})
    for name, r in res.items():
        emit({"case": f"2d{n2}_points360_{name}", "kind": "points", "ndim": 2, "N": n2 * n2, "nrecv": 360, "nrhs": 1, **r,
              **rates("points", 2, n2 * n2, 360, 1, r["ms"], R2.info()["receivers_per_thread"])})
    R2.close()


if __name__ == "__main__":
    if any(a in ("-h", "--help") for a in sys.argv[1:]):
        sys.exit(__doc__)
    if "--out" in sys.argv:
        OUT = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    main("--quick" in sys.argv)
