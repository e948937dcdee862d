"""SHA-256 of the output of a fixed list of small applies: the bitwise fingerprint of the host side of a plan (csrc/plan.hip,
csrc/apply.hip, csrc/host_apply.hip).  Two builds of the library that print the same lines create the same plans, choose the same
kernels and hand them the same arguments.

The applies (seeded inputs; device vectors unless "host" is said):
  3D pruned            Greengard-Vico on 16^3 and on 24 x 20 x 40: M * b and the bare convolution
  2D pruned            Greengard-Vico on 64 x 64, natural rows and tiles (LSFC_2D_TILED=1)
  rocFFT-reduced       a random even symbol on 5 x 4 x 3
  LSFC_FLAG_LITERAL_PAD   the same kind of symbol in 2D, on its own (48 x 40) grid
  apply_batch          16^3, three right-hand sides, modes 0, 1, 2, fused (batch_fuse = 1) and member by member (0)
  host vectors         16^3 with LSFC_HOST_PIPELINE = 0 and 2, one and three right-hand sides
  M.T, M.H             16^3 and 5 x 4 x 3
  sampleG3D            16^3, three sources
  describe_passes      every plan above under the defaults, one and three right-hand sides
  line lengths         every line length of tests/test_gpu_apply_forms.py (LENGTHS) as the long axis L/2 of thin plans -- 3D along
                       x, y and z, 2D along y (the fused axis), 16 points along the other axes -- on random even symbols: M * b, the
                       bare convolution and describe_passes under the default tuning and under z_persist = 3, 5, 6; apply_batch of
                       three right-hand sides under the default tuning
  slab plans           MultiDeviceFastM3D with a device listed several times -- 64 x 16 x 16 on [0]*4 (K = 4) under LSFC_DIST_OVERLAP
                       1 / 0, LSFC_DIST_SPLIT_EDGES 1 / 0 and LSFC_DIST_COMPUTE_STREAMS 1 / 2, 16 x 16 x 12 on [0]*4 (three planes per
                       rank: no split of the pipeline ends), 32 x 16 x 16 on [0]*8 --, SimulatedRanks with two ranks, and
                       build_distributed_3d with one rank, sequential and under LSFC_DIST_FORCE_OVERLAP=1 LSFC_DIST_CHUNKS=4:
                       M * b and the bare convolution, host vectors and device slabs

    python tools/apply_digest.py                                    one JSON line per apply, this tree's library
    python tools/apply_digest.py --libs parent=/path/to/liblsfc.so,this= [--out profiles/plan_split_refactor.jsonl]
                                                                    one fresh child process per build (LSFC_LIBRARY; an empty
                                                                    path is the library of this tree), one line per apply
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

ENV = ("LSFC_2D_TILED", "LSFC_HOST_PIPELINE", "LSFC_BATCH_FUSE", "LSFC_HOST_COPY", "LSFC_DIST_OVERLAP", "LSFC_DIST_SPLIT_EDGES",
       "LSFC_DIST_COMPUTE_STREAMS", "LSFC_DIST_CHUNKS", "LSFC_DIST_FORCE_OVERLAP", "LSFC_DIST_FORCE_COMM", "LSFC_MULTI_TRANSPORT")


def emit(label, a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    data = a.encode() if isinstance(a, str) else np.ascontiguousarray(a).tobytes()
    print("DIGEST " + json.dumps({"apply": label, "sha256": hashlib.sha256(data).hexdigest()}), flush=True)


def child():
    import torch
    import fast_solver_lippmann_schwinger_amd as lsfc

    for k in ENV:
        os.environ.pop(k, None)
    rng = np.random.default_rng(2024)

    def vec(N, rows=None):
        shape = (N,) if rows is None else (rows, N)
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)

    def bump(*axes):
        g = [np.exp(-40 * a ** 2) for a in axes]
        out = 0.3 * g[0]
        for a in g[1:]:
            out = out[..., None] * a
        return out.reshape(-1)

    def even_symbol(grid):                              # centred order, even in every axis: the Green's matrix is symmetric
        G = rng.standard_normal(grid) + 1j * rng.standard_normal(grid)
        for ax in range(len(grid)):
            G = 0.5 * (G + np.roll(np.flip(G, axis=ax), 1, axis=ax))
        return np.fft.fftshift(G)

    def describe(label, M):
        emit(f"{label} describe_passes", M.pipeline + "\n" + M.describe_passes(1) + M.describe_passes(3))

    def applies(label, M, convolve=True):
        describe(label, M)
        b = torch.from_numpy(vec(M.N)).cuda()
        emit(f"{label} M*b", M * b)
        if convolve:
            emit(f"{label} convolution", lsfc.FFTconvolution(M, b))
        return b

    def axis(n):
        return -0.5 + np.arange(n) / 16.0

    # 3D pruned
    x = axis(16)
    M16 = lsfc.buildFastConvolution3D(x, x, x, None, None, None, 1.0 / 16, 16.0, bump(x, x, x))
    b16 = applies("3D 16^3", M16)
    x, y, z = axis(24), axis(20), axis(40)
    M = lsfc.buildFastConvolution3D(x, y, z, None, None, None, 1.0 / 16, 12.0, bump(x, y, z))
    applies("3D 24x20x40", M)
    M.close()

    # 2D pruned: natural rows, tiles
    x = -0.5 + np.arange(64) / 64.0
    for tiled in ("0", "1"):
        os.environ["LSFC_2D_TILED"] = tiled
        M = lsfc.buildFastConvolution(x, x, 1.0 / 64, 40.0, lambda X, Y: 0.3 * np.exp(-40 * (X ** 2 + Y ** 2)), quadRule="Greengard_Vico")
        applies(f"2D 64x64 LSFC_2D_TILED={tiled}", M)
        M.close()
    os.environ.pop("LSFC_2D_TILED")

    # rocFFT-reduced, and the literal grid in 2D
    Mr = lsfc.FastM3D(even_symbol((10, 8, 6)), rng.uniform(-0.3, 0.3, 60), 10, 8, 6, 5, 4, 3, 2.0)
    br = applies("rocFFT 5x4x3", Mr)
    M = lsfc.FastM(even_symbol((48, 40)), rng.uniform(-0.3, 0.3, 24 * 20), 48, 40, 24, 20, 2.0, quadRule="Greengard_Vico", flags=lsfc._lib.LSFC_FLAG_LITERAL_PAD)
    applies("2D 24x20 LITERAL_PAD", M, convolve=False)
    M.close()

    # transpose and adjoint
    for label, M, b in (("3D 16^3", M16, b16), ("rocFFT 5x4x3", Mr, br)):
        emit(f"{label} M.T*b", M.T * b)
        emit(f"{label} M.H*b", M.H * b)
    Mr.close()

    # batches of three
    B = vec(M16.N, 3)
    Bd = torch.from_numpy(B).cuda()
    for fuse in (1, 0):
        M16.set_tuning(batch_fuse=fuse)
        for mode in (0, 1, 2):
            emit(f"apply_batch 16^3 nrhs=3 mode={mode} batch_fuse={fuse}", lsfc.apply_batch(M16, Bd, mode))
    M16.set_tuning(batch_fuse=-1)

    # host vectors: one staged copy each way, the chunked pipeline
    for K in ("0", "2"):
        os.environ["LSFC_HOST_PIPELINE"] = K
        emit(f"host 16^3 LSFC_HOST_PIPELINE={K} nrhs=1", M16 * B[0])
        emit(f"host 16^3 LSFC_HOST_PIPELINE={K} nrhs=3", lsfc.apply_batch(M16, B, 0))
    os.environ.pop("LSFC_HOST_PIPELINE")

    emit("sampleG3D 16^3 three sources", lsfc.sampleG3D(16.0, None, None, None, [0, M16.N // 2 + 3, M16.N - 1], M16))
    M16.close()

    # every line length, in every pass that can run it (the bare convolution as a batch of one: FFTconvolution takes square
    # grids only in 2D)
    from test_gpu_apply_forms import LENGTHS

    def conv(M, b):
        return lsfc.apply_batch(M, b.reshape(1, -1), 1)

    for L in LENGTHS:
        thin = {f"3D long {'xyz'[a]}": tuple(L // 2 if d == a else 16 for d in range(3)) for a in range(3)}
        thin["2D long y"] = (16, L // 2)
        for name, dims in thin.items():
            grid = tuple(2 * d for d in dims)
            nu = rng.uniform(-0.3, 0.3, int(np.prod(dims)))
            if len(dims) == 3:
                M = lsfc.FastM3D(even_symbol(grid), nu, *grid, *dims, 2.0)
            else:
                M = lsfc.FastM(even_symbol(grid), nu, *grid, *dims, 2.0, quadRule="Greengard_Vico")
            assert M.pipeline == "pruned-hip", M.pipeline
            label = f"L={L} {name}"
            b = applies(label, M, convolve=False)
            emit(f"{label} convolution", conv(M, b))
            emit(f"{label} apply_batch nrhs=3", lsfc.apply_batch(M, torch.from_numpy(vec(M.N, 3)).cuda(), 0))
            for zp in (3, 5, 6):
                M.set_tuning(z_persist=zp)
                describe(f"{label} z_persist={zp}", M)
                emit(f"{label} z_persist={zp} M*b", M * b)
                emit(f"{label} z_persist={zp} convolution", conv(M, b))
            M.close()


    # slab plans: the ranks of one process (a device listed several times), simulated ranks, one rank of a multi-process plan
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D, SimulatedRanks, build_distributed_3d

    def slab_applies(label, dims, devices):
        n, m, l = dims
        N, P = n * m * l, len(devices)
        M = MultiDeviceFastM3D(n, 1.0 / n, 9.0, rng.uniform(-0.3, 0.3, N), devices=devices, m=m, l=l)
        b = vec(N)
        emit(f"{label} host M*b", M * b)
        emit(f"{label} host convolution", lsfc.FFTconvolution(M, b))
        xs = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in np.split(b, P)]
        ys = [torch.empty_like(x) for x in xs]
        for mode, what in ((0, "M*b"), (1, "convolution")):
            for _ in range(2):                             # back to back: the buffers of the first apply are re-used
                M.apply_dev(xs, ys, mode)
            M.synchronize()
            emit(f"{label} device slabs {what}", torch.cat(ys))
        M.close()

    for overlap in ("1", "0"):
        for edges in ("1", "0"):
            for streams in ("1", "2"):
                os.environ.update(LSFC_DIST_OVERLAP=overlap, LSFC_DIST_SPLIT_EDGES=edges, LSFC_DIST_COMPUTE_STREAMS=streams)
                slab_applies(f"multi 64x16x16 [0]*4 overlap={overlap} edges={edges} streams={streams}", (64, 16, 16), [0] * 4)
    for k in ("LSFC_DIST_OVERLAP", "LSFC_DIST_SPLIT_EDGES", "LSFC_DIST_COMPUTE_STREAMS"):
        os.environ.pop(k)
    slab_applies("multi 16x16x12 [0]*4", (16, 16, 12), [0] * 4)
    slab_applies("multi 32x16x16 [0]*8", (32, 16, 16), [0] * 8)

    n, m, l = 32, 16, 16
    nu, b = rng.uniform(-0.3, 0.3, n * m * l), vec(n * m * l)
    S = SimulatedRanks(n, m, l, 1.0 / n, 9.0, nu, 2)
    emit("SimulatedRanks 32x16x16 P=2 M*b", S.apply(b))
    emit("SimulatedRanks 32x16x16 P=2 convolution", S.convolve(b))
    S.close()
    for label, env in (("sequential", {}), ("LSFC_DIST_FORCE_OVERLAP=1 LSFC_DIST_CHUNKS=4", {"LSFC_DIST_FORCE_OVERLAP": "1", "LSFC_DIST_CHUNKS": "4"})):
        os.environ.update(env)
        M = build_distributed_3d(n, 1.0 / n, 9.0, nu, 0, 1, 0, m=m, l=l)
        emit(f"build_distributed_3d one rank {label} host M*b", M * b)
        emit(f"build_distributed_3d one rank {label} host convolution", lsfc.FFTconvolution(M, b))
        xb = torch.from_numpy(b).cuda()
        yb = torch.empty_like(xb)
        for _ in range(2):
            M.mul_(yb, xb)
        M.synchronize()
        emit(f"build_distributed_3d one rank {label} device M*b", yb)
        emit(f"build_distributed_3d one rank {label} device convolution", lsfc.FFTconvolution(M, xb))
        M.close()
        for k in env:
            os.environ.pop(k)


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
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:                              # (nothing more is started on the device after a child that failed)
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        got[name] = [json.loads(ln[len("DIGEST "):]) for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    a, b = got[na], got[nb]
    if [d["apply"] for d in a] != [d["apply"] for d in b]:
        sys.exit("the two builds ran different lists of applies")
    bad = 0
    for da, db in zip(a, b):
        equal = da["sha256"] == db["sha256"]
        bad += not equal
        line = json.dumps({"check": "apply_digest", "apply": da["apply"], f"sha256_{na}": da["sha256"], f"sha256_{nb}": db["sha256"], "equal": equal})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    print(f"# {len(a)} applies, {bad} differ", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
