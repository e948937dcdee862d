"""The device code of the three line-length families, kernel by kernel: the check that a change to the host half of
csrc/fft_kernels.hip left every kernel as it was.  No GPU is needed.

For each of build/fft_kernels_f{2,3,5}.o under a csrc directory: take the .hip_fatbin section (llvm-objcopy), unbundle the gfx950
code object (clang-offload-bundler), read its sections and symbols (llvm-readelf), and give per kernel
  name   the mangled name of the kernel
  code   SHA-256 of its bytes in .text
  kd     SHA-256 of its 64-byte descriptor <name>.kd, with the 8-byte code-entry offset at byte 16 zeroed (that field moves when
         the kernels are emitted in another order)
The code objects have no relocations and .rodata holds nothing but the descriptors, so a kernel's bytes do not depend on where it
is placed.

    python tools/kernel_set.py [CSRC]                  one JSON line per kernel (CSRC: this tree's csrc directory)
    python tools/kernel_set.py --compare A B [--out profiles/pruned_args_refactor.jsonl]
                                                       A, B: csrc directories of two builds.  One JSON line per family: kernels,
                                                       names only in A, names only in B, kernels whose code or descriptor
                                                       differs; exit status 1 if any of the three counts is not zero
    python tools/kernel_set.py --compare-objects A1.o[,A2.o...] B1.o[,B2.o...] [--out profiles/blocktri_split_refactor.jsonl]
                                                       the same comparison between the union of the kernels of the objects A
                                                       and the union of those of B (a source file split in two, say): one JSON
                                                       line.  A name in two objects of one side is an error.  Names that
                                                       contain k_warmup_ (one empty kernel per unit) are listed apart and are
                                                       no difference."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast_solver_lippmann_schwinger_amd", "csrc")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FAMILIES = (2, 3, 5)


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def kernels(obj):
    """{kernel name: {"code": sha256, "kd": sha256}} of the gfx950 code object inside a host object file"""
    with tempfile.TemporaryDirectory() as tmp:
        fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin)
        if os.path.getsize(fatbin) == 0:            # no such section: a unit without device code
            return {}
        tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={co}")
        listing = tool("llvm-readelf", "-S", "-s", "-W", co)
        with open(co, "rb") as f:
            image = f.read()
    sections, symbols = {}, {}                      # index -> (name, address, file offset); name -> (address, size, section index)
    for ln in listing.splitlines():
        if ln.lstrip().startswith("["):             # "  [ 7] .text PROGBITS <address> <offset> <size> ..."
            w = ln[ln.index("]") + 1:].split()
            if len(w) >= 5 and w[0].startswith("."):
                sections[int(ln[ln.index("[") + 1:ln.index("]")])] = (w[0], int(w[2], 16), int(w[3], 16))
            continue
        w = ln.split()                              # "  Num: Value Size Type Bind Vis Ndx Name"
        if len(w) == 8 and w[0].endswith(":") and w[0][:-1].isdigit() and w[6].isdigit():
            symbols[w[7]] = (int(w[1], 16), int(w[2]), int(w[6]))

    def content(name):
        addr, size, ndx = symbols[name]
        _, saddr, soff = sections[ndx]
        return image[soff + addr - saddr:soff + addr - saddr + size]

    out = {}
    for name, (_, size, ndx) in symbols.items():
        if not name.endswith(".kd"):
            continue
        kernel = name[:-3]
        if size != 64 or kernel not in symbols or sections[symbols[kernel][2]][0] != ".text":
            sys.exit(f"{obj}: {name}: not a 64-byte descriptor of a kernel in .text")
        kd = bytearray(content(name))
        kd[16:24] = bytes(8)
        out[kernel] = {"code": hashlib.sha256(content(kernel)).hexdigest(), "kd": hashlib.sha256(kd).hexdigest()}
    return out


def family_object(csrc, fam):
    return os.path.join(csrc, "build", f"fft_kernels_f{fam}.o")


def union(objs):
    """the kernels of several object files as one set, without the warm-up kernels: (kernels, sorted names of the warm-up kernels)"""
    out, warmup = {}, []
    for obj in objs:
        for name, h in kernels(obj).items():
            if name in out or name in warmup:
                sys.exit(f"{obj}: kernel {name} is in another object of the same side as well")
            if "k_warmup_" in name:
                warmup.append(name)
            else:
                out[name] = h
    return out, sorted(warmup)


def compare(what, a, b, out, **more):
    """One JSON line on the kernel sets a and b (printed, appended to `out`); the number of names on one side only or differing"""
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for tag, names in (("only in A", only_a), ("only in B", only_b), ("differs", differ)):
        for k in names:
            print(f"# {what}, {tag}: {k}", file=sys.stderr)
    line = json.dumps({"check": "kernel_set", **more, "kernels_a": len(a), "kernels_b": len(b), "only_in_a": len(only_a),
                       "only_in_b": len(only_b), "differ": len(differ)})
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")
    return len(only_a) + len(only_b) + len(differ)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("csrc", nargs="?", default=CSRC, help="csrc directory of a build (default: this tree's)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="csrc directories of two builds")
    ap.add_argument("--compare-objects", nargs=2, metavar=("A", "B"), help="two comma-separated lists of object files")
    ap.add_argument("--out", default="", help="append the comparison lines to this file")
    args = ap.parse_args()
    if args.compare_objects:
        sides = [spec.split(",") for spec in args.compare_objects]
        (a, warm_a), (b, warm_b) = (union(objs) for objs in sides)
        names = [[os.path.basename(o) for o in objs] for objs in sides]
        bad = compare(" ".join(names[0]), a, b, args.out, objects_a=names[0], objects_b=names[1], warmup_a=warm_a, warmup_b=warm_b)
        return 1 if bad else 0
    if not args.compare:
        for fam in FAMILIES:
            for name, h in sorted(kernels(family_object(args.csrc, fam)).items()):
                print(json.dumps({"family": fam, "name": name, **h}))
        return 0
    bad = 0
    for fam in FAMILIES:
        a, b = (kernels(family_object(d, fam)) for d in args.compare)
        bad += compare(f"family {fam}", a, b, args.out, family=fam)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
