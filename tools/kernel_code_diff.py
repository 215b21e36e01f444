#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, function by function.  For each translation unit (engine.o, resnet.o) the code
object is unbundled as tools/kernel_resources.py does; every FUNC symbol's byte range in .text comes from llvm-readelf -sW -S and
the bytes from the section's file offset.  Reported per unit: the symbols of both builds with equal bytes, those whose bytes differ,
and those of one side only.  A host-only change must leave every function byte-identical.  CPU only.
usage: python tools/kernel_code_diff.py BUILD_A BUILD_B [--json out.json]     (BUILD_x: a directory holding engine.o and resnet.o,
       e.g. grok_alpha_zero_amd/csrc/build of two checkouts; A is reported as "parent", B as "this")"""
import json, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
UNITS = ("engine.o", "resnet.o")


def functions(obj):
    """demangled name -> the function's bytes in .text of obj's gfx950 code object"""
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "dev.co"); fb = os.path.join(td, "dev.fatbin")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        txt = subprocess.check_output([f"{LLVM}/llvm-readelf", "-sW", "-S", co], text=True)
        blob = open(co, "rb").read()
    # section header line: [Nr] Name Type Address Off Size ...
    m = re.search(r"^\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", txt, re.M)
    ndx, addr, off, size = int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16)
    syms = {}
    # symbol line: Num: Value Size Type Bind Vis Ndx Name
    for s in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+(\d+)\s+(\S+)", txt, re.M):
        if int(s.group(3)) != ndx:
            continue
        v, n = int(s.group(1), 16), int(s.group(2))
        assert addr <= v and v + n <= addr + size, s.group(4)
        syms[s.group(4)] = blob[off + v - addr: off + v - addr + n]
    names = subprocess.check_output(["c++filt"], input="\n".join(syms), text=True).split("\n")
    return {d: syms[k] for k, d in zip(syms, names)}


def compare(dir_a, dir_b):
    report = {}
    for u in UNITS:
        a, b = functions(os.path.join(dir_a, u)), functions(os.path.join(dir_b, u))
        both = sorted(set(a) & set(b))
        report[u] = dict(functions_parent=len(a), functions_this=len(b),
                         identical=sum(a[k] == b[k] for k in both),
                         different=[dict(function=k, bytes=[len(a[k]), len(b[k])]) for k in both if a[k] != b[k]],
                         only_in_parent=sorted(set(a) - set(b)), only_in_this=sorted(set(b) - set(a)))
    return report


if __name__ == "__main__":
    args = [x for i, x in enumerate(sys.argv[1:], 1) if x != "--json" and sys.argv[i - 1] != "--json"]
    if len(args) != 2:
        sys.exit(__doc__)
    rep = compare(*args)
    for u, r in rep.items():
        print(f'{u}: {r["functions_parent"]} | {r["functions_this"]} functions, {r["identical"]} identical, {len(r["different"])} different, '
              f'{len(r["only_in_parent"])} only in the first build, {len(r["only_in_this"])} only in the second')
        for d in r["different"]:
            print(f'  differs ({d["bytes"][0]} | {d["bytes"][1]} bytes): {d["function"]}')
        for k in r["only_in_parent"]:
            print(f"  only in the first:  {k}")
        for k in r["only_in_this"]:
            print(f"  only in the second: {k}")
    if "--json" in sys.argv:
        json.dump(dict(what="gfx950 device code per function symbol (tools/kernel_code_diff.py): bytes of .text, the parent's build against this one",
                       units=rep), open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
