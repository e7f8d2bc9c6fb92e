#!/usr/bin/env python3
"""Compare the gfx950 device code of two checkouts of this repository, function by function.  No GPU needed.

    python tools/device_code_diff.py <tree_a> <tree_b> [--jobs N] [--keep DIR] [--opcodes]

Every entry of SOURCES in each tree's highres-net_amd/hrnet_hip/build.py is compiled with that file's FLAGS plus
`--offload-device-only -S`.  The assembly is split per function symbol (the order in which templates are instantiated may move with
the host code), and for every symbol the instructions and the `.amdhsa_kernel` descriptor (VGPR / SGPR counts, LDS size, scratch)
are compared.  What is ignored: comments, the lines that mention `__hip_cuid_` (the compilation-unit id, which differs between any
two compiles), and the per-file running number inside local labels (`.LBB7_3` is block 3 of the file's 8th function).

Prints the device functions per source and every symbol that differs, and exits non-zero on any difference - a symbol present in one
tree only included.  A refactor that claims to touch host code only has to come out of this with "device code identical".  For one
that moves device code without changing what it computes, --opcodes lists under every differing symbol the opcodes whose counts differ
and the descriptor lines that differ.
"""
import argparse
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.join("highres-net_amd", "hrnet_hip")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")      # .LBB7_3 -> .LBB_3, .Lfunc_end7 -> .Lfunc_end
FUNC_BEGIN = re.compile(r"^\s*\.type\s+(\S+),@function")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")


def load_build(tree):
    """SOURCES, FLAGS and the compiler of one tree, from its own build.py."""
    path = os.path.join(tree, PKG, "build.py")
    spec = importlib.util.spec_from_file_location("hrnet_build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.SOURCES), list(mod.FLAGS), mod._hipcc()


def compile_asm(tree, out_dir, jobs):
    """-> {source: path of its device assembly}"""
    sources, flags, hipcc = load_build(tree)
    os.makedirs(out_dir, exist_ok=True)

    def run(src):
        out = os.path.join(out_dir, src.replace(".hip", ".s"))
        cmd = [hipcc] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(tree, PKG, "csrc", src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout}{r.stderr}")
        return src, out

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        return dict(ex.map(run, sources))


def clean(line):
    line = line.split(";", 1)[0].strip()
    return LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), " ".join(line.split()))


def functions(path):
    """-> {symbol: (instructions, descriptor)}: the cleaned lines of each function of one assembly file, its `.amdhsa_kernel` block
    (None for a device function that is no kernel) apart."""
    out, name, code, desc, in_desc = {}, None, [], None, False
    with open(path) as f:
        for raw in f:
            if "__hip_cuid_" in raw:
                continue
            if name is None:
                m = FUNC_BEGIN.match(raw)
                if m:
                    name, code, desc, in_desc = m.group(1), [], None, False
                continue
            if FUNC_END.match(raw):
                out[name] = (tuple(code), tuple(desc) if desc is not None else None)
                name = None
                continue
            line = clean(raw)
            if not line:
                continue
            if line.startswith(".amdhsa_kernel "):
                desc, in_desc = [], True
            elif line == ".end_amdhsa_kernel":
                in_desc = False
            elif in_desc:
                desc.append(line)
            else:
                code.append(line)
    if name is not None:
        raise RuntimeError(f"{path}: function {name} has no end label")
    return out


def library(asm):
    """-> ({symbol: set of (instructions, descriptor)} over every source, {source: number of device functions})"""
    lib, per_source = {}, {}
    for src, path in sorted(asm.items()):
        fns = functions(path)
        per_source[src] = len(fns)
        for sym, body in fns.items():
            lib.setdefault(sym, set()).add(body)
    return lib, per_source


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {i}: `{x}` / `{y}`"
    return f"{len(a)} / {len(b)} lines"


def opcode_differences(a, b):
    """-> [(opcode, count in a, count in b)] of the opcodes that two instruction lists do not hold equally often; labels are left out"""
    count = lambda code: collections.Counter(line.split()[0] for line in code if not line.endswith(":"))
    ca, cb = count(a), count(b)
    return [(op, ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(6, os.cpu_count() or 1), help="parallel compiles (default %(default)s)")
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly under DIR/a and DIR/b instead of a temporary directory")
    ap.add_argument("--opcodes", action="store_true", help="under every symbol that differs, the opcodes whose counts differ: a / b")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        libs = []
        for tag, tree in (("a", args.tree_a), ("b", args.tree_b)):
            libs.append(library(compile_asm(os.path.abspath(tree), os.path.join(work, tag), args.jobs)))
    (la, na), (lb, nb) = libs
    print(f"{'source':<22}{'device functions a':>20}{'b':>6}")
    for src in sorted(set(na) | set(nb)):
        print(f"{src:<22}{na.get(src, '-'):>20}{nb.get(src, '-'):>6}")
    kernels = lambda lib: sum(1 for bodies in lib.values() if any(d is not None for _, d in bodies))
    print(f"{len(la)} / {len(lb)} device functions, {kernels(la)} / {kernels(lb)} of them kernels")
    bad = 0
    for sym in sorted(set(la) | set(lb)):
        if sym not in la or sym not in lb:
            print(f"ONLY IN {'b' if sym not in la else 'a'}: {sym}")
        elif la[sym] != lb[sym]:
            (ca, da), (cb, db) = min(la[sym], key=repr), min(lb[sym], key=repr)
            what = "instructions, " + first_difference(ca, cb) if ca != cb else "descriptor, " + first_difference(da or (), db or ())
            print(f"DIFFERS: {sym} ({what})")
            if args.opcodes:
                for op, x, y in opcode_differences(ca, cb):
                    print(f"    {op:<28}{x:>7}{y:>7}")
                for x, y in zip(da or (), db or ()):
                    if x != y:
                        print(f"    {x} / {y.split()[-1]}")
        else:
            continue
        bad += 1
    print("device code identical" if not bad else f"{bad} symbols differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
