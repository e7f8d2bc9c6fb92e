#!/usr/bin/env python3
"""Build a variant of the library: one source compiled with extra defines, linked with the in-tree objects of every other source.

    python tools/variant.py NAME SOURCE.hip [-DFLAG ...]      e.g.  python tools/variant.py v6_abl1 conv3x3_v6.hip -DV6_ABL=1

writes scratch/x/NAME/lib.so and prints its path; HRNET_HIP_LIB=<that path> then makes any tool or test run on it.  The compiler, its
flags, the source list and the object directory are hrnet_hip/build.py's own; missing or stale in-tree objects are built first.  Needs
no GPU: hipcc cross-compiles."""
import os
import subprocess

import _common
from hrnet_hip import build


PARSER = _common.parser(__doc__)
PARSER.add_argument("name", metavar="NAME")
PARSER.add_argument("source", metavar="SOURCE.hip", choices=build.SOURCES)
PARSER.add_argument("-D", dest="defines", action="append", default=[], metavar="FLAG")


def main():
    o = PARSER.parse_args()
    build.build_library(verbose=False)
    out = os.path.join(_common.ROOT, "scratch", "x", o.name)
    os.makedirs(out, exist_ok=True)
    obj = lambda src, where: os.path.join(where, src.replace(".hip", ".o"))
    subprocess.run([build._hipcc()] + build.FLAGS + ["-D" + d for d in o.defines]
                   + ["-c", os.path.join(build.CSRC, o.source), "-o", obj(o.source, out)], check=True)
    lib = os.path.join(out, "lib.so")
    subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib]
                   + [obj(s, out if s == o.source else build.OBJ) for s in build.SOURCES], check=True)
    print(lib)


if __name__ == "__main__":
    main()
