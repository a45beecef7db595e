#!/usr/bin/env python3
"""Is the device code of two trees the same?  The gate for source-only refactors of hpc-ops_amd/csrc.

    python tools/isa_same.py PARENT_ROOT BRANCH_ROOT [-j N] [--only stem[,stem...]]

Every csrc/*.hip of both trees is compiled to device assembly (`-S --cuda-device-only`) with the flags of that tree's own
build.py (_flags() + _PER_FILE_FLAGS), once as the product and once with -DHPC_DEV=1.  `__hip_cuid_<hash>` hashes the
source path, so it is replaced by a constant; every other line must match.  Needs hipcc, no GPU.  Exit status 1 on any
difference (or a file that exists in one tree only).
"""
import argparse
import concurrent.futures as cf
import difflib
import importlib.util
import re
import subprocess
import sys
from pathlib import Path

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def load_build(root: Path):
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(root))), root / "hpc-ops_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def asm(bld, stem: str, dev: bool) -> list:
    src = bld.CSRC / (stem + ".hip")
    cmd = ["hipcc"] + bld._flags() + (["-DHPC_DEV=1"] if dev else []) + bld._PER_FILE_FLAGS.get(stem, [])
    cmd += ["-S", "--cuda-device-only", str(src), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-3000:]))
    return CUID.sub("__hip_cuid_X", r.stdout).splitlines()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent", type=Path)
    ap.add_argument("branch", type=Path)
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", default="", help="comma-separated file stems (default: every csrc/*.hip)")
    a = ap.parse_args()
    blds = [load_build(a.parent.resolve()), load_build(a.branch.resolve())]
    stems = [sorted(p.stem for p in b.CSRC.glob("*.hip")) for b in blds]
    if stems[0] != stems[1]:
        print("the trees do not hold the same .hip files: %s" % sorted(set(stems[0]) ^ set(stems[1])))
        return 1
    only = [s for s in a.only.split(",") if s]
    jobs = [(s, dev) for s in stems[0] if not only or s in only for dev in (False, True)]
    with cf.ThreadPoolExecutor(max_workers=max(1, min(a.j, 16))) as ex:
        futs = {(s, dev, i): ex.submit(asm, blds[i], s, dev) for s, dev in jobs for i in (0, 1)}
        bad = 0
        for s, dev in jobs:
            old, new = futs[s, dev, 0].result(), futs[s, dev, 1].result()
            diff = [] if old == new else [d for d in difflib.unified_diff(old, new, "parent", "branch", n=0, lineterm="")
                    if d[0] in "+-" and d[:3] not in ("+++", "---")]
            bad += bool(diff)
            print("%-26s %-7s %7d lines  %s" % (s, "dev" if dev else "product", len(old),
                                                 "same" if not diff else "%d DIFFERING LINES" % len(diff)))
            for d in diff[:10]:
                print("    " + d[:160])
    print("%d of %d (file, build) pairs differ" % (bad, len(jobs)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
