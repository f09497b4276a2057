#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?  The acceptance test of a refactor of the hand-scheduled bodies.

    python tools/isa_diff.py TREE_A TREE_B [unit ...] [--map old=new ...]

Compiles each listed source of build.py's SOURCES (default: all) at both trees, device side only, to assembly (build.py's flags
plus --cuda-device-only -S), cuts it into kernels at their `_Z...k_...:` labels, drops comments and blank lines, and prints SAME or
DIFF per kernel with its line counts, then `TOTAL unit kernels identical`.  A kernel's text is its body up to the function's end
label plus the .amdhsa_ lines of its descriptor (registers, LDS, scratch); function numbers in local labels are dropped.  --map
pairs a kernel of TREE_A with a renamed one of TREE_B by the part of the symbol that changed.  Text is all that is compared.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mdt_policy_amd.build import ARCH, SOURCES, _hipcc  # noqa: E402

LABEL = re.compile(r"^(_Z\w*k_\w*):")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def compile_unit(tree: str, unit: str, out: str) -> str:
    csrc = os.path.join(tree, "mdt_policy_amd", "csrc")
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
           f"-I{os.path.join(tree, 'include')}", f"-I{csrc}", "-o", out, os.path.join(csrc, unit)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}: {unit}\n{res.stderr}")
    return out


def kernels(path: str) -> dict:
    """symbol -> lines of the kernel (its own symbol spelled KERNEL)"""
    out, name, body = {}, None, False
    with open(path) as f:
        for line in f:
            m = LABEL.match(line)
            if m:
                name, body = m.group(1), True
                out[name] = []
                continue
            if name is None:
                continue
            text = line.split(";", 1)[0].strip()
            if text.startswith(".Lfunc_end"):
                body = False
            elif text == ".end_amdhsa_kernel":
                name = None
            elif text and (body or text.startswith(".amdhsa_")):
                out[name].append(LOCAL.sub(r".L\1", text.replace(name, "KERNEL")))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("units", nargs="*", default=SOURCES)
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="symbol part OLD of TREE_A is NEW in TREE_B")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 4))
    args = ap.parse_args()
    renames = [m.split("=", 1) for m in args.map]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, args.jobs)) as ex:
        jobs = {(t, u): ex.submit(compile_unit, tree, u, os.path.join(tmp, f"{t}_{u}.s"))
                for u in args.units for t, tree in (("a", args.tree_a), ("b", args.tree_b))}
        for u in args.units:
            ka, kb = kernels(jobs["a", u].result()), kernels(jobs["b", u].result())
            same = 0
            for name, la in ka.items():
                other = name
                for old, new in renames:
                    if old in name and name.replace(old, new) in kb:
                        other = name.replace(old, new)
                lb = kb.pop(other, None)
                if lb is None:
                    print(f"DIFF {u} {name}: {len(la)} lines, missing in {args.tree_b}")
                elif la == lb:
                    same += 1
                    print(f"SAME {u} {name}: {len(la)} lines")
                else:
                    n = sum(1 for d in difflib.unified_diff(la, lb, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
                    print(f"DIFF {u} {name} -> {other}: {len(la)} / {len(lb)} lines, {n} differ")
            for name, lb in kb.items():
                print(f"DIFF {u} {name}: {len(lb)} lines, missing in {args.tree_a}")
            total = len(ka) + len(kb)
            bad += total - same
            print(f"TOTAL {u} {total} {same}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
