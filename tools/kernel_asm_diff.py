#!/usr/bin/env python3
"""Which kernels of libleon_hip's device code changed between two trees: compiles leon_hip.cpp of each with hipcc -S
--cuda-device-only for gfx950 (no GPU needed) and compares the instructions kernel by kernel, block labels normalised.
    python tools/kernel_asm_diff.py OTHER_TREE [THIS_TREE]        e.g. OTHER_TREE = a `git worktree` of the parent commit
Prints the kernels that are identical, differ, are new and are gone; exit status 1 when a kernel both trees have differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernels(tree):
    src = os.path.join(tree, "mpeg1video-decoder-webgl_amd", "csrc", "leon_hip.cpp")
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-o", f.name, src], check=True, capture_output=True, timeout=900)
        out, cur = {}, None
        for line in open(f.name):
            m = re.match(r"^(_Z\w+):", line)
            if m and "k_" in m.group(1):
                cur = m.group(1)
                out[cur] = []
            elif cur is not None:
                if line.startswith(".Lfunc_end"):
                    cur = None
                    continue
                ins = re.sub(r";.*", "", re.sub(r"\.LBB\d+_", ".LBB_", line)).strip()
                if ins and not ins.startswith("."):
                    out[cur].append(ins)
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2] if len(sys.argv) > 2 else ROOT)
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print("%d kernels there, %d here: %d identical, %d differ, %d new, %d gone" % (
        len(a), len(b), sum(1 for k in a if b.get(k) == a[k]), len(differ), len(set(b) - set(a)), len(set(a) - set(b))))
    for what, names in (("differs", differ), ("new", sorted(set(b) - set(a))), ("gone", sorted(set(a) - set(b)))):
        for k in names:
            print("  %s: %s" % (what, k))
    sys.exit(1 if differ else 0)
