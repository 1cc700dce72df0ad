#!/usr/bin/env python3
"""Which kernels of libleon_hip's device code changed between two trees: compiles leon_hip.cpp of each with hipcc -S
--cuda-device-only for gfx950 (no GPU needed) and compares kernel by kernel the instructions (block labels normalised) and,
separately, the kernel descriptor (the .amdhsa_* lines: static LDS, kernarg size, register counts, ...).
    python tools/kernel_asm_diff.py OTHER_TREE [THIS_TREE] [--show KERNEL] [--rename OLD=NEW ...]
e.g. OTHER_TREE = a `git worktree` of the parent commit.
Prints the kernels that are identical, differ, are new and are gone; --show prints a unified diff of the normalised instructions
and descriptors of every kernel whose name contains KERNEL.  --rename pairs a kernel that was renamed, or whose template arguments
changed: OLD is its (mangled) name in OTHER_TREE, NEW its name here, both spelled out by the user (`c++filt` shows what a
name says); it is then compared with its predecessor instead of showing as gone + new.  A rename onto a name that OTHER_TREE has
too wins: that kernel of OTHER_TREE's is compared with nothing and shows as gone.  Exit status 1 when a kernel both trees have differs
in either."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(lines):
    """{kernel: (instructions, descriptor lines)} of an assembly listing"""
    ins, desc, cur, hsa = {}, {}, None, None
    for line in lines:
        m = re.match(r"^(_Z\w+):", line)
        text = re.sub(r";.*", "", re.sub(r"\.LBB\d+_", ".LBB_", line)).strip()
        if m and "k_" in m.group(1):
            cur = m.group(1)
            ins[cur] = []
        elif text.startswith(".amdhsa_kernel "):
            hsa = text.split()[1]
            desc[hsa] = []
        elif text == ".end_amdhsa_kernel":
            hsa = None
        elif hsa is not None:
            if text.startswith(".amdhsa_"):
                desc[hsa].append(text)
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            elif text and not text.startswith("."):
                ins[cur].append(text)
    return {k: (ins[k], desc.get(k, [])) for k in ins}


def kernels(tree):
    src = os.path.join(tree, "mpeg1video-decoder-webgl_amd", "csrc", "leon_hip.cpp")
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S",
                        "--cuda-device-only", "-o", f.name, src], check=True, capture_output=True, timeout=900)
        with open(f.name) as s:
            return parse(s)


def rename(a, renamed):
    """(OTHER_TREE's kernels under this tree's names, the names of those a rename displaced): a renamed kernel takes its new name
    whichever kernel had it there"""
    out = {renamed[k]: v for k, v in a.items() if k in renamed}
    displaced = sorted(k for k in a if k not in renamed and k in out)
    out.update((k, v) for k, v in a.items() if k not in renamed and k not in out)
    return out, displaced


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other_tree")
    ap.add_argument("this_tree", nargs="?", default=ROOT)
    ap.add_argument("--show", metavar="KERNEL", help="print the diffs of the kernels whose name contains KERNEL")
    ap.add_argument("--rename", metavar="OLD=NEW", action="append", default=[], help="compare OTHER_TREE's kernel OLD with this tree's NEW")
    args = ap.parse_args(argv)
    show = args.show
    renamed = dict(r.split("=", 1) for r in args.rename)
    a, b = kernels(args.other_tree), kernels(args.this_tree)
    n_there = len(a)
    a, displaced = rename(a, renamed)
    gone = sorted(set(a) - set(b)) + displaced
    both = sorted(k for k in a if k in b)
    differ = [k for k in both if a[k][0] != b[k][0]]
    desc_differ = [k for k in both if a[k][1] != b[k][1]]
    print("%d kernels there, %d here: %d identical, %d differ, %d descriptor differs, %d new, %d gone" % (
        n_there, len(b), sum(1 for k in both if a[k] == b[k]), len(differ), len(desc_differ), len(set(b) - set(a)), len(gone)))
    for what, names in (("differs", differ), ("descriptor differs", desc_differ), ("new", sorted(set(b) - set(a))), ("gone", gone)):
        for k in names:
            print("  %s: %s" % (what, k))
    if show is not None:
        if not any(show in k for k in both):
            print("--show: no kernel of both trees has %r in its name" % show)
        for k in both:
            if show in k:
                for part, what in ((0, "instructions"), (1, "descriptor")):
                    sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[k][part], b[k][part], "there/%s %s" % (k, what),
                                                                                "here/%s %s" % (k, what), lineterm=""))
    return 1 if differ or desc_differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
