"""CPU: what the single front of the dense display tasks (leon_kernels.h, layout 2) may cost and must leave alone.
* The dense P and B display kernels have at most 27 306 bytes of static LDS (163 840 / 6: six workgroups per CU) and use no scratch;
  the B kernel, which runs the single front, keeps its whole LDS there -- three tiles per wave -- and its launch adds none.
* Every other reconstruction kernel (I, sparse, yuva, k_recon, k_recon_display_out) has the instructions it had before the change:
  tests/golden/kernel_asm/recon_kernels_before_single_front.json holds a SHA-256 of each kernel's normalised listing
  (tools/kernel_asm_diff.py parse()), taken from the commit before it with the compiler named there.  Listings of another compiler
  version say nothing about the sources, so they are compared only where the version is the recorded one.
Compiles the device code only (hipcc cross-compiles without a GPU)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_asm_diff  # noqa: E402
import kernel_resources  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
PAIR = ("k_recon_displayILi2ELb0ELb0E", "k_recon_displayILi3ELb0ELb0E")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_asm", "recon_kernels_before_single_front.json")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def test_pair_kernels_fit_six_workgroups_per_cu_without_scratch():
    seen = kernel_resources.report()
    for key in PAIR:
        hit = [v for n, v in seen.items() if key in n]
        assert len(hit) == 1, "kernel %s not found in the resource report" % key
        assert hit[0]["lds"] <= 27306, "%s: %d bytes of LDS per workgroup" % (key, hit[0]["lds"])
        if key == PAIR[1]:      # B: the single front
            assert hit[0]["lds"] >= 3 * 4 * 2048, "%s: the three tiles of four waves are static LDS" % key
        assert hit[0]["scratch"] == 0, "%s spills %d bytes per lane" % (key, hit[0]["scratch"])
    # the launch adds no dynamic LDS on top (leon_hip.cpp, recon_lds_bytes)
    with open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_hip.cpp")) as f:
        assert re.search(r"if \(out == kOutRgba && front3_task\(type, sparse, alpha\)\) return 0;", f.read())


def test_the_other_reconstruction_kernels_kept_their_instructions():
    with open(GOLDEN) as f:
        golden = json.load(f)
    here = kernel_asm_diff.kernels(ROOT)
    ours = {k: v for k, v in here.items() if "k_recon" in k and not any(p in k for p in PAIR)}
    assert set(ours) == set(golden["instructions_sha256"]), "the set of reconstruction kernels changed"
    assert sum(1 for k in here if any(p in k for p in PAIR)) == 2
    version = re.search(r"clang version .*", subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout)
    if version and version.group(0).strip() == golden["compiler"]:
        differ = [k for k, v in ours.items() if hashlib.sha256("\n".join(v[0]).encode()).hexdigest() != golden["instructions_sha256"][k]]
        assert not differ, "kernels whose instructions changed: %s" % differ
