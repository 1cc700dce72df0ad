"""CPU: k_suppress and k_match, the kernels behind leon_pipeline_suppress_regions and leon_pipeline_match_regions
(csrc/leon_overlap.h), exist once each, spill nothing, hold no static LDS -- all of it is dynamic and sized by the launch from
leon_overlap.h's layouts -- and stay within the 128 vector registers below which four waves per SIMD remain resident.  The LDS
figures DESIGN.md 4c states are the layouts' at the largest K: 32768 bytes for a set of 1024 rows, 49156 for a pair of such sets,
inside a CU's 160 KiB.  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import functools
import os
import re
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def report():
    import kernel_resources
    return kernel_resources.report()


def suppress_lds(k):
    """leon_overlap.h's suppress_lds in Python: boxes, keys for K rounded up to a power of two, by, order"""
    slots = 1
    while slots < k:
        slots *= 2
    return 16 * k + 8 * slots + 4 * k + 4 * k


def match_lds(ka, kb):
    """... and match_lds: the boxes, match and best words of either set, the pairs"""
    return 24 * (ka + kb) + 4


@HIPCC
@pytest.mark.parametrize("kernel", ["k_suppress", "k_match"])
def test_each_kernel_exists_once_without_scratch_and_with_dynamic_lds_only(kernel):
    ks = {n: v for n, v in report().items() if kernel in n}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
    assert v["lds"] == 0, "%s: %d bytes of static LDS (the launch gives all of it)" % (name, v["lds"])
    assert 0 < v["vgpr"] <= 128, "%s: %d VGPRs" % (name, v["vgpr"])


def test_the_lds_is_what_design_states():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("k_suppress"):]
    stated = {int(m.replace(" ", "")) for m in re.findall(r"\b(\d{1,3} ?\d{3}) bytes", section)}
    assert suppress_lds(1024) == 32768 <= 160 * 1024 and 32768 in stated, stated
    assert match_lds(1024, 1024) == 49156 <= 160 * 1024 and 49156 in stated, stated
    assert suppress_lds(64) == 2048 and 2048 in stated and match_lds(256, 256) == 12292 and 12292 in stated, stated
    text = open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_overlap.h")).read()
    assert "kOverlapThreads = 256" in text and "suppress_lds(" in text and "match_lds(" in text
    impl = open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_pipeline_impl.h")).read()
    assert "suppress_lds(leon::kOverlapMaxRows).bytes == 32768" in impl and "match_lds(leon::kOverlapMaxRows, leon::kOverlapMaxRows).bytes == 49156" in impl, \
        "the library asserts the figures when it is compiled"
    for launch, after in (("int suppress_launch", "int match_launch"), ("int match_launch", "int overlap_window_frames")):
        assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl[impl.index(launch):impl.index(after)]
