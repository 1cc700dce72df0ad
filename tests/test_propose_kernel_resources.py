"""CPU: k_propose, the kernel behind leon_pipeline_propose_regions (csrc/leon_kernels.h), exists once, spills nothing and stays
within the 128 vector registers below which four waves per SIMD remain resident.  Its LDS is the placement DESIGN.md 4c states:
none of it static, all of it dynamic and sized by the launch from leon_propose.h's layout -- 2 bytes a padded cell of labels, two bit
masks, 8 bytes a row, a word a wave: 155680 bytes for the largest grid with the most rows, inside a CU's 160 KiB.  From hipcc
-Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
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


def lds_bytes(mbs, k, waves=8):
    """leon_propose.h's propose_lds in Python: labels, hot mask, root mask, rows, scan"""
    groups = (mbs + 63) // 64
    return 4 * (32 * groups + 2 * (2 * groups) + 2 * k + waves)


@HIPCC
def test_propose_kernel_exists_once_without_scratch_and_with_dynamic_lds_only():
    ks = {n: v for n, v in report().items() if "k_propose" in n}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
    assert v["lds"] == 0, "%s: %d bytes of static LDS (the launch gives all of it)" % (name, v["lds"])
    assert 0 < v["vgpr"] <= 128, "%s: %d VGPRs" % (name, v["vgpr"])


def test_the_lds_is_what_design_states():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("k_propose"):]
    stated = {int(m.replace(" ", "")) for m in re.findall(r"\b(\d{2,3} ?\d{3}) bytes", section)}
    assert lds_bytes(65536, 1024) == 155680 <= 160 * 1024 and 155680 in stated, stated
    assert lds_bytes(120 * 68, 16) == 18592 and 18592 in stated, stated
    text = open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_propose.h")).read()
    assert "kProposeThreads = 512" in text and "propose_lds(" in text
    impl = open(os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "csrc", "leon_pipeline_impl.h")).read()
    assert "propose_lds(leon::kProposeMaxCells, leon::kProposeMaxBoxes).bytes == 155680" in impl, "the library asserts the figure when it is compiled"
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in impl[impl.index("int propose_launch"):impl.index("int propose_regions_device")]
