"""CPU: k_accumulate, the kernel behind leon_pipeline_accumulate (csrc/leon_kernels.h), exists once, spills nothing, holds nothing in LDS
(its lanes share nothing) and stays within the 64 vector registers at which occupancy would begin to drop.  From hipcc
-Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import functools
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def report():
    import kernel_resources
    return kernel_resources.report()


@HIPCC
def test_accumulate_kernel_exists_once_without_scratch_or_lds():
    ks = {n: v for n, v in report().items() if "k_accumulate" in n}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
    assert v["lds"] == 0, "%s: %d bytes of LDS" % (name, v["lds"])
    assert 0 < v["vgpr"] <= 64, "%s: %d VGPRs" % (name, v["vgpr"])
