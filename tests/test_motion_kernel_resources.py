"""CPU: k_motion, the kernel of the pipeline's MOTION output (csrc/leon_kernels.h), exists once, spills nothing, stays well under the
64 vector registers that would begin to limit occupancy, and holds only its four waves' partial summaries in LDS.  From hipcc
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
def test_motion_kernel_exists_spills_nothing_and_is_small():
    ks = {n: v for n, v in report().items() if "k_motion" in n}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
    assert 0 < v["vgpr"] <= 64, "%s: %d VGPRs" % (name, v["vgpr"])
    assert v["lds"] == 4 * 8 * 4, "%s: %d bytes of LDS (four waves x eight words)" % (name, v["lds"])
