"""CPU: the kernel of the pipeline's tensor output, k_tensor, exists in its three element types and spills nothing -- from hipcc
-Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_tensor_kernels_exist_and_spill_nothing():
    import kernel_resources
    rep = kernel_resources.report()
    ks = {n: v for n, v in rep.items() if "k_tensor" in n}
    assert len(ks) == 3, sorted(ks)          # fp16, bf16, fp32
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        # conversion tables 5 KB + the element table (1.5 KB, 3 KB for fp32): nothing else in LDS
        assert v["lds"] <= 5120 + 3072, "%s: %d bytes of LDS" % (name, v["lds"])
