"""CPU: the kernels of the 8-bit and channels-last tensor outputs, k_image (frame size) and k_image_scaled (a model's input size),
exist in their four combinations each -- uint8 CHW, and HWC of 1-, 2- and 4-byte elements --, spill nothing and stay inside the LDS
that does not limit occupancy: 20 KiB at frame size (a CU holds 8 workgroups of 256 threads by waves; 160 KiB / 8), 80 KiB resized
(k_resample's bound: two workgroups per CU).  k_tensor and k_resample keep their three instantiations.  From hipcc
-Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_image_kernels_exist_spill_nothing_and_fit():
    import kernel_resources
    rep = kernel_resources.report()
    scaled = {n: v for n, v in rep.items() if "k_image_scaled" in n}
    full = {n: v for n, v in rep.items() if "k_image" in n and "k_image_scaled" not in n}
    # template arguments <element bytes, layout> as the mangled names spell them
    combos = ["ILi1ELi0EE", "ILi1ELi1EE", "ILi2ELi1EE", "ILi4ELi1EE"]
    for ks, bound in ((full, 20 * 1024), (scaled, 80 * 1024)):
        assert len(ks) == 4, sorted(ks)
        for c in combos:
            assert sum(c in n for n in ks) == 1, (c, sorted(ks))
        for name, v in ks.items():
            assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
            assert 0 < v["lds"] <= bound, "%s: %d bytes of LDS" % (name, v["lds"])
    # uint8 needs no element table: its kernels hold less LDS than the 2-byte ones
    by = lambda ks, c: next(v["lds"] for n, v in ks.items() if c in n)
    assert by(full, "ILi1ELi1EE") < by(full, "ILi2ELi1EE") and by(scaled, "ILi1ELi1EE") < by(scaled, "ILi2ELi1EE")
    assert len([n for n in rep if "k_tensor" in n]) == 3 and len([n for n in rep if "k_resample" in n]) == 3
