"""CPU: the kernels of the pipeline's YCbCr output (k_recon_display_out, k_planes_crop) spill nothing, and each
k_recon_display_out instantiation allows at least the waves per SIMD of its RGBA twin (k_recon_display, same type,
boundary and alpha) -- from hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os
import re
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_planes_kernels_spill_nothing_and_keep_their_occupancy():
    import kernel_resources
    rep = kernel_resources.report()
    outs = {n: v for n, v in rep.items() if "k_recon_display_out" in n}
    assert len(outs) == 12, sorted(outs)          # I / P / B x alpha x (YCbCr, both), group-list boundary
    crop = [v for n, v in rep.items() if "k_planes_crop" in n]
    assert crop and crop[0]["scratch"] == 0
    for name, v in outs.items():
        m = re.search(r"k_recon_display_outILi(\d)ELb(\d)ELb(\d)ELi(\d)E", name)
        assert m, name
        twin = [t for n, t in rep.items() if "k_recon_displayILi%sELb%sELb%sE" % m.groups()[:3] in n]
        assert twin, name
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert v["occupancy"] >= twin[0]["occupancy"], "%s: %d waves per SIMD, its RGBA twin %d" % (name, v["occupancy"], twin[0]["occupancy"])
