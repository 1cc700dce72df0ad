"""CPU: k_warp<element bytes, layout> -- rotated boxes and affine crops -- exists in exactly its six instantiations, spills nothing and
keeps its static LDS inside 64 KiB.  Their names carry none of the other families' (the resource tests count families by substring),
and those still count what they counted.  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os

import pytest

from test_regions_kernel_resources import COMBOS, report          # (one compilation for the resource modules: report() is cached there)

OTHERS = ("k_regions", "k_resample", "k_letterbox", "k_tensor", "k_box_tables", "k_axis_tables", "k_fitted", "k_fit_tables")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def family(name):
    return {n: v for n, v in report().items() if name in n}


def test_six_warp_kernels_without_scratch_inside_64k_of_lds():
    ks = family("k_warp")
    assert len(ks) == 6, sorted(ks)
    for combo in COMBOS:
        assert len([n for n in ks if combo[:-1] in n]) == 1, (combo, sorted(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= 64 * 1024, "%s: %d bytes of LDS" % (name, v["lds"])


def test_the_other_families_are_still_theirs():
    assert [len(family(f)) for f in OTHERS] == [12, 12, 12, 6, 1, 1, 12, 1]
    assert not any(other in n for n in family("k_warp") for other in OTHERS)
    assert not any("k_warp" in n for f in OTHERS for n in family(f))
