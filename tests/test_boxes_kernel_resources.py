"""CPU: the kernels of leon_pipeline_resample_regions_device.  The road launches k_regions<element bytes, layout, filter>, the host
road's family, whose first statement is the status test: there is no k_boxes family any more, and k_regions still exists in exactly its
twelve instantiations, spills nothing and uses exactly the LDS of the matching k_resample (it is resample_body behind a descriptor
read).  k_box_tables, which builds the regions' tables in doubles, spills nothing either (no array of doubles per
lane) and has a reduction's LDS only.  Their names carry none of the other families' (the resource tests count families by substring),
and those still count what they counted.  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os

import pytest

from test_regions_kernel_resources import COMBOS, FILTERS, report          # (one compilation for both modules: report() is cached there)

OTHERS = ("k_regions", "k_resample", "k_letterbox", "k_tensor")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def family(name):
    return {n: v for n, v in report().items() if name in n}


def test_no_boxes_kernels_and_twelve_regions_kernels_with_the_lds_of_their_k_resample():
    assert not family("k_boxes"), sorted(family("k_boxes"))
    ks, rs = family("k_regions"), family("k_resample")
    assert len(ks) == 12, sorted(ks)
    for combo in COMBOS:
        for filt in FILTERS:
            mine = [v for n, v in ks.items() if combo[:-1] in n and filt in n]
            theirs = [v for n, v in rs.items() if combo[:-1] in n and filt in n]
            assert len(mine) == 1 and len(theirs) == 1, (combo, filt, sorted(ks))
            assert mine[0]["lds"] == theirs[0]["lds"] > 0, (combo, filt)
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])


def test_the_table_kernels():
    ks = family("k_box_tables")
    assert len(ks) == 1, sorted(ks)
    for name, v in list(ks.items()) + list(family("k_axis_tables").items()):
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert v["lds"] <= 256, "%s: %d bytes of LDS" % (name, v["lds"])
    assert len(family("k_axis_tables")) == 1


def test_the_other_tensor_kernels_are_still_theirs():
    assert [len(family(f)) for f in OTHERS] == [12, 12, 12, 6]
    for mine in ("k_box_tables", "k_axis_tables"):
        assert not any(other in n for n in family(mine) for other in OTHERS)
