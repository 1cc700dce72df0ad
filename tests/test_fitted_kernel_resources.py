"""CPU: k_fitted<element bytes, layout, filter> -- every region letterboxed into the call's tensor size -- exists in exactly its twelve
instantiations, spills nothing and uses exactly the LDS of the matching k_resample (its image tiles are resample_body, its pad
workgroups use none).  The table kernel of the fit spills nothing and has a reduction's LDS only.  Their names carry none of the other
families' (the resource tests count families by substring), and those still count what they counted.  From hipcc -Rpass-analysis
(tools/kernel_resources.py), no GPU needed."""
import os

import pytest

from test_regions_kernel_resources import COMBOS, FILTERS, report          # (one compilation for the resource modules: report() is cached there)

OTHERS = ("k_regions", "k_resample", "k_letterbox", "k_tensor", "k_box_tables", "k_axis_tables")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def family(name):
    return {n: v for n, v in report().items() if name in n}


def test_twelve_fitted_kernels_with_the_lds_of_their_k_resample():
    ks, rs = family("k_fitted"), family("k_resample")
    assert len(ks) == 12, sorted(ks)
    for combo in COMBOS:
        for filt in FILTERS:
            mine = [v for n, v in ks.items() if combo[:-1] in n and filt in n]
            theirs = [v for n, v in rs.items() if combo[:-1] in n and filt in n]
            assert len(mine) == 1 and len(theirs) == 1, (combo, filt, sorted(ks))
            assert mine[0]["lds"] == theirs[0]["lds"] > 0, (combo, filt)
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])


def test_the_fit_table_kernel():
    ks = family("k_fit_tables")
    assert len(ks) == 1, sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert v["lds"] <= 256, "%s: %d bytes of LDS" % (name, v["lds"])


def test_the_other_families_are_still_theirs():
    assert [len(family(f)) for f in OTHERS] == [12, 12, 12, 6, 1, 1]
    for mine in ("k_fitted", "k_fit_tables"):
        assert family(mine) and not any(other in n for n in family(mine) for other in OTHERS)
    assert not any("k_fitted" in n for n in family("k_fit_tables"))
