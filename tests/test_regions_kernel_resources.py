"""CPU: k_regions<element bytes, layout, filter> -- regions of delivered frames as a tensor batch -- exists in exactly its twelve
instantiations, spills nothing, stays inside k_resample's LDS bound of 80 KiB and uses exactly the LDS of the matching k_resample (it
is resample_body behind a descriptor read).  Its names carry none of the other families' (the resource tests count families by
substring).  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import functools
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

COMBOS = ["ILi%dELi%dE" % (eb, layout) for eb in (1, 2, 4) for layout in (0, 1)]
FILTERS = ["NS_11ResTriangleE", "NS_8ResCubicE"]

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


@functools.lru_cache(maxsize=None)
def report():
    import kernel_resources
    return kernel_resources.report()


def family(name):
    return {n: v for n, v in report().items() if name in n}


def test_twelve_regions_kernels():
    ks = family("k_regions")
    assert len(ks) == 12, sorted(ks)
    for combo in COMBOS:
        for filt in FILTERS:
            assert sum(1 for n in ks if combo[:-1] in n and filt in n) == 1, (combo, filt, sorted(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= 80 * 1024, "%s: %d bytes of LDS" % (name, v["lds"])


def test_the_other_tensor_kernels_are_still_theirs():
    assert len(family("k_resample")) == 12 and len(family("k_letterbox")) == 12 and len(family("k_tensor")) == 6
    assert not any("k_resample" in n or "k_tensor" in n or "k_letterbox" in n for n in family("k_regions"))


def test_regions_use_the_lds_of_their_k_resample():
    rs, gs = family("k_resample"), family("k_regions")
    for combo in COMBOS:
        for filt in FILTERS:
            r = next(v for n, v in rs.items() if combo[:-1] in n and filt in n)
            g = next(v for n, v in gs.items() if combo[:-1] in n and filt in n)
            assert g["lds"] == r["lds"], (combo, filt)
