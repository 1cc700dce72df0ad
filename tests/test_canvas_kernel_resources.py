"""CPU: k_letterbox<element bytes, layout, filter> -- the resampled image in a padded canvas -- exists in exactly its twelve
instantiations, spills nothing and stays inside k_resample's LDS bound of 80 KiB (two workgroups per CU); the report still lists
exactly twelve k_resample and six k_tensor.  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
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


def test_twelve_letterbox_kernels():
    ks = family("k_letterbox")
    assert len(ks) == 12, sorted(ks)
    for combo in COMBOS:
        for filt in FILTERS:
            assert sum(1 for n in ks if combo[:-1] in n and filt in n) == 1, (combo, filt, sorted(ks))
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= 80 * 1024, "%s: %d bytes of LDS" % (name, v["lds"])


def test_the_other_tensor_kernels_are_still_theirs():
    assert len(family("k_resample")) == 12 and len(family("k_tensor")) == 6
    assert not any("k_resample" in n or "k_tensor" in n for n in family("k_letterbox"))


def test_letterbox_uses_no_more_lds_than_its_k_resample():
    """the pad workgroups use none, the image tiles resample_body's"""
    rs, ls = family("k_resample"), family("k_letterbox")
    for combo in COMBOS:
        for filt in FILTERS:
            r = next(v for n, v in rs.items() if combo[:-1] in n and filt in n)
            l = next(v for n, v in ls.items() if combo[:-1] in n and filt in n)
            assert l["lds"] == r["lds"], (combo, filt)
