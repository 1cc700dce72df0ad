"""CPU: k_fields, the kernel behind leon_pipeline_field_tensors (csrc/leon_kernels.h), exists in its three instantiations (fp16, bf16,
fp32 elements), spills nothing, keeps its static LDS (the tile's table rows, the h rows, the packed tile) far within 64 KiB and its
vector registers within the 64 at which occupancy would begin to drop; and the kernel families other resource tests select by
substring still count what they counted before there was a k_fields.  From hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU
needed."""
import functools
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

FAMILIES = {"k_tensor": 6, "k_resample": 12, "k_regions": 12, "k_letterbox": 12, "k_fit": 13, "k_box": 1, "k_warp": 6, "k_motion": 1, "k_residual": 1, "k_activity": 2, "k_carry": 1,
            "k_gauge": 1, "k_propose": 1, "k_propagate": 1, "k_accumulate": 1, "k_suppress": 1, "k_match": 1, "k_recon": 30, "k_planes": 1}


@functools.lru_cache(maxsize=None)
def report():
    import kernel_resources
    return kernel_resources.report()


@HIPCC
def test_fields_kernels_exist_without_scratch_within_lds():
    ks = {n: v for n, v in report().items() if "k_fields" in n}
    assert sorted(n[n.index("k_fieldsILi"):][:13] for n in ks) == ["k_fieldsILi1E", "k_fieldsILi2E", "k_fieldsILi3E"], sorted(ks)
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= 65536, "%s: %d bytes of LDS" % (name, v["lds"])
        assert v["lds"] == 16992, "%s: %d bytes of LDS, leon_fields.h's FieldTile is 16992" % (name, v["lds"])
        assert 0 < v["vgpr"] <= 64, "%s: %d VGPRs" % (name, v["vgpr"])


@HIPCC
def test_the_other_families_count_what_they_counted():
    names = list(report())
    assert {f: sum(f in n for n in names) for f in FAMILIES} == FAMILIES
    assert not any(f in n for n in names if "k_fields" in n for f in FAMILIES)
