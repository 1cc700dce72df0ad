"""CPU: the kernel of the resized tensor output, k_resample, exists in its three element types, spills nothing and leaves room for
two workgroups per CU (160 KiB of LDS: at most 80 KiB each) -- from hipcc -Rpass-analysis (tools/kernel_resources.py), no GPU needed."""
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_resample_kernels_exist_spill_nothing_and_fit_two_per_cu():
    import kernel_resources
    rep = kernel_resources.report()
    ks = {n: v for n, v in rep.items() if "k_resample" in n}
    assert len(ks) == 3, sorted(ks)          # fp16, bf16, fp32
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= 80 * 1024, "%s: %d bytes of LDS" % (name, v["lds"])


def source_bytes_requested(fw, fh, crop, ow, oh):
    """What k_resample's workgroups load for one frame, relative to the planes' bytes (Y + Cb + Cr = 1.5 per pixel), from the tables
    themselves and the kernel's tile: 32 x 8 output pixels; columns from first_x of the tile's first output rounded down to 8 to the end of
    its last, rounded up to 8; rows from first_y rounded down to a pair to the end of the last, as whole pairs."""
    import leon_ctypes as L
    x, y, w, h = crop or (0, 0, fw, fh)
    fx, nx, _ = L.resize_weights(fw, x, w, ow)
    fy, ny, _ = L.resize_weights(fh, y, h, oh)
    total, widest, tallest = 0, 0, 0
    for ty in range(0, oh, 8):
        last = min(ty + 8, oh) - 1
        r0, r1 = int(fy[ty]) & ~1, int(fy[last] + ny[last])
        for tx in range(0, ow, 32):
            m = min(tx + 32, ow) - 1
            sw = (int(fx[m] + nx[m]) - (int(fx[tx]) & ~7) + 7) & ~7
            total += sw * ((r1 - r0 + 1) & ~1)
            widest, tallest = max(widest, sw), max(tallest, r1 - r0)
    return total / float(fw * fh), widest, tallest


def test_tile_shape_keeps_the_source_redundancy_and_the_lds_bounds():
    """1080p -> 224 x 224 requests less than 1.5 x the planes' bytes (DESIGN.md 4c quotes these figures); at the largest ratio a tile's
    footprint stays inside what the kernel's LDS is sized for: 544 columns (6 padded rows of staging), 147 + 1 of 160 h rows"""
    r224, _, _ = source_bytes_requested(1920, 1080, None, 224, 224)
    assert r224 < 1.5
    assert abs(r224 - 1.20) < 0.005
    assert abs(source_bytes_requested(1920, 1080, None, 384, 216)[0] - 1.25) < 0.005
    r16, widest, tallest = source_bytes_requested(1920, 1080, None, 120, 68)
    assert abs(r16 - 1.15) < 0.005 and widest <= 544 and tallest <= 147
    _, widest, tallest = source_bytes_requested(4096, 4096, None, 256, 256)          # ratio 16 on both axes, the largest frame
    assert widest <= 544 and tallest <= 147 and (widest + (widest >> 4)) * 6 <= 4096
