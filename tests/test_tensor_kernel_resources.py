"""CPU: the kernels of the pipeline's tensor output -- k_tensor<element bytes, layout> at frame size, k_resample<element bytes,
layout, filter> at a model's input size -- exist in exactly their instantiations, spill nothing and stay inside the LDS that does not
limit occupancy: at frame size the conversion tables and the element table alone for float CHW, 20 KiB otherwise (a CU holds 8
workgroups of 256 threads by waves; 160 KiB / 8); 80 KiB resized (two workgroups per CU).  From hipcc -Rpass-analysis
(tools/kernel_resources.py), no GPU needed.
The counts were 7 + 14 while fp16 and bf16 were compiled twice (the same instructions: the two differ in the host's table only);
per element SIZE they are 6 + 12.  Every combination and every bound of the earlier per-kernel tests is here."""
import functools
import os
import sys

import pytest

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

# template arguments <element bytes, layout> as the mangled names spell them: CHW and HWC of 1, 2 and 4 bytes
COMBOS = ["ILi%dELi%dE" % (eb, layout) for eb in (1, 2, 4) for layout in (0, 1)]
FILTERS = ["NS_11ResTriangleE", "NS_8ResCubicE"]


@functools.lru_cache(maxsize=None)
def report():
    import kernel_resources
    return kernel_resources.report()


def lds_of(ks, fragment):
    return next(v["lds"] for n, v in ks.items() if fragment in n)


HIPCC = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")


def no_scratch_and_lds(ks, bound):
    for name, v in ks.items():
        assert v["scratch"] == 0, "%s spills %d bytes per lane" % (name, v["scratch"])
        assert 0 < v["lds"] <= bound, "%s: %d bytes of LDS" % (name, v["lds"])


@HIPCC
def test_tensor_kernels_exist_and_spill_nothing():
    """frame size: exactly the six k_tensor, each once; float CHW holds the conversion tables 5 KB + the element table (1.5 KB, 3 KB
    for fp32) and nothing else in LDS"""
    ks = {n: v for n, v in report().items() if "k_tensor" in n}
    assert len(ks) == 6, sorted(ks)
    for c in COMBOS:
        assert sum("k_tensor" + c + "E" in n for n in ks) == 1, (c, sorted(ks))
    no_scratch_and_lds(ks, 20 * 1024)
    no_scratch_and_lds({n: v for n, v in ks.items() if "ILi2ELi0E" in n or "ILi4ELi0E" in n}, 5120 + 3072)


@HIPCC
def test_image_kernels_exist_spill_nothing_and_fit():
    """8-bit elements and the channels-last layout -- uint8 CHW, HWC of 1-, 2- and 4-byte elements: each once at frame size (20 KiB)
    and resized (80 KiB) for both filters; uint8 needs no element table, so its kernels hold less LDS than the 2-byte ones"""
    combos = ["ILi1ELi0E", "ILi1ELi1E", "ILi2ELi1E", "ILi4ELi1E"]
    for kernel, tails, bound in (("k_tensor", ["E"], 20 * 1024), ("k_resample", [f + "E" for f in FILTERS], 80 * 1024)):
        for tail in tails:
            ks = {n: v for n, v in report().items() if any(kernel + c + tail in n for c in combos)}
            assert len(ks) == 4, sorted(ks)
            no_scratch_and_lds(ks, bound)
            assert lds_of(ks, "ILi1ELi1E") < lds_of(ks, "ILi2ELi1E")


@HIPCC
def test_resample_kernels_exist_spill_nothing_and_fit_two_per_cu():
    """resized: exactly the twelve k_resample, each once, room for two workgroups per CU (160 KiB of LDS: at most 80 KiB each)"""
    ks = {n: v for n, v in report().items() if "k_resample" in n}
    assert len(ks) == 12, sorted(ks)
    for f in FILTERS:
        for c in COMBOS:
            assert sum("k_resample" + c + f + "E" in n for n in ks) == 1, (c, f, sorted(ks))
    no_scratch_and_lds(ks, 80 * 1024)


@HIPCC
def test_bicubic_kernels_exist_spill_nothing_and_fit_two_per_cu():
    """the bicubic filter's six instantiations (its h rows and weight tables are the larger ones)"""
    ks = {n: v for n, v in report().items() if "k_resample" in n and "ResCubic" in n}
    assert len(ks) == 6, sorted(ks)
    no_scratch_and_lds(ks, 80 * 1024)


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
