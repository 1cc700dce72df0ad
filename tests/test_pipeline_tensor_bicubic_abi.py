"""CPU: the bicubic filter of the resized tensor output (include/leon_pipeline.h, LEON_RESIZE_BICUBIC) -- signed tables of up to 65 taps
an axis computed on the host: leon_pipeline_resize_weights(filter 3) must equal leon_ctypes.resize_weights(filter=3), the Python
statement of the same definition, entry for entry, and the triangle tables must be what they were.  Where Pillow is installed it is an
independent witness: leon_ctypes.resize_rgb(filter=3) equals Image.resize(size, BICUBIC, box, reducing_gap=None) and filter 0 equals
BILINEAR, 0 differing bytes.  (The bicubic kernels' resources: test_tensor_kernel_resources.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

# (in_size, crop_start, crop_size, out_size)
AXES = [(96, 0, 96, 40), (96, 3, 80, 7), (352, 0, 352, 22), (96, 0, 96, 150), (30, 0, 30, 30)]
# (frame (w, h), crop (x, y, w, h) or None, size (w, h)): reductions, a crop down to 7 x 9, ratio 16, enlargements, a same-size crop
GEOMETRIES = [((96, 64), None, (40, 40)), ((96, 64), (3, 5, 80, 50), (7, 9)), ((352, 240), None, (22, 15)), ((96, 64), (3, 5, 40, 31), (80, 62)),
              ((96, 64), None, (150, 100)), ((96, 64), (3, 5, 40, 31), (40, 31))]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    return leon_ctypes


def c_weights(L, in_size, crop_start, crop_size, out_size, filt, max_taps):
    n = max(1, min(out_size, 4096))
    first, count, w = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full((n, max(1, max_taps)), -7, np.int32)
    rc = L.load().leon_pipeline_resize_weights(in_size, crop_start, crop_size, out_size, filt, first.ctypes.data, count.ctypes.data, w.ctypes.data, max_taps)
    return rc, first, count, w


def test_constants_of_the_header(tmp_path, L):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "leon.h"\n#include "leon_pipeline.h"\nint main(void){\n'
                   'printf("%d %d %d %d\\n", LEON_RESIZE_TRIANGLE, LEON_RESIZE_BICUBIC, LEON_RESIZE_MAX_TAPS, LEON_RESIZE_MAX_TAPS_BICUBIC);\nreturn 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include")])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [L.RESIZE_TRIANGLE, L.RESIZE_BICUBIC, L.RESIZE_MAX_TAPS, L.RESIZE_MAX_TAPS_BICUBIC] == [0, 3, 33, 65]
    assert L.RESIZE_FILTERS == {"triangle": 0, "bicubic": 3}


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "%d[%d+%d]to%d" % a)
def test_bicubic_weights_equal_the_python_definition(L, axis):
    in_size, c0, cs, out = axis
    rc, first, count, w = c_weights(L, *axis, L.RESIZE_BICUBIC, L.RESIZE_MAX_TAPS_BICUBIC)
    assert rc == L.OK, L.load().leon_last_error()
    pf, pn, pw = L.resize_weights(*axis, filter=L.RESIZE_BICUBIC)
    assert pw.shape == (out, int(pn.max())) and pn.max() <= L.RESIZE_MAX_TAPS_BICUBIC
    assert np.array_equal(first, pf) and np.array_equal(count, pn)
    assert np.array_equal(w[:, :pw.shape[1]], pw) and not w[:, pw.shape[1]:].any()
    assert np.array_equal(L.resize_weights(*axis, filter="bicubic")[2], pw)
    # what the definition promises: taps inside the axis, rows that sum to 2^22 within a unit per tap, and the bounds the kernel's
    # 24-bit multiplies and 32-bit sums rest on
    assert (pf >= 0).all() and (pf + pn <= in_size).all() and (pn >= 1).all()
    assert (np.abs(pw.sum(axis=1) - (1 << 22)) <= L.RESIZE_MAX_TAPS_BICUBIC).all()
    assert all(not pw[o, pn[o]:].any() for o in range(out))
    p64 = pw.astype(np.int64)
    assert (np.abs(p64) < 1 << 23).all()
    assert ((1 << 21) + 255 * np.where(p64 > 0, p64, 0).sum(axis=1) < 1 << 31).all() and (255 * np.where(p64 < 0, -p64, 0).sum(axis=1) < 1 << 31).all()
    if cs > out:
        assert (pw < 0).any()          # a reduction's rows carry the filter's negative lobes
    # the same rows with max_taps = the largest count; one less is refused
    rc, f2, n2, w2 = c_weights(L, *axis, L.RESIZE_BICUBIC, int(pn.max()))
    assert rc == L.OK and np.array_equal(w2, pw) and np.array_equal(f2, pf) and np.array_equal(n2, pn)
    assert c_weights(L, *axis, L.RESIZE_BICUBIC, int(pn.max()) - 1)[0] == L.ERR_INVALID


def test_ratio_16_reaches_the_tap_limit_and_same_size_is_the_identity(L):
    _, pn, pw = L.resize_weights(352, 0, 352, 22, filter=L.RESIZE_BICUBIC)
    assert int(pn.max()) in (64, 65)
    first, count, w = L.resize_weights(30, 0, 30, 30, filter=L.RESIZE_BICUBIC)
    # scale 1: the filter is sampled at -1.5 .. 1.5 in steps of 1 -- 0 everywhere but at the centre, where it is 1
    assert ((w != 0).sum(axis=1) == 1).all() and (w.max(axis=1) == 1 << 22).all()
    assert np.array_equal(first + w.argmax(axis=1), np.arange(30))
    img = np.random.default_rng(7).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(L.resize_rgb(img, None, (64, 96), filter=L.RESIZE_BICUBIC), img)
    assert np.array_equal(L.resize_rgb(img, (3, 5, 40, 31), (31, 40), filter=L.RESIZE_BICUBIC), img[5:36, 3:43])


@pytest.mark.parametrize("axis", AXES + [(1920, 0, 1920, 224), (1080, 0, 1080, 68)], ids=lambda a: "%d[%d+%d]to%d" % a)
def test_triangle_tables_are_unchanged(L, axis):
    """filter 0 through the new keyword = the function without it = the C tables"""
    pf, pn, pw = L.resize_weights(*axis)
    kf, kn, kw = L.resize_weights(*axis, filter=L.RESIZE_TRIANGLE)
    assert np.array_equal(pf, kf) and np.array_equal(pn, kn) and np.array_equal(pw, kw)
    assert np.array_equal(L.resize_weights(*axis, filter="triangle")[2], pw)
    assert (pw >= 0).all() and pn.max() <= L.RESIZE_MAX_TAPS
    rc, first, count, w = c_weights(L, *axis, L.RESIZE_TRIANGLE, L.RESIZE_MAX_TAPS)
    assert rc == L.OK and np.array_equal(first, pf) and np.array_equal(count, pn)
    assert np.array_equal(w[:, :pw.shape[1]], pw) and not w[:, pw.shape[1]:].any()
    # a longer row changes nothing but the zeros behind the counts
    rc, first, count, w = c_weights(L, *axis, L.RESIZE_TRIANGLE, L.RESIZE_MAX_TAPS_BICUBIC)
    assert rc == L.OK and np.array_equal(w[:, :pw.shape[1]], pw) and not w[:, pw.shape[1]:].any()


def test_refusals(L):
    lib = L.load()
    # 1920 -> 224 (ratio 8.57) has rows of 35 taps: LEON_RESIZE_MAX_TAPS is the triangle filter's, not enough here
    _, pn, _ = L.resize_weights(1920, 0, 1920, 224, filter=L.RESIZE_BICUBIC)
    assert int(pn.max()) == 35
    assert c_weights(L, 1920, 0, 1920, 224, L.RESIZE_BICUBIC, 33)[0] == L.ERR_INVALID
    assert b"max_taps" in lib.leon_last_error()
    assert c_weights(L, 1920, 0, 1920, 224, L.RESIZE_BICUBIC, 35)[0] == L.OK
    for filt in (1, 2, 4, -1):
        assert c_weights(L, 100, 0, 100, 50, filt, L.RESIZE_MAX_TAPS_BICUBIC)[0] == L.ERR_INVALID
        assert b"filter" in lib.leon_last_error()
        with pytest.raises(ValueError):
            L.resize_weights(100, 0, 100, 50, filter=filt)
    assert c_weights(L, 1601, 0, 1601, 100, L.RESIZE_BICUBIC, L.RESIZE_MAX_TAPS_BICUBIC)[0] == L.ERR_INVALID          # ratio 16.01
    assert c_weights(L, 1600, 0, 1600, 100, L.RESIZE_BICUBIC, L.RESIZE_MAX_TAPS_BICUBIC)[0] == L.OK                   # ratio 16
    with pytest.raises(ValueError):
        L.resize_weights(1601, 0, 1601, 100, filter=L.RESIZE_BICUBIC)
    # create refuses before any device is touched: filter 3 without the TENSOR bit, with no size, the filters that do not exist
    data = open(os.path.join(ROOT, "tests", "golden", "streams", "ibbp_96x64.jsv"), "rb").read()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    cb = L.PIPELINE_CB(lambda *a: None)
    for output, rz in ((L.PIPELINE_OUTPUT_RGBA, (0, 0, 0, 0, 40, 40, 3)), (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 0, 0, 3)),
                       (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 40, 40, 2)), (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 40, 40, 4)),
                       (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 40, 3, 3))):
        cfg = L.PipelineConfig()
        cfg.output = output
        h = C.c_void_p()
        r = L.PipelineTensorResize(*rz)
        assert lib.leon_pipeline_create_tensor_resized(C.byref(cfg), None, C.byref(r), buf, len(data), len(data), cb, None, C.byref(h)) == L.ERR_INVALID, (output, rz)
        assert b"resize" in lib.leon_last_error() and not h.value


def hard_edged(fw, fh, seed):
    """random rows between saturated checkerboard rows, and a block of black and white stripes: overshoot on both sides"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:fh, 0:fw]
    img[::2] = ((((yy + xx) & 1) * 255).astype(np.uint8))[::2, :, None]
    img[fh // 4:fh // 2, fw // 4:fw // 2] = ((((xx // 5 + yy // 3) & 1) * 255).astype(np.uint8))[fh // 4:fh // 2, fw // 4:fw // 2, None]
    return img


@pytest.mark.parametrize("filt", [3, 0], ids=["bicubic", "triangle"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d-%s-%dx%d" % (g[0] + ("crop" if g[1] else "whole",) + g[2]))
def test_resize_rgb_equals_pillow(L, geometry, filt):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    (fw, fh), crop, (ow, oh) = geometry
    x, y, w, h = crop or (0, 0, fw, fh)
    for img in (np.random.default_rng(fw * 31 + ow).integers(0, 256, (fh, fw, 3), dtype=np.uint8), hard_edged(fw, fh, fw + oh)):
        got = L.resize_rgb(img, crop, (oh, ow), filter=filt)
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC if filt == 3 else Image.BILINEAR, box=(x, y, x + w, y + h), reducing_gap=None))
        assert got.shape == ref.shape == (oh, ow, 3)
        assert int((got != ref).sum()) == 0, "%d bytes differ from Pillow %s" % (int((got != ref).sum()), PIL.__version__)
        if filt == 0:
            assert np.array_equal(got, L.resize_rgb(img, crop, (oh, ow)))


def test_tile_footprint_stays_inside_the_lds_at_ratio_16(L):
    """ratio 16 on both axes at the largest frame and at the GPU test's 608 x 256 -> 38 x 16: a 32 x 8 tile's source footprint stays inside
    what the bicubic kernels' LDS is sized for -- 576 columns (6 padded rows of the 4096-dword staging buffer), 179 + 1 of 192 h rows"""
    for fw, fh, ow, oh in ((4096, 4096, 256, 256), (608, 256, 38, 16), (1920, 1080, 120, 68)):
        fx, nx, _ = L.resize_weights(fw, 0, fw, ow, filter=3)
        fy, ny, _ = L.resize_weights(fh, 0, fh, oh, filter=3)
        widest = max((int(fx[m] + nx[m]) - (int(fx[t]) & ~7) + 7) & ~7 for t in range(0, ow, 32) for m in [min(t + 32, ow) - 1])
        tallest = max(int(fy[m] + ny[m]) - (int(fy[t]) & ~1) for t in range(0, oh, 8) for m in [min(t + 8, oh) - 1])
        assert widest <= 576 and (widest + (widest >> 4)) * 6 <= 4096 and tallest <= 179
