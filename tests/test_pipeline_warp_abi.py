"""CPU, no device: the host-only half of the warp calls (include/leon_pipeline.h, leon_pipeline_warp_regions) -- struct sizes, the two
quantisers, the checks with their order and their status words, the slack of the scale thresholds -- and the anchors of
leon_ctypes.warp_rgb, the numpy statement of the definition every GPU test of the family compares with: the identity is the crop,
rotations by multiples of 90 degrees are np.rot90 of it, scales 2 and 4 at integer offsets are the box means, a map wholly outside is
all pad, and S = 1 stays within 1.5 of float64 bilinear at the same Q16 coordinates (255 * 2 * 2^-9 for the 8-bit fractions + 0.5)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import warp_structure as W
from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def img():
    rgb = np.random.default_rng(57).integers(0, 256, (57, 100, 3), dtype=np.uint8)
    rgb[56] = 255          # the fill row of an odd height
    rgb.setflags(write=False)
    return rgb


IDENT = (65536, 0, 0, 0, 65536, 0)


def test_struct_sizes(L):
    assert C.sizeof(L.PipelineWarpRegion) == 32 and C.sizeof(L.PipelineWarpConfig) == 32 and C.sizeof(L.PipelineWarpRegionsCall) == 64
    assert C.sizeof(L.PipelineRegion) == 32 and C.sizeof(L.PipelineRegionsConfig) == 32 and C.sizeof(L.PipelineRegionsDevice) == 64 and C.sizeof(L.PipelineRegionsFit) == 32
    assert (L.REGION_SCALE, L.REGION_OFFSET) == (7, 8)
    assert L.PipelineWarpRegionsCall.device_out.offset == 16 and L.PipelineWarpRegionsCall.stream.offset == 40 and L.PipelineWarpRegion.reserved.offset == 28
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    assert "#define LEON_REGION_SCALE    7 " in header and "#define LEON_REGION_OFFSET   8 " in header


def test_from_matrix(L):
    assert L.warp_matrix([1, 0, 0, 0, 1, 0]) == IDENT
    assert L.warp_matrix([[0.5, -0.25, 3.5], [2, 1e-9, -7.25]]) == (32768, -16384, 229376, 131072, 0, -475136)
    # floor(v * 65536 + 0.5): halves go up on both sides of zero
    assert L.warp_matrix([1.5 / 65536, -1.5 / 65536, 2.5 / 65536, -2.5 / 65536, 0.49 / 65536, -0.51 / 65536]) == (2, -1, 3, -2, 0, -1)
    assert L.warp_matrix([32767.99999, -32768, 0, 0, 0, 0])[:2] == (2147483647, -2147483648)
    for bad in (float("nan"), float("inf"), -float("inf"), 32768.0, -32768.1):
        with pytest.raises(L.LeonError) as e:
            L.warp_matrix([1, 0, bad, 0, 1, 0])
        assert e.value.code == L.ERR_INVALID and "entry 2" in str(e.value)
    out = (C.c_int32 * 6)(*([77] * 6))
    assert L.load().leon_pipeline_warp_from_matrix((C.c_double * 6)(1, 2, 3, 4, float("nan"), 6), out) == L.ERR_INVALID and list(out) == [77] * 6
    assert L.load().leon_pipeline_warp_from_matrix(None, out) == L.ERR_INVALID


def test_from_rotated_box(L):
    # a box of the out size, not rotated: the identity at the box's corner
    assert L.warp_matrix_rotated_box(50, 28, 20, 10, 0, (10, 20)) == (65536, 0, 40 * 65536, 0, 65536, 23 * 65536)
    # the documented formulas
    cx, cy, w, h, deg, (oh, ow) = 301.25, 20.5, 64.0, 24.0, 33.0, (13, 37)
    cs, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    A = [w / ow * cs, -h / oh * sn, 0, w / ow * sn, h / oh * cs, 0]
    A[2] = cx - (A[0] * ow / 2 + A[1] * oh / 2)
    A[5] = cy - (A[3] * ow / 2 + A[4] * oh / 2)
    got = L.warp_matrix_rotated_box(cx, cy, w, h, deg, (oh, ow))
    assert all(abs(a - b) <= 1 for a, b in zip(got, L.warp_matrix(A))), (got, L.warp_matrix(A))
    # the centre of the out size maps to the centre of the box
    X = got[0] * ow / 2 + got[1] * oh / 2 + got[2]
    assert abs(X / 65536 - cx) < 1e-3
    with pytest.raises(L.LeonError):
        L.warp_matrix_rotated_box(1, 1, 1, 1, 0, (0, 8))
    with pytest.raises(L.LeonError):
        L.warp_matrix_rotated_box(1, 1, float("nan"), 1, 0, (8, 8))


def test_the_thresholds_have_slack_for_the_quantiser(L):
    """a rotated box at 45 degrees and scale exactly 1, 2 and 4 gives g = 0, 1, 2; a hair above 4 is refused"""
    for scale, g in ((1, 0), (2, 1), (4, 2)):
        for deg in (45, 30, 0, 90, 133):
            m = L.warp_matrix_rotated_box(50, 28, scale * 32, scale * 32, deg, (32, 32))
            assert W.supersample(m) == g, (scale, deg, m)
            assert L.warp_region_status(100, 57, 9, (0, m), (32, 32)) == L.REGION_OK
    assert W.supersample((65537, 0, 0, 0, 65537, 0)) == 0 and W.supersample((65538, 0, 0, 0, 1, 0)) == 1
    assert W.supersample((0, 262145, 0, 0, 0, 0)) == 2 and W.supersample((0, 262146, 0, 0, 0, 0)) is None
    assert L.warp_region_status(100, 57, 9, (0, (0, 262145, 0, 0, 0, 0)), (8, 8)) == L.REGION_OK
    assert L.warp_region_status(100, 57, 9, (0, (0, 262146, 0, 0, 0, 0)), (8, 8)) == L.REGION_SCALE
    assert L.warp_region_status(100, 57, 9, (0, (-2147483648, 0, 0, -2147483648, 0, 0)), (8, 8)) == L.REGION_SCALE          # 2^63 in all: no overflow


def test_checks_their_order_and_the_status_words(L):
    n_frames = 9
    for name, (frame, m, reserved), word, text in W.refused_records(n_frames):
        rec = L.PipelineWarpRegion(frame, (C.c_int32 * 6)(*m), reserved)
        assert L.warp_region_status(96, 64, n_frames, rec, (8, 8)) == word == W.record_status(frame, m, reserved, n_frames), name
        with pytest.raises(L.LeonError) as e:
            L.warp_regions_check(96, 64, n_frames, [(0, IDENT), rec, (1, IDENT)], (8, 8))
        assert e.value.code == L.ERR_INVALID and e.value.bad == 1 and "region 1" in str(e.value) and text in str(e.value), str(e.value)
    # the order: reserved, frame, scale, offset
    big, far = (5 * 65536, 0, 0, 0, 65536, 0), (65536, 0, -(1 << 29) - 1, 0, 65536, 0)
    both = (5 * 65536, 0, (1 << 30), 0, 65536, 0)
    st = lambda frame, m, reserved: L.warp_region_status(96, 64, n_frames, L.PipelineWarpRegion(frame, (C.c_int32 * 6)(*m), reserved), (8, 8))
    assert st(-1, both, 1) == L.REGION_RESERVED and st(-1, both, 0) == L.REGION_FRAME and st(0, both, 0) == L.REGION_SCALE
    assert st(0, far, 0) == L.REGION_OFFSET and st(0, big, 0) == L.REGION_SCALE
    assert st(0, (65536, 0, 1 << 29, 0, 65536, -(1 << 29)), 0) == L.REGION_OK
    assert st(0, (65536, 0, 0, 0, 65536, -2147483648), 0) == L.REGION_OFFSET
    assert st(8, IDENT, 0) == L.REGION_OK and st(9, IDENT, 0) == L.REGION_FRAME
    # accepted: regions partly and wholly outside the frame
    assert L.warp_regions_check(96, 64, n_frames, [(0, (65536, 0, -(1 << 29), 0, 65536, 1 << 29)), (8, IDENT)], (8, 8)) is None


def test_the_config_and_n(L):
    ok = [(0, IDENT)]
    for size, pad, text in (((0, 8), None, "out_height"), ((8, 4097), None, "out_width"), ((8, 8), (0, 256, 0), "pad value 1"), ((8, 8), (-1, 0, 0), "pad value 0")):
        with pytest.raises(L.LeonError) as e:
            L.warp_regions_check(96, 64, 9, ok, size, pad)
        assert e.value.bad == -1 and text in str(e.value), str(e.value)
    cfg = L.PipelineWarpConfig(8, 8)
    cfg.reserved[2] = 1
    with pytest.raises(L.LeonError, match="reserved word 2"):
        L.warp_regions_check(96, 64, 9, ok, cfg)
    with pytest.raises(L.LeonError, match="0 regions"):
        L.warp_regions_check(96, 64, 9, [], (8, 8))
    with pytest.raises(L.LeonError):
        L.warp_region_status(96, 64, 9, ok[0], (8, 5000))
    assert L.warp_regions_check(96, 64, 9, ok, (4096, 4096), (255, 0, 255)) is None


# ---- warp_rgb ---------------------------------------------------------------------------------------------------------------------
def test_identity_is_the_crop(L, img):
    assert np.array_equal(L.warp_rgb(img, L.warp_matrix([1, 0, 5, 0, 1, 7]), (13, 37)), img[7:20, 5:42])
    assert np.array_equal(L.warp_rgb(img, IDENT, (57, 100)), img)


@pytest.mark.parametrize("quarter", [1, 2, 3])
def test_quarter_turns_are_rot90_of_the_crop(L, img, quarter):
    # a box of 20 x 10 frame pixels at (40, 23), turned: the out size is 10 x 20 for the odd quarters
    size = (20, 10) if quarter & 1 else (10, 20)
    w, h = (size[1], size[0])
    out = L.warp_rgb(img, L.warp_matrix_rotated_box(50, 28, w, h, 90 * quarter, size), size, (1, 2, 3))
    crop = img[23:33, 40:60]
    # positive angles turn clockwise on the screen (y points down): np.rot90 turns the other way
    assert np.array_equal(out, np.rot90(crop, quarter)), quarter


def test_scales_2_and_4_are_the_box_means(L, img):
    out = L.warp_rgb(img, L.warp_matrix([2, 0, 4, 0, 2, 6]), (8, 8))
    assert np.array_equal(out, (img[6:22, 4:20].astype(int).reshape(8, 2, 8, 2, 3).sum((1, 3)) + 2) >> 2)
    out = L.warp_rgb(img, L.warp_matrix([4, 0, 4, 0, 4, 4]), (4, 5))
    assert np.array_equal(out, (img[4:20, 4:24].astype(int).reshape(4, 4, 5, 4, 3).sum((1, 3)) + 8) >> 4)


def test_outside_is_pad_and_refusals(L, img):
    pad = (114, 7, 250)
    for m in (L.warp_matrix([1, 0, 140, 0, 1, 3]), L.warp_matrix([1, 0, 3, 0, 1, -80]), L.warp_matrix_rotated_box(-200, 400, 30, 30, 45, (8, 8)),
              (65536, 0, 1 << 29, 0, 65536, -(1 << 29))):
        assert (L.warp_rgb(img, m, (8, 8), pad) == np.array(pad, dtype=np.uint8)).all()
    # half in: the columns left of the frame are pad, the others the frame's
    out = L.warp_rgb(img, L.warp_matrix([1, 0, -4, 0, 1, 0]), (8, 8), pad)
    assert (out[:, :4] == np.array(pad, dtype=np.uint8)).all() and np.array_equal(out[:, 4:], img[:8, :4])
    with pytest.raises(ValueError):
        L.warp_rgb(img, (0, 262146, 0, 0, 0, 0), (8, 8))
    with pytest.raises(ValueError):
        L.warp_rgb(img, (65536, 0, (1 << 29) + 1, 0, 65536, 0), (8, 8))


def test_s1_stays_within_the_derived_bound_of_float_bilinear(L, img):
    H, Wd = img.shape[:2]
    worst = 0.0
    for m in (L.warp_matrix_rotated_box(50, 28, 24, 16, 30, (16, 24)), L.warp_matrix_rotated_box(50, 28, 24, 16, 45, (16, 24)),
              L.warp_matrix_rotated_box(50, 28, 6, 4, 10, (16, 24)), L.warp_matrix([0.7, 0.1, 20.3, -0.2, 0.9, 11.7])):
        assert W.supersample(m) == 0
        got = L.warp_rgb(img, m, (16, 24)).astype(np.float64)
        ox, oy = np.meshgrid(np.arange(24) + 0.5, np.arange(16) + 0.5)
        X = (m[0] * ox + m[1] * oy + m[2]) / 65536.0 - 0.5
        Y = (m[3] * ox + m[4] * oy + m[5]) / 65536.0 - 0.5
        x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
        assert x0.min() >= 0 and x0.max() + 1 < Wd and y0.min() >= 0 and y0.max() + 1 < H          # (inside: no pad in this comparison)
        fx, fy = (X - x0)[..., None], (Y - y0)[..., None]
        f = img.astype(np.float64)
        want = (1 - fx) * (1 - fy) * f[y0, x0] + fx * (1 - fy) * f[y0, x0 + 1] + (1 - fx) * fy * f[y0 + 1, x0] + fx * fy * f[y0 + 1, x0 + 1]
        worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1.5, worst
