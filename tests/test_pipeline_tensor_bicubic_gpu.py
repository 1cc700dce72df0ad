"""GPU: the resized tensor output with the bicubic filter (LEON_RESIZE_BICUBIC, include/leon_pipeline.h) -- k_resample<..., ResCubic>, for float CHW
tensors and for 8-bit elements and the channels-last layout: up to 65 signed taps an axis, both 8-bit results clamped to
0 .. 255.  Expected = T[c][resize_rgb(ORACLE RGBA, crop, size, filter=3)]: the oracle's RGBA through the numpy statement of the two
integer passes and the element table; compared as bit patterns, no tolerance."""
import numpy as np
import pytest

from test_pipeline_gpu import ibbp_stream, oracle_frames
from test_pipeline_tensor_format_gpu import assert_tensors, bits, fixture, run_format

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
ALL_FORMATS = [(d, l) for d in ("float16", "bfloat16", "float32", "uint8") for l in ("chw", "hwc")]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def expected(L, rgba, dtype, layout, size, crop=None):
    """{key: bit patterns in the layout's order}: T[c][resize_rgb(oracle RGB, crop, size, bicubic)]"""
    T = bits(L.tensor_table(dtype))
    out = {}
    for k, v in rgba.items():
        rgb = L.resize_rgb(v[..., :3], crop, size, filter=L.RESIZE_BICUBIC)
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        out[k] = np.ascontiguousarray(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return out


def run_cubic(L, data, dtype, layout, size, crop=None, **kw):
    kw.setdefault("parser_threads", 2)
    kw.setdefault("gops_per_window", 2)
    kw.setdefault("gpu_parser", True)
    return run_format(L, data, dtype, layout, tensor_size=size, tensor_crop=crop, tensor_filter=L.RESIZE_BICUBIC, **kw)[0]


def unclamped_range(L, rgb, crop, size):
    """(lowest, highest) value of (2^21 + sum) >> 22 before the clamp, over both passes (the vertical one on the clamped h)"""
    fh, fw = rgb.shape[:2]
    x, y, w, h = crop or (0, 0, fw, fh)
    lo, hi = 0, 255

    def one_pass(img, first, count, weights):
        nonlocal lo, hi
        out = np.empty((img.shape[0], len(first), 3), dtype=np.uint8)
        src = img.astype(np.int64)
        for o in range(len(first)):
            n = int(count[o])
            v = (np.tensordot(src[:, first[o]:first[o] + n], weights[o, :n].astype(np.int64), axes=([1], [0])) + (1 << 21)) >> 22
            lo, hi = min(lo, int(v.min())), max(hi, int(v.max()))
            out[:, o] = np.clip(v, 0, 255)
        return out
    fx, nx, wx = L.resize_weights(fw, x, w, size[1], filter=L.RESIZE_BICUBIC)
    fy, ny, wy = L.resize_weights(fh, y, h, size[0], filter=L.RESIZE_BICUBIC)
    r0, r1 = int(fy.min()), int((fy + ny).max())
    hz = one_pass(rgb[r0:r1], fx, nx, wx)
    one_pass(hz.transpose(1, 0, 2), fy - r0, ny, wy)
    return lo, hi


@pytest.fixture(scope="module")
def ratio16(L):
    data = ibbp_stream(608, 256, [3], seed=608)
    return data, oracle_frames(data)


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_ratio_16_on_both_axes(L, ratio16, dtype, layout):
    """608 x 256 -> 38 x 16: two tiles in x and in y, the widest staged footprint and the tallest h column, rows of 64 - 65 taps"""
    data, rgba = ratio16
    size = (16, 38)
    assert int(L.resize_weights(608, 0, 608, 38, filter=3)[1].max()) >= 64 and int(L.resize_weights(256, 0, 256, 16, filter=3)[1].max()) >= 64
    assert_tensors(run_cubic(L, data, dtype, layout, size), expected(L, rgba, dtype, layout, size), "ratio 16 %s %s" % (dtype, layout))


@pytest.fixture(scope="module")
def small(L):
    data = ibbp_stream(96, 64, [6, 9], seed=2718)
    return data, oracle_frames(data)


@pytest.mark.parametrize("size,crop", [((62, 80), (3, 5, 40, 31)), ((100, 150), None)], ids=["crop-80x62", "whole-150x100"])
def test_enlargements_clamp_on_both_sides(L, small, size, crop):
    data, rgba = small
    ranges = [unclamped_range(L, v[..., :3], crop, size) for v in rgba.values()]
    assert min(r[0] for r in ranges) < 0 and max(r[1] for r in ranges) > 255, ranges          # undershoot and overshoot both happen
    for dtype, layout in (("float16", "chw"), ("uint8", "chw")):
        assert_tensors(run_cubic(L, data, dtype, layout, size, crop), expected(L, rgba, dtype, layout, size, crop), "enlargement %s %s %s" % (dtype, size, crop))


def test_same_size_crop_is_the_crop_of_the_full_size_tensor(L, small):
    """bicubic at scale 1 is the identity"""
    data, rgba = small
    full = run_format(L, data, "float32", "chw", parser_threads=2, gops_per_window=2, gpu_parser=True)[0]
    same = run_cubic(L, data, "float32", "chw", (31, 40), (3, 5, 40, 31))
    assert_tensors(same, {k: np.ascontiguousarray(v[:, 5:36, 3:43]) for k, v in full.items()}, "same size")


@PARSERS
@pytest.mark.parametrize("case", ["360x199", "100x60"])
def test_layout_edges(L, case, gpu_parser):
    """360 x 199: an odd height -- the twin's fill row of 255 under negative taps.  100 x 60: the unfused road (k_planes_crop), a width
    that is no multiple of 8"""
    fw, fh = (360, 199) if case == "360x199" else (100, 60)
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    rgba = oracle_frames(data)
    if fh & 1:
        assert all((v[fh - 1] == 255).all() for v in rgba.values())
    for (size, crop), (dtype, layout) in zip((((fh * 2 // 3, fw * 2 // 3), None), ((13, 23), (1, 1, fw - 3, fh - 2))), (("float16", "chw"), ("uint8", "hwc"))):
        got = run_cubic(L, data, dtype, layout, size, crop, gpu_parser=gpu_parser)
        assert_tensors(got, expected(L, rgba, dtype, layout, size, crop), "%s %s %s %s %s" % (case, dtype, layout, size, crop))


@pytest.fixture(scope="module")
def plain(L):
    data = fixture("ibbp_96x64")
    return data, oracle_frames(data)


@pytest.mark.parametrize("dtype,layout", ALL_FORMATS, ids=["%s-%s" % f for f in ALL_FORMATS])
def test_every_element_type_and_layout(L, plain, dtype, layout):
    data, rgba = plain
    size = (39, 61)
    want = expected(L, rgba, dtype, layout, size)
    assert_tensors(run_cubic(L, data, dtype, layout, size), want, "%s %s" % (dtype, layout))
    if (dtype, layout) == ("bfloat16", "hwc"):          # both front ends on one of them
        assert_tensors(run_cubic(L, data, dtype, layout, size, gpu_parser=False), want, "%s %s, host parser" % (dtype, layout))


def test_yuva_stream(L):
    """a yuva stream: the alpha plane lies behind Cr in the planes record and is not in the tensor"""
    data = fixture("yuva_ibbp_96x64")
    size = (48, 48)
    assert_tensors(run_cubic(L, data, "float16", "chw", size), expected(L, oracle_frames(data), "float16", "chw", size), "yuva")


def test_geometry_reports_the_taps(L, plain):
    data, _ = plain
    for name in ("bicubic", L.RESIZE_BICUBIC):
        pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, output="tensor", tensor_size=(4, 6), tensor_filter=name)
        try:
            pipe.wait()
            assert pipe.error is None, pipe.error
            g = pipe.tensor_geometry
            assert (g.width, g.height, g.resized) == (6, 4, 1)
            fw, fh = pipe.info.frame_width, pipe.info.frame_height          # (the display size: smaller than the coded 96 x 64)
            assert (g.taps_x, g.taps_y) == (L.resize_weights(fw, 0, fw, 6, filter=3)[2].shape[1], L.resize_weights(fh, 0, fh, 4, filter=3)[2].shape[1])
            assert g.taps_x > L.RESIZE_MAX_TAPS and g.taps_y > L.RESIZE_MAX_TAPS
        finally:
            pipe.close()


def test_refusals(L, plain):
    data, rgba = plain
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="rgba", tensor_size=(40, 40), tensor_filter="bicubic")          # filter 3 without the TENSOR bit
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="tensor", tensor_filter=3)                                      # ... with no size
    for filt in (2, 4):
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output="tensor", tensor_size=(40, 40), tensor_filter=filt)
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="tensor", tensor_size=(3, 40), tensor_filter=3)                 # 64 / 3 > 16
    with pytest.raises(KeyError):
        L.Pipeline(data, output="tensor", tensor_size=(40, 40), tensor_filter="lanczos")
