"""GPU: 8-bit tensor elements and the channels-last layout (include/leon_pipeline.h, LEON_TENSOR_U8 / leon_pipeline_tensor_format) --
k_tensor<element bytes, layout> at frame size, k_resample<element bytes, layout, filter> at a model's input size.  Expected values come from the ORACLE's RGBA alone: uint8 tensors are
its bytes [..., :3] (moved to [3, H, W] for CHW), float HWC tensors the table T (leon_ctypes.tensor_table) looked up with them, resized
ones leon_ctypes.resize_rgb of them first.  Compared as bit patterns, no tolerance."""
import os
import threading

import numpy as np
import pytest

from test_pipeline_gpu import STREAMS, ibbp_stream, oracle_frames, run_pipeline
from test_pipeline_planes_gpu import FIXTURES, assert_planes, oracle_planes

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
# every combination but float CHW (test_pipeline_tensor_gpu.py, test_pipeline_tensor_resize_gpu.py)
FORMATS = [("uint8", "chw"), ("uint8", "hwc"), ("float16", "hwc"), ("bfloat16", "hwc"), ("float32", "hwc")]
FORMAT = pytest.mark.parametrize("dtype,layout", FORMATS, ids=["%s-%s" % f for f in FORMATS])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def fixture(name):
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


def bits(a):
    """an array of elements as unsigned bit patterns"""
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def expected(L, rgba, dtype, layout, size=None, crop=None):
    """{key: bit patterns in the layout's order}: T[c][colour value], the colour values the oracle's RGB -- resized with
    leon_ctypes.resize_rgb when size = (out_h, out_w) is given"""
    T = bits(L.tensor_table(dtype))
    out = {}
    for k, v in rgba.items():
        rgb = v[..., :3] if size is None else L.resize_rgb(v[..., :3], crop, size)
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        out[k] = np.ascontiguousarray(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return out


def run_format(L, data, dtype, layout, output="tensor", **kw):
    """({key: tensor bits}, {key: RGBA or None}, {key: planes or None}) of a whole run"""
    kw.setdefault("gpu_parser", False)
    tensors, rgba, planes, lock = {}, {}, {}, threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                k = (f["gop"], f["display_index"])
                p = f["_pipe"]
                assert f["tensor"] and f["tensor"] % 256 == 0
                tensors[k] = bits(p.read_tensor(f))
                rgba[k] = L.read_frame(f) if f["rgba"] else None
                planes[k] = p.read_planes(f) if f["y"] else None
    pipe = L.Pipeline(data, on_window=on_window, output=output, tensor_dtype=dtype, tensor_layout=layout, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return tensors, rgba, planes


def assert_tensors(got, want, what):
    assert set(got) == set(want), "%s: frames %s" % (what, sorted(set(got) ^ set(want))[:8])
    for k in sorted(want):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s, want %s %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d of %d elements differ, first at %s: got %#x, want %#x" % (
                what, k, len(bad), g.size, bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])])))


@FORMAT
@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams(L, name, gpu_parser, dtype, layout):
    data = fixture(name)
    want = expected(L, oracle_frames(data), dtype, layout)
    got, rgba, planes = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert_tensors(got, want, "%s %s %s" % (name, dtype, layout))
    assert all(v is None for v in rgba.values()) and all(v is None for v in planes.values())


# 360 x 199: fw % 8 == 0 and not % 16, an odd height (the fill row); 100 x 60: an even width that is no multiple of 8 (the per-quad
# path, the unfused road); 352 x 96: a multiple of 16; 200 x 64: a multiple of 8 whose row pair (25 lanes) never ends with a wave
EDGES = {"360x199": (360, 199), "100x60": (100, 60), "352x96": (352, 96), "200x64": (200, 64)}


@FORMAT
@PARSERS
@pytest.mark.parametrize("case", sorted(EDGES))
def test_layout_edges(L, case, gpu_parser, dtype, layout):
    fw, fh = EDGES[case]
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    rgba = oracle_frames(data)
    want = expected(L, rgba, dtype, layout)
    if fh & 1:
        T = bits(L.tensor_table(dtype))
        assert all((v[fh - 1] == 255).all() for v in rgba.values())
        last = (lambda w: w[fh - 1]) if layout == "hwc" else (lambda w: w[:, fh - 1].T)
        assert all((last(w) == T[:, 255]).all() for w in want.values())
    got, _, _ = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert_tensors(got, want, "%s %s %s" % (case, dtype, layout))


@pytest.fixture(scope="module")
def hd(L):
    import stream_1080p
    data = stream_1080p.load()
    return data, oracle_frames(data)


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "hwc"), ("uint8", "chw"), ("float32", "hwc")])
def test_1080p_two_gops(L, hd, dtype, layout):
    """1920 x 1080 in a 1088-row coded picture: the fast path at the size the figures are quoted on (240 lanes a row pair: waves cross
    row pairs)"""
    data, rgba = hd
    got, _, _ = run_format(L, data, dtype, layout, gops_per_window=2, gpu_parser=True)
    assert_tensors(got, expected(L, rgba, dtype, layout), "1080p %s %s" % (dtype, layout))


@pytest.mark.parametrize("size,crop", [((224, 224), None), ((68, 120), None), ((224, 224), (419, 1, 1001, 1079))], ids=["224x224", "120x68-ratio16", "odd-offset-crop"])
@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("uint8", "chw"), ("float16", "hwc")])
def test_1080p_resized(L, hd, size, crop, dtype, layout):
    data, rgba = hd
    got, _, _ = run_format(L, data, dtype, layout, gops_per_window=2, gpu_parser=True, tensor_size=size, tensor_crop=crop)
    assert_tensors(got, expected(L, rgba, dtype, layout, size, crop), "1080p %s %s %s %s" % (dtype, layout, size, crop))


@FORMAT
@PARSERS
@pytest.mark.parametrize("case", ["360x199", "100x60"])
def test_resized_edges(L, case, gpu_parser, dtype, layout):
    """the crop and size cases of the resized float CHW tests: a reduction of the whole frame, a crop with taps outside the box down to an
    odd 23 x 13 (rows whose start is aligned to nothing), a quarter-size crop of the lower right quadrant"""
    fw, fh = EDGES[case]
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    rgba = oracle_frames(data)
    for size, crop in (((fh * 2 // 3, fw * 2 // 3), None), ((13, 23), (1, 1, fw - 3, fh - 2)), ((fh // 4, fw // 4), (fw // 2, fh // 2, fw - fw // 2, fh - fh // 2))):
        got, _, _ = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_size=size, tensor_crop=crop)
        assert_tensors(got, expected(L, rgba, dtype, layout, size, crop), "%s %s %s %s %s" % (case, dtype, layout, size, crop))


@FORMAT
def test_enlargement_largest_ratio_and_same_size(L, dtype, layout):
    data = ibbp_stream(96, 64, [6, 9], seed=2718)
    rgba = oracle_frames(data)
    for size, crop in (((62, 80), (3, 5, 40, 31)), ((200, 200), None), ((4, 6), None), ((31, 40), (3, 5, 40, 31)), ((40, 33), None)):
        got, _, _ = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_size=size, tensor_crop=crop)
        assert_tensors(got, expected(L, rgba, dtype, layout, size, crop), "%s %s %s %s" % (dtype, layout, size, crop))


@PARSERS
def test_beside_the_other_outputs(L, gpu_parser):
    """output = all with display_flavour GL: RGBA and the planes are what they are without the tensor, the tensor is the CPU twin's bytes"""
    data = fixture("leon_synth_352x240")
    got, rgba, planes = run_format(L, data, "uint8", "hwc", "all", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert_tensors(got, expected(L, oracle_frames(data), "uint8", "hwc"), "all, GL")
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert set(ref) == set(rgba) and all(np.array_equal(rgba[k], ref[k]) for k in ref)
    assert_planes(planes, oracle_planes(data), "all, GL")


def test_yuva_stream(L):
    """a yuva stream's alpha is in neither layout"""
    data = fixture("yuva_ibbp_96x64")
    for dtype, layout in (("uint8", "hwc"), ("uint8", "chw")):
        got, _, _ = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=True)
        assert_tensors(got, expected(L, oracle_frames(data), dtype, layout), "yuva %s" % layout)


@FORMAT
@pytest.mark.parametrize("size", [None, (97, 150)], ids=["frame-size", "resized"])
def test_views_info_and_shape(L, dtype, layout, size):
    """tensor_view / window_tensor have the shape, dtype and strides tensor_shape reports, are contiguous and equal read_tensor"""
    import torch
    data = ibbp_stream(368, 208, [6, 6], seed=5, frame=(360, 199))
    h, w = size or (199, 360)
    shape = (h, w, 3) if layout == "hwc" else (3, h, w)
    tdt = getattr(torch, dtype)
    raw = (lambda t: t.view(torch.int16) if dtype == "bfloat16" else t)
    seen = []

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        fl = list(frames)
        one = [bits(p.read_tensor(f)) for f in fl]
        views = [p.tensor_view(f) for f in fl]
        t = p.tensor_shape
        es = {"c": t.stride_c, "y": t.stride_y, "x": t.stride_x}
        want_strides = tuple(es[a] for a in ("yxc" if layout == "hwc" else "cyx"))
        assert all(v.dtype == tdt and tuple(v.shape) == shape and v.is_contiguous() and tuple(v.stride()) == want_strides for v in views)
        whole = p.window_tensor(fl[:6])
        gops = p.window_tensor(fl)
        assert whole is not None and whole.dtype == tdt and tuple(whole.stride())[1:] == want_strides and whole.stride()[0] * t.element_bytes == p.info.tensor_frame_pitch
        seen.append((one, [bits(raw(v).cpu().numpy()) for v in views], bits(raw(whole).cpu().numpy()), None if gops is None else tuple(gops.shape)))
    pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, on_window=on_window, output="all", tensor_dtype=dtype, tensor_layout=layout, tensor_size=size)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        i, t = pipe.info, pipe.tensor_shape
        e = {"uint8": 1, "float32": 4}.get(dtype, 2)
        code = L.TENSOR_U8 if dtype == "uint8" else L.TENSOR_DTYPES[dtype]
        assert (i.output, i.tensor_dtype, i.tensor_element_bytes, i.tensor_frame_bytes) == (19, code, e, 3 * h * w * e)
        assert i.tensor_frame_pitch == (i.tensor_frame_bytes + 255) // 256 * 256 and i.tensor_gop_pitch == 6 * i.tensor_frame_pitch
        assert (t.dtype, t.element_bytes, t.layout, t.channels, t.height, t.width) == (code, e, L.TENSOR_LAYOUTS[layout], 3, h, w)
        assert (t.stride_c, t.stride_y, t.stride_x) == ((1, 3 * w, 3) if layout == "hwc" else (h * w, w, 1))
    finally:
        pipe.close()
    assert seen
    for one, views, whole, gops_shape in seen:
        assert all(np.array_equal(a, b) for a, b in zip(one, views))
        assert whole.shape == (6,) + shape and all(np.array_equal(whole[k], one[k]) for k in range(6))
        assert gops_shape == (12,) + shape


def test_default_format_is_the_float_chw_pipeline(L):
    """tensor_layout "chw" with a float type goes the way it went (k_tensor); tensor_shape describes it"""
    data = fixture("ibbp_96x64")
    from test_pipeline_tensor_gpu import expected as expected_chw, run_tensor
    got, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_layout="chw")
    want = expected_chw(L, oracle_frames(data))
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    pipe = L.Pipeline(data, output="tensor")
    try:
        pipe.wait()
        t = pipe.tensor_shape
        assert (t.dtype, t.element_bytes, t.layout, t.stride_c, t.stride_y, t.stride_x) == (L.TENSOR_F16, 2, 0, t.height * t.width, t.width, 1)
    finally:
        pipe.close()
    pipe = L.Pipeline(data)
    try:
        pipe.wait()
        assert pipe.tensor_shape is None
        assert pipe.lib.leon_pipeline_get_tensor_shape(pipe.h, L.C.byref(L.PipelineTensorShape())) == L.ERR_INVALID
    finally:
        pipe.close()


def test_seek_exact(L):
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    want = expected(L, oracle_frames(data), "uint8", "hwc")
    import leon_vlc_ctypes as V
    rate = V.Stream(data, threads=1).info.picture_rate or 25.0
    t = 31.2 / rate
    cv, windows = threading.Condition(), {}

    def on_window(window, frames):
        got = {(f["gop"], f["display_index"]): bits(f["_pipe"].read_tensor(f)) for f in frames}
        with cv:
            windows[window] = got
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=True, on_window=on_window, output="tensor", tensor_dtype="uint8", tensor_layout="hwc")
    try:
        pipe.wait()
        first = pipe.seek(t, exact=True)
        pipe.wait()
        assert pipe.error is None
    finally:
        pipe.close()
    got = {}
    for wdw in sorted(windows):
        if wdw >= first:
            got.update(windows[wdw])
    assert got and min(got) > (0, 0)
    assert_tensors(got, {k: want[k] for k in got}, "seek")


def test_refusals(L):
    data = fixture("ibbp_96x64")
    for kw in (dict(tensor_layout=2), dict(tensor_dtype=4), dict(tensor_dtype=9), dict(tensor_dtype="uint8", tensor_scale=[1, 1, 1]),
               dict(tensor_dtype="uint8", tensor_layout="hwc", tensor_bias=[0, 0, 1]), dict(tensor_layout="hwc", tensor_filter=1, tensor_size=(40, 40))):
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output="tensor", **kw)
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="rgba", tensor_layout="hwc")
    odd = ibbp_stream(64, 48, [3], seed=3, frame=(61, 45))
    with pytest.raises(L.LeonError):
        L.Pipeline(odd, output="tensor", tensor_dtype="uint8", tensor_layout="hwc")          # an odd frame width stays refused
