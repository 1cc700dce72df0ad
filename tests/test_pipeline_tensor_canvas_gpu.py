"""GPU: the resampled image in a padded canvas (include/leon_pipeline.h, leon_pipeline_tensor_canvas) -- k_letterbox<element bytes,
layout, filter>, the image's tiles and the pad's workgroups in one launch per window.  Expected values never come from the code under
test: the ORACLE's RGBA through leon_ctypes.resize_rgb and the element table T, pasted with numpy into an array filled with
T[c][pad[c]].  Compared as bit patterns, no tolerance.  The geometries are tests/canvas_structure.py's CASES, each with the fact it
is here for (tests/test_canvas_structure.py proves them on the CPU)."""
import threading

import numpy as np
import pytest

import canvas_structure as S
from canvas_structure import BICUBIC, CASES, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_gpu import ibbp_stream, oracle_frames, run_pipeline
from test_pipeline_planes_gpu import assert_planes, oracle_planes
from test_pipeline_tensor_format_gpu import assert_tensors, bits, run_format

pytestmark = pytest.mark.gpu

# float16 and float32 CHW (one element store per lane and channel) and the four packed kernels
FORMATS = [("float16", "chw"), ("float32", "chw"), ("uint8", "chw"), ("uint8", "hwc"), ("float16", "hwc"), ("float32", "hwc")]
PAD = (114, 7, 250)          # differs per channel: a swapped channel shows
IMAGENET_SCALE = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)]
IMAGENET_BIAS = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
RUNS = [(c, f, d, l) for c in CASES for f in c.filters for d, l in FORMATS]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def streams():
    """name -> (stream bytes, {(gop, display index): the oracle's RGBA}): written and decoded once per module"""
    made = {}

    def get(name):
        if name not in made:
            cw, ch, gops, seed, (fw, fh) = STREAMS[name]
            data = ibbp_stream(cw, ch, gops, seed=seed, frame=(fw, fh))
            rgba = oracle_frames(data)
            assert all(v.shape == (fh, fw, 4) for v in rgba.values())
            if fh & 1:
                assert all((v[fh - 1, :, :3] == 255).all() for v in rgba.values())          # the fill row
            made[name] = (data, rgba)
        return made[name]
    return get


_resized = {}


def resized(L, key, rgba, crop, size, filt):
    """leon_ctypes.resize_rgb of the oracle's frames, computed once per (stream, crop, size, filter) and left unchanged"""
    k = (key, crop, size, filt)
    if k not in _resized:
        _resized[k] = {f: L.resize_rgb(v[..., :3], crop, size, filt) for f, v in rgba.items()}
        for v in _resized[k].values():
            v.setflags(write=False)
    return _resized[k]


def paste(L, images, dtype, layout, size, origin, canvas, pad, scale=None, bias=None):
    """{key: bit patterns in the layout's order}: full(T[c][pad[c]]) of the canvas with T[c][image] pasted at the origin"""
    T = bits(L.tensor_table(dtype, scale, bias))
    (oh, ow), (x, y), (ch, cw) = size, origin, canvas
    out = {}
    for k, rgb in images.items():
        assert rgb.shape == (oh, ow, 3)
        hwc = np.empty((ch, cw, 3), dtype=T.dtype)
        for c in range(3):
            hwc[..., c] = T[c][pad[c]]
            hwc[y:y + oh, x:x + ow, c] = T[c][rgb[..., c]]
        out[k] = np.ascontiguousarray(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return out


def canvas_kw(case, filt, pad=PAD):
    return dict(tensor_size=case.size, tensor_crop=case.crop, tensor_filter=filt, tensor_canvas=case.canvas, tensor_origin=case.origin, tensor_pad_value=pad)


def check(L, streams, case, filt, dtype, layout, pad=PAD, **kw):
    data, rgba = streams(case.stream)
    want = paste(L, resized(L, case.stream, rgba, case.crop, case.size, filt), dtype, layout, case.size, case.origin, case.canvas, pad,
                 kw.get("tensor_scale"), kw.get("tensor_bias"))
    kw.setdefault("gops_per_window", 2)
    kw.setdefault("gpu_parser", True)
    got, _, _ = run_format(L, data, dtype, layout, parser_threads=2, **canvas_kw(case, filt, pad), **kw)
    assert_tensors(got, want, "%s %s %s %s" % (case.name, FILTER_NAMES[filt], dtype, layout))
    return got


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "-".join([r[0].name, FILTER_NAMES[r[1]], r[2], r[3]]))
def test_case(L, streams, run):
    case, filt, dtype, layout = run
    assert case.holds(), case.why
    got = check(L, streams, case, filt, dtype, layout)
    if case.name == "unfused-road":          # the fill row of 255 is in the image (its last rows tap it), not in the pad
        fy, ny, _ = L.resize_weights(case.frame[1], 0, case.frame[1], case.size[0], filt)
        assert case.frame[1] & 1 and int(fy[-1] + ny[-1]) == case.frame[1] and 255 not in PAD
    if case.name == "canvas-equals-image":          # equals the run without a canvas, bit for bit
        data, _ = streams(case.stream)
        plain, _, _ = run_format(L, data, dtype, layout, parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_size=case.size, tensor_crop=case.crop, tensor_filter=filt)
        assert_tensors(got, plain, "canvas = image against no canvas")


def test_imagenet_scale_and_bias(L, streams):
    """pad values go through the element table like the image's: T[c][pad[c]] with a scale and bias per channel"""
    case = S.BY_NAME["all-start-classes"]
    for dtype, layout in (("float16", "chw"), ("float32", "hwc")):
        check(L, streams, case, TRIANGLE, dtype, layout, tensor_scale=IMAGENET_SCALE, tensor_bias=IMAGENET_BIAS)


def test_pad_defaults_and_centred_origin(L, streams):
    """tensor_pad_value defaults to (0, 0, 0), tensor_origin to centred; tensor_letterbox derives size, canvas and origin"""
    case = S.BY_NAME["letterbox"]
    data, rgba = streams(case.stream)
    want = paste(L, resized(L, case.stream, rgba, case.crop, case.size, TRIANGLE), "uint8", "hwc", case.size, case.origin, case.canvas, (0, 0, 0))
    got, _, _ = run_format(L, data, "uint8", "hwc", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_size=case.size, tensor_canvas=case.canvas)
    assert_tensors(got, want, "centred, pad 0")
    got, _, _ = run_format(L, data, "uint8", "hwc", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_letterbox=case.canvas)
    assert_tensors(got, want, "tensor_letterbox")
    case = S.BY_NAME["pillarbox"]
    want = paste(L, resized(L, case.stream, rgba, case.crop, case.size, TRIANGLE), "float16", "chw", case.size, case.origin, case.canvas, PAD)
    got, _, _ = run_format(L, data, "float16", "chw", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_letterbox=case.canvas, tensor_crop=case.crop,
                           tensor_pad_value=PAD)
    assert_tensors(got, want, "tensor_letterbox of a crop box")


def test_identity_resize_is_the_padded_full_frame(L, streams):
    data, rgba = streams("96x64")
    T = bits(L.tensor_table("uint8"))
    assert T is not None
    want = {}
    for k, v in rgba.items():
        hwc = np.empty((70, 101, 3), dtype=np.uint8)
        hwc[:] = np.asarray(PAD, dtype=np.uint8)
        hwc[3:67, 5:101] = v[..., :3]
        want[k] = hwc
    got, _, _ = run_format(L, data, "uint8", "hwc", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_size=(64, 96), tensor_canvas=(70, 101),
                           tensor_origin=(5, 3), tensor_pad_value=PAD)
    assert_tensors(got, want, "identity resize in a larger canvas")


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "chw")])
def test_ring_reuse_every_element_written_every_window(L, dtype, layout):
    """Six GOPs, one a window, two windows in flight: every ring entry is used three times.  The consumer overwrites every delivered
    tensor with 0xA5 bytes in place, synchronises, and only then releases: every later window must still be exact in every byte."""
    import torch
    case = S.BY_NAME["letterbox"]
    data = ibbp_stream(96, 64, [3, 6, 3, 6, 3, 6], seed=4242)
    rgba = oracle_frames(data)
    want = paste(L, {k: L.resize_rgb(v[..., :3], case.crop, case.size) for k, v in rgba.items()}, dtype, layout, case.size, case.origin, case.canvas, PAD)
    assert not any((w == (0xA5 if dtype == "uint8" else 0xA5A5)).all() for w in want.values())
    got, ptrs, lock = {}, [], threading.Lock()

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        fl = list(frames)
        with lock:
            for f in fl:
                got[(f["gop"], f["display_index"])] = bits(p.read_tensor(f))
                ptrs.append(f["tensor"])
        for f in fl:
            v = p.tensor_view(f)
            v.view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()
        for f in fl:
            assert (bits(p.read_tensor(f)) == (0xA5 if dtype == "uint8" else 0xA5A5)).all()          # the consumer's bytes are there
    pipe = L.Pipeline(data, on_window=on_window, output="tensor", tensor_dtype=dtype, tensor_layout=layout, parser_threads=2, gops_per_window=1, windows_in_flight=2,
                      gpu_parser=True, **canvas_kw(case, TRIANGLE))
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        assert pipe.windows == 6
    finally:
        pipe.close()
    assert len(set(ptrs)) < len(ptrs), "no ring entry was used twice"
    assert_tensors(got, want, "ring reuse %s %s" % (dtype, layout))


def test_host_parser(L, streams):
    case = S.BY_NAME["all-start-classes"]
    for dtype, layout in (("uint8", "chw"), ("float32", "chw")):
        check(L, streams, case, BICUBIC, dtype, layout, gpu_parser=False)


def test_a_window_per_gop(L, streams):
    """two windows of unequal length"""
    check(L, streams, S.BY_NAME["one-element-pad"], TRIANGLE, "float16", "hwc", gops_per_window=1)


def test_beside_the_other_outputs(L, streams):
    """output = all: RGBA and the planes are what they are without the tensor"""
    case = S.BY_NAME["letterbox"]
    data, rgba = streams(case.stream)
    want = paste(L, resized(L, case.stream, rgba, case.crop, case.size, TRIANGLE), "uint8", "hwc", case.size, case.origin, case.canvas, PAD)
    got, frames, planes = run_format(L, data, "uint8", "hwc", "all", parser_threads=2, gops_per_window=2, gpu_parser=True, **canvas_kw(case, TRIANGLE))
    assert_tensors(got, want, "all")
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=True)
    assert set(ref) == set(frames) and all(np.array_equal(frames[k], ref[k]) for k in ref)
    assert all(np.array_equal(frames[k], rgba[k]) for k in rgba)
    assert_planes(planes, oracle_planes(data), "all")


def test_seek_key(L):
    case = S.BY_NAME["pillarbox"]
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    want = paste(L, {k: L.resize_rgb(v[..., :3], case.crop, case.size) for k, v in oracle_frames(data).items()}, "uint8", "chw", case.size, case.origin, case.canvas, PAD)
    import leon_vlc_ctypes as V
    rate = V.Stream(data, threads=1).info.picture_rate or 25.0
    t = 31.2 / rate
    lock, windows = threading.Lock(), {}

    def on_window(window, frames):
        got = {(f["gop"], f["display_index"]): bits(f["_pipe"].read_tensor(f)) for f in frames}
        with lock:
            windows[window] = got
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=True, on_window=on_window, output="tensor", tensor_dtype="uint8", tensor_layout="chw",
                      **canvas_kw(case, TRIANGLE))
    try:
        pipe.wait()
        first = pipe.seek(t)
        pipe.wait()
        assert pipe.error is None
    finally:
        pipe.close()
    got = {}
    for wdw in sorted(windows):
        if wdw >= first:
            got.update(windows[wdw])
    assert got and min(got) > (0, 0) and min(got)[1] == 0          # from a GOP's first frame
    assert_tensors(got, {k: want[k] for k in got}, "seek")


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_views_geometry_and_shape(L, dtype, layout):
    """tensor_view / window_tensor, tensor_frame_bytes, the pitches, tensor_shape and tensor_geometry are the canvas's; the geometry's
    crop and taps describe the resampling; tensor_canvas_geometry reports the image rectangle"""
    import torch
    case = S.BY_NAME["all-start-classes"]
    data = ibbp_stream(96, 64, [6, 6], seed=5)
    (ch, cw), (oh, ow), (x, y) = case.canvas, case.size, case.origin
    shape = (ch, cw, 3) if layout == "hwc" else (3, ch, cw)
    e = 1 if dtype == "uint8" else 2
    raw = (lambda t: t)
    seen = []

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        fl = list(frames)
        one = [bits(p.read_tensor(f)) for f in fl]
        views = [p.tensor_view(f) for f in fl]
        assert all(tuple(v.shape) == shape and v.is_contiguous() and v.dtype == getattr(torch, dtype) for v in views)
        gops = p.window_tensor(fl)
        seen.append((one, [bits(raw(v).cpu().numpy()) for v in views], None if gops is None else (tuple(gops.shape), bits(gops.cpu().numpy()))))
    pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, on_window=on_window, output="tensor", tensor_dtype=dtype, tensor_layout=layout, **canvas_kw(case, TRIANGLE))
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        i, t, g, c = pipe.info, pipe.tensor_shape, pipe.tensor_geometry, pipe.tensor_canvas_geometry
        assert i.tensor_frame_bytes == 3 * ch * cw * e and i.tensor_frame_pitch == (i.tensor_frame_bytes + 255) // 256 * 256 and i.tensor_gop_pitch == 6 * i.tensor_frame_pitch
        assert (t.height, t.width, t.element_bytes) == (ch, cw, e)
        assert (t.stride_c, t.stride_y, t.stride_x) == ((1, 3 * cw, 3) if layout == "hwc" else (ch * cw, cw, 1))
        assert (g.width, g.height, g.crop_x, g.crop_y, g.crop_width, g.crop_height, g.resized) == (cw, ch, 0, 0, 96, 64, 1)
        fx, nx, _ = L.resize_weights(96, 0, 96, ow)
        fy, ny, _ = L.resize_weights(64, 0, 64, oh)
        assert (g.taps_x, g.taps_y) == (int(nx.max()), int(ny.max()))
        assert (c.width, c.height, c.x, c.y, c.image_width, c.image_height, tuple(c.pad), tuple(c.reserved)) == (cw, ch, x, y, ow, oh, PAD, (0,) * 7)
    finally:
        pipe.close()
    assert seen
    for one, views, gops in seen:
        assert all(np.array_equal(a, b) for a, b in zip(one, views))
        assert gops is not None and gops[0] == (12,) + shape and all(np.array_equal(gops[1][k], one[k]) for k in range(12))
    # without canvas settings the canvas reported is the tensor itself
    pipe = L.Pipeline(data, output="tensor", tensor_size=(oh, ow))
    try:
        pipe.wait()
        c = pipe.tensor_canvas_geometry
        assert (c.width, c.height, c.x, c.y, c.image_width, c.image_height, tuple(c.pad)) == (ow, oh, 0, 0, ow, oh, (0, 0, 0))
    finally:
        pipe.close()


@pytest.fixture(scope="module")
def hd(L):
    import stream_1080p
    data = stream_1080p.load()
    rgba = oracle_frames(data)
    ow, oh, x, y = L.letterbox(1920, 1080, 640, 640)
    assert (ow, oh, x, y) == (640, 360, 0, 140)
    return data, {k: L.resize_rgb(v[..., :3], None, (oh, ow)) for k, v in rgba.items()}


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_1080p_letterbox_640(L, hd, dtype, layout):
    """the typical size: 1920 x 1080 -> 640 x 360 at (0, 140) in 640 x 640"""
    data, images = hd
    want = paste(L, images, dtype, layout, (360, 640), (0, 140), (640, 640), PAD)
    got, _, _ = run_format(L, data, dtype, layout, gops_per_window=2, gpu_parser=True, tensor_letterbox=(640, 640), tensor_pad_value=PAD)
    assert_tensors(got, want, "1080p letterbox %s %s" % (dtype, layout))
