"""GPU: the tensor output at a model's input size (leon_pipeline_tensor_resize, include/leon_pipeline.h) -- a crop box of every frame
resampled on the device to [3, out_h, out_w] by k_resample.  Expected = T[c][resize_rgb(ORACLE RGBA, crop, size)]: the oracle's
RGBA through the numpy statement of the two integer passes (leon_ctypes.resize_rgb) and the element table; compared as bit
patterns, no tolerance.  Both roads into the planes, both front ends, the three element types, reductions up to 16, crops,
an enlargement, every output combination, seek, held windows, partial streams, shards."""
import threading
import time

import numpy as np
import pytest

from test_pipeline_gpu import ibbp_stream, oracle_frames, run_pipeline
from test_pipeline_planes_gpu import FIXTURES, assert_planes, oracle_planes
from test_pipeline_tensor_gpu import IMAGENET, Log, assert_tensors, bits, fixture, run_tensor

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
DTYPES = pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def expected(L, rgba, size, crop=None, dtype="float16", scale=None, bias=None):
    """{key: [3, out_h, out_w] bit patterns}: T[c][resize_rgb(oracle RGBA, crop, size)[..., c]]"""
    T = bits(L.tensor_table(dtype, scale, bias))
    out = {}
    for k, v in rgba.items():
        r = L.resize_rgb(v[..., :3], crop, size)
        out[k] = np.stack([T[c][r[..., c]] for c in range(3)])
    return out


def fixture_size(L, data):
    """a reducing size for a fixture stream: about 5 / 8 of the frame, odd on purpose"""
    import leon_vlc_ctypes as V
    i = V.Stream(data, threads=1).info
    return (max(1, i.frame_height * 5 // 8) | 1, max(1, i.frame_width * 5 // 8) | 1)


@DTYPES
@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams_resized(L, name, gpu_parser, dtype):
    data = fixture(name)
    size = fixture_size(L, data)
    want = expected(L, oracle_frames(data), size, None, dtype)
    got, rgba, planes, order = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_dtype=dtype, tensor_size=size)
    assert_tensors(got, want, "%s %s -> %s" % (name, dtype, size))
    assert all(v is None for v in rgba.values()) and all(v is None for v in planes.values())
    assert order == sorted(order)


@DTYPES
@PARSERS
@pytest.mark.parametrize("case", ["360x199", "100x60"])
def test_layout_edges(L, case, gpu_parser, dtype):
    """360 x 199: an odd height -- the twin's fill row of 255 takes part in the last output rows.  100 x 60: the unfused road
    (k_planes_crop), a width that is no multiple of 8: the last staged group of 8 columns reaches into the row's padding"""
    fw, fh = (360, 199) if case == "360x199" else (100, 60)
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    rgba = oracle_frames(data)
    if fh & 1:
        assert all((v[fh - 1] == 255).all() for v in rgba.values())
    for size, crop in (((fh * 2 // 3, fw * 2 // 3), None), ((13, 23), (1, 1, fw - 3, fh - 2)), ((fh // 4, fw // 4), (fw // 2, fh // 2, fw - fw // 2, fh - fh // 2))):
        want = expected(L, rgba, size, crop, dtype)
        got, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_dtype=dtype, tensor_size=size, tensor_crop=crop)
        assert_tensors(got, want, "%s %s %s %s" % (case, dtype, size, crop))


@PARSERS
def test_yuva_stream(L, gpu_parser):
    """a yuva stream: the alpha plane lies behind Cr in the planes record and is not in the tensor"""
    data = fixture("yuva_ibbp_96x64")
    size = (48, 48)
    want = expected(L, oracle_frames(data), size)
    got, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_size=size)
    assert_tensors(got, want, "yuva")


@pytest.fixture(scope="module")
def hd(L):
    import stream_1080p
    data = stream_1080p.load()
    return data, oracle_frames(data)


@pytest.mark.parametrize("size,crop", [((224, 224), None), ((68, 120), None), ((224, 224), (420, 0, 1080, 1080)), ((224, 224), (419, 1, 1001, 1079)),
                                       ((216, 384), None)],
                         ids=["224x224", "120x68-ratio16", "centre-crop", "odd-offset-crop", "384x216"])
def test_1080p_two_gops(L, hd, size, crop):
    """1080p: 18 and 10 taps (224 x 224), the largest ratio (1920 / 120 = 16, 1080 / 68 = 15.9: 32 taps, the staging buffer takes 6 rows
    at a time), crops with even and odd offsets"""
    data, rgba = hd
    want = expected(L, rgba, size, crop)
    got, _, _, _ = run_tensor(L, data, "tensor", gops_per_window=2, gpu_parser=True, tensor_size=size, tensor_crop=crop)
    assert_tensors(got, want, "1080p %s %s" % (size, crop))


@DTYPES
def test_enlargement_and_same_size_crop(L, dtype):
    data = ibbp_stream(96, 64, [6, 9], seed=2718)
    rgba = oracle_frames(data)
    crop = (3, 5, 40, 31)
    got, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_dtype=dtype, tensor_size=(62, 80), tensor_crop=crop)
    assert_tensors(got, expected(L, rgba, (62, 80), crop, dtype), "enlargement %s" % dtype)
    whole, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_dtype=dtype, tensor_size=(200, 200))
    assert_tensors(whole, expected(L, rgba, (200, 200), None, dtype), "enlargement of the whole frame %s" % dtype)
    # same size with a crop = the crop of the full-size tensor pipeline's output
    full, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_dtype=dtype)
    same, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_dtype=dtype, tensor_size=(31, 40), tensor_crop=crop)
    assert_tensors(same, {k: np.ascontiguousarray(v[:, 5:36, 3:43]) for k, v in full.items()}, "same size %s" % dtype)


@PARSERS
@pytest.mark.parametrize("output", ["rgba+tensor", "ycbcr+tensor", "all"])
def test_output_combinations(L, output, gpu_parser):
    """the tensor resized, RGBA and planes a default pipeline's, full size"""
    data = fixture("leon_synth_352x240")
    size = (112, 160)
    want = expected(L, oracle_frames(data), size, None, "float16", IMAGENET["tensor_scale"], IMAGENET["tensor_bias"])
    got, rgba, planes, _ = run_tensor(L, data, output, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_size=size, **IMAGENET)
    assert_tensors(got, want, output)
    if "rgba" in output or output == "all":
        ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
        assert set(ref) == set(rgba) and all(np.array_equal(rgba[k], ref[k]) for k in ref)
    else:
        assert all(v is None for v in rgba.values())
    if "ycbcr" in output or output == "all":
        assert_planes(planes, oracle_planes(data), output)
    else:
        assert all(v is None for v in planes.values())


SIZE = (40, 56)


@pytest.mark.parametrize("exact", [False, True], ids=["key", "exact"])
def test_seek(L, exact):
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    want = expected(L, oracle_frames(data), SIZE)
    import leon_vlc_ctypes as V
    rate = V.Stream(data, threads=1).info.picture_rate or 25.0
    t = 31.2 / rate
    log = Log(True)
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=True, on_window=log.on_window, output="tensor", tensor_size=SIZE)
    try:
        pipe.wait()
        first = pipe.seek(t, exact=exact)
        pipe.wait()
        assert pipe.error is None
    finally:
        pipe.close()
    got = log.since(first)
    assert got
    assert_tensors(got, {k: want[k] for k in got}, "seek")
    ref = Log(False)
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=True, on_window=ref.on_window)
    try:
        pipe.wait()
        first = pipe.seek(t, exact=exact)
        pipe.wait()
    finally:
        pipe.close()
    assert set(got) == set(ref.since(first))


def test_held_window_keeps_its_tensors(L):
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=99)
    want = expected(L, oracle_frames(data), SIZE)
    held, later, cv = [], {}, threading.Condition()

    def on_window(window, frames):
        with cv:
            if not held:
                held.append((window, [dict(f) for f in frames]))
                cv.notify_all()
                return False
            for f in frames:
                later[(f["gop"], f["display_index"])] = bits(f["_pipe"].read_tensor(f))
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, windows_in_flight=2, gpu_parser=True, on_window=on_window, output="tensor", tensor_size=SIZE)
    try:
        with cv:
            assert cv.wait_for(lambda: held, 30)
        t0 = time.time()
        while time.time() - t0 < 5 and len(later) < 6:
            time.sleep(0.01)
        window, frames = held[0]
        got = {(f["gop"], f["display_index"]): bits(pipe.read_tensor(f)) for f in frames}
        assert_tensors(got, {k: want[k] for k in got}, "held window")
        pipe.release_window(window)
        pipe.wait()
    finally:
        pipe.close()
    assert len(later) > 0
    assert_tensors(later, {k: want[k] for k in later}, "later windows")


def test_partial_stream(L):
    import leon_vlc_ctypes as V
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=77)
    want = expected(L, oracle_frames(data), SIZE, None, "float32")
    offs = V.Stream(data, threads=1).keymap()
    got, lock = {}, threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                got[(f["gop"], f["display_index"])] = bits(f["_pipe"].read_tensor(f))
    first = offs[1] + 3
    buf = bytearray(len(data))
    buf[:first] = data[:first]
    pipe = L.Pipeline(bytes(buf), parser_threads=2, gops_per_window=1, gpu_parser=True, on_window=on_window, valid_bytes=first, output="tensor",
                      tensor_dtype="float32", tensor_size=SIZE)
    try:
        at = first
        for step in (500, 1, 1800, 700, 10 ** 9):
            n = min(step, len(data) - at)
            pipe.feed(at + n, data[at:at + n], at)
            at += n
            if at == len(data):
                break
        pipe.wait()
    finally:
        pipe.close()
    assert_tensors(got, want, "partial")


def test_gop_shards(L):
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=31)
    want = expected(L, oracle_frames(data), SIZE)
    got = {}
    for r in range(2):
        part, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, shard_index=r, shard_count=2, gpu_parser=True, tensor_size=SIZE)
        assert {g for g, _ in part} == {g for g in range(5) if g % 2 == r}
        got.update(part)
    assert_tensors(got, want, "shards")


@DTYPES
def test_views_info_and_geometry(L, dtype):
    import torch
    data = ibbp_stream(368, 208, [6, 6], seed=5, frame=(360, 199))
    oh, ow = 97, 150
    crop = (10, 3, 340, 190)
    seen = []

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        fl = list(frames)
        one = [bits(p.read_tensor(f)) for f in fl]
        views = [p.tensor_view(f) for f in fl]
        assert all(v.dtype == getattr(torch, dtype) and tuple(v.shape) == (3, oh, ow) and v.is_contiguous() for v in views)
        whole = p.window_tensor(fl[:6])
        gops = p.window_tensor(fl)
        seen.append((one, [bits(v.cpu().view(torch.int16).numpy() if dtype == "bfloat16" else v.cpu().numpy()) for v in views],
                     None if whole is None else bits((whole.view(torch.int16) if dtype == "bfloat16" else whole).cpu().numpy()),
                     None if gops is None else tuple(gops.shape)))
    pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, on_window=on_window, output="all", tensor_dtype=dtype, tensor_size=(oh, ow), tensor_crop=crop)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        i, g = pipe.info, pipe.tensor_geometry
        e = 4 if dtype == "float32" else 2
        assert (i.output, i.tensor_dtype, i.tensor_element_bytes, i.tensor_frame_bytes) == (19, L.TENSOR_DTYPES[dtype], e, 3 * oh * ow * e)
        assert i.tensor_frame_pitch == (i.tensor_frame_bytes + 255) // 256 * 256 and i.tensor_gop_pitch == 6 * i.tensor_frame_pitch
        assert (i.frame_width, i.frame_height) == (360, 199)
        assert (g.width, g.height, g.crop_x, g.crop_y, g.crop_width, g.crop_height, g.resized) == (ow, oh) + crop + (1,)
        assert (g.taps_x, g.taps_y) == (L.resize_weights(360, 10, 340, ow)[2].shape[1], L.resize_weights(199, 3, 190, oh)[2].shape[1])
    finally:
        pipe.close()
    assert seen
    for one, views, whole, gops_shape in seen:
        assert all(np.array_equal(a, b) for a, b in zip(one, views))
        assert whole is not None and whole.shape == (6, 3, oh, ow) and all(np.array_equal(whole[k], one[k]) for k in range(6))
        assert gops_shape == (12, 3, oh, ow)
    # without resize settings the geometry is the frame's
    pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, output="tensor", tensor_dtype=dtype)
    try:
        pipe.wait()
        g = pipe.tensor_geometry
        assert (g.width, g.height, g.crop_x, g.crop_y, g.crop_width, g.crop_height, g.taps_x, g.taps_y, g.resized) == (360, 199, 0, 0, 360, 199, 1, 1, 0)
    finally:
        pipe.close()


def test_refusals(L):
    data = fixture("ibbp_96x64")
    for kw in (dict(tensor_size=(0, 40)), dict(tensor_size=(40, 4097)), dict(tensor_size=(3, 40)),                     # 64 / 3 > 16
               dict(tensor_size=(40, 40), tensor_crop=(60, 0, 40, 40)), dict(tensor_size=(40, 40), tensor_crop=(0, 0, 0, 40)),
               dict(tensor_size=(40, 40), tensor_crop=(-1, 0, 40, 40)), dict(tensor_size=(40, 40), tensor_filter=1), dict(tensor_crop=(0, 0, 40, 40))):
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output="tensor", **kw)
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="rgba", tensor_size=(40, 40))            # resize settings without the TENSOR bit
    with pytest.raises(L.LeonError):
        L.Pipeline(data, output="ycbcr", tensor_size=(40, 40))
    got, _, _, _ = run_tensor(L, data, "tensor", gops_per_window=1, tensor_size=(4, 6))      # 64 / 4 = 96 / 6 = 16: the edge works
    assert_tensors(got, expected(L, oracle_frames(data), (4, 6)), "ratio 16")
