"""GPU: LEON_PIPELINE_OUTPUT_TENSOR (include/leon_pipeline.h) -- the pipeline delivers every frame as a planar [3, H, W] tensor of
fp16 / bf16 / fp32 elements, tensor[c][y][x] = T[c][RGBA of the CPU twin], T the host-built table (leon_ctypes.tensor_table states
it in numpy).  Expected = T looked up with the ORACLE's RGBA; compared as bit patterns, no tolerance: both roads (k_recon_display_out
/ k_planes_crop feeding k_tensor), both front ends, the three element types, every combination of outputs, seek, held windows,
partial streams, shards."""
import os
import threading
import time

import numpy as np
import pytest

from test_pipeline_gpu import STREAMS, ibbp_stream, oracle_frames, run_pipeline
from test_pipeline_planes_gpu import FIXTURES, assert_planes, oracle_planes

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
DTYPES = pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
IMAGENET = dict(tensor_scale=[1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)], tensor_bias=[-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def fixture(name):
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


def bits(a):
    """an array of elements as unsigned bit patterns"""
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def expected(L, rgba, dtype="float16", scale=None, bias=None):
    """{key: [3, H, W] bit patterns}: T[c][oracle RGBA[..., c]]"""
    T = bits(L.tensor_table(dtype, scale, bias))
    return {k: np.stack([T[c][v[..., c]] for c in range(3)]) for k, v in rgba.items()}


def run_tensor(L, data, output="tensor", **kw):
    """({key: tensor bits}, {key: RGBA or None}, {key: planes or None}, [(gop, display_index, ts_ms)]) of a whole run"""
    kw.setdefault("gpu_parser", False)
    tensors, rgba, planes, order, lock = {}, {}, {}, [], threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                k = (f["gop"], f["display_index"])
                p = f["_pipe"]
                assert f["tensor"] and f["tensor"] % 256 == 0
                tensors[k] = bits(p.read_tensor(f))
                rgba[k] = L.read_frame(f) if f["rgba"] else None
                planes[k] = p.read_planes(f) if f["y"] else None
                assert (f["y"] is None) == (f["cb"] is None) == (f["cr"] is None)
                order.append((f["gop"], f["display_index"], f["ts_ms"]))
    pipe = L.Pipeline(data, on_window=on_window, output=output, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return tensors, rgba, planes, order


def assert_tensors(got, want, what):
    assert set(got) == set(want), "%s: frames %s" % (what, sorted(set(got) ^ set(want))[:8])
    for k in sorted(want):
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s, want %s %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s: %d of %d elements differ, first at [c, y, x] = %s: got %#x, want %#x" % (
                what, k, len(bad), g.size, bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])])))


@DTYPES
@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams_tensor(L, name, gpu_parser, dtype):
    data = fixture(name)
    want = expected(L, oracle_frames(data), dtype)
    got, rgba, planes, order = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_dtype=dtype)
    assert_tensors(got, want, "%s %s" % (name, dtype))
    assert all(v is None for v in rgba.values()) and all(v is None for v in planes.values())      # frame.rgba and the planes are NULL
    assert order == sorted(order)


@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams_all(L, name, gpu_parser):
    """output = all: the tensor as above (ImageNet normalisation here), the RGBA a default pipeline's, the planes the oracle's"""
    data = fixture(name)
    want = expected(L, oracle_frames(data), "float16", IMAGENET["tensor_scale"], IMAGENET["tensor_bias"])
    got, rgba, planes, _ = run_tensor(L, data, "all", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, **IMAGENET)
    assert_tensors(got, want, name)
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert set(ref) == set(rgba)
    for k in ref:
        assert np.array_equal(rgba[k], ref[k]), "%s %s: RGBA of output=all differs from the default pipeline's" % (name, k)
    assert_planes(planes, oracle_planes(data), name)
    got2, rgba2, planes2, _ = run_tensor(L, data, "ycbcr+tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, **IMAGENET)
    assert_tensors(got2, want, name + " ycbcr+tensor")
    assert all(v is None for v in rgba2.values())
    assert_planes(planes2, oracle_planes(data), name + " ycbcr+tensor")


@DTYPES
@PARSERS
@pytest.mark.parametrize("case", ["360x199", "100x60", "200x64"])
def test_layout_edges(L, case, gpu_parser, dtype):
    """360 x 199: the fused road and an odd height -- the last row is the twin's fill value, T[c][255].
    100 x 60: the unfused road (k_planes_crop), width % 8 = 4: k_tensor's per-quad path.
    200 x 64: a multiple of 8 whose row pair (25 lanes of 8 pixels, 50 of 4) never ends with a wave, and whose last workgroup ends
    inside one: float CHW shares the kernel in which the lanes behind the frame matter (the HWC exchange)"""
    fw, fh = {"360x199": (360, 199), "100x60": (100, 60), "200x64": (200, 64)}[case]
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    rgba = oracle_frames(data)
    want = expected(L, rgba, dtype)
    if fh & 1:
        T = bits(L.tensor_table(dtype))
        assert all((v[fh - 1] == 255).all() for v in rgba.values())
        assert all((w[c, fh - 1] == T[c][255]).all() for w in want.values() for c in range(3))
    for output in ("tensor", "rgba+tensor"):
        got, _, _, _ = run_tensor(L, data, output, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, tensor_dtype=dtype)
        assert_tensors(got, want, "%s %s %s" % (case, output, dtype))


def test_1080p_two_gops(L):
    import stream_1080p
    data = stream_1080p.load()
    want = expected(L, oracle_frames(data), "float16")
    got, _, _, _ = run_tensor(L, data, "tensor", gops_per_window=2, gpu_parser=True)
    assert_tensors(got, want, "1080p")


@DTYPES
def test_every_table_entry_is_read(L, dtype):
    """The conversion's arithmetic is tested for all 2^24 (Y, Cb, Cr) elsewhere (test_fused_display_gpu.py); here every one of the
    768 entries of T is looked up: the oracle's RGBA of this stream holds all 256 values in each of R, G and B (asserted first), and
    the table has 768 different entries (a range of its own per channel), so a wrong entry or a wrong channel's entry shows."""
    data = ibbp_stream(96, 64, [6, 9], seed=2718)
    rgba = oracle_frames(data)
    allf = np.stack(list(rgba.values()))
    for c in range(3):
        assert len(np.unique(allf[..., c])) == 256, "channel %d of the stream's frames lacks values" % c
    scale, bias = [1.0, -1.0, 2.0 ** -10], [0.0, -1.0, 2.0 ** -10]       # 0 .. 255, -1 .. -256, 1/1024 .. 1/4: exact in all three types
    T = bits(L.tensor_table(dtype, scale, bias))
    assert len(np.unique(T)) == 768
    got, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, gpu_parser=True, tensor_dtype=dtype, tensor_scale=scale, tensor_bias=bias)
    assert_tensors(got, expected(L, rgba, dtype, scale, bias), "every entry %s" % dtype)
    seen = np.unique(np.concatenate([g.ravel() for g in got.values()]))
    assert np.array_equal(seen, np.unique(T))


@PARSERS
def test_gl_flavour_leaves_the_tensor_alone(L, gpu_parser):
    """display_flavour = GL governs frame.rgba only: the RGBA is a GL pipeline's, the tensor still the CPU twin's through T"""
    data = fixture("leon_synth_352x240")
    want = expected(L, oracle_frames(data), "bfloat16")
    got, rgba, _, _ = run_tensor(L, data, "rgba+tensor", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL, tensor_dtype="bfloat16")
    assert_tensors(got, want, "GL rgba+tensor")
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert set(ref) == set(rgba) and all(np.array_equal(rgba[k], ref[k]) for k in ref)


class Log:
    def __init__(self, read):
        self.cv = threading.Condition()
        self.windows = {}
        self.read = read

    def on_window(self, window, frames):
        got = {(f["gop"], f["display_index"]): (bits(f["_pipe"].read_tensor(f)) if self.read else None) for f in frames}
        with self.cv:
            self.windows[window] = got
            self.cv.notify_all()

    def since(self, first):
        with self.cv:
            out = {}
            for w in sorted(self.windows):
                if w >= first:
                    out.update(self.windows[w])
            return out


def frames_after_seek(L, data, gpu_parser, t, exact, output):
    log = Log(output != "rgba")
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=log.on_window, output=output)
    try:
        pipe.wait()
        first = pipe.seek(t, exact=exact)
        pipe.wait()
        assert pipe.error is None
    finally:
        pipe.close()
    return log.since(first)


@PARSERS
@pytest.mark.parametrize("exact", [False, True], ids=["key", "exact"])
def test_seek(L, gpu_parser, exact):
    """after a KEY or EXACT seek: the oracle's tensors, for exactly the frames an RGBA pipeline delivers after the same seek"""
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    want = expected(L, oracle_frames(data))
    import leon_vlc_ctypes as V
    rate = V.Stream(data, threads=1).info.picture_rate or 25.0
    for t in (0.0, 13.5 / rate, 31.2 / rate):
        got = frames_after_seek(L, data, gpu_parser, t, exact, "tensor")
        assert got, "nothing delivered after seeking to %.3f s" % t
        assert_tensors(got, {k: want[k] for k in got}, "seek %.3f" % t)
        assert set(got) == set(frames_after_seek(L, data, gpu_parser, t, exact, "rgba")), "seek %.3f: other frames than the RGBA pipeline's" % t


@PARSERS
def test_held_window_keeps_its_tensors(L, gpu_parser):
    """W = 1, R = 2: window 0 is held while the later windows decode through the other ring entry; its tensors are unchanged"""
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=99)
    want = expected(L, oracle_frames(data))
    held, later, cv = [], {}, threading.Condition()

    def on_window(window, frames):
        with cv:
            if not held:
                held.append((window, [dict(f) for f in frames]))
                cv.notify_all()
                return False
            for f in frames:
                later[(f["gop"], f["display_index"])] = bits(f["_pipe"].read_tensor(f))
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, windows_in_flight=2, gpu_parser=gpu_parser, on_window=on_window, output="tensor")
    try:
        with cv:
            assert cv.wait_for(lambda: held, 30)
        t0 = time.time()
        while time.time() - t0 < 5 and len(later) < 6:
            time.sleep(0.01)
        window, frames = held[0]
        got = {(f["gop"], f["display_index"]): bits(pipe.read_tensor(f)) for f in frames}
        views = {(f["gop"], f["display_index"]): bits(pipe.tensor_view(f).cpu().numpy()) for f in frames}
        assert_tensors(got, {k: want[k] for k in got}, "held window")
        assert_tensors(views, got, "held window, in place")
        pipe.release_window(window)
        with pytest.raises(L.LeonError):
            pipe.read_tensor(frames[0])                  # released: its tensors are no longer handed out
        pipe.wait()
    finally:
        pipe.close()
    assert len(later) > 0
    assert_tensors(later, {k: want[k] for k in later}, "later windows")


@PARSERS
def test_partial_stream(L, gpu_parser):
    import leon_vlc_ctypes as V
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=77)
    want = expected(L, oracle_frames(data), "float32")
    offs = V.Stream(data, threads=1).keymap()
    got, lock = {}, threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                got[(f["gop"], f["display_index"])] = bits(f["_pipe"].read_tensor(f))
    first = offs[1] + 3
    buf = bytearray(len(data))
    buf[:first] = data[:first]
    pipe = L.Pipeline(bytes(buf), parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=on_window, valid_bytes=first, output="tensor",
                      tensor_dtype="float32")
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


@PARSERS
def test_gop_shards(L, gpu_parser):
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=31)
    want = expected(L, oracle_frames(data))
    got = {}
    for r in range(2):
        part, _, _, _ = run_tensor(L, data, "tensor", parser_threads=2, gops_per_window=2, shard_index=r, shard_count=2, gpu_parser=gpu_parser)
        assert {g for g, _ in part} == {g for g in range(5) if g % 2 == r}
        assert not set(part) & set(got)
        got.update(part)
    assert_tensors(got, want, "shards")


@DTYPES
def test_views_and_info(L, dtype):
    """tensor_view / window_tensor wrap the ring in place (torch, no copy) and equal read_tensor; leon_pipeline_info reports the layout"""
    import torch
    data = ibbp_stream(368, 208, [6, 6], seed=5, frame=(360, 199))
    seen = []

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        fl = list(frames)
        one = [bits(p.read_tensor(f)) for f in fl]
        views = [p.tensor_view(f) for f in fl]
        assert all(v.dtype == getattr(torch, dtype) and tuple(v.shape) == (3, 199, 360) and v.is_contiguous() for v in views)
        whole = p.window_tensor(fl[:6])                  # the six display positions of the window's first GOP: evenly spaced
        gops = p.window_tensor(fl)                       # two GOPs of six: the lanes are max_gop_pictures = 6 positions apart, too
        mixed = p.window_tensor([fl[0], fl[2], fl[3]])   # not evenly spaced
        seen.append((one, [bits(v.cpu().view(torch.int16).numpy() if dtype == "bfloat16" else v.cpu().numpy()) for v in views],
                     None if whole is None else bits((whole.view(torch.int16) if dtype == "bfloat16" else whole).cpu().numpy()),
                     None if gops is None else tuple(gops.shape), mixed))
    pipe = L.Pipeline(data, gops_per_window=2, gpu_parser=True, on_window=on_window, output="all", tensor_dtype=dtype)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        i = pipe.info
        e = 4 if dtype == "float32" else 2
        assert (i.output, i.tensor_dtype, i.tensor_element_bytes, i.tensor_frame_bytes) == (19, L.TENSOR_DTYPES[dtype], e, 3 * 199 * 360 * e)
        assert i.tensor_frame_pitch == (i.tensor_frame_bytes + 255) // 256 * 256 and i.tensor_gop_pitch == 6 * i.tensor_frame_pitch
    finally:
        pipe.close()
    assert seen
    for one, views, whole, gops_shape, mixed in seen:
        assert all(np.array_equal(a, b) for a, b in zip(one, views))
        assert whole is not None and whole.shape == (6, 3, 199, 360) and all(np.array_equal(whole[k], one[k]) for k in range(6))
        assert gops_shape == (12, 3, 199, 360) and mixed is None


def test_refusals(L):
    odd = ibbp_stream(64, 48, [3], seed=3, frame=(61, 45))
    with pytest.raises(L.LeonError):
        L.Pipeline(odd, output="tensor")                 # odd frame width: the twin's index drift is not carried into the tensor
    run_pipeline(L, odd, gops_per_window=1)              # (the RGBA pipeline decodes it)
    data = fixture("ibbp_96x64")
    for kw in (dict(tensor_dtype=4), dict(tensor_scale=[float("nan"), 1, 1]), dict(tensor_scale=[1e3, 1e3, 1e3]), dict(tensor_bias=[0, float("inf"), 0])):
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output="tensor", **kw)
    lib = L.load()
    import ctypes as C
    cfg = L.PipelineConfig()
    cfg.output = L.PIPELINE_OUTPUT_RGBA
    t = L.PipelineTensorConfig(L.TENSOR_F32, (C.c_float * 3)(), (C.c_float * 3)())
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h = C.c_void_p()
    cb = L.PIPELINE_CB(lambda *a: None)
    assert lib.leon_pipeline_create_tensor(C.byref(cfg), C.byref(t), buf, len(data), len(data), cb, None, C.byref(h)) == L.ERR_INVALID      # a dtype without the bit
    seen = {}

    def on_window(window, frames):
        f = frames[0]
        p = f["_pipe"]
        ptrs = (C.c_void_p * len(frames))()
        host = np.empty(3 * 96 * 64 * 4, np.uint8)
        seen["rgba pipeline"] = (f["tensor"], p.lib.leon_pipeline_window_tensors(p.h, window, ptrs, len(frames)),
                                 p.lib.leon_pipeline_read_tensor(p.h, window, 0, host.ctypes.data))
    pipe = L.Pipeline(data, gops_per_window=1, gpu_parser=False, on_window=on_window)
    try:
        pipe.wait()
    finally:
        pipe.close()
    assert seen["rgba pipeline"] == (None, L.ERR_INVALID, L.ERR_INVALID)

    def on_tensor_window(window, frames):
        f = frames[0]
        p = f["_pipe"]
        rec = f["_frames"][f["_i"]]
        buf4 = np.empty(96 * 64 * 4, np.uint8)
        host = np.empty(3 * 96 * 64 * 2, np.uint8)
        ptrs = (C.c_void_p * (len(frames) + 1))()
        seen.setdefault("tensor pipeline", (p.lib.leon_pipeline_read_frame(p.h, C.byref(rec), buf4.ctypes.data),
                                            p.lib.leon_pipeline_read_frame_planes(p.h, C.byref(rec), buf4.ctypes.data, buf4.ctypes.data, buf4.ctypes.data, None),
                                            p.lib.leon_pipeline_window_tensors(p.h, window, ptrs, len(frames) + 1),
                                            p.lib.leon_pipeline_read_tensor(p.h, window, len(frames), host.ctypes.data),
                                            p.lib.leon_pipeline_read_tensor(p.h, window + 1000, 0, host.ctypes.data),
                                            p.lib.leon_pipeline_read_tensor(p.h, window, 0, host.ctypes.data)))
    pipe = L.Pipeline(data, gops_per_window=1, gpu_parser=False, on_window=on_tensor_window, output="tensor")
    try:
        pipe.wait()
    finally:
        pipe.close()
    assert seen["tensor pipeline"] == (L.ERR_INVALID,) * 5 + (L.OK,)
