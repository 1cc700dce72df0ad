"""GPU: regions of delivered frames as a tensor batch (include/leon_pipeline.h, leon_pipeline_resample_regions) -- k_regions<element
bytes, layout, filter>, one launch per call, every region with its own source frame, destination and tables.  Expected values never
come from the code under test: the ORACLE's RGBA of the region's frame through leon_ctypes.resize_rgb(rgb, box, size, filter) and the
element table T, compared as bit patterns, no tolerance.  The calls are tests/regions_structure.py's (tests/test_regions_structure.py
proves on the CPU what each holds): their boxes dealt over every frame of a window of two GOPs (3 and 6 pictures), out of the frames'
order, two regions on one frame."""
import ctypes as C
import threading

import numpy as np
import pytest

import regions_structure as S
from regions_structure import BICUBIC, CALLS, FILTERS, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_gpu import ibbp_stream, oracle_frames
from test_pipeline_tensor_format_gpu import bits

pytestmark = pytest.mark.gpu

FORMATS = [("float16", "chw"), ("float32", "chw"), ("uint8", "chw"), ("uint8", "hwc"), ("float16", "hwc"), ("float32", "hwc")]
IMAGENET_SCALE = [1.0 / (255.0 * s) for s in (0.229, 0.224, 0.225)]
IMAGENET_BIAS = [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))]
RUNS = [(c, f, d, l) for c in sorted(CALLS) for f in FILTERS for d, l in FORMATS]
CANARY = 0xA5


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
            assert len(rgba) == 9 and all(v.shape == (fh, fw, 4) for v in rgba.values())
            if fh & 1:
                assert all((v[fh - 1, :, :3] == 255).all() for v in rgba.values())          # the fill row
            made[name] = (data, rgba)
        return made[name]
    return get


_resized = {}


def resized(L, name, key, rgba, box, size, filt):
    """leon_ctypes.resize_rgb of one oracle frame, computed once per (stream, frame, box, size, filter) and left unchanged"""
    k = (name, key, box, size, filt)
    if k not in _resized:
        _resized[k] = L.resize_rgb(rgba[key][..., :3], box, size, filt)
        _resized[k].setflags(write=False)
    return _resized[k]


def want_regions(L, name, rgba, keys, regs, size, filt, dtype, layout, scale=None, bias=None):
    """[N, ...] bit patterns in the layout's order: T[c][resize_rgb(the region's frame, its box)]"""
    T = bits(L.tensor_table(dtype, scale, bias))
    out = []
    for r in regs:
        rgb = resized(L, name, keys[r[0]], rgba, tuple(r[1:]), size, filt)
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        out.append(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def assert_regions(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, want %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d elements differ in regions %s, first at %s: got %#x, want %#x" % (
            what, len(bad), got.size, sorted({int(b[0]) for b in bad})[:10], bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])])))


def run(L, data, dtype, layout, on_frames, keep=False, output="tensor", **kw):
    """one window of the stream's two GOPs; on_frames(pipe, window, keys, frames) runs inside the callback.  Returns the pipeline, waited
    for; the caller closes it"""
    kw.setdefault("gops_per_window", 2)
    kw.setdefault("gpu_parser", True)
    seen = []

    def on_window(window, frames):
        fl = list(frames)
        seen.append(window)
        on_frames(fl[0]["_pipe"], window, [(f["gop"], f["display_index"]) for f in fl], fl)
        return False if keep else None
    pipe = L.Pipeline(data, on_window=on_window, output=output, tensor_dtype=dtype, tensor_layout=layout, parser_threads=2, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        assert len(seen) == 1
    except BaseException:
        pipe.close()
        raise
    return pipe


def check_call(L, streams, name, filt, dtype, layout, **kw):
    call = CALLS[name]
    data, rgba = streams(name)
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        got["keys"], got["regs"] = keys, regs
        got["out"] = bits(p.read_regions(window, regs, call.size, filt))
    run(L, data, dtype, layout, on_frames, **kw).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], call.size, filt, dtype, layout, kw.get("tensor_scale"), kw.get("tensor_bias"))
    assert_regions(got["out"], want, "%s %s %s %s" % (name, FILTER_NAMES[filt], dtype, layout))
    return got["out"]


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join([r[0], FILTER_NAMES[r[1]], r[2], r[3]]))
def test_call(L, streams, run_):
    name, filt, dtype, layout = run_
    check_call(L, streams, name, filt, dtype, layout)


def test_bfloat16(L, streams):
    check_call(L, streams, "608x57", TRIANGLE, "bfloat16", "chw")


def test_imagenet_scale_and_bias(L, streams):
    """the pipeline's element table is the regions' too"""
    check_call(L, streams, "100x57", BICUBIC, "float32", "chw", tensor_scale=IMAGENET_SCALE, tensor_bias=IMAGENET_BIAS)


def test_host_parser(L, streams):
    a = check_call(L, streams, "96x64", TRIANGLE, "float16", "chw", gpu_parser=False)
    b = check_call(L, streams, "96x64", TRIANGLE, "float16", "chw", gpu_parser=True)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype,layout", [("uint8", "chw"), ("uint8", "hwc"), ("float16", "chw")])
def test_callers_buffer_pitch_and_canary(L, streams, dtype, layout):
    """resample_regions into a caller's buffer filled with a canary, regions default pitch + 256 apart: each region's bytes are the expected
    ones, every byte between region_bytes and the pitch and behind the last region is the canary's"""
    import torch
    name, filt = "608x57", BICUBIC
    call = CALLS[name]
    data, rgba = streams(name)
    e = 1 if dtype == "uint8" else 2
    nbytes, dflt = S.placement(call.size, e)
    assert nbytes < dflt          # a gap even at the default pitch
    pitch = dflt + 256
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        n = len(regs)
        assert p.region_bytes(call.size) == (nbytes, dflt)
        buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
        view = p.resample_regions(window, regs, call.size, filt, out=buf, pitch=pitch)
        shape = (n,) + ((call.size[0], call.size[1], 3) if layout == "hwc" else (3, call.size[0], call.size[1]))
        assert tuple(view.shape) == shape and view.dtype == getattr(torch, dtype) and view.data_ptr() == buf.data_ptr() and view.stride(0) * e == pitch
        got.update(keys=keys, regs=regs, view=bits(view.cpu().numpy()), raw=buf.cpu().numpy())
        # the default pitch, into a buffer the method allocates
        got["own"] = bits(p.resample_regions(window, regs, call.size, filt).cpu().numpy())
    run(L, data, dtype, layout, on_frames).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], call.size, filt, dtype, layout)
    assert_regions(got["view"], want, "the view over the caller's buffer")
    assert_regions(got["own"], want, "the view over the method's buffer")
    raw, n = got["raw"], len(got["regs"])
    for i in range(n):
        assert raw[i * pitch:i * pitch + nbytes].tobytes() == want[i].tobytes(), "region %d" % i
        assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
    assert (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_region_equals_the_pipelines_own_crop_and_size(L, streams, dtype, layout):
    """a region equal to the pipeline's tensor_crop / tensor_size is the pipeline's delivered tensor, bit for bit; the window's own tensors
    are what they were after the calls"""
    name = "100x57"
    call = CALLS[name]
    data, rgba = streams(name)
    box = call.boxes[2]
    for filt in FILTERS:
        got = {}

        def on_frames(p, window, keys, frames):
            got["before"] = [bits(p.read_tensor(f)) for f in frames]
            got["regions"] = bits(p.read_regions(window, [(f["_i"],) + box for f in frames], call.size, filt))
            p.read_regions(window, call.regions(len(frames)), call.size, filt)
            got["after"] = [bits(p.read_tensor(f)) for f in frames]
            got["keys"] = keys
        run(L, data, dtype, layout, on_frames, tensor_crop=box, tensor_size=call.size, tensor_filter=filt).close()
        want = want_regions(L, name, rgba, got["keys"], [(i,) + box for i in range(9)], call.size, filt, dtype, layout)
        for i in range(9):
            assert np.array_equal(got["regions"][i], got["before"][i]), "frame %d %s" % (i, FILTER_NAMES[filt])
            assert np.array_equal(got["after"][i], want[i]) and np.array_equal(got["before"][i], want[i])


def test_held_window_from_the_main_thread(L, streams):
    """the callback returns False: the call is made after it has returned, from another thread; a second call gives the same bytes; after
    release_window the call is refused"""
    name, filt = "96x64", BICUBIC
    call = CALLS[name]
    data, rgba = streams(name)
    held = {}

    def on_frames(p, window, keys, frames):
        held.update(window=window, keys=keys, thread=threading.get_ident())
    pipe = run(L, data, "uint8", "hwc", on_frames, keep=True)
    try:
        assert held["thread"] != threading.get_ident()
        regs = call.regions(len(held["keys"]))
        a = bits(pipe.read_regions(held["window"], regs, call.size, filt))
        b = bits(pipe.read_regions(held["window"], regs, call.size, filt))
        assert_regions(a, want_regions(L, name, rgba, held["keys"], regs, call.size, filt, "uint8", "hwc"), "held window")
        assert np.array_equal(a, b)
        pipe.release_window(held["window"])
        with pytest.raises(L.LeonError, match="not out for delivery"):
            pipe.read_regions(held["window"], regs, call.size, filt)
    finally:
        pipe.close()


def test_the_pipelines_letterbox_plays_no_part(L, streams):
    name, filt = "96x64", TRIANGLE
    plain = check_call(L, streams, name, filt, "float16", "hwc")
    boxed = check_call(L, streams, name, filt, "float16", "hwc", tensor_letterbox=(40, 40), tensor_pad_value=(114, 7, 250))
    sized = check_call(L, streams, name, filt, "float16", "hwc", tensor_size=(7, 9), tensor_crop=(3, 3, 50, 40), tensor_filter=BICUBIC)
    assert np.array_equal(plain, boxed) and np.array_equal(plain, sized)


def test_refusals_leave_the_buffer_alone(L, streams):
    import torch
    name = "608x57"
    call = CALLS[name]
    data, _ = streams(name)
    nbytes, dflt = S.placement(call.size, 2)
    seen = []

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        buf = torch.full((len(regs) * (dflt + 256) + 512,), CANARY, dtype=torch.uint8, device="cuda")

        def refused(word, window=window, regs=regs, out=buf, pitch=None, size=call.size, filt=TRIANGLE):
            with pytest.raises(L.LeonError) as e:
                p.resample_regions(window, regs, size, filt, out=out, pitch=pitch)
            assert e.value.code == L.ERR_INVALID and word in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        refused("not out for delivery", window=window + 1000)
        refused("not out for delivery", window=-1)
        refused("region 3: frame 9", regs=regs[:3] + [(len(frames),) + call.boxes[0]] + regs[3:])
        refused("not 256-byte aligned", out=buf[16:])
        refused("out_pitch_bytes", pitch=dflt + 128)
        refused("out_pitch_bytes", pitch=dflt - 256)
        refused("region 4: resize: width 600 -> 37 reduces by more than 16", regs=regs[:4] + [(2,) + call.refused] + regs[4:])
        refused("filter 2", filt=2)
        rc = p.lib.leon_pipeline_resample_regions(p.h, window, L._regions_args(regs, call.size, 0)[0], len(regs), C.byref(L.PipelineRegionsConfig(37, 13, 0)), None, 0)
        assert rc == L.ERR_INVALID and b"null device_out" in p.lib.leon_last_error()
        # and the call still works afterwards
        p.resample_regions(window, regs, call.size, TRIANGLE, out=buf, pitch=dflt + 256)
        torch.cuda.synchronize()
        assert not bool((buf[:nbytes] == CANARY).all())
    run(L, data, "float16", "chw", on_frames).close()
    assert len(seen) == 8

    # a pipeline without the TENSOR bit
    def on_rgba(p, window, keys, frames):
        buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        arr, n, cfg = L._regions_args([(0, 0, 0, 8, 8)], (8, 8), 0)
        assert p.lib.leon_pipeline_resample_regions(p.h, window, arr, n, C.byref(cfg), buf.data_ptr(), 0) == L.ERR_INVALID
        assert b"LEON_PIPELINE_OUTPUT_TENSOR" in p.lib.leon_last_error()
        host = np.full(192, CANARY, dtype=np.uint8)
        assert p.lib.leon_pipeline_read_regions(p.h, window, arr, n, C.byref(cfg), host.ctypes.data) == L.ERR_INVALID
        with pytest.raises(L.LeonError):
            p.read_regions(window, [(0, 0, 0, 8, 8)], (8, 8))
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all()) and (host == CANARY).all()
        seen.append("rgba")
    run(L, data, "float16", "chw", on_rgba, output="rgba").close()
    assert seen[-1] == "rgba"
