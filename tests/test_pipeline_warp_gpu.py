"""GPU: rotated boxes and affine crops of delivered frames (include/leon_pipeline.h, leon_pipeline_warp_regions) -- k_warp<element
bytes, layout>, one launch per call.  Expected values never come from the code under test: the ORACLE's RGBA of the region's frame
through leon_ctypes.warp_rgb (the numpy statement of the definition; tests/test_pipeline_warp_abi.py holds its anchors) and the element
table T, compared as bit patterns, no tolerance.  The calls are tests/warp_structure.py's (tests/test_warp_structure.py proves on the
CPU what each holds): per stream and out size every listed matrix -- S = 1, 2 and 4 side by side in one launch -- dealt over every
frame of a window of two GOPs, out of the frames' order, several regions on one frame."""
import ctypes as C

import numpy as np
import pytest

import warp_structure as W
from resample_structure import STREAMS
from test_pipeline_gpu import ibbp_stream, oracle_frames
from test_pipeline_regions_gpu import CANARY, FORMATS, IMAGENET_BIAS, IMAGENET_SCALE, assert_regions, run
from test_pipeline_tensor_format_gpu import bits

pytestmark = pytest.mark.gpu


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


RUNS = [(name, d, l) for name in sorted(W.SIZES) for d, l in FORMATS]
_warped = {}


def warped(L, name, key, rgba, m, size):
    """leon_ctypes.warp_rgb of one oracle frame, computed once per (stream, frame, matrix, size) and left unchanged"""
    k = (name, key, tuple(m), size)
    if k not in _warped:
        _warped[k] = L.warp_rgb(rgba[key][..., :3], m, size, W.PAD)
        _warped[k].setflags(write=False)
    return _warped[k]


def want_regions(L, name, rgba, keys, regs, size, dtype, layout, scale=None, bias=None):
    """[N, ...] bit patterns in the layout's order: T[c][warp_rgb(the region's frame, its matrix)]"""
    T = bits(L.tensor_table(dtype, scale, bias))
    out = []
    for frame, m in regs:
        rgb = warped(L, name, keys[frame], rgba, m, size)
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        out.append(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def assert_named_regions(got, want, names, layout, what):
    """assert_regions, and on a mismatch the name of the first differing region's record and the output pixel: a failure points at a
    family of tests/warp_structure.py, not at an index"""
    if got.shape == want.shape and not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i, a, b, c = (int(v) for v in bad[0])
        (oy, ox, ch) = (a, b, c) if layout == "hwc" else (b, c, a)
        differing = sorted({int(v) for v in bad[:, 0]})
        what = "%s: first in record %r at output pixel (x %d, y %d) channel %d; differing records %s" % (what, names[i], ox, oy, ch, [names[k] for k in differing[:10]])
    assert_regions(got, want, what)


def check_stream(L, streams, name, dtype, layout, sizes=None, regions=None, **kw):
    """regions: (named records, regions) as W.matrices and W.regions are, the default"""
    data, rgba = streams(name)
    sizes = sizes or W.SIZES[name]
    named, regions = regions or (W.matrices, W.regions)
    got = {}

    def on_frames(p, window, keys, frames):
        got["keys"] = keys
        for size in sizes:
            got[size] = bits(p.read_warp_regions(window, regions(W.frame_wh(name), size, len(frames)), size, W.PAD))
    run(L, data, dtype, layout, on_frames, **kw).close()
    for size in sizes:
        regs = regions(W.frame_wh(name), size, 9)
        want = want_regions(L, name, rgba, got["keys"], regs, size, dtype, layout, kw.get("tensor_scale"), kw.get("tensor_bias"))
        assert_named_regions(got[size], want, [n for n, _ in named(W.frame_wh(name), size)], layout, "%s %s %s %s" % (name, size, dtype, layout))
    return [got[size] for size in sizes]


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join(r))
def test_stream(L, streams, run_):
    name, dtype, layout = run_
    check_stream(L, streams, name, dtype, layout)


def test_bfloat16(L, streams):
    check_stream(L, streams, "608x57", "bfloat16", "chw")


def test_imagenet_scale_and_bias(L, streams):
    """the pipeline's element table is the warp calls' too"""
    check_stream(L, streams, "100x57", "float32", "chw", sizes=[(13, 37)], tensor_scale=IMAGENET_SCALE, tensor_bias=IMAGENET_BIAS)


def test_host_parser(L, streams):
    a = check_stream(L, streams, "96x64", "float16", "chw", gpu_parser=False)
    b = check_stream(L, streams, "96x64", "float16", "chw", gpu_parser=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype,layout", [("uint8", "chw"), ("uint8", "hwc"), ("float16", "chw")])
def test_callers_buffer_pitch_and_canary(L, streams, dtype, layout):
    """warp_regions into a caller's buffer filled with a canary, regions default pitch + 256 apart: each region's bytes are the expected
    ones, every byte between region_bytes and the pitch and behind the last region is the canary's"""
    import torch
    name, size = "608x57", (13, 37)
    data, rgba = streams(name)
    e = 1 if dtype == "uint8" else 2
    nbytes = 3 * size[0] * size[1] * e
    dflt = (nbytes + 255) // 256 * 256
    assert nbytes < dflt
    pitch = dflt + 256
    got = {}

    def on_frames(p, window, keys, frames):
        regs = W.regions(W.frame_wh(name), size, len(frames))
        n = len(regs)
        buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
        view = p.warp_regions(window, regs, size, W.PAD, out=buf, pitch=pitch)
        shape = (n,) + ((size[0], size[1], 3) if layout == "hwc" else (3, size[0], size[1]))
        assert tuple(view.shape) == shape and view.dtype == getattr(torch, dtype) and view.data_ptr() == buf.data_ptr() and view.stride(0) * e == pitch
        got.update(keys=keys, regs=regs, view=bits(view.cpu().numpy()), raw=buf.cpu().numpy())
        got["own"] = bits(p.warp_regions(window, regs, size, W.PAD).cpu().numpy())          # the default pitch, the method's own buffer
    run(L, data, dtype, layout, on_frames).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], size, dtype, layout)
    assert_regions(got["view"], want, "the view over the caller's buffer")
    assert_regions(got["own"], want, "the view over the method's buffer")
    raw, n = got["raw"], len(got["regs"])
    for i in range(n):
        assert raw[i * pitch:i * pitch + nbytes].tobytes() == want[i].tobytes(), "region %d" % i
        assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
    assert (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_the_identity_is_read_regions_of_the_same_box(L, streams, dtype, layout):
    """where the two families meet: the identity map at an integer offset and read_regions of that box at its own size"""
    name, size, (x, y) = "100x57", (13, 37), (40, 30)
    data, _ = streams(name)
    got = {}

    def on_frames(p, window, keys, frames):
        got["warp"] = bits(p.read_warp_regions(window, [(f["_i"], L.warp_matrix([1, 0, x, 0, 1, y])) for f in frames], size))
        got["crop"] = bits(p.read_regions(window, [(f["_i"], x, y, size[1], size[0]) for f in frames], size))
    run(L, data, dtype, layout, on_frames).close()
    assert_regions(got["warp"], got["crop"], "identity against read_regions")


def test_refusals_leave_the_buffer_alone(L, streams):
    import torch
    name, size = "96x64", (8, 32)
    data, _ = streams(name)
    seen = []

    def on_frames(p, window, keys, frames):
        regs = W.regions(W.frame_wh(name), size, len(frames))
        nbytes, dflt = p.region_bytes(size)
        buf = torch.full((len(regs) * (dflt + 256) + 512,), CANARY, dtype=torch.uint8, device="cuda")

        def refused(word, window=window, regs=regs, out=buf, pitch=None, size=size, pad=None):
            with pytest.raises(L.LeonError) as e:
                p.warp_regions(window, regs, size, pad, out=out, pitch=pitch)
            assert e.value.code == L.ERR_INVALID and word in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        for _, (frame, m, reserved), _, text in W.refused_records(len(frames)):
            rec = L.PipelineWarpRegion(frame, (C.c_int32 * 6)(*m), reserved)
            refused("region 3: ", regs=regs[:3] + [rec] + regs[3:])
            refused(text, regs=regs[:3] + [rec] + regs[3:])
        refused("not out for delivery", window=window + 1000)
        refused("not 256-byte aligned", out=buf[16:])
        refused("out_pitch_bytes", pitch=dflt + 128)
        refused("pad value 2", pad=(0, 0, 300))
        refused("out_width 0", size=(8, 0))
        arr, n, cfg = L._warp_args(regs, size, None)
        assert p.lib.leon_pipeline_warp_regions(p.h, window, arr, n, C.byref(cfg), None, 0) == L.ERR_INVALID and b"null device_out" in p.lib.leon_last_error()
        # and the call still works afterwards
        p.warp_regions(window, regs, size, W.PAD, out=buf, pitch=dflt + 256)
        torch.cuda.synchronize()
        assert not bool((buf[:nbytes] == CANARY).all())
    run(L, data, "float16", "chw", on_frames).close()
    assert len(seen) == 13

    def on_rgba(p, window, keys, frames):          # a pipeline without the TENSOR bit
        arr, n, cfg = L._warp_args([(0, (65536, 0, 0, 0, 65536, 0))], (8, 8), None)
        host = np.full(192, CANARY, dtype=np.uint8)
        assert p.lib.leon_pipeline_read_warp_regions(p.h, window, arr, n, C.byref(cfg), host.ctypes.data) == L.ERR_INVALID
        assert b"LEON_PIPELINE_OUTPUT_TENSOR" in p.lib.leon_last_error() and (host == CANARY).all()
        seen.append("rgba")
    run(L, data, "float16", "chw", on_rgba, output="rgba").close()
    assert seen[-1] == "rgba"
