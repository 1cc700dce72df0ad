"""GPU: regions letterboxed into the batch's tensor size on the host path (include/leon_pipeline.h, leon_pipeline_regions_fit,
leon_pipeline_resample_regions_fit) -- k_fitted<element bytes, layout, filter>, one launch per call, every region with an image
rectangle of its own.  Expected values never come from the code under test: the ORACLE's RGBA of the region's frame through
leon_ctypes.canvas_rgb(rgb, box, (oh_i, ow_i), (ch, cw), (X_i, Y_i), pad, filter) and the element table T, compared as bit patterns, no
tolerance; the rectangle is tests/fitted_structure.py's pure-Python restatement of the letterbox integers.  The calls are
fitted_structure.CALLS (tests/test_fitted_structure.py proves on the CPU what each box is there for), their boxes dealt over every
frame of a window of two GOPs (3 and 6 pictures) as regions_structure.Call.regions deals them."""
import ctypes as C

import numpy as np
import pytest

import fitted_structure as F
import regions_structure as S
from fitted_structure import CALLS, CENTRE, TOP_LEFT
from regions_structure import BICUBIC, FILTERS, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_gpu import ibbp_stream, oracle_frames
from test_pipeline_regions_gpu import CANARY, FORMATS, IMAGENET_BIAS, IMAGENET_SCALE, assert_regions, run
from test_pipeline_tensor_format_gpu import bits

pytestmark = pytest.mark.gpu

RUNS = [(c, f, d, l) for c in sorted(CALLS) for f in FILTERS for d, l in FORMATS]
PAD = (114, 7, 250)          # three different channel values


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
            made[name] = (data, rgba)
        return made[name]
    return get


_canvases = {}


def canvas(L, name, key, rgba, box, size, filt, anchor, pad):
    """leon_ctypes.canvas_rgb of one oracle frame with the box's rectangle, computed once per argument list and left unchanged"""
    k = (name, key, box, size, filt, anchor, pad)
    if k not in _canvases:
        x, y, ow, oh = F.rect(box, size, anchor)
        _canvases[k] = L.canvas_rgb(rgba[key], box, (oh, ow), size, (x, y), pad, filt)
        _canvases[k].setflags(write=False)
    return _canvases[k]


def want_regions(L, name, rgba, keys, regs, size, filt, dtype, layout, anchor=CENTRE, pad=PAD, scale=None, bias=None):
    """[N, ...] bit patterns in the layout's order: T[c][canvas_rgb(the region's frame, its box, its rectangle)]"""
    T = bits(L.tensor_table(dtype, scale, bias))
    out = []
    for r in regs:
        rgb = canvas(L, name, keys[r[0]], rgba, tuple(r[1:]), tuple(size), filt, anchor, tuple(pad))
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        out.append(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


def check_call(L, streams, name, filt, dtype, layout, anchor=CENTRE, pad=PAD, **kw):
    call = CALLS[name]
    data, rgba = streams(name)
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        got["keys"], got["regs"] = keys, regs
        got["out"] = bits(p.read_regions(window, regs, call.size, filt, fit="letterbox", anchor=anchor, pad_value=pad))
    run(L, data, dtype, layout, on_frames, **kw).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], call.size, filt, dtype, layout, anchor, (0, 0, 0) if pad is None else pad,
                        kw.get("tensor_scale"), kw.get("tensor_bias"))
    assert_regions(got["out"], want, "%s %s %s %s %s" % (name, FILTER_NAMES[filt], dtype, layout, anchor))
    return got["out"]


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join([r[0], FILTER_NAMES[r[1]], r[2], r[3]]))
def test_call(L, streams, run_):
    name, filt, dtype, layout = run_
    check_call(L, streams, name, filt, dtype, layout)


def test_bfloat16(L, streams):
    check_call(L, streams, "608x57", TRIANGLE, "bfloat16", "chw")


def test_imagenet_scale_and_bias(L, streams):
    """the pipeline's element table is the regions' and the pad's too"""
    check_call(L, streams, "100x57", BICUBIC, "float32", "chw", tensor_scale=IMAGENET_SCALE, tensor_bias=IMAGENET_BIAS)


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "chw")])
def test_both_anchors_and_the_default_pad(L, streams, dtype, layout):
    name = "96x64"
    a = check_call(L, streams, name, TRIANGLE, dtype, layout, anchor=CENTRE, pad=None)
    b = check_call(L, streams, name, TRIANGLE, dtype, layout, anchor=TOP_LEFT, pad=None)
    c = check_call(L, streams, name, TRIANGLE, dtype, layout, anchor=TOP_LEFT)
    regs = CALLS[name].regions(9)
    fills = [F.rect(r[1:], CALLS[name].size)[2:] == CALLS[name].size[::-1] for r in regs]
    assert any(fills) and not all(fills)
    for i, fill in enumerate(fills):          # the anchor and the pad move every region but the ones that fill the canvas
        assert np.array_equal(a[i], b[i]) == fill and np.array_equal(b[i], c[i]) == fill, i


@pytest.mark.parametrize("dtype,layout", [("uint8", "chw"), ("uint8", "hwc"), ("float16", "chw"), ("float32", "hwc")])
def test_callers_buffer_pitch_and_canary(L, streams, dtype, layout):
    """into a caller's buffer filled with a canary, regions default pitch + 256 apart: every one of a region's region_bytes is the expected
    one -- pad included -- and every byte between region_bytes and the pitch and behind the last region is the canary's"""
    import torch
    name, filt = "96x64", BICUBIC
    call = CALLS[name]
    data, rgba = streams(name)
    e = {"uint8": 1, "float16": 2, "float32": 4}[dtype]
    nbytes, dflt = S.placement(call.size, e)
    assert nbytes < dflt
    pitch = dflt + 256
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        n = len(regs)
        buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
        view = p.resample_regions(window, regs, call.size, filt, out=buf, pitch=pitch, fit="letterbox", pad_value=PAD)
        assert view.data_ptr() == buf.data_ptr() and view.stride(0) * e == pitch
        got.update(keys=keys, regs=regs, view=bits(view.cpu().numpy()), raw=buf.cpu().numpy())
        got["own"] = bits(p.resample_regions(window, regs, call.size, filt, fit="letterbox", pad_value=PAD).cpu().numpy())
    run(L, data, dtype, layout, on_frames).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], call.size, filt, dtype, layout)
    assert_regions(got["view"], want, "the view over the caller's buffer")
    assert_regions(got["own"], want, "the view over the method's buffer")
    raw, n = got["raw"], len(got["regs"])
    for i in range(n):
        assert raw[i * pitch:i * pitch + nbytes].tobytes() == want[i].tobytes(), "region %d" % i
        assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
    assert (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


def test_a_refused_call_writes_nothing(L, streams):
    import torch
    name = "608x57"
    call = CALLS[name]
    data, _ = streams(name)
    nbytes, dflt = S.placement(call.size, 2)
    seen = []

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        buf = torch.full(((len(regs) + 1) * dflt + 512,), CANARY, dtype=torch.uint8, device="cuda")          # (room for one region more)

        def refused(word, regs=regs, **kw):
            kw.setdefault("fit", "letterbox")
            with pytest.raises(L.LeonError) as e:
                p.resample_regions(window, regs, call.size, TRIANGLE, out=buf, **kw)
            assert e.value.code == L.ERR_INVALID and word in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        for box, boxed, _ in call.refusals:          # the last region of the call: every region before it is valid
            refused("region %d: resize: %s" % (len(regs), "width 600 -> 37" if boxed == "REGION_RATIO_X" else "height 52 -> 3"), regs=regs + [(1,) + box])
        refused("pad value 1 is 256", pad_value=(0, 256, 0))
        refused("anchor 7", anchor=7)
        refused("mode 2", fit=2)
        refused("LEON_REGIONS_FIT_STRETCH", fit="stretch", anchor="top_left")
        # the box letterboxing refuses is fine stretched; and the call still works afterwards
        p.resample_regions(window, regs + [(1,) + call.refusals[1][0]], call.size, TRIANGLE, out=torch.empty_like(buf))
        p.resample_regions(window, regs, call.size, TRIANGLE, out=buf, fit="letterbox")
        torch.cuda.synchronize()
        assert not bool((buf[:nbytes] == CANARY).all())
    run(L, data, "float16", "chw", on_frames).close()
    assert len(seen) == 6


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float32", "chw")])
def test_without_a_fit_the_call_is_the_one_it_was(L, streams, dtype, layout):
    name = "100x57"
    call = S.CALLS[name]
    data, _ = streams(name)
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        arr, n, cfg = L._regions_args(regs, call.size, BICUBIC)
        got["plain"] = bits(p.read_regions(window, regs, call.size, BICUBIC))
        got["none"] = bits(p.read_regions(window, regs, call.size, BICUBIC, fit=None))
        got["stretch"] = bits(p.read_regions(window, regs, call.size, BICUBIC, fit="stretch"))
        for key, fit in (("null", None), ("zero", C.byref(L.PipelineRegionsFit()))):
            out = np.empty_like(got["plain"])
            assert p.lib.leon_pipeline_read_regions_fit(p.h, window, arr, n, C.byref(cfg), fit, out.ctypes.data) == L.OK
            got[key] = out
    run(L, data, dtype, layout, on_frames).close()
    for key in ("none", "stretch", "null", "zero"):
        assert np.array_equal(got[key], got["plain"]), key


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_a_region_equals_the_pipelines_own_letterbox(L, streams, dtype, layout):
    """a pipeline created with tensor_crop = the box and tensor_letterbox = the canvas delivers, for every frame, the region's tensor"""
    name = "100x57"
    call = CALLS[name]
    data, rgba = streams(name)
    box = call.boxes[2]
    for filt in FILTERS:
        got = {}

        def on_frames(p, window, keys, frames):
            got["own"] = [bits(p.read_tensor(f)) for f in frames]
            got["regions"] = bits(p.read_regions(window, [(f["_i"],) + box for f in frames], call.size, filt, fit="letterbox", pad_value=PAD))
            got["keys"] = keys
        run(L, data, dtype, layout, on_frames, tensor_crop=box, tensor_letterbox=call.size, tensor_pad_value=PAD, tensor_filter=filt).close()
        want = want_regions(L, name, rgba, got["keys"], [(i,) + box for i in range(9)], call.size, filt, dtype, layout)
        for i in range(9):
            assert np.array_equal(got["regions"][i], got["own"][i]), "frame %d %s" % (i, FILTER_NAMES[filt])
            assert np.array_equal(got["regions"][i], want[i])
