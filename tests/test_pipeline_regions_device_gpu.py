"""GPU: regions whose boxes lie in device memory (include/leon_pipeline.h, leon_pipeline_resample_regions_device) -- k_box_tables builds
each region's descriptor and tables on the device, k_boxes<element bytes, layout, filter> is k_regions behind the status word.  The
expected values are the HOST path's of the same build (leon_pipeline_read_regions, leon_pipeline_resize_weights), which
tests/test_pipeline_regions_gpu.py and the resize tests pin to the oracle and to Pillow: bytes and table words are compared for
equality, no tolerance.  The calls are tests/regions_structure.py's, dealt over a window of two GOPs (3 and 6 pictures)."""
import ctypes as C

import numpy as np
import pytest

import regions_structure as S
from regions_structure import BICUBIC, CALLS, FILTERS, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_gpu import ibbp_stream
from test_pipeline_regions_gpu import CANARY, run

pytestmark = pytest.mark.gpu

FORMATS = [("uint8", "hwc"), ("float16", "chw"), ("float32", "chw"), ("bfloat16", "hwc")]
RUNS = [(c, f, d, l) for c in sorted(CALLS) for f in FILTERS for d, l in FORMATS]
MAX_TAPS = {TRIANGLE: 33, BICUBIC: 65}
FILL = -77


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def streams():
    """name -> stream bytes, written once per module"""
    made = {}

    def get(name):
        if name not in made:
            cw, ch, gops, seed, (fw, fh) = STREAMS[name]
            made[name] = ibbp_stream(cw, ch, gops, seed=seed, frame=(fw, fh))
        return made[name]
    return get


def ubits(a):
    """a host array, or a torch tensor on the device, as unsigned bit patterns on the host"""
    if not isinstance(a, np.ndarray):
        import torch
        if a.dtype == torch.bfloat16:
            a = a.view(torch.int16)
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def slot_bytes(size, filt):
    """what one region takes of the scratch (include/leon_pipeline.h): its table slot and its descriptor"""
    oh, ow = size
    return 4 * (2 * ow + ow * MAX_TAPS[filt] + 2 * oh + oh * MAX_TAPS[filt]) + 64


# ---- the tables: the device's rows equal the host's, word for word ------------------------------------------------------------

def host_rows(L, axis, filt):
    """(first, count, weights[out, max taps]) of leon_pipeline_resize_weights, or None where it refuses"""
    in_size, start, size, out = (int(v) for v in axis)
    t = MAX_TAPS[filt]
    first, count, weights = np.zeros(out, np.int32), np.zeros(out, np.int32), np.zeros((out, t), np.int32)
    rc = L.load().leon_pipeline_resize_weights(in_size, start, size, out, filt, first.ctypes.data, count.ctypes.data, weights.ctypes.data, t)
    return (first, count, weights) if rc == L.OK else None


def compare_axes(L, axes, filt):
    """every axis of the batch: refused by both, or equal in first, count and every weight (and untouched behind its out size).
    Returns the indices the host refuses."""
    axes = np.asarray(axes, dtype=np.int32)
    first, count, weights, status = L.resize_weights_device(axes, filt, fill=FILL)
    refused = []
    for i, axis in enumerate(axes):
        want = host_rows(L, axis, filt)
        out = int(axis[3])
        if want is None:
            assert status[i] != 0, (axis, "the host refuses, the device does not")
            assert (first[i] == FILL).all() and (count[i] == FILL).all() and (weights[i] == FILL).all(), axis
            refused.append(i)
            continue
        assert status[i] == 0, (axis, int(status[i]))
        assert np.array_equal(first[i, :out], want[0]) and np.array_equal(count[i, :out], want[1]), (axis, FILTER_NAMES[filt])
        if not np.array_equal(weights[i, :out], want[2]):
            bad = np.argwhere(weights[i, :out] != want[2])[0]
            raise AssertionError("axis %s %s: weight [%d][%d] is %d on the device, %d on the host" % (
                axis.tolist(), FILTER_NAMES[filt], bad[0], bad[1], weights[i, bad[0], bad[1]], want[2][bad[0], bad[1]]))
        assert (first[i, out:] == FILL).all() and (count[i, out:] == FILL).all() and (weights[i, out:] == FILL).all(), axis
    return refused, status


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: FILTER_NAMES[f])
@pytest.mark.parametrize("out", [1, 2, 3, 7, 8, 37])
def test_tables_exhaustively_on_an_axis_of_64(L, filt, out):
    axes = [(64, start, size, out) for size in range(1, 65) for start in range(0, 65 - size)]
    assert len(axes) == 64 * 65 // 2
    refused, status = compare_axes(L, axes, filt)
    # nothing is dropped silently: what is not compared is exactly the ratio above 16, judged here
    assert refused == [i for i, a in enumerate(axes) if a[2] > 16 * out]
    assert all(status[i] == L.REGION_RATIO_X for i in refused)
    assert (len(refused) > 0) == (out < 4)


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: FILTER_NAMES[f])
def test_tables_of_the_usual_axes_and_seeded_boxes(L, filt):
    refused, _ = compare_axes(L, [(1920, 0, 1920, 224), (1080, 0, 1080, 224), (4096, 0, 4096, 256), (1, 0, 1, 4096)], filt)
    assert refused == []
    rng = np.random.default_rng(1920)
    size = rng.integers(1, 1921, 300)
    start = (rng.random(300) * (1920 - size + 1)).astype(np.int64)
    out = rng.choice([224, 100, 37], 300)
    axes = np.stack([np.full(300, 1920), start, size, out], axis=1)
    refused, status = compare_axes(L, axes, filt)
    assert refused == [i for i in range(300) if size[i] > 16 * out[i]] and 0 < len(refused) < 150
    # a box that leaves the axis, an empty one, a row longer than max_taps
    _, _, _, status = L.resize_weights_device([(64, 60, 5, 8), (64, 0, 0, 8), (64, -1, 8, 8), (64, 0, 64, 8), (64, 0, 64, 8)], filt, max_taps=MAX_TAPS[filt])
    assert status.tolist() == [L.REGION_BOX, L.REGION_BOX, L.REGION_BOX, 0, 0]
    _, _, weights, status = L.resize_weights_device([(64, 0, 64, 8)], filt, max_taps=3, fill=FILL)
    assert status.tolist() == [L.REGION_TAPS] and (weights == FILL).all()


# ---- the tensors: the device path equals the host path, byte for byte ---------------------------------------------------------

def side_stream():
    import torch
    return torch.cuda.Stream()


def check_call(L, streams, name, filt, dtype, layout, on_side_stream=True, **kw):
    import torch
    call = CALLS[name]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        got["want"] = ubits(p.read_regions(window, regs, call.size, filt))
        st = side_stream() if on_side_stream else torch.cuda.current_stream()
        with torch.cuda.stream(st):
            boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
            view, status = p.resample_regions_device(window, boxes, call.size, filt)
        st.synchronize()
        got["out"], got["status"] = ubits(view), status.cpu().numpy()
    run(L, streams(name), dtype, layout, on_frames, **kw).close()
    what = "%s %s %s %s" % (name, FILTER_NAMES[filt], dtype, layout)
    assert got["out"].shape == got["want"].shape and got["out"].dtype == got["want"].dtype, what
    assert (got["status"] == 0).all(), (what, got["status"])
    if not np.array_equal(got["out"], got["want"]):
        bad = np.argwhere(got["out"] != got["want"])
        raise AssertionError("%s: %d of %d elements differ from the host path in regions %s, first at %s" % (
            what, len(bad), got["out"].size, sorted({int(b[0]) for b in bad})[:10], bad[0].tolist()))


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join([r[0], FILTER_NAMES[r[1]], r[2], r[3]]))
def test_call(L, streams, run_):
    name, filt, dtype, layout = run_
    check_call(L, streams, name, filt, dtype, layout)


def test_host_parser_and_the_default_stream(L, streams):
    """torch's legacy default stream has no handle to queue on: the binding falls back to the pipeline's stream and the call waits"""
    check_call(L, streams, "96x64", TRIANGLE, "float16", "chw", on_side_stream=False, gpu_parser=False)


def records(regs):
    """[N, 8] int32 leon_pipeline_region records of [(frame, x, y, w, h)]"""
    full = np.zeros((len(regs), 8), dtype=np.int32)
    full[:, :5] = regs
    return full


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refused_regions_among_good_ones(L, streams, name):
    """non-zero status exactly at the refused positions and equal to region_status; their bytes, the gaps up to an explicit pitch and
    everything behind the last region still the canary's; the good regions equal the host path"""
    import torch
    call, filt, dtype, layout, e = CALLS[name], BICUBIC, "float16", "chw", 2
    fw, fh = call.frame
    nbytes, dflt = S.placement(call.size, e)
    pitch = dflt + 256
    got = {}

    def on_frames(p, window, keys, frames):
        good = call.regions(len(frames))
        # the call's refused box (a ratio above 16) where its frame has room for one, else a box that leaves the frame below
        bad = [(2,) + tuple(call.refused if call.refused else (0, fh - 7, 8, 8)), (len(frames), 0, 0, 8, 8), (0, 0, 0, 8, 8), (1, 4, 4, 0, 8), (-1, 0, 0, 8, 8), (3, fw - 7, 0, 8, 8)]
        rec, at = [], []
        for i, g in enumerate(good):
            rec.append(g)
            if i < len(bad):
                at.append(len(rec))
                rec.append(bad[i])
        full = records(rec)
        full[at[2], 6] = 5          # a reserved word
        n = len(rec)
        want_status = [L.region_status(fw, fh, len(frames), L.PipelineRegion(*[int(v) for v in r[:5]], (C.c_int32 * 3)(*[int(v) for v in r[5:]])),
                                       call.size, filt) for r in full]
        assert [i for i in range(n) if want_status[i]] == at and len(set(want_status)) == (5 if call.refused else 4)
        got["want"] = ubits(p.read_regions(window, good, call.size, filt))
        st = side_stream()
        with torch.cuda.stream(st):
            buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
            status = torch.full((n + 4,), -9, dtype=torch.int32, device="cuda")
            view, ret = p.resample_regions_device(window, torch.from_numpy(full).cuda(), call.size, filt, out=buf, pitch=pitch, status=status)
        st.synchronize()
        assert view.data_ptr() == buf.data_ptr() and view.stride(0) * e == pitch and ret.data_ptr() == status.data_ptr()
        got.update(n=n, at=at, raw=buf.cpu().numpy(), status=status.cpu().numpy(), want_status=want_status)
    run(L, streams(name), dtype, layout, on_frames).close()
    n, at, raw = got["n"], got["at"], got["raw"]
    assert got["status"][:n].tolist() == got["want_status"] and (got["status"][n:] == -9).all()
    k = 0
    for i in range(n):
        if i in at:
            assert (raw[i * pitch:(i + 1) * pitch] == CANARY).all(), "the refused region %d was written" % i
        else:
            assert raw[i * pitch:i * pitch + nbytes].tobytes() == got["want"][k].tobytes(), "region %d" % i
            assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
            k += 1
    assert k == len(got["want"]) and (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: FILTER_NAMES[f])
def test_chunks_of_one_and_of_three_regions(L, streams, filt):
    import torch
    name = "100x57"
    call = CALLS[name]
    per = slot_bytes(call.size, filt)
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        assert len(regs) == 10
        st = side_stream()
        with torch.cuda.stream(st):
            boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
            outs = [p.resample_regions_device(window, boxes, call.size, filt, scratch_limit=limit) for limit in (None, per, 2 * per - 1, 3 * per, 4 * per - 1)]
        st.synchronize()
        got["outs"] = [(ubits(v), s.cpu().numpy()) for v, s in outs]
        got["want"] = ubits(p.read_regions(window, regs, call.size, filt))
        with pytest.raises(L.LeonError, match="scratch_limit_bytes") as e:
            p.resample_regions_device(window, boxes, call.size, filt, scratch_limit=per - 1)
        assert e.value.code == L.ERR_INVALID
    run(L, streams(name), "uint8", "chw", on_frames).close()
    for out, status in got["outs"]:
        assert np.array_equal(out, got["want"]) and (status == 0).all()


def test_ordering_without_host_waits(L, streams):
    """boxes made by torch ops on a side stream, the call behind them and a torch reduction of its output behind the call, all enqueued
    before the host waits once; then two calls back to back into different buffers, on one stream and on two (the scratch's event)"""
    import torch
    name, filt = "96x64", TRIANGLE
    call = CALLS[name]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        other = [(f,) + tuple(b) for (f, *_), b in zip(regs, reversed(call.boxes + call.boxes[:2]))]
        assert other != regs and len(other) == len(regs)
        got["want"] = [ubits(p.read_regions(window, r, call.size, filt)) for r in (regs, other)]
        jitter = torch.tensor([0.0, 0.25, -0.25, 0.125, -0.375], dtype=torch.float32)
        s1, s2 = side_stream(), side_stream()

        def enqueue(st, r):
            with torch.cuda.stream(st):
                fb = (torch.tensor(r, dtype=torch.float32) + jitter).to("cuda", non_blocking=True)
                boxes = fb.round().to(torch.int32)
                view, status = p.resample_regions_device(window, boxes, call.size, filt)
                return view, status, view.to(torch.int64).sum(dim=(1, 2, 3))
        a = enqueue(s1, regs)          # one stream, back to back, no host wait in between
        b = enqueue(s1, other)
        c = enqueue(s1, regs)          # two streams: the second call's stream waits for the first call's event
        d = enqueue(s2, other)
        s1.synchronize()
        s2.synchronize()
        got["runs"] = [(ubits(v), st.cpu().numpy(), red.cpu().numpy()) for v, st, red in (a, b, c, d)]
    run(L, streams(name), "uint8", "hwc", on_frames).close()
    for i, (out, status, red) in enumerate(got["runs"]):
        want = got["want"][i % 2]
        assert (status == 0).all() and np.array_equal(out, want), "call %d" % i
        assert np.array_equal(red, want.reshape(len(want), -1).astype(np.int64).sum(axis=1)), "the reduction behind call %d" % i


def test_host_refusals_leave_the_buffer_alone(L, streams):
    import torch
    name = "608x57"
    call = CALLS[name]
    nbytes, dflt = S.placement(call.size, 2)
    seen, held = [], {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        n = len(regs)
        boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
        recs = torch.from_numpy(records(regs)).cuda()
        buf = torch.full((n * (dflt + 256) + 512,), CANARY, dtype=torch.uint8, device="cuda")
        status = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        st = side_stream()
        torch.cuda.synchronize()
        held.update(window=window, regs=regs)

        def untouched(word):
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()) and bool((status == -9).all()), "a refused call wrote (%s)" % word
            seen.append(word)

        def refused(word, window=window, boxes=boxes, out=buf, pitch=None, size=call.size, filt=TRIANGLE, limit=None):
            with pytest.raises(L.LeonError) as e:
                p.resample_regions_device(window, boxes, size, filt, out=out, pitch=pitch, status=status, stream=st, scratch_limit=limit)
            assert e.value.code == L.ERR_INVALID and word in str(e.value), str(e.value)
            untouched(word)

        def raw(word, cfg=None, **fields):
            d = dict(regions=recs.data_ptr(), n=n, device_out=buf.data_ptr(), device_status=status.data_ptr(), stream=st.cuda_stream)
            d.update(fields)
            dev = L.PipelineRegionsDevice(d["regions"], d["n"], d.get("reserved0", 0), d["device_out"], 0, d["device_status"], d["stream"], 0)
            dev.reserved[0] = d.get("reserved", 0)
            cfg = cfg or L.PipelineRegionsConfig(call.size[1], call.size[0], TRIANGLE)
            assert p.lib.leon_pipeline_resample_regions_device(p.h, window, C.byref(cfg), C.byref(dev)) == L.ERR_INVALID
            assert word.encode() in p.lib.leon_last_error(), p.lib.leon_last_error()
            untouched(word)
        refused("not out for delivery", window=window + 1000)
        refused("not 256-byte aligned", out=buf[16:])
        refused("out_pitch_bytes", pitch=dflt + 128)
        refused("out_pitch_bytes", pitch=dflt - 256)
        refused("filter 2", filt=2)
        refused("scratch_limit_bytes", limit=1000)
        refused("1 .. 65535", boxes=boxes[:0])
        many = torch.zeros((65536, 8), dtype=torch.int32, device="cuda")
        room = torch.empty(65536 * dflt, dtype=torch.uint8, device="cuda")          # valid memory of the stated size, whatever the call does
        with pytest.raises(L.LeonError, match="1 .. 65535"):
            p.resample_regions_device(window, many, call.size, TRIANGLE, out=room, stream=st)
        untouched("65536")
        raw("null regions", regions=None)
        raw("null device_out", device_out=None)
        raw("4-byte aligned", regions=recs.data_ptr() + 2)
        raw("reserved word", reserved0=1)
        raw("reserved word", reserved=1 << 40)
        bad = L.PipelineRegionsConfig(call.size[1], call.size[0], TRIANGLE)
        bad.reserved[4] = 1
        raw("reserved word 4", cfg=bad)
        raw("out_width", cfg=L.PipelineRegionsConfig(4097, call.size[0], TRIANGLE))
        assert p.lib.leon_pipeline_resample_regions_device(p.h, window, None, None) == L.ERR_INVALID
        # and the call still works afterwards
        p.resample_regions_device(window, boxes, call.size, TRIANGLE, out=buf, status=status, stream=st)
        st.synchronize()
        assert not bool((buf[:nbytes] == CANARY).all()) and bool((status == 0).all())
        return buf, status, st
    pipe = run(L, streams(name), "float16", "chw", on_frames, keep=True)
    try:
        assert len(seen) == 15
        # a released window
        pipe.release_window(held["window"])
        buf = torch.full((4096 * 10,), CANARY, dtype=torch.uint8, device="cuda")
        with pytest.raises(L.LeonError, match="not out for delivery"):
            pipe.resample_regions_device(held["window"], torch.tensor(held["regs"], dtype=torch.int32, device="cuda"), call.size, out=buf, stream=side_stream())
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all())
    finally:
        pipe.close()

    # a pipeline without the TENSOR bit
    def on_rgba(p, window, keys, frames):
        buf = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
        recs = torch.from_numpy(records([(0, 0, 0, 8, 8)])).cuda()
        torch.cuda.synchronize()
        dev = L.PipelineRegionsDevice(recs.data_ptr(), 1, 0, buf.data_ptr(), 0, None, None, 0)
        assert p.lib.leon_pipeline_resample_regions_device(p.h, window, C.byref(L.PipelineRegionsConfig(8, 8, 0)), C.byref(dev)) == L.ERR_INVALID
        assert b"LEON_PIPELINE_OUTPUT_TENSOR" in p.lib.leon_last_error()
        with pytest.raises(L.LeonError):
            p.resample_regions_device(window, recs, (8, 8))
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all())
        seen.append("rgba")
    run(L, streams(name), "float16", "chw", on_rgba, output="rgba").close()
    assert seen[-1] == "rgba"
