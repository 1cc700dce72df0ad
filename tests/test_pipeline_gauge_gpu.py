"""GPU: boxes gauged against the motion and activity records of delivered windows (include/leon_pipeline.h,
leon_pipeline_gauge_regions; k_gauge) -- for every frame of a window and each set of sources, statistics and status of the host road,
of the device road on a caller's stream and of the device road on the pipeline's own stream, all three exactly equal to
leon_ctypes.gauge_box (the header's text in Python integers) on the records read_motion and read_activity give; whole-frame boxes
against the delivered records' own summaries; pipelines with one of the two record outputs only; a window held across ring reuse.
Then the chain a user runs: carry_regions_gop's [F, N, 8] records straight into gauge_regions_device on one torch stream with no host
wait between, against the same chain on the host; and every call-level refusal, with nothing written."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import gauge_cases as G
from test_pipeline_carry_gpu import gop_chain_on_the_host
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import stream

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
FILL = -55


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def boxes_of(fw, fh):
    return [(0, 0, fw, fh), (fw // 3, fh // 4, fw // 2, fh // 2), (fw - 1, fh - 1, 1, 1), (5, 7, 12, 10), (15, 15, 2, 2)]


def gauge_window(L, pipe, window, frames, roads=("host", "stream", "null"), sources=G.SOURCES):
    """everything of one delivered window: every frame with five boxes, and three refused records, on each road and for each set of sources"""
    import torch
    n, fw, fh = len(list(frames)), pipe.info.frame_width, pipe.info.frame_height
    motion = [pipe.read_motion(window, i) for i in range(n)] if pipe.motion_layout is not None else None
    activity = [pipe.read_activity(window, i) for i in range(n)] if pipe.activity_layout is not None else None
    regions = [(f, x, y, w, h, 0, 0, 0) for f in range(n) for (x, y, w, h) in boxes_of(fw, fh)]
    regions += [(n, 0, 0, 8, 8, 0, 0, 0), (0, 0, 0, fw + 1, 8, 0, 0, 0), (0, 0, 0, 8, 8, 0, 7, 0)]
    r = dict(n=n, regions=regions, summaries=(None if motion is None else [m[2] for m in motion], None if activity is None else [a[1] for a in activity]), roads={})
    full = np.array(regions, dtype=np.int32)
    for src in sources:
        got = {}
        got["want"] = G.expected(L, fw, fh, None if motion is None else [m[:2] for m in motion], None if activity is None else [a[0] for a in activity], regions, src, FILL, n)
        if "host" in roads:
            got["host"] = pipe.gauge_regions(window, regions, sources=src, fill=FILL)

        def tensors():
            return (torch.tensor(full, dtype=torch.int32, device="cuda"), torch.full((len(regions), 16), FILL, dtype=torch.int64, device="cuda"),
                    torch.full((len(regions),), FILL, dtype=torch.int32, device="cuda"))
        if "stream" in roads:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                rec, stats, status = tensors()
                out = pipe.gauge_regions_device(window, rec, sources=src, stats=stats, status=status)
                assert out[0].data_ptr() == stats.data_ptr() and out[1].data_ptr() == status.data_ptr()
            st.synchronize()
            got["stream"] = (stats.cpu().numpy(), status.cpu().numpy())
        if "null" in roads:          # stream NULL: the pipeline's regions stream, and the call waits
            rec, stats, status = tensors()
            torch.cuda.synchronize()
            cfg = L.PipelineGaugeConfig(src)
            call = L.PipelineGaugeRegionsCall(rec.data_ptr(), len(regions), 0, stats.data_ptr(), status.data_ptr(), None)
            assert pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
            got["null"] = (stats.cpu().numpy(), status.cpu().numpy())
        r["roads"][src] = got
    return r


def assert_window(L, r, what):
    for src, got in r["roads"].items():
        stats, status = got["want"]
        assert status[-3:].tolist() == [L.REGION_FRAME, L.REGION_BOX, L.REGION_RESERVED] and (status[:-3] == 0).all()
        for road in ("host", "stream", "null"):
            if road in got:
                G.assert_equal(got[road], got["want"], r["regions"], "%s, sources %d, %s road" % (what, src, road))


def run_windows(L, data, work, **kw):
    """work(pipe, window, frames) inside the callback of every window; its results by window"""
    kw.setdefault("parser_threads", 2)
    kw.setdefault("motion", True)
    kw.setdefault("activity", True)
    got = {}

    def on_window(window, frames):
        got[window] = work(frames[0]["_pipe"], window, frames)
    pipe = L.Pipeline(data, on_window=on_window, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return got


@PARSERS
@pytest.mark.parametrize("name", ["ibbp_96x64_coded", "cropped_61x45", "ibbp_352x240"])
def test_every_frame_of_a_window(L, name, gpu_parser):
    data, kw = stream(name)
    got = run_windows(L, data, functools.partial(gauge_window, L), gops_per_window=2, gpu_parser=gpu_parser, **kw)
    assert got
    everything = []
    for window, r in got.items():
        assert_window(L, r, "%s window %d" % (name, window))
        everything.append(r["roads"][3]["want"])
        if name != "cropped_61x45":
            # the frame is its coded size: the whole-frame boxes (every fifth record) against the delivered records' own summaries
            stats = r["roads"][3]["stream"][0][0:5 * r["n"]:5]
            msum, asum = r["summaries"]
            for f in range(r["n"]):
                assert stats[f, 1:7].tolist() == [256 * int(asum[f][k]) for k in (0, 1, 2, 3, 5, 6)] and stats[f, 7] == int(asum[f][4]), (window, f)
                assert stats[f, 8:16].tolist() == [256 * int(v) for v in msum[f]], (window, f)
    G.assert_not_vacuous(np.concatenate([s for s, _ in everything]), np.concatenate([s for _, s in everything]), 3, name)


@pytest.mark.parametrize("has", ["activity", "motion"])
def test_a_pipeline_with_one_record_output(L, has):
    """ACTIVITY alone takes sources 2 and refuses 1 and 3 by the missing output's name, MOTION alone is the mirror; sources=None means
    what the pipeline has"""
    import torch
    data, kw = stream("ibbp_96x64_coded")
    mine, other = (2, "motion") if has == "activity" else (1, "activity")

    def work(pipe, window, frames):
        r = gauge_window(L, pipe, window, frames, sources=(mine,))
        r["default"] = pipe.gauge_regions(window, r["regions"], fill=FILL)
        rec = torch.tensor(np.array(r["regions"], dtype=np.int32), device="cuda")
        stats = torch.full((len(rec), 16), FILL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        r["refused"] = []
        for src in (3 - mine, 3):
            cfg = L.PipelineGaugeConfig(src)
            call = L.PipelineGaugeRegionsCall(rec.data_ptr(), len(rec), 0, stats.data_ptr(), None, None)
            rc = pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, C.byref(cfg), C.byref(call))
            r["refused"].append((rc, pipe.lib.leon_last_error().decode()))
            with pytest.raises(L.LeonError):
                pipe.gauge_regions(window, r["regions"], sources=src)
        torch.cuda.synchronize()
        r["untouched"] = bool((stats == FILL).all())
        # the carry family goes on refusing a pipeline without MOTION
        if has == "activity":
            with pytest.raises(L.LeonError) as e:
                pipe.carry_regions(window, [(0, 0, 0, 8, 8, 0)])
            assert "no motion output" in str(e.value)
        return r
    got = run_windows(L, data, work, gops_per_window=2, gpu_parser=True, motion=has == "motion", activity=has == "activity", **kw)
    assert got
    for window, r in got.items():
        assert_window(L, r, "%s only, window %d" % (has, window))
        G.assert_equal(r["default"], r["roads"][mine]["want"], r["regions"], "sources=None")
        G.assert_not_vacuous(*r["roads"][mine]["want"], mine, has)
        assert r["untouched"] and [rc for rc, _ in r["refused"]] == [L.ERR_INVALID] * 2
        assert all("no %s output" % other in msg for _, msg in r["refused"]), r["refused"]


@PARSERS
def test_a_window_held_across_ring_reuse(L, gpu_parser):
    """window 0 held while windows 1 .. 4 reuse the other ring entry: both records of its frames and its table still gauge exactly"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    held, done = [], threading.Event()

    def on_window(window, frames):
        if window == 0:
            held.append((window, list(frames)))
            return False
        if window == 4:
            done.set()
    pipe = L.Pipeline(data, on_window=on_window, motion=True, activity=True, gops_per_window=1, windows_in_flight=2, gpu_parser=gpu_parser, parser_threads=2)
    try:
        assert done.wait(60), "windows 1 .. 4 were not delivered while window 0 was held"
        window, frames = held[0]
        r = gauge_window(L, pipe, window, frames)
        pipe.release_window(window)
        with pytest.raises(L.LeonError):          # released: no longer out for delivery
            pipe.gauge_regions(window, [(0, 0, 0, 8, 8)])
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_window(L, r, "held window")
    G.assert_not_vacuous(*r["roads"][3]["want"], 3, "held window")


def test_carry_regions_gop_into_gauge_on_one_stream(L):
    """a detector's boxes carried to every frame of a window of two GOPs and gauged where they arrive, with no host wait in between.  The
    rows of the other GOP never arrive (carry status NO_REFERENCE, all zeros: an empty box) and come out as gauge status words."""
    import torch
    data, kw = stream("ibbp_96x64_coded")
    boxes = np.array([[30, 20, 40, 30], [0, 0, 96, 64], [70, 40, 26, 24], [17, 3, 33, 48], [95, 63, 1, 1]], dtype=np.int32)

    def work(pipe, window, frames):
        frames = list(frames)
        n = len(frames)
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        src = [i for i, k in enumerate(keys) if k[2] == 1][0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            records, votes, cstatus = pipe.carry_regions_gop(window, torch.tensor(boxes, device="cuda"), src)
            stats = torch.full((n * len(boxes), 16), FILL, dtype=torch.int64, device="cuda")
            stats, status = pipe.gauge_regions_device(window, records, stats=stats)
        st.synchronize()
        motion = [pipe.read_motion(window, i)[:2] for i in range(n)]
        activity = [pipe.read_activity(window, i)[0] for i in range(n)]
        refs = [a.tolist() for a in pipe.carry_refs(window)]
        rec, _, want_cstatus = gop_chain_on_the_host(L, pipe.info.frame_width, pipe.info.frame_height, motion, refs, keys, boxes, src)[:3]
        rows = rec.reshape(-1, 8).tolist()
        want = G.expected(L, pipe.info.frame_width, pipe.info.frame_height, motion, activity, rows, 3, FILL, n)
        return (stats.cpu().numpy(), status.cpu().numpy()), want, rows, cstatus.cpu().numpy().reshape(-1), want_cstatus.reshape(-1)
    (got, want, rows, cstatus, want_cstatus), = run_windows(L, data, work, gops_per_window=2, gpu_parser=True, **kw).values()
    assert np.array_equal(cstatus, want_cstatus) and (cstatus == 0).any() and (cstatus != 0).any()
    G.assert_equal(got, want, rows, "carry_regions_gop into gauge_regions_device")
    assert (want[1][cstatus != 0] == L.REGION_BOX).all() and (want[1][cstatus == 0] == 0).all()
    G.assert_not_vacuous(*want, 3, "carried boxes")


def test_the_host_road_without_a_status_and_on_a_window_that_is_not_out(L):
    data = ibbp_stream(96, 64, [6], 47)

    def work(pipe, window, frames):
        n, cfg = len(frames), L.PipelineGaugeConfig(3)
        r = L._records_array([(s, 9, 5, 70, 50) for s in range(n)] + [(n, 1, 1, 8, 8)])
        want, status = pipe.gauge_regions(window, r, fill=FILL)
        assert (status[:-1] == 0).all() and status[-1] == L.REGION_FRAME
        stats, st = np.full_like(want, FILL), np.full(len(r), FILL, np.int32)
        assert pipe.lib.leon_pipeline_gauge_regions(pipe.h, window, C.byref(cfg), r.ctypes.data, len(r), stats.ctypes.data, None) == L.OK, pipe.lib.leon_last_error()
        assert np.array_equal(stats, want)
        # a window that is not out for delivery: refused before anything is allocated or uploaded, the caller's arrays as they were
        stats[:] = FILL
        assert pipe.lib.leon_pipeline_gauge_regions(pipe.h, window + 7, C.byref(cfg), r.ctypes.data, len(r), stats.ctypes.data, st.ctypes.data) == L.ERR_INVALID
        assert pipe.lib.leon_last_error() == b"window %d is not out for delivery" % (window + 7)
        assert (stats == FILL).all() and (st == FILL).all()
        return True
    got = run_windows(L, data, work, gops_per_window=1, gpu_parser=True)
    assert got and all(got.values())


def test_the_call_is_refused_as_a_whole(L):
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    seen = []

    def work(pipe, window, frames):
        rec = torch.zeros((4, 8), dtype=torch.int32, device="cuda")
        rec[:, 3:5] = 8
        stats = torch.full((4, 16), FILL, dtype=torch.int64, device="cuda")
        status = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = dict(regions=rec.data_ptr(), n=4, reserved0=0, device_stats=stats.data_ptr(), device_status=status.data_ptr())

        def refused(word, window_=window, reserved=(0, 0, 0), sources=3, cfg_reserved=None, **kw):
            a = dict(ok, **kw)
            cfg = L.PipelineGaugeConfig(sources)
            if cfg_reserved is not None:
                cfg.reserved[cfg_reserved] = 1
            call = L.PipelineGaugeRegionsCall(a["regions"], a["n"], a["reserved0"], a["device_stats"], a["device_status"], None, (C.c_uint64 * 3)(*reserved))
            rc = pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window_, C.byref(cfg), C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert bool((stats == FILL).all()) and bool((status == FILL).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        refused("sources 0", sources=0)
        refused("sources 4", sources=4)
        refused("sources -1", sources=-1)
        for k in range(7):
            refused("reserved word of the config", cfg_reserved=k)
        refused("not out for delivery", window_=window + 7)
        refused("null regions", regions=None)
        refused("null device_stats", device_stats=None)
        refused("4-byte aligned", regions=rec.data_ptr() + 2)
        refused("4-byte aligned", device_status=status.data_ptr() + 3)
        refused("8-byte aligned", device_stats=stats.data_ptr() + 4)
        refused("8-byte aligned", device_stats=stats.data_ptr() + 1)
        refused("0 regions", n=0)
        refused("65536 regions", n=65536)
        refused("-1 regions", n=-1)
        refused("reserved word of the call", reserved0=1)
        for k in range(3):
            refused("reserved word of the call", reserved=tuple(int(j == k) for j in range(3)))
        cfg = L.PipelineGaugeConfig(3)
        call = L.PipelineGaugeRegionsCall(rec.data_ptr(), 4, 0, stats.data_ptr(), status.data_ptr(), None)
        assert pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, C.byref(cfg), None) == L.ERR_INVALID
        assert pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, None, C.byref(call)) == L.ERR_INVALID
        assert pipe.lib.leon_pipeline_gauge_regions_device(None, window, C.byref(cfg), C.byref(call)) == L.ERR_INVALID
        # the host road refuses the same; a record's fault is no refusal
        host, s, t = np.zeros((2, 8), dtype=np.int32), np.zeros((2, 16), np.int64), np.zeros(2, np.int32)
        for args in ((window + 7, C.byref(cfg), host.ctypes.data, 2, s.ctypes.data), (window, C.byref(cfg), None, 2, s.ctypes.data), (window, C.byref(cfg), host.ctypes.data, 2, None),
                     (window, C.byref(cfg), host.ctypes.data, 0, s.ctypes.data), (window, C.byref(cfg), host.ctypes.data, 65536, s.ctypes.data),
                     (window, None, host.ctypes.data, 2, s.ctypes.data), (window, C.byref(L.PipelineGaugeConfig(0)), host.ctypes.data, 2, s.ctypes.data)):
            assert pipe.lib.leon_pipeline_gauge_regions(pipe.h, *args, t.ctypes.data) == L.ERR_INVALID
        s, t = pipe.gauge_regions(window, [(0, 0, 0, 0, 0), (99, 0, 0, 8, 8), (0, 0, 0, 8, 8)], fill=FILL)
        assert t.tolist() == [L.REGION_BOX, L.REGION_FRAME, 0] and (s[:2] == FILL).all() and s[2, 0] == 64
        # status may be NULL
        call = L.PipelineGaugeRegionsCall(rec.data_ptr(), 4, 0, stats.data_ptr(), None, None)
        assert pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK
        assert bool((stats[:, 0] == 64).all()) and bool((status == FILL).all())
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()) and len(seen) == 24
    # a pipeline with neither record output
    refusals = []

    def neither(window, frames):
        pipe = frames[0]["_pipe"]
        z = np.zeros(64, dtype=np.int64)
        for src in (1, 2, 3):
            cfg = L.PipelineGaugeConfig(src)
            call = L.PipelineGaugeRegionsCall(z.ctypes.data, 1, 0, z.ctypes.data, None, None)
            refusals.append(pipe.lib.leon_pipeline_gauge_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)))
            refusals.append(pipe.lib.leon_pipeline_gauge_regions(pipe.h, window, C.byref(cfg), z.ctypes.data, 1, z.ctypes.data, None))
    pipe = L.Pipeline(data, on_window=neither, gops_per_window=1, output="tensor")
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert refusals and all(rc == L.ERR_INVALID for rc in refusals)
