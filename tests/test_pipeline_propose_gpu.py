"""GPU: boxes proposed from the motion and activity records of delivered windows (include/leon_pipeline.h,
leon_pipeline_propose_regions; k_propose) -- for every frame of a window, regions, count, info and status of the host road, of the
device road on a caller's stream and of the device road on the pipeline's own stream, all exactly equal to leon_ctypes.propose_boxes
(the header's text as a breadth-first fill in Python integers) on the records read_motion and read_activity give; from the delivered
data alone, the cells of the boxes sum to the hot cells and every hot cell lies inside a box; the [F, K, 8] result straight into
gauge_regions_device and resample_regions_device on one stream; pipelines with one of the two record outputs only; a window held
across ring reuse; and every call-level refusal, with nothing written."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import propose_cases as P
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import stream

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
FILL = -55
K = 24


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def thresholds(motion, activity):
    """thresholds the window's own records split: the median of the vector magnitudes and of the ac_mag that are not 0 (1 where there are none)"""
    kw = {}
    if motion is not None:
        mag = np.concatenate([np.abs(m[0].astype(np.int64)).max(axis=2).reshape(-1) for m in motion])
        kw["mv_min"] = int(np.median(mag[mag > 0])) if (mag > 0).any() else 1
    if activity is not None:
        ac = np.concatenate([a[0]["ac_mag"].astype(np.int64).reshape(-1) for a in activity])
        kw["ac_min"] = int(np.median(ac[ac > 0])) if (ac > 0).any() else 1
    return kw


def propose_window(L, pipe, window, frames, roads=("host", "stream", "null"), variants=None):
    """everything of one delivered window: every frame, the first frame again and two frames outside it, on each road"""
    import torch
    n, fw, fh = len(list(frames)), pipe.info.frame_width, pipe.info.frame_height
    motion = [pipe.read_motion(window, i) for i in range(n)] if pipe.motion_layout is not None else None
    activity = [pipe.read_activity(window, i) for i in range(n)] if pipe.activity_layout is not None else None
    m2, a2 = None if motion is None else [m[:2] for m in motion], None if activity is None else [a[0] for a in activity]
    base = thresholds(motion, activity)
    requests = list(range(n)) + [0, n, -1]
    r = dict(n=n, fw=fw, fh=fh, requests=requests, motion=m2, activity=a2, base=base, roads=[])
    if variants is None:
        variants = [dict(connectivity=8), dict(connectivity=4, min_cells=2, max_boxes=3)] + ([dict(intra=True, connectivity=4)] if motion is not None else [])
    for v in variants:
        kw = dict(base, max_boxes=K)
        kw.update(v)
        got = dict(kw=kw, want=P.expected(L, fw, fh, m2, a2, requests, FILL, **kw))
        k = kw["max_boxes"]
        if "host" in roads:
            regions, count, info, status = pipe.propose_regions(window, requests, fill=FILL, **kw)
            got["host"] = (regions, info, count, status)
        if "stream" in roads:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                regions, count, info, status = pipe.propose_regions_device(window, torch.tensor(requests, dtype=torch.int32, device="cuda"), **kw)
            st.synchronize()
            want = got["want"]
            ok = want[3] == 0          # (the method's tensors are not initialised: a refused request's rows say nothing)
            got["stream"] = tuple(np.where(ok.reshape((-1,) + (1,) * (w.ndim - 1)), g.cpu().numpy(), FILL) for g, w in zip((regions, info, count), want[:3])) + (status.cpu().numpy(),)
        if "null" in roads:          # stream NULL: the pipeline's regions stream, and the call waits; sentinels in every output
            t = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((len(requests), k, 8), (len(requests), k, 2), (len(requests),), (len(requests),))]
            fr = torch.tensor(requests, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            cfg = L._propose_config(None, k, kw.get("mv_min"), kw.get("ac_min"), kw.get("intra", False), kw["connectivity"], kw.get("min_cells", 1))
            call = L.PipelineProposeRegionsCall(fr.data_ptr(), len(requests), 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
            assert pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
            got["null"] = tuple(x.cpu().numpy() for x in t)
        r["roads"].append(got)
    return r


def assert_window(L, r, what):
    for got in r["roads"]:
        assert got["want"][3].tolist() == [0] * (r["n"] + 1) + [L.REGION_FRAME] * 2
        assert np.array_equal(got["want"][0][0], got["want"][0][r["n"]]), "the same frame named twice"
        for road in ("host", "stream", "null"):
            if road in got:
                P.assert_equal(got[road], got["want"], "%s, %s, %s road" % (what, got["kw"], road))


def assert_covers(L, r, what):
    """from the delivered data alone (min_cells 1): where count <= K the cells sum to the hot cells and every hot cell lies inside a box"""
    got = r["roads"][0]
    assert got["kw"].get("min_cells", 1) == 1
    regions, info, count, _ = got["stream"]
    seen = 0
    for f in range(r["n"]):
        hot = P.hot_cells(L, r["fw"], r["fh"], None if r["motion"] is None else r["motion"][f], None if r["activity"] is None else r["activity"][f],
                          mv_min=got["kw"].get("mv_min"), ac_min=got["kw"].get("ac_min"), intra=got["kw"].get("intra", False))
        if count[f] > K:
            continue
        assert info[f, :count[f], 0].sum() == hot.sum(), (what, f)
        inside = np.zeros_like(hot)
        for _, x, y, w, h, *_ in regions[f, :count[f]].tolist():
            assert x % 16 == 0 and y % 16 == 0 and w >= 1 and h >= 1 and x + w <= r["fw"] and y + h <= r["fh"]
            inside[y // 16:(y + h + 15) // 16, x // 16:(x + w + 15) // 16] = True
        assert (inside | ~hot).all(), (what, f)
        seen += int(hot.sum())
    return seen


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
    got = run_windows(L, data, functools.partial(propose_window, L), gops_per_window=2, gpu_parser=gpu_parser, **kw)
    assert got
    seen, counts = 0, []
    for window, r in got.items():
        assert_window(L, r, "%s window %d" % (name, window))
        seen += assert_covers(L, r, "%s window %d" % (name, window))
        counts += r["roads"][0]["want"][2][:r["n"]].tolist()
    assert seen > 0 and max(counts) >= 1, "nothing was hot"


@pytest.mark.parametrize("has", ["activity", "motion"])
def test_a_pipeline_with_one_record_output(L, has):
    """ACTIVITY alone takes the activity source and refuses the other two by the missing output's name, MOTION alone is the mirror;
    sources=None means what the pipeline has, with its threshold"""
    import torch
    data, kw = stream("ibbp_96x64_coded")
    mine, other = (2, "motion") if has == "activity" else (1, "activity")

    def work(pipe, window, frames):
        r = propose_window(L, pipe, window, frames, variants=[dict(connectivity=8)])
        t = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((2, 4, 8), (2, 4, 2), (2,), (2,))]
        fr = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r["refused"] = []
        for src in (3 - mine, 3):
            cfg = L._propose_config(src, 4, 1 if src & 1 else None, 1 if src & 2 else None, False, 8, 1)
            call = L.PipelineProposeRegionsCall(fr.data_ptr(), 2, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
            rc = pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, C.byref(cfg), C.byref(call))
            r["refused"].append((rc, pipe.lib.leon_last_error().decode()))
            with pytest.raises(L.LeonError):
                pipe.propose_regions(window, [0], sources=src, mv_min=1 if src & 1 else None, ac_min=1 if src & 2 else None)
        with pytest.raises(ValueError):          # sources=None asks for the threshold of the output the pipeline has
            pipe.propose_regions(window, [0], **{"ac_min" if has == "motion" else "mv_min": 1})
        torch.cuda.synchronize()
        r["untouched"] = all(bool((x == FILL).all()) for x in t)
        return r
    got = run_windows(L, data, work, gops_per_window=2, gpu_parser=True, motion=has == "motion", activity=has == "activity", **kw)
    assert got
    for window, r in got.items():
        assert_window(L, r, "%s only, window %d" % (has, window))
        assert set(r["base"]) == {"mv_min" if has == "motion" else "ac_min"}
        assert r["untouched"] and [rc for rc, _ in r["refused"]] == [L.ERR_INVALID] * 2
        assert all("no %s output" % other in msg for _, msg in r["refused"]), r["refused"]


@PARSERS
def test_a_window_held_across_ring_reuse(L, gpu_parser):
    """window 0 held while windows 1 .. 4 reuse the other ring entry: both records of its frames and its table still give its boxes"""
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
        r = propose_window(L, pipe, window, frames)
        pipe.release_window(window)
        with pytest.raises(L.LeonError):          # released: no longer out for delivery
            pipe.propose_regions(window, [0], mv_min=1, ac_min=1)
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_window(L, r, "held window")
    assert assert_covers(L, r, "held window") > 0


def test_the_result_goes_into_gauge_and_resample_as_it_is(L):
    """output tensor + both records: propose_regions_device over every frame (frames=None), its [F, K, 8] tensor unchanged into
    gauge_regions_device and into resample_regions_device on the same stream, one wait at the end.  The first count rows: gauge word 0 =
    w * h and a resampled region equal to read_regions of the same box; the rows behind: REGION_BOX from both"""
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    size = (16, 24)

    def work(pipe, window, frames):
        n = len(frames)
        motion, activity = [pipe.read_motion(window, i) for i in range(n)], [pipe.read_activity(window, i) for i in range(n)]
        kw = thresholds(motion, activity)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            regions, count, info, status = pipe.propose_regions_device(window, max_boxes=6, connectivity=4, **kw)
            stats, gstatus = pipe.gauge_regions_device(window, regions)
            batch, rstatus = pipe.resample_regions_device(window, regions.view(-1, 8), size)
        st.synchronize()
        regions, count = regions.cpu().numpy(), count.cpu().numpy()
        want = P.expected(L, pipe.info.frame_width, pipe.info.frame_height, [m[:2] for m in motion], [a[0] for a in activity], list(range(n)), FILL, max_boxes=6,
                          connectivity=4, **kw)
        P.assert_equal((regions, info.cpu().numpy(), count, status.cpu().numpy()), want, "frames=None")
        used = (np.arange(6)[None, :] < count[:, None]).reshape(-1)
        boxes = [tuple(b[:5]) for b in regions.reshape(-1, 8)[used].tolist()]
        return (used, regions.reshape(-1, 8), stats.cpu().numpy(), gstatus.cpu().numpy(), rstatus.cpu().numpy(), batch.cpu().numpy()[used],
                pipe.read_regions(window, boxes, size))
    (used, rows, stats, gstatus, rstatus, batch, want), = run_windows(L, data, work, gops_per_window=1, gpu_parser=True, output="tensor").values()
    assert used.any() and (~used).any()
    for status in (gstatus, rstatus):
        assert (status[used] == 0).all() and (status[~used] == L.REGION_BOX).all()
    assert stats[used, 0].tolist() == (rows[used, 3] * rows[used, 4]).tolist()
    assert batch.shape == want.shape and np.array_equal(batch.view(np.uint16), want.view(np.uint16))


def test_the_call_is_refused_as_a_whole(L):
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    seen = []

    def work(pipe, window, frames):
        t = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((4, 4, 8), (4, 4, 2), (4,), (4,))]
        fr = torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = dict(frames=fr.data_ptr(), n=4, reserved0=0, device_regions=t[0].data_ptr(), device_info=t[1].data_ptr(), device_count=t[2].data_ptr(),
                  device_status=t[3].data_ptr())
        good = (3, 0, 1, 1, 8, 1, 4, 0)

        def refused(word, window_=window, reserved=0, cfg=good, **kw):
            a = dict(ok, **kw)
            c = L.PipelineProposeConfig(*cfg)
            call = L.PipelineProposeRegionsCall(a["frames"], a["n"], a["reserved0"], a["device_regions"], a["device_info"], a["device_count"], a["device_status"], None,
                                                (C.c_uint64 * 1)(reserved))
            rc = pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window_, C.byref(c), C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert all(bool((x == FILL).all()) for x in t), "a refused call wrote (%s)" % word
            seen.append(word)
        for words, text in ((( 0, 0, 1, 1, 8, 1, 4, 0), "sources 0"), ((4, 0, 1, 1, 8, 1, 4, 0), "sources 4"), ((2, 1, 0, 1, 8, 1, 4, 0), "flags"), ((3, 2, 1, 1, 8, 1, 4, 0), "flags"),
                            ((3, 0, 0, 1, 8, 1, 4, 0), "mv_min 0"), ((3, 0, 32769, 1, 8, 1, 4, 0), "mv_min 32769"), ((2, 0, 1, 1, 8, 1, 4, 0), "mv_min 1"),
                            ((3, 0, 1, 0, 8, 1, 4, 0), "ac_min 0"), ((3, 0, 1, 65536, 8, 1, 4, 0), "ac_min 65536"), ((1, 0, 1, 1, 8, 1, 4, 0), "ac_min 1"),
                            ((3, 0, 1, 1, 6, 1, 4, 0), "connectivity 6"), ((3, 0, 1, 1, 8, 0, 4, 0), "min_cells 0"), ((3, 0, 1, 1, 8, 65537, 4, 0), "min_cells 65537"),
                            ((3, 0, 1, 1, 8, 1, 0, 0), "max_boxes 0"), ((3, 0, 1, 1, 8, 1, 1025, 0), "max_boxes 1025"), ((3, 0, 1, 1, 8, 1, 4, 1), "reserved word of the config")):
            refused(text, cfg=words)
        refused("not out for delivery", window_=window + 7)
        refused("null frames", frames=None)
        refused("null device_regions", device_regions=None)
        refused("null device_count", device_count=None)
        for name in ("frames", "device_regions", "device_info", "device_count", "device_status"):
            refused("4-byte aligned", **{name: ok[name] + 2})
        refused("0 frames", n=0)
        refused("65536 frames", n=65536)
        refused("-1 frames", n=-1)
        refused("reserved word of the call", reserved0=1)
        refused("reserved word of the call", reserved=1)
        cfg = L.PipelineProposeConfig(*good)
        call = L.PipelineProposeRegionsCall(fr.data_ptr(), 4, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
        assert pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, C.byref(cfg), None) == L.ERR_INVALID
        assert pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, None, C.byref(call)) == L.ERR_INVALID
        assert pipe.lib.leon_pipeline_propose_regions_device(None, window, C.byref(cfg), C.byref(call)) == L.ERR_INVALID
        # the host road refuses the same, with the caller's arrays as they were; a request's fault is no refusal
        h = [np.full(s, FILL, dtype=np.int32) for s in ((2, 4, 8), (2, 4, 2), (2,), (2,))]
        hf = np.zeros(2, dtype=np.int32)
        H = [x.ctypes.data for x in h]
        for args in ((window + 7, C.byref(cfg), hf.ctypes.data, 2, H[0], H[1], H[2], H[3]), (window, C.byref(cfg), None, 2, H[0], H[1], H[2], H[3]),
                     (window, C.byref(cfg), hf.ctypes.data, 2, None, H[1], H[2], H[3]), (window, C.byref(cfg), hf.ctypes.data, 2, H[0], H[1], None, H[3]),
                     (window, C.byref(cfg), hf.ctypes.data, 0, H[0], H[1], H[2], H[3]), (window, C.byref(cfg), hf.ctypes.data, 65536, H[0], H[1], H[2], H[3]),
                     (window, None, hf.ctypes.data, 2, H[0], H[1], H[2], H[3]), (window, C.byref(L.PipelineProposeConfig(0)), hf.ctypes.data, 2, H[0], H[1], H[2], H[3])):
            assert pipe.lib.leon_pipeline_propose_regions(pipe.h, *args) == L.ERR_INVALID
        assert all((x == FILL).all() for x in h)
        regions, count, info, status = pipe.propose_regions(window, [99, 0, -1], mv_min=1, ac_min=1, max_boxes=4, fill=FILL)
        assert status.tolist() == [L.REGION_FRAME, 0, L.REGION_FRAME] and (regions[[0, 2]] == FILL).all() and (count[[0, 2]] == FILL).all() and count[1] >= 0
        # info and status may be NULL on both roads
        call = L.PipelineProposeRegionsCall(fr.data_ptr(), 4, 0, t[0].data_ptr(), None, t[2].data_ptr(), None, None)
        assert pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK
        assert bool((t[0] != FILL).all()) and bool((t[2] >= 0).all()) and bool((t[1] == FILL).all()) and bool((t[3] == FILL).all())
        assert pipe.lib.leon_pipeline_propose_regions(pipe.h, window, C.byref(cfg), hf.ctypes.data, 2, H[0], None, H[2], None) == L.OK
        assert np.array_equal(h[0], t[0].cpu().numpy()[:2]) and (h[1] == FILL).all() and (h[3] == FILL).all()
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()) and len(seen) == 30
    # a pipeline with neither record output
    refusals = []

    def neither(window, frames):
        pipe = frames[0]["_pipe"]
        z = np.zeros(64, dtype=np.int32)
        for src in (1, 2, 3):
            cfg = L._propose_config(src, 1, 1 if src & 1 else None, 1 if src & 2 else None, False, 8, 1)
            call = L.PipelineProposeRegionsCall(z.ctypes.data, 1, 0, z.ctypes.data, None, z.ctypes.data, None, None)
            refusals.append(pipe.lib.leon_pipeline_propose_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)))
            refusals.append(pipe.lib.leon_pipeline_propose_regions(pipe.h, window, C.byref(cfg), z.ctypes.data, 1, z.ctypes.data, None, z.ctypes.data, None))
    pipe = L.Pipeline(data, on_window=neither, gops_per_window=1, output="tensor")
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert refusals and all(rc == L.ERR_INVALID for rc in refusals)
