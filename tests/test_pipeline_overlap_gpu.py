"""GPU: boxes suppressed and matched through a pipeline (include/leon_pipeline.h, leon_pipeline_suppress_regions and
leon_pipeline_match_regions; k_suppress, k_match) on delivered windows of the synthetic stream: the device road on a caller's stream,
the device road on the pipeline's own stream and the host road, all exactly equal to leon_ctypes.suppress_boxes / match_boxes;
propose_regions_device -> suppress_regions_device -> gauge_regions_device chained on one stream with one wait at the end, the rows
behind count coming back REGION_BOX; the boxes carry_regions_gop brings to the last frame of a GOP matched with the boxes on the
first frame of the next one; a pipeline made with RGBA alone; and every call-level refusal, with nothing written."""
import ctypes as C

import numpy as np
import pytest

import overlap_cases as O
from test_pipeline_gpu import ibbp_stream
from test_pipeline_propose_gpu import run_windows, thresholds

pytestmark = pytest.mark.gpu

FILL = O.FILL


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def window_sets(n_frames, fw, fh, n=3, k=20, seed=0):
    """n sets of k rows on the window's frames, sides 16 .. 48, with a row of each refused kind and propose's filler between them"""
    r = O.random_rows(n, k, fw, fh, 16, 48, seed=seed, frames=n_frames)
    r[0, 3] = O.row(0, 0, 16, 16, r1=1)
    r[1, 5] = O.row(0, 0, 16, 16, frame=n_frames)
    r[n - 1, 7] = O.row(fw - 8, 0, 16, 16)
    r[n - 1, 9] = O.row(0, 0, 0, 0)
    return r


def want_suppress(L, fw, fh, n_frames, rows, scores, stride, t, measure):
    outs = [L.suppress_boxes(fw, fh, n_frames, rows[s].tolist(), None if scores is None else [int(scores[(s * rows.shape[1] + i) * stride]) for i in range(rows.shape[1])], t, measure)
            for s in range(rows.shape[0])]
    k = rows.shape[1]
    return [np.stack([O.filled(sum(o[0], []), (k, 8)) for o in outs]), np.stack([O.filled(o[1], k) for o in outs]), np.stack([O.filled(o[2], k) for o in outs]),
            np.array([o[3] for o in outs], dtype=np.int32), np.stack([O.filled(o[4], k) for o in outs])]


def want_match(L, fw, fh, n_frames, a, b, t, measure):
    outs = [L.match_boxes(fw, fh, n_frames, a[s].tolist(), b[s].tolist(), t, measure) for s in range(a.shape[0])]
    ka, kb = a.shape[1], b.shape[1]
    return [np.stack([O.filled(o[0], ka) for o in outs]), np.stack([O.filled(o[1], kb) for o in outs]), np.stack([O.filled(o[2], ka) for o in outs]),
            np.array([o[3] for o in outs], dtype=np.int32), np.stack([O.filled(o[4], ka) for o in outs]), np.stack([O.filled(o[5], kb) for o in outs])]


def masked(got, want):
    """the method's tensors are not initialised: where the definition writes nothing the device's words say nothing"""
    return [np.where(w == FILL, FILL, g) for g, w in zip(got, want)]


def roads(L, pipe, window, frames):
    """one delivered window: both steps on each of the three roads"""
    import torch
    n_frames, fw, fh = len(frames), pipe.info.frame_width, pipe.info.frame_height
    rows, other = window_sets(n_frames, fw, fh, seed=window), window_sets(n_frames, fw, fh, k=13, seed=window + 50)
    scores = np.random.default_rng(window).integers(-3, 4, size=rows.shape[0] * rows.shape[1] * 2).astype(np.int32)
    t, measure = 19661, O.IOMIN
    r = dict(n_frames=n_frames, want_s=want_suppress(L, fw, fh, n_frames, rows, scores, 2, t, measure), want_m=want_match(L, fw, fh, n_frames, rows, other, 6554, O.IOU))
    # the host roads
    r["host_s"] = pipe.suppress_regions(window, rows, scores, threshold_q16=t, measure="iomin", score_stride=2, fill=FILL)
    r["host_m"] = pipe.match_regions(window, rows, other, threshold=0.1, measure="iou", fill=FILL)
    # the device roads on a side stream
    st = torch.cuda.Stream()
    d_rows, d_other, d_scores = (torch.tensor(x, dtype=torch.int32, device="cuda") for x in (rows, other, scores))
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got_s = pipe.suppress_regions_device(window, d_rows, d_scores, threshold_q16=t, measure="iomin", score_stride=2)
        got_m = pipe.match_regions_device(window, d_rows, d_other, threshold=0.1)
    st.synchronize()
    r["stream_s"] = masked([g.cpu().numpy() for g in got_s], r["want_s"])
    r["stream_m"] = masked([g.cpu().numpy() for g in got_m], r["want_m"])
    # stream NULL: the pipeline's regions stream, and the call waits; sentinels in every output
    n, k, kb = rows.shape[0], rows.shape[1], other.shape[1]
    ts = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((n, k, 8), (n, k), (n, k), (n,), (n, k))]
    tm = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((n, k), (n, kb), (n, k), (n,), (n, k), (n, kb))]
    torch.cuda.synchronize()
    cfg = L.PipelineOverlapConfig(measure, t)
    call = L.PipelineSuppressRegionsCall(d_rows.data_ptr(), d_scores.data_ptr(), n, k, 2, 0, *[x.data_ptr() for x in ts], None)
    assert pipe.lib.leon_pipeline_suppress_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
    r["null_s"] = [x.cpu().numpy() for x in ts]
    cfg = L.PipelineOverlapConfig(O.IOU, 6554)
    call = L.PipelineMatchRegionsCall(d_rows.data_ptr(), d_other.data_ptr(), n, k, kb, 0, *[x.data_ptr() for x in tm], None)
    assert pipe.lib.leon_pipeline_match_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
    r["null_m"] = [x.cpu().numpy() for x in tm]
    # a single set goes in as [K, 8]
    one = pipe.suppress_regions_device(window, d_rows[0], threshold_q16=t, measure="iomin")
    torch.cuda.synchronize()
    r["one"] = (one[2].cpu().numpy().shape, int(one[3].cpu().numpy()[0]))
    return r


def assert_roads(r, what):
    for road in ("host", "stream", "null"):
        O.assert_equal(r[road + "_s"], r["want_s"], O.SUPPRESS_NAMES, "%s, suppress, %s road" % (what, road))
        O.assert_equal(r[road + "_m"], r["want_m"], O.MATCH_NAMES, "%s, match, %s road" % (what, road))
    assert {1, 2, 3} <= set(r["want_s"][4].reshape(-1).tolist()) and (r["want_s"][3] >= 1).all() and (r["want_m"][3] >= 1).all()
    assert ((r["want_s"][4] == 0).sum(axis=1) > r["want_s"][3]).any(), "no set has a suppressed row"
    assert r["one"][0] == (1, r["want_s"][2].shape[1])


@pytest.mark.parametrize("rgba_only", [False, True], ids=["records", "rgba-only"])
def test_the_three_roads_agree_with_the_definition(L, rgba_only):
    """with motion and activity outputs, and on a pipeline created with RGBA alone: the calls read no record"""
    data = ibbp_stream(96, 64, [6, 6], 47)
    got = run_windows(L, data, lambda pipe, window, frames: roads(L, pipe, window, frames), gops_per_window=2, gpu_parser=True, motion=not rgba_only, activity=not rgba_only)
    assert got
    for window, r in got.items():
        assert r["n_frames"] >= 6
        assert_roads(r, "window %d" % window)


def test_propose_suppress_gauge_on_one_stream(L):
    """propose_regions_device's [F, K, 8] and the cells column of its info into suppress_regions_device (IOMIN, score_stride 2), the
    result into gauge_regions_device, all on one side stream with one wait at the end"""
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    K = 12

    def work(pipe, window, frames):
        n = len(frames)
        motion, activity = [pipe.read_motion(window, i) for i in range(n)], [pipe.read_activity(window, i) for i in range(n)]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            regions, count, info, status = pipe.propose_regions_device(window, max_boxes=K, connectivity=4, **thresholds(motion, activity))
            out, order, by, kept, sstatus = pipe.suppress_regions_device(window, regions, info, threshold_q16=65536, measure="iomin", score_stride=2)
            stats, gstatus = pipe.gauge_regions_device(window, out)
        st.synchronize()
        return [x.cpu().numpy() for x in (regions, count, info, out, order, by, kept, sstatus, stats, gstatus)]
    (regions, count, info, out, order, by, kept, sstatus, stats, gstatus), = run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()
    n = regions.shape[0]
    want = want_suppress(L, 96, 64, n, regions, info.reshape(-1), 2, 65536, O.IOMIN)
    O.assert_equal(masked([out, order, by, kept, sstatus], want), want, O.SUPPRESS_NAMES, "the proposed boxes")
    used = (np.arange(K)[None, :] < kept[:, None]).reshape(-1)
    assert used.any() and (~used).any() and (kept <= np.minimum(count, K)).all() and (kept >= np.minimum(count, 1)).all()
    assert (sstatus[np.arange(K)[None, :] >= np.minimum(count, K)[:, None]] == L.REGION_BOX).all(), "propose's filler rows are refused"
    assert (gstatus[used] == 0).all() and (gstatus[~used] == L.REGION_BOX).all()
    rows = out.reshape(-1, 8)
    assert stats[used, 0].tolist() == (rows[used, 3].astype(np.int64) * rows[used, 4]).tolist()


def test_carried_boxes_matched_across_the_gop_border(L):
    """two closed GOPs in one window: boxes on the first frame carried to the last frame of GOP 0 (carry_regions_gop), matched there
    with "detections" on the first frame of GOP 1 -- the carried boxes themselves, moved by a pixel or two and in another order, among
    others -- although k_carry has no road across the border (REGION_NO_REFERENCE)"""
    import torch
    data = ibbp_stream(96, 64, [6, 6], 47)

    def work(pipe, window, frames):
        gop0 = [i for i, f in enumerate(frames) if f["gop"] == frames[0]["gop"]]
        last, first = gop0[-1], gop0[-1] + 1
        boxes = torch.tensor([[8, 8, 24, 24], [50, 20, 30, 30], [30, 40, 20, 16], [70, 4, 16, 20]], dtype=torch.int32, device="cuda")
        records, votes, status = pipe.carry_regions_gop(window, boxes, 0)
        carried = records[last].cpu().numpy()
        det = np.zeros((6, 8), dtype=np.int32)
        det[[4, 0, 2, 5]] = carried          # another order
        det[:, 0] = first
        det[[4, 0, 2, 5], 1] = np.clip(det[[4, 0, 2, 5], 1] + [1, -1, 0, 2], 0, 96 - det[[4, 0, 2, 5], 3])
        det[1], det[3] = O.row(0, 48, 12, 12, frame=first), O.row(84, 52, 12, 12, frame=first)
        got = pipe.match_regions_device(window, records[last], torch.tensor(det, device="cuda"), threshold=0.5)
        crossing = status[first].cpu().numpy()
        torch.cuda.synchronize()
        return carried, det, [g.cpu().numpy() for g in got], status[last].cpu().numpy(), crossing, len(frames)
    (carried, det, got, st_last, crossing, n), = run_windows(L, data, work, gops_per_window=2, gpu_parser=True, activity=False).values()
    assert (st_last == 0).all() and (crossing == L.REGION_NO_REFERENCE).all()
    want = want_match(L, 96, 64, n, carried[None], det[None], 32768, O.IOU)
    O.assert_equal(got, want, O.MATCH_NAMES, "carried against detected")
    assert got[0][0].tolist() == [4, 0, 2, 5] and got[1][0].tolist() == [1, -1, 2, -1, 0, 3] and got[3][0] == 4 and (got[2][0] >= 32768).all()


def test_the_calls_are_refused_as_a_whole(L):
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    seen = []

    def work(pipe, window, frames):
        ts = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((2, 4, 8), (2, 4), (2, 4), (2,), (2, 4))]
        tm = [torch.full(s, FILL, dtype=torch.int32, device="cuda") for s in ((2, 4), (2, 4), (2, 4), (2,), (2, 4), (2, 4))]
        rows = torch.tensor(O.random_rows(2, 4, 96, 64, 16, 40, seed=1), dtype=torch.int32, device="cuda")
        scores = torch.zeros(2 * 4 * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok_s = dict(regions=rows.data_ptr(), scores=scores.data_ptr(), n=2, k=4, score_stride=1, reserved0=0, device_out=ts[0].data_ptr(), device_order=ts[1].data_ptr(),
                    device_by=ts[2].data_ptr(), device_count=ts[3].data_ptr(), device_status=ts[4].data_ptr())
        ok_m = dict(a=rows.data_ptr(), b=rows.data_ptr(), n=2, ka=4, kb=4, reserved0=0, device_match_a=tm[0].data_ptr(), device_match_b=tm[1].data_ptr(),
                    device_overlap=tm[2].data_ptr(), device_count=tm[3].data_ptr(), device_status_a=tm[4].data_ptr(), device_status_b=tm[5].data_ptr())

        def refused(step, word, window_=window, reserved=0, cfg=(0, 32768, 0, 0), **kw):
            c = L.PipelineOverlapConfig(cfg[0], cfg[1], (C.c_int32 * 2)(cfg[2], cfg[3]))
            if step == "suppress":
                a = dict(ok_s, **kw)
                call = L.PipelineSuppressRegionsCall(*[a[f] for f in ok_s], None, (C.c_uint64 * 2)(0, reserved))
                rc = pipe.lib.leon_pipeline_suppress_regions_device(pipe.h, window_, C.byref(c), C.byref(call))
            else:
                a = dict(ok_m, **kw)
                call = L.PipelineMatchRegionsCall(*[a[f] for f in ok_m], None, (C.c_uint64 * 1)(reserved))
                rc = pipe.lib.leon_pipeline_match_regions_device(pipe.h, window_, C.byref(c), C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (step, word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert all(bool((x == FILL).all()) for x in ts + tm), "a refused call wrote (%s, %s)" % (step, word)
            seen.append((step, word))
        for step, ok in (("suppress", ok_s), ("match", ok_m)):
            for cfg, word in (((2, 32768, 0, 0), "measure 2"), ((-1, 32768, 0, 0), "measure -1"), ((0, 0, 0, 0), "threshold 0"), ((0, 65537, 0, 0), "threshold 65537"),
                              ((0, 32768, 1, 0), "reserved word of the config"), ((0, 32768, 0, 1), "reserved word of the config")):
                refused(step, word, cfg=cfg)
            refused(step, "not out for delivery", window_=window + 7)
            refused(step, "reserved word of the call", reserved0=1)
            refused(step, "reserved word of the call", reserved=1)
            for n in (0, -1, 65536):
                refused(step, "%d " % n, n=n)
            for name in [f for f in ok if f.startswith("k")]:
                for k in (0, -1, 1025):
                    refused(step, "%s %d" % (name, k), **{name: k})
            for name in [f for f in ok if f in ("regions", "device_by", "device_count", "a", "b", "device_match_a", "device_match_b", "device_overlap")]:
                refused(step, "null %s" % name, **{name: None})
            for name in [f for f in ok if isinstance(ok[f], int) and ok[f] > 65536]:
                refused(step, "4-byte aligned", **{name: ok[name] + 2})
        for stride in (0, -1, 9):
            refused("suppress", "score_stride %d" % stride, score_stride=stride)
            refused("suppress", "score_stride %d" % stride, score_stride=stride, scores=None)
        # the order of the refusals: the config before the window, the window before the counts, the counts before the pointers
        refused("suppress", "measure", cfg=(5, 32768, 0, 0), window_=window + 7, n=0)
        refused("match", "not out for delivery", window_=window + 7, n=0, a=None)
        refused("suppress", "k 0", k=0, regions=None)
        cfg = L.PipelineOverlapConfig(0, 32768)
        call_s = L.PipelineSuppressRegionsCall(*[ok_s[f] for f in ok_s], None)
        call_m = L.PipelineMatchRegionsCall(*[ok_m[f] for f in ok_m], None)
        lib = pipe.lib
        assert lib.leon_pipeline_suppress_regions_device(pipe.h, window, C.byref(cfg), None) == L.ERR_INVALID and lib.leon_pipeline_match_regions_device(pipe.h, window, C.byref(cfg), None) == L.ERR_INVALID
        assert lib.leon_pipeline_suppress_regions_device(pipe.h, window, None, C.byref(call_s)) == L.ERR_INVALID and lib.leon_pipeline_match_regions_device(pipe.h, window, None, C.byref(call_m)) == L.ERR_INVALID
        assert lib.leon_pipeline_suppress_regions_device(None, window, C.byref(cfg), C.byref(call_s)) == L.ERR_INVALID and lib.leon_pipeline_match_regions_device(None, window, C.byref(cfg), C.byref(call_m)) == L.ERR_INVALID
        torch.cuda.synchronize()
        assert all(bool((x == FILL).all()) for x in ts + tm)
        # the host roads refuse the same, with the caller's arrays as they were
        h_rows = rows.cpu().numpy()
        h = [np.full(s, FILL, dtype=np.int32) for s in ((2, 4, 8), (2, 4), (2, 4), (2,), (2, 4))]
        R, H = h_rows.ctypes.data, [x.ctypes.data for x in h]
        for args in ((window + 7, C.byref(cfg), R, 2, 4, None, 1, *H), (window, None, R, 2, 4, None, 1, *H), (window, C.byref(cfg), None, 2, 4, None, 1, *H),
                     (window, C.byref(cfg), R, 0, 4, None, 1, *H), (window, C.byref(cfg), R, 2, 1025, None, 1, *H), (window, C.byref(cfg), R, 2, 4, None, 9, *H),
                     (window, C.byref(cfg), R, 2, 4, None, 1, H[0], H[1], None, H[3], H[4]), (window, C.byref(cfg), R, 2, 4, None, 1, H[0], H[1], H[2], None, H[4])):
            assert lib.leon_pipeline_suppress_regions(pipe.h, *args) == L.ERR_INVALID
        for args in ((window + 7, C.byref(cfg), R, 4, R, 4, 2, H[1], H[2], H[4], H[3], None, None), (window, C.byref(cfg), None, 4, R, 4, 2, H[1], H[2], H[4], H[3], None, None),
                     (window, C.byref(cfg), R, 0, R, 4, 2, H[1], H[2], H[4], H[3], None, None), (window, C.byref(cfg), R, 4, R, 4, 65536, H[1], H[2], H[4], H[3], None, None),
                     (window, C.byref(cfg), R, 4, R, 4, 2, H[1], None, H[4], H[3], None, None)):
            assert lib.leon_pipeline_match_regions(pipe.h, *args) == L.ERR_INVALID
        assert all((x == FILL).all() for x in h)
        # the optional outputs may be NULL on both roads
        call = L.PipelineSuppressRegionsCall(rows.data_ptr(), None, 2, 4, 1, 0, None, None, ts[2].data_ptr(), ts[3].data_ptr(), None, None)
        assert lib.leon_pipeline_suppress_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK
        assert bool((ts[3] >= 1).all()) and bool((ts[2] != FILL).all()) and all(bool((ts[i] == FILL).all()) for i in (0, 1, 4))
        call = L.PipelineMatchRegionsCall(rows.data_ptr(), rows.data_ptr(), 2, 4, 4, 0, tm[0].data_ptr(), tm[1].data_ptr(), tm[2].data_ptr(), tm[3].data_ptr(), None, None, None)
        assert lib.leon_pipeline_match_regions_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK
        assert tm[0].cpu().numpy().tolist() == [[0, 1, 2, 3]] * 2 and tm[3].cpu().numpy().tolist() == [4, 4] and all(bool((tm[i] == FILL).all()) for i in (4, 5))
        assert lib.leon_pipeline_suppress_regions(pipe.h, window, C.byref(cfg), R, 2, 4, None, 1, None, None, H[2], H[3], None) == L.OK
        assert np.array_equal(h[2], ts[2].cpu().numpy()) and np.array_equal(h[3], ts[3].cpu().numpy()) and all((h[i] == FILL).all() for i in (0, 1, 4))
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()) and len(seen) == 2 * 12 + (3 + 6) + (3 + 6) + (7 + 8) + 6 + 3
