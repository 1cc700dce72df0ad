"""GPU: boxes carried along the motion vectors of delivered windows (include/leon_pipeline.h, leon_pipeline_carry_regions; k_carry) --
for every pair of delivered frames of a window, out, votes and status of the host road, of the device road on a caller's stream and of
the device road on the pipeline's own stream, all three exactly equal to leon_ctypes.carry_box (the header's text in Python integers)
on the records read_motion gives and the references carry_refs gives; the references themselves against an independent look-up.
Then the chain a user runs: carry_regions_gop against the same hops done on the host, and boxes a torch op wrote, carried and
resampled on one stream with no host wait between."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import carry_cases as K
from test_open_gop import open_stream
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
    return [(0, 0, fw, fh), (fw // 3, fh // 4, fw // 2, fh // 2), (fw - 1, fh - 1, 1, 1), (5, 7, 12, 10)]


def refs_by_lookup(frames):
    """the header's resolution rule with a dictionary: independent of the library"""
    at = {(f["gop"], f["display_index"]): i for i, f in enumerate(frames)}
    fwd = [at.get((f["motion"]["fwd_gop"], f["motion"]["fwd_display"]), -1) if f["motion"]["fwd_display"] >= 0 else -1 for f in frames]
    bwd = [at.get((f["gop"], f["motion"]["bwd_display"]), -1) if f["motion"]["bwd_display"] >= 0 else -1 for f in frames]
    return fwd, bwd


def carry_window(L, pipe, window, frames, roads=("host", "stream", "null")):
    """everything of one delivered window: the references three ways, and every (S, T) pair with four boxes on each road"""
    import torch
    frames = list(frames)
    n, fw, fh = len(frames), pipe.info.frame_width, pipe.info.frame_height
    records = [pipe.read_motion(window, i)[:2] for i in range(n)]
    fwd, bwd = pipe.carry_refs(window)
    r = dict(n=n, keys=[(f["gop"], f["display_index"], f["type"]) for f in frames], fwd=fwd.tolist(), bwd=bwd.tolist(), lookup=refs_by_lookup(frames),
             host_refs=[a.tolist() for a in L.carry_refs(frames, [f["motion"] for f in frames])])
    regions = [(s, x, y, w, h, t) for s in range(n) for t in range(n) for (x, y, w, h) in boxes_of(fw, fh)]
    r["regions"] = regions
    r["want"] = K.expected(L, fw, fh, records, regions, FILL, fwd, bwd, n)
    if "host" in roads:
        r["host"] = pipe.carry_regions(window, regions, fill=FILL)
    full = np.zeros((len(regions), 8), dtype=np.int32)
    full[:, :6] = regions

    def tensors():
        return (torch.tensor(full, dtype=torch.int32, device="cuda"), torch.full((len(regions), 8), FILL, dtype=torch.int32, device="cuda"),
                torch.full((len(regions), 4), FILL, dtype=torch.int32, device="cuda"), torch.full((len(regions),), FILL, dtype=torch.int32, device="cuda"))
    if "stream" in roads:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            rec, out, votes, status = tensors()
            got = pipe.carry_regions_device(window, rec, out=out, votes=votes, status=status)
            assert got[0].data_ptr() == out.data_ptr() and got[2].data_ptr() == status.data_ptr()
        st.synchronize()
        r["stream"] = tuple(t.cpu().numpy() for t in (out, votes, status))
    if "null" in roads:          # stream NULL: the pipeline's regions stream, and the call waits
        rec, out, votes, status = tensors()
        torch.cuda.synchronize()
        call = L.PipelineCarryRegionsCall(rec.data_ptr(), len(regions), 0, out.data_ptr(), votes.data_ptr(), status.data_ptr(), None)
        assert pipe.lib.leon_pipeline_carry_regions_device(pipe.h, window, C.byref(call)) == L.OK, pipe.lib.leon_last_error()
        r["null"] = tuple(t.cpu().numpy() for t in (out, votes, status))
    return r


def assert_window(r, what):
    assert (r["fwd"], r["bwd"]) == r["lookup"], (what, "get_carry_refs", r["keys"])
    assert tuple(r["host_refs"]) == r["lookup"], (what, "carry_refs", r["keys"])
    for road in ("host", "stream", "null"):
        if road in r:
            K.assert_equal(r[road], r["want"], r["regions"], "%s, %s road" % (what, road))


def run_windows(L, data, work, **kw):
    """work(pipe, window, frames) inside the callback of every window; its results by window"""
    kw.setdefault("parser_threads", 2)
    got = {}

    def on_window(window, frames):
        got[window] = work(frames[0]["_pipe"], window, frames)
    pipe = L.Pipeline(data, on_window=on_window, motion=True, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return got


@PARSERS
@pytest.mark.parametrize("name", ["ibbp_96x64_coded", "cropped_61x45", "ibbp_352x240"])
def test_every_pair_of_a_window(L, name, gpu_parser):
    data, kw = stream(name)
    got = run_windows(L, data, functools.partial(carry_window, L), gops_per_window=2, gpu_parser=gpu_parser, **kw)
    assert got
    for window, r in got.items():
        assert_window(r, "%s window %d" % (name, window))
        status, votes = r["want"][2], r["want"][1]
        assert (status == 0).any() and (status == L.REGION_NO_REFERENCE).any()
        assert (votes[status == 0][:, 2:] != 0).any(), "no box of the window moved"
        # a closed GOP's leading B pictures name their I picture for both directions
        lead = [i for i, k in enumerate(r["keys"]) if k[2] == 3 and r["fwd"][i] == r["bwd"][i] >= 0]
        assert lead


@PARSERS
@pytest.mark.parametrize("gops_per_window", [1, 2])
def test_open_gops(L, gops_per_window, gpu_parser):
    """a leading B picture of an open GOP points forward into the GOP before: with one GOP a window that picture is in no window with
    it (fwd -1, and nothing joins the two GOPs); with two it is resolved and the hop across the GOP border votes with D = 1"""
    data = open_stream(96, 64, 31)[0]
    got = run_windows(L, data, functools.partial(carry_window, L, roads=("host", "stream")), gops_per_window=gops_per_window, gpu_parser=gpu_parser)
    across = 0
    for window, r in got.items():
        assert_window(r, "open GOPs, %d a window, window %d" % (gops_per_window, window))
        gop = [k[0] for k in r["keys"]]
        for (s, x, y, w, h, t), st in zip(r["regions"], r["want"][2]):
            if gop[s] != gop[t]:
                across += st == 0
                assert st in (0, L.REGION_NO_REFERENCE)
        if gops_per_window == 1:
            assert len(set(gop)) == 1
    assert (across > 0) == (gops_per_window == 2)


@PARSERS
def test_a_window_held_across_ring_reuse(L, gpu_parser):
    """window 0 held while windows 1 .. 4 reuse the other ring entry: its records and its table still carry exactly"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    held, done = [], threading.Event()

    def on_window(window, frames):
        if window == 0:
            held.append((window, list(frames)))
            return False
        if window == 4:
            done.set()
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=1, windows_in_flight=2, gpu_parser=gpu_parser, parser_threads=2)
    try:
        assert done.wait(60), "windows 1 .. 4 were not delivered while window 0 was held"
        window, frames = held[0]
        r = carry_window(L, pipe, window, frames)
        pipe.release_window(window)
        with pytest.raises(L.LeonError):          # released: no longer out for delivery
            pipe.carry_regions(window, [(0, 0, 0, 8, 8, 1)])
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_window(r, "held window")
    assert (r["want"][2] == 0).sum() > r["n"] * 4


@PARSERS
def test_exact_seek_trims_an_anchor(L, gpu_parser):
    """LEON_PIPELINE_SEEK_EXACT onto display position 4 of GOP 3: its I picture is reconstructed and not delivered, so what pointed into it
    points nowhere (-1) and those hops are NO_REFERENCE, while the P picture behind still joins its neighbours"""
    import leon_vlc_ctypes as V
    data = open_stream(96, 64, 31)[0]
    st = V.Stream(data, threads=1)
    gop_ts, g = {}, -1
    while True:
        p = st.next_picture()
        if p is None:
            break
        if p["type"] == 1:
            g += 1
            gop_ts[g] = p["ts"]
    st.close()
    t = (gop_ts[3] + 40.0 * 4 + 1.0) / 1000.0
    lock, log = threading.Lock(), []

    def on_window(window, frames):
        r = carry_window(L, frames[0]["_pipe"], window, frames, roads=("host", "stream"))
        with lock:
            log.append((window, r))
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=1, gpu_parser=gpu_parser, parser_threads=2)
    try:
        pipe.wait()
        first = pipe.seek(t, exact=True)
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    (r,) = [r for w, r in log if w == first]
    assert r["keys"][0][:2] == (3, 4) and (3, 2) not in [k[:2] for k in r["keys"]]
    assert_window(r, "EXACT seek")
    at = {k[:2]: i for i, k in enumerate(r["keys"])}
    assert r["fwd"][at[(3, 4)]] == -1 and r["bwd"][at[(3, 4)]] == at[(3, 5)] and r["fwd"][at[(3, 5)]] == -1 and r["fwd"][at[(3, 8)]] == at[(3, 5)]
    for w, other in log:
        assert_window(other, "window %d" % w)


def gop_chain_on_the_host(L, fw, fh, records, refs, keys, boxes, src):
    """carry_regions_gop's contract with carry_box: zero-filled outputs, NO_REFERENCE where no hop arrives, a failed hop an empty box"""
    n, m = len(keys), len(boxes)
    levels, unreachable = L.carry_plan(refs, keys, src)
    rec, votes, status = np.zeros((n, m, 8), np.int64), np.zeros((n, m, 4), np.int64), np.full((n, m), L.REGION_NO_REFERENCE, np.int64)
    rec[src, :, 0], rec[src, :, 1:5], status[src] = src, boxes, 0
    for hops in levels:
        for a, b in hops:
            for k in range(m):
                st, o, v = L.carry_box(fw, fh, n, refs[0], refs[1], records, [a] + rec[a, k, 1:5].tolist() + [b, 0, 0])
                status[b, k] = st
                rec[b, k], votes[b, k] = (o, v) if st == 0 else (0, 0)
    return rec, votes, status, levels, unreachable


@pytest.mark.parametrize("start", ["I", "last P"])
def test_carry_regions_gop_against_the_chain_on_the_host(L, start):
    import torch
    data, kw = stream("ibbp_352x240")
    boxes = np.array([[100, 60, 120, 90], [0, 0, 352, 240], [300, 200, 52, 40], [17, 33, 64, 48], [351, 239, 1, 1]], dtype=np.int32)

    def work(pipe, window, frames):
        frames = list(frames)
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        src = [i for i, k in enumerate(keys) if k[2] == (1 if start == "I" else 2)][-1]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = pipe.carry_regions_gop(window, torch.tensor(boxes, device="cuda"), src)
        st.synchronize()
        records = [pipe.read_motion(window, i)[:2] for i in range(len(frames))]
        refs = [a.tolist() for a in pipe.carry_refs(window)]
        return tuple(t.cpu().numpy() for t in got), gop_chain_on_the_host(L, pipe.info.frame_width, pipe.info.frame_height, records, refs, keys, boxes, src), keys
    (got, want, keys), = run_windows(L, data, work, gops_per_window=1, gpu_parser=True, **kw).values()
    rec, votes, status, levels, unreachable = want
    assert unreachable == [] and sum(len(h) for h in levels) == len(keys) - 1 and (status == 0).all()
    assert got[0].shape == (len(keys), len(boxes), 8) and got[1].shape == (len(keys), len(boxes), 4) and got[2].shape == (len(keys), len(boxes))
    assert np.array_equal(got[2], status) and np.array_equal(got[0], rec) and np.array_equal(got[1], votes)
    assert (votes[:, :, 2:] != 0).any(), "no box moved along the GOP"


def test_carry_regions_gop_with_frames_out_of_reach(L):
    """one open GOP a window: frames of the window that no chain reaches keep zeros and NO_REFERENCE (here: none of GOP 4's are out of
    reach from its I picture, its leading B pictures go through their backward reference; from a leading B picture only the I picture's
    chain is)"""
    import torch
    data = open_stream(96, 64, 31)[0]
    boxes = np.array([[10, 10, 40, 30], [0, 0, 96, 64]], dtype=np.int32)

    def work(pipe, window, frames):
        frames = list(frames)
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        out = {}
        for src in {0, [i for i, k in enumerate(keys) if k[2] == 1][0]}:
            got = pipe.carry_regions_gop(window, torch.tensor(boxes, device="cuda"), src)
            torch.cuda.synchronize()
            records = [pipe.read_motion(window, i)[:2] for i in range(len(frames))]
            refs = [a.tolist() for a in pipe.carry_refs(window)]
            out[src] = (tuple(t.cpu().numpy() for t in got), gop_chain_on_the_host(L, 96, 64, records, refs, keys, boxes, src)[:3])
        return out
    for window, by_src in run_windows(L, data, work, gops_per_window=1, gpu_parser=True).items():
        for src, (got, want) in by_src.items():
            for g, w, name in zip(got, want, ("records", "votes", "status")):
                assert np.array_equal(g, w), (window, src, name)


def test_boxes_from_a_torch_op_carried_and_resampled_on_one_stream(L):
    """output tensor + motion: the boxes are written by a torch op on a side stream, carried to every frame of the GOP, and the OUT
    records of each frame go straight into resample_regions_device on that stream -- the host waits once, at the end.  The batch equals
    read_regions of the boxes the host computes with carry_box"""
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    size = (16, 24)
    base = np.array([[8, 4, 40, 30], [30, 20, 50, 40], [0, 0, 96, 64]], dtype=np.int32)

    def work(pipe, window, frames):
        frames = list(frames)
        n = len(frames)
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        src = [i for i, k in enumerate(keys) if k[2] == 1][0]
        fwd, bwd = [a.tolist() for a in pipe.carry_refs(window)]
        targets = [t for t in range(n) if t != src and (fwd[t] == src or bwd[t] == src)]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            half = torch.tensor(base // 2, device="cuda")
            boxes = half * 2          # the "detector": a torch op on this stream
            rec = torch.zeros((len(targets) * len(base), 8), dtype=torch.int32, device="cuda")
            rec[:, 0] = src
            rec[:, 1:5] = boxes.repeat(len(targets), 1)
            rec[:, 5] = torch.tensor(targets, dtype=torch.int32, device="cuda").repeat_interleave(len(base))
            out, votes, status = pipe.carry_regions_device(window, rec)
            batch, rstatus = pipe.resample_regions_device(window, out, size)
        st.synchronize()
        records = [pipe.read_motion(window, i)[:2] for i in range(n)]
        moved = []
        for t in targets:
            for b in (base // 2 * 2).tolist():
                s, o, v = L.carry_box(96, 64, n, fwd, bwd, records, [src] + b + [t, 0, 0])
                assert s == 0
                moved.append(tuple(o[:5]))
        want = pipe.read_regions(window, moved, size)
        return batch.cpu().numpy(), want, status.cpu().numpy(), rstatus.cpu().numpy(), out.cpu().numpy()[:, :5].tolist(), moved
    (batch, want, status, rstatus, out, moved), = run_windows(L, data, work, gops_per_window=1, gpu_parser=True, output="tensor").values()
    assert (status == 0).all() and (rstatus == 0).all() and [tuple(o) for o in out] == moved and len(moved) >= 9
    assert batch.shape == want.shape and np.array_equal(batch.view(np.uint16), want.view(np.uint16))


def test_the_host_road_without_votes_and_status_and_on_a_window_that_is_not_out(L):
    data = ibbp_stream(96, 64, [6], 47)

    def work(pipe, window, frames):
        n = len(frames)
        r = L._records_array([(s, 9, 5, 70, 50, t) for s in range(n) for t in range(n)] + [(n, 1, 1, 8, 8, 0)])
        want, _, status = pipe.carry_regions(window, r, fill=FILL)
        assert (status == 0).any() and status[-1] == L.REGION_FRAME
        out, votes, st = np.full_like(want, FILL), np.full((len(r), 4), FILL, np.int32), np.full(len(r), FILL, np.int32)
        assert pipe.lib.leon_pipeline_carry_regions(pipe.h, window, r.ctypes.data, len(r), out.ctypes.data, None, None) == L.OK, pipe.lib.leon_last_error()
        assert np.array_equal(out, want)
        # a window that is not out for delivery: refused before anything is allocated or uploaded, the caller's arrays as they were
        out[:] = FILL
        assert pipe.lib.leon_pipeline_carry_regions(pipe.h, window + 7, r.ctypes.data, len(r), out.ctypes.data, votes.ctypes.data, st.ctypes.data) == L.ERR_INVALID
        assert pipe.lib.leon_last_error() == b"window %d is not out for delivery" % (window + 7)
        assert (out == FILL).all() and (votes == FILL).all() and (st == FILL).all()
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
        rec[:, 5] = 2
        out = torch.full((4, 8), FILL, dtype=torch.int32, device="cuda")
        votes = torch.full((4, 4), FILL, dtype=torch.int32, device="cuda")
        status = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok = dict(regions=rec.data_ptr(), n=4, reserved0=0, device_out=out.data_ptr(), device_votes=votes.data_ptr(), device_status=status.data_ptr())

        def refused(word, window_=window, reserved=(0, 0), **kw):
            a = dict(ok, **kw)
            call = L.PipelineCarryRegionsCall(a["regions"], a["n"], a["reserved0"], a["device_out"], a["device_votes"], a["device_status"], None, (C.c_uint64 * 2)(*reserved))
            rc = pipe.lib.leon_pipeline_carry_regions_device(pipe.h, window_, C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert bool((out == FILL).all()) and bool((votes == FILL).all()) and bool((status == FILL).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        refused("not out for delivery", window_=window + 7)
        refused("null regions", regions=None)
        refused("null device_out", device_out=None)
        refused("4-byte aligned", regions=rec.data_ptr() + 2)
        refused("4-byte aligned", device_out=out.data_ptr() + 1)
        refused("4-byte aligned", device_votes=votes.data_ptr() + 2)
        refused("4-byte aligned", device_status=status.data_ptr() + 3)
        refused("0 regions", n=0)
        refused("65536 regions", n=65536)
        refused("-1 regions", n=-1)
        refused("reserved word", reserved0=1)
        refused("reserved word", reserved=(1, 0))
        refused("reserved word", reserved=(0, 1))
        assert pipe.lib.leon_pipeline_carry_regions_device(pipe.h, window, None) == L.ERR_INVALID
        # the host road refuses the same; a record's fault is no refusal
        host = np.zeros((2, 8), dtype=np.int32)
        o, v, s = np.zeros((2, 8), np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
        for args in ((window + 7, host.ctypes.data, 2, o.ctypes.data), (window, None, 2, o.ctypes.data), (window, host.ctypes.data, 2, None),
                     (window, host.ctypes.data, 0, o.ctypes.data), (window, host.ctypes.data, 65536, o.ctypes.data)):
            assert pipe.lib.leon_pipeline_carry_regions(pipe.h, args[0], args[1], args[2], args[3], v.ctypes.data, s.ctypes.data) == L.ERR_INVALID
        o, v, s = pipe.carry_regions(window, [(0, 0, 0, 0, 0, 1), (99, 0, 0, 8, 8, 1), (0, 0, 0, 8, 8, 0)], fill=FILL)
        assert s.tolist() == [L.REGION_BOX, L.REGION_FRAME, 0] and (o[:2] == FILL).all() and o[2].tolist() == [0, 0, 0, 8, 8, 0, 0, 0]
        # votes and status may be NULL
        call = L.PipelineCarryRegionsCall(rec.data_ptr(), 4, 0, out.data_ptr(), None, None, None)
        assert pipe.lib.leon_pipeline_carry_regions_device(pipe.h, window, C.byref(call)) == L.OK
        assert bool((out[:, 0] == 2).all()) and bool((votes == FILL).all()) and bool((status == FILL).all())
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()) and len(seen) == 13
    # a pipeline without the MOTION bit
    refusals = []

    def no_motion(window, frames):
        pipe = frames[0]["_pipe"]
        z = np.zeros(64, dtype=np.int32)
        call = L.PipelineCarryRegionsCall(z.ctypes.data, 1, 0, z.ctypes.data, None, None, None)
        refusals.append(pipe.lib.leon_pipeline_carry_regions_device(pipe.h, window, C.byref(call)))
        refusals.append(pipe.lib.leon_pipeline_carry_regions(pipe.h, window, z.ctypes.data, 1, z.ctypes.data, None, None))
        refusals.append(pipe.lib.leon_pipeline_get_carry_refs(pipe.h, window, z.ctypes.data, z.ctypes.data, len(frames)))
    pipe = L.Pipeline(data, on_window=no_motion, gops_per_window=1, output="tensor")
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        with pytest.raises(L.LeonError):
            pipe.carry_refs(0)
    finally:
        pipe.close()
    assert refusals and all(rc == L.ERR_INVALID for rc in refusals)
