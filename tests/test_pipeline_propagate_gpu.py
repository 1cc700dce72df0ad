"""GPU: dense maps propagated along the motion vectors of delivered windows (include/leon_pipeline.h, leon_pipeline_propagate_maps;
k_propagate) -- for every delivered frame of a window, with random maps in the reference slots: the host road, the device road on a
caller's stream and the device road on the pipeline's own stream, all three exactly equal to leon_ctypes.propagate_map (the header's
text in numpy integers) on the records read_motion gives.  Then the chain a user runs: propagate_maps_gop against the same hops done on
the host, and a mask a torch op wrote, propagated and read on one stream with no host wait between.  Last the decoder's own prediction
as the oracle: in a stream whose P and B pictures are pure full-pel copies of one reference each, the luma plane of each reference
propagated at stride 1 IS the luma plane of the picture, in every sample."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import propagate_cases as M
from test_open_gop import open_stream
from test_pipeline_carry_gpu import run_windows
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import stream

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
FILL = 0xC3B2A190
SINT = {1: np.uint8, 2: np.int16, 4: np.int32}          # what torch takes the bits as
# (stride, element bytes, planes): a map's bytes are a multiple of 4 at 96 x 64 and at 61 x 45
SHAPES = [(1, 1, 4), (4, 2, 3), (16, 4, 2)]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def propagate_window(L, pipe, window, frames, roads=("host", "stream", "null"), shapes=SHAPES):
    """everything of one delivered window: every frame as a target, with both reference slots, with the forward one alone and with
    the backward one alone, on each road"""
    import torch
    n, fw, fh = len(frames), pipe.info.frame_width, pipe.info.frame_height
    records = [pipe.read_motion(window, i)[:2] for i in range(n)]
    r = dict(n=n, keys=[(f["gop"], f["display_index"], f["type"]) for f in frames], runs=[])
    # slots 0 and 1: the references; 2 + 3 i .. 4 + 3 i: frame i's map with both, forward only, backward only; then two refused hops
    hops = [h for i in range(n) for h in ((i, 2 + 3 * i, 0, 1), (i, 3 + 3 * i, 0, -1), (i, 4 + 3 * i, -1, 1))] + [(n, 2, 0, 1), (0, 2, 2, 1)]
    full = np.zeros((len(hops), 8), dtype=np.int32)
    full[:, :4] = hops
    for s, e, planes in shapes:
        maps = M.rand_maps(np.random.default_rng(window * 100 + s), 2 + 3 * n, planes, fw, fh, s, e)
        run = dict(shape=(s, e, planes), want=M.expected(L, fw, fh, n, records, hops, s, maps, FILL))
        if "host" in roads:
            m = np.array(maps, copy=True)
            via, status = pipe.propagate_maps(window, m, hops, s, fill=FILL, via_fill=M.VIA_FILL)
            run["host"] = (m, via, status)

        def tensors():
            return (torch.from_numpy(maps.view(SINT[e]).copy()).cuda(), torch.tensor(full, dtype=torch.int32, device="cuda"),
                    torch.full((len(hops),) + maps.shape[2:], M.VIA_FILL, dtype=torch.uint8, device="cuda"), torch.full((len(hops),), -55, dtype=torch.int32, device="cuda"))
        if "stream" in roads:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                m, h, via, status = tensors()
                got = pipe.propagate_maps_device(window, m, h, s, fill=FILL, via=via, status=status)
                assert got[0].data_ptr() == via.data_ptr() and got[1].data_ptr() == status.data_ptr()
            st.synchronize()
            run["stream"] = (m.cpu().numpy().view(M.UINT[e]), via.cpu().numpy(), status.cpu().numpy())
        if "null" in roads:          # stream NULL: the pipeline's regions stream, and the call waits
            m, h, via, status = tensors()
            torch.cuda.synchronize()
            cfg = L.PipelinePropagateConfig(s, planes, e, maps.shape[0], FILL, 0, maps[0].nbytes, maps.nbytes)
            call = L.PipelinePropagateMapsCall(h.data_ptr(), len(hops), 0, m.data_ptr(), via.data_ptr(), status.data_ptr(), None)
            assert pipe.lib.leon_pipeline_propagate_maps_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
            run["null"] = (m.cpu().numpy().view(M.UINT[e]), via.cpu().numpy(), status.cpu().numpy())
        r["runs"].append(run)
    return r


def assert_window(L, r, what):
    assert r["runs"]
    for run in r["runs"]:
        want = run["want"]
        assert want[2][:-2].tolist() == [0] * (3 * r["n"]) and want[2][-2:].tolist() == [L.REGION_FRAME, L.REGION_SLOT]
        for road in ("host", "stream", "null"):
            if road in run:
                M.assert_equal(run[road], want, "%s, shape %s, %s road" % (what, run["shape"], road))
        # an I picture is all fill; a P picture never goes backward
        for i, k in enumerate(r["keys"]):
            if k[2] == 1:
                assert (want[1][3 * i:3 * i + 3] == 0).all()
            if k[2] == 2:
                assert (want[1][3 * i + 2] == 0).all() and (want[1][3 * i] != 2).all()


@PARSERS
@pytest.mark.parametrize("name", ["ibbp_96x64_coded", "cropped_61x45"])
def test_every_delivered_frame_of_a_window(L, name, gpu_parser):
    data, kw = stream(name)
    got = run_windows(L, data, functools.partial(propagate_window, L), gops_per_window=2, gpu_parser=gpu_parser, **kw)
    assert got
    for window, r in got.items():
        assert_window(L, r, "%s window %d" % (name, window))
        via = r["runs"][0]["want"][1]
        assert {0, 1, 2} <= set(np.unique(via).tolist())


@PARSERS
def test_open_gops(L, gpu_parser):
    data = open_stream(96, 64, 31)[0]
    got = run_windows(L, data, functools.partial(propagate_window, L, shapes=SHAPES[:2]), gops_per_window=1, gpu_parser=gpu_parser)
    assert got
    for window, r in got.items():
        assert_window(L, r, "open GOPs, window %d" % window)


@PARSERS
def test_a_window_held_across_ring_reuse(L, gpu_parser):
    """window 0 held while windows 1 .. 4 reuse the other ring entry: its records and its table still serve"""
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
        r = propagate_window(L, pipe, window, frames, shapes=SHAPES[:2])
        pipe.release_window(window)
        with pytest.raises(L.LeonError):          # released: no longer out for delivery
            pipe.propagate_maps(window, M.rand_maps(np.random.default_rng(0), 3, 1, 96, 64, 4, 1), [(0, 2, 0, 1)], 4)
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_window(L, r, "held window")


@PARSERS
def test_exact_seek_trims_an_anchor(L, gpu_parser):
    """LEON_PIPELINE_SEEK_EXACT onto display position 4 of GOP 3: its I picture is reconstructed and not delivered; the records of the
    frames that are delivered still propagate (the caller vouches for the slots), and propagate_plan reaches nothing through the
    missing anchor"""
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
        pipe = frames[0]["_pipe"]
        r = propagate_window(L, pipe, window, frames, roads=("host", "stream"), shapes=SHAPES[1:2])
        r["plan"] = L.propagate_plan(pipe.carry_refs(window), r["keys"], 0)
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
    assert_window(L, r, "EXACT seek")
    levels, unreachable = r["plan"]          # from the B picture at (3, 4): nothing predicts from a B picture
    assert levels == [] and unreachable == list(range(1, r["n"]))
    for w, other in log:
        assert_window(L, other, "window %d" % w)


def gop_chain_on_the_host(L, fw, fh, records, refs, keys, map_, src, s, fill):
    """propagate_maps_gop's contract with propagate_map: src's row a copy with via 3, the levels of propagate_plan in order, a frame
    out of reach all fill, via 0, NO_REFERENCE"""
    n = len(keys)
    group = [i for i, k in enumerate(keys) if k[0] == keys[src][0]]
    levels, unreachable = L.propagate_plan(refs, keys, src)
    maps = np.zeros((n,) + map_.shape, dtype=map_.dtype)          # slot = window frame
    via, status = np.zeros((n,) + map_.shape[1:], dtype=np.uint8), np.zeros(n, dtype=np.int64)
    maps[src], via[src] = map_, 3
    for u in unreachable:
        maps[u] = np.array([fill & 0xffffffff], dtype="<u4").view(np.uint8)[:map_.dtype.itemsize].view(map_.dtype)[0]
        status[u] = L.REGION_NO_REFERENCE
    for hops in levels:
        for t, f, b in hops:
            st, v = L.propagate_map(fw, fh, n, records, (t, t, f, b), s, maps, fill)
            assert st == 0
            via[t] = v
    return maps[group], via[group], status[group], levels, unreachable, group


@pytest.mark.parametrize("start", ["I", "first P", "last P"])
@pytest.mark.parametrize("name,s,e,planes", [("ibbp_96x64_coded", 4, 2, 3), ("cropped_61x45", 1, 1, 1)])
def test_propagate_maps_gop_against_the_chain_on_the_host(L, name, s, e, planes, start):
    """cropped_61x45 at stride 1 with one plane: a map of 2745 bytes, so the slots of the result lie 2748 bytes apart"""
    import torch
    data, kw = stream(name)

    def work(pipe, window, frames):
        frames = list(frames)
        fw, fh = pipe.info.frame_width, pipe.info.frame_height
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        anchors = [i for i, k in enumerate(keys) if k[2] == (1 if start == "I" else 2)]
        src = anchors[-1] if start != "first P" else anchors[0]
        map_ = M.rand_maps(np.random.default_rng(window), 1, planes, fw, fh, s, e)[0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = pipe.propagate_maps_gop(window, torch.from_numpy(map_.view(SINT[e])).cuda(), src, s, fill=FILL)
        st.synchronize()
        records = [pipe.read_motion(window, i)[:2] for i in range(len(frames))]
        refs = [a.tolist() for a in pipe.carry_refs(window)]
        want = gop_chain_on_the_host(L, fw, fh, records, refs, keys, map_, src, s, FILL)
        return (got[0].cpu().numpy().view(M.UINT[e]), got[1].cpu().numpy(), got[2].cpu().numpy()), want, pipe.gop_frames(window, src), keys, src
    for (got, want, rows, keys, src) in run_windows(L, data, work, gops_per_window=2, gpu_parser=True, **kw).values():
        maps, via, status, levels, unreachable, group = want
        assert rows == group and keys[src][0] == keys[group[0]][0] and len(group) < len(keys)
        M.assert_equal(got, (maps, via, status), "%s from %s" % (name, start))
        assert (unreachable == []) == (start == "I") and sum(len(h) for h in levels) + len(unreachable) == len(group) - 1
        seen = set(np.unique(via).tolist())          # (from a P picture only the B pictures in front of it and the chain behind it: backward first)
        assert (via[group.index(src)] == 3).all() and 2 in seen and (start != "I" or 1 in seen)


def test_a_mask_from_a_torch_op_propagated_and_read_on_one_stream(L):
    """the mask is written by a torch op on a side stream, propagated to every frame of the GOP, and a torch op on that stream reads
    the result -- the host waits once, at the end"""
    import torch
    data = ibbp_stream(96, 64, [9], 47)

    def work(pipe, window, frames):
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        src = [i for i, k in enumerate(keys) if k[2] == 1][0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            yy, xx = torch.meshgrid(torch.arange(32, device="cuda"), torch.arange(48, device="cuda"), indexing="ij")
            mask = ((yy // 3 + 2 * (xx // 5)) % 21).to(torch.uint8)[None]          # the "segmentation": labels 0 .. 20 at stride 2
            maps, via, status = pipe.propagate_maps_gop(window, mask, src, 2, fill=255)
            counts = torch.stack([(maps == label).sum(dim=(1, 2, 3)) for label in range(21)] + [(maps == 255).sum(dim=(1, 2, 3))])          # reads on the stream
        st.synchronize()
        records = [pipe.read_motion(window, i)[:2] for i in range(len(frames))]
        refs = [a.tolist() for a in pipe.carry_refs(window)]
        yy, xx = np.mgrid[0:32, 0:48]
        want = gop_chain_on_the_host(L, 96, 64, records, refs, keys, ((yy // 3 + 2 * (xx // 5)) % 21).astype(np.uint8)[None], src, 2, 255)
        return (maps.cpu().numpy(), via.cpu().numpy(), status.cpu().numpy()), want, counts.cpu().numpy()
    (got, want, counts), = run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()
    M.assert_equal(got, want[:3], "mask")
    assert (want[2] == 0).all() and len(want[3]) == 3
    assert np.array_equal(counts, np.stack([(want[0] == label).sum(axis=(1, 2, 3)) for label in list(range(21)) + [255]])) and (counts.sum(axis=0) == 32 * 48).all()


def test_the_host_road_without_via_and_status_and_on_a_window_that_is_not_out(L):
    data = ibbp_stream(96, 64, [6], 47)

    def work(pipe, window, frames):
        n, s = len(frames), 4
        maps = M.rand_maps(np.random.default_rng(7), 2 + n, 2, 96, 64, s, 2)
        h = L._records_array([(t, 2 + t, 0, 1) for t in range(n)] + [(n, 2, 0, 1)])
        want = maps.copy()
        via, status = pipe.propagate_maps(window, want, h, s, fill=0x3C00)
        assert (status[:-1] == 0).all() and status[-1] == L.REGION_FRAME and not np.array_equal(want, maps)
        got, cfg = maps.copy(), L._propagate_config(maps, s, 0x3C00)
        assert pipe.lib.leon_pipeline_propagate_maps(pipe.h, window, C.byref(cfg), h.ctypes.data, len(h), got.ctypes.data, None, None) == L.OK, pipe.lib.leon_last_error()
        assert np.array_equal(got, want)
        # a window that is not out for delivery: refused before anything is allocated or uploaded, the caller's arrays as they were
        got, v, st = maps.copy(), np.full_like(via, M.VIA_FILL), np.full(len(h), -55, np.int32)
        assert pipe.lib.leon_pipeline_propagate_maps(pipe.h, window + 7, C.byref(cfg), h.ctypes.data, len(h), got.ctypes.data, v.ctypes.data, st.ctypes.data) == L.ERR_INVALID
        assert pipe.lib.leon_last_error() == b"window %d is not out for delivery" % (window + 7)
        assert np.array_equal(got, maps) and (v == M.VIA_FILL).all() and (st == -55).all()
        return True
    got = run_windows(L, data, work, gops_per_window=1, gpu_parser=True)
    assert got and all(got.values())


def test_the_call_is_refused_as_a_whole(L):
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    seen = []

    def work(pipe, window, frames):
        s, e, planes, slots = 4, 2, 2, 4
        maps = torch.full((slots, planes, 16, 24), 0x1234, dtype=torch.int16, device="cuda")
        hops = torch.tensor([[1, 2, 0, 1, 0, 0, 0, 0], [2, 3, 0, 1, 0, 0, 0, 0]], dtype=torch.int32, device="cuda")
        via = torch.full((2, 16, 24), M.VIA_FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        slot_bytes = planes * 16 * 24 * e
        ok_cfg = dict(stride=s, planes=planes, elem_bytes=e, n_slots=slots, fill=0, reserved0=0, slot_pitch_bytes=slot_bytes, maps_bytes=slots * slot_bytes)
        ok = dict(hops=hops.data_ptr(), n=2, reserved0=0, maps=maps.data_ptr(), device_via=via.data_ptr(), device_status=status.data_ptr())

        def refused(word, window_=window, reserved=(0, 0), cfg=None, null_cfg=False, **kw):
            a, c = dict(ok, **kw), dict(ok_cfg, **(cfg or {}))
            call = L.PipelinePropagateMapsCall(a["hops"], a["n"], a["reserved0"], a["maps"], a["device_via"], a["device_status"], None, (C.c_uint64 * 2)(*reserved))
            config = L.PipelinePropagateConfig(c["stride"], c["planes"], c["elem_bytes"], c["n_slots"], c["fill"], c["reserved0"], c["slot_pitch_bytes"], c["maps_bytes"])
            rc = pipe.lib.leon_pipeline_propagate_maps_device(pipe.h, window_, None if null_cfg else C.byref(config), C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert bool((maps == 0x1234).all()) and bool((via == M.VIA_FILL).all()) and bool((status == -55).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        # the carry call's refusals
        refused("not out for delivery", window_=window + 7)
        refused("null hops", hops=None)
        refused("null maps", maps=None)
        refused("4-byte aligned", hops=hops.data_ptr() + 2)
        refused("4-byte aligned", maps=maps.data_ptr() + 2)
        refused("4-byte aligned", device_via=via.data_ptr() + 1)
        refused("4-byte aligned", device_status=status.data_ptr() + 3)
        refused("0 hops", n=0)
        refused("65536 hops", n=65536)
        refused("-1 hops", n=-1)
        refused("reserved word of the call", reserved0=1)
        refused("reserved word of the call", reserved=(1, 0))
        refused("reserved word of the call", reserved=(0, 1))
        # the maps' own
        refused("null cfg", null_cfg=True)
        for stride in (0, 3, 32, -1):
            refused("stride", cfg=dict(stride=stride))
        for elem in (0, 3, 8):
            refused("elem_bytes", cfg=dict(elem_bytes=elem))
        for p in (0, 4097):
            refused("planes", cfg=dict(planes=p))
        for n_slots in (0, 65536):
            refused("slots", cfg=dict(n_slots=n_slots))
        refused("slot_pitch_bytes", cfg=dict(slot_pitch_bytes=slot_bytes - 4))
        refused("slot_pitch_bytes", cfg=dict(slot_pitch_bytes=slot_bytes + 2))
        refused("maps_bytes", cfg=dict(maps_bytes=slots * slot_bytes - 1))
        refused("maps_bytes", cfg=dict(slot_pitch_bytes=slot_bytes + 4))
        refused("reserved word of cfg", cfg=dict(reserved0=1))
        assert pipe.lib.leon_pipeline_propagate_maps_device(pipe.h, window, None, None) == L.ERR_INVALID
        # the host road refuses the same; a record's fault is no refusal
        host = np.full((slots, planes, 16, 24), 0x1234, dtype=np.uint16)
        hh = np.array([[1, 2, 0, 1, 0, 0, 0, 0]], dtype=np.int32)
        config = L.PipelinePropagateConfig(s, planes, e, slots, 0, 0, slot_bytes, slots * slot_bytes)
        for args in ((window + 7, C.byref(config), hh.ctypes.data, 1, host.ctypes.data), (window, None, hh.ctypes.data, 1, host.ctypes.data),
                     (window, C.byref(config), None, 1, host.ctypes.data), (window, C.byref(config), hh.ctypes.data, 1, None),
                     (window, C.byref(config), hh.ctypes.data, 0, host.ctypes.data), (window, C.byref(config), hh.ctypes.data, 65536, host.ctypes.data)):
            assert pipe.lib.leon_pipeline_propagate_maps(pipe.h, *args, None, None) == L.ERR_INVALID
        assert (host == 0x1234).all()
        v, st_ = pipe.propagate_maps(window, host, [(99, 2, 0, 1), (1, 2, 2, 1), (1, 2, 0, 1)], s, via_fill=M.VIA_FILL)
        assert st_.tolist() == [L.REGION_FRAME, L.REGION_SLOT, 0] and (v[:2] == M.VIA_FILL).all() and (v[2] != M.VIA_FILL).all() and (host[3] == 0x1234).all()
        # via and status may be NULL
        call = L.PipelinePropagateMapsCall(hops.data_ptr(), 2, 0, maps.data_ptr(), None, None, None)
        assert pipe.lib.leon_pipeline_propagate_maps_device(pipe.h, window, C.byref(config), C.byref(call)) == L.OK
        assert bool((via == M.VIA_FILL).all()) and bool((status == -55).all()) and bool((maps[:2] == 0x1234).all())
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True).values()) and len(seen) == 30
    # a pipeline without the MOTION bit
    refusals = []

    def no_motion(window, frames):
        pipe = frames[0]["_pipe"]
        z = np.zeros(4 * 2 * 16 * 24, dtype=np.int32)
        config = L.PipelinePropagateConfig(4, 2, 2, 4, 0, 0, 1536, 6144)
        call = L.PipelinePropagateMapsCall(z.ctypes.data, 1, 0, z.ctypes.data, None, None, None)
        refusals.append(pipe.lib.leon_pipeline_propagate_maps_device(pipe.h, window, C.byref(config), C.byref(call)))
        refusals.append(pipe.lib.leon_pipeline_propagate_maps(pipe.h, window, C.byref(config), z.ctypes.data, 1, z.ctypes.data, None, None))
    pipe = L.Pipeline(data, on_window=no_motion, gops_per_window=1, output="tensor")
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert refusals and all(rc == L.ERR_INVALID for rc in refusals)


def copy_stream(cw, ch, gops, seed):
    """like ibbp_stream, with P and B pictures that are pure copies: no intra macroblock, no coefficients, one direction per B picture,
    every vector full-pel -- the prediction is then a copy of reference samples and there is no residual"""
    import jsv_writer as W
    import synth as S
    rng = np.random.default_rng(seed)
    pics, starts = [], []
    for n in gops:
        starts.append(len(pics))
        k = 0
        for ptype, disp, f, b in S.gop_ibbp(n):
            if ptype == S.PIC_I:
                t = S.make_picture(rng, cw, ch, ptype)
            else:
                force = None
                if ptype == S.PIC_B:
                    force = 2 if f is None else 1 + k % 2
                    k += 1
                t = S.make_picture(rng, cw, ch, ptype, intra_frac=0, uncoded_frac=1.0, force_dir=force)
                for key in ("mv_fwd", "mv_bwd"):
                    if key in t:
                        t[key] &= ~1
            t["display"] = disp
            pics.append(t)
    return W.write_stream(pics, cw, ch, cw, ch, gop_starts=starts)[0]


@pytest.mark.parametrize("cw,ch,gop,seed", [(96, 64, 6, 51), (64, 48, 9, 52), (352, 240, 6, 53)])
def test_the_decoders_own_prediction_is_the_oracle(L, cw, ch, gop, seed):
    """With full-pel vectors, one direction and no residual the decoder's prediction of a P or B picture is a copy of its reference's
    samples along the vectors: the delivered luma plane of each reference, propagated with s = 1 and e = 1 through the picture's
    record, equals the picture's delivered luma plane in EVERY sample.  (Checked on the CPU against the oracle's planes when this was
    written: 96 x 64 IBBP-6, 64 x 48 IBBP-9 and 352 x 240 IBBP-6 gave 0 differing samples over 18 pictures and 1802 moving
    macroblocks.)"""
    data = copy_stream(cw, ch, [gop], seed)

    def work(pipe, window, frames):
        frames = list(frames)
        n = len(frames)
        luma = [pipe.read_planes(f)[0] for f in frames]
        records = [pipe.read_motion(window, i) for i in range(n)]
        fwd, bwd = [a.tolist() for a in pipe.carry_refs(window)]
        out = []
        for t in range(n):
            if frames[t]["type"] == 1:
                continue
            mv, info, _ = records[t]
            maps = np.zeros((3, 1, ch, cw), dtype=np.uint8)
            if fwd[t] >= 0:
                maps[0, 0] = luma[fwd[t]]
            if bwd[t] >= 0:
                maps[1, 0] = luma[bwd[t]]
            maps[2] = 0x5A
            via, status = pipe.propagate_maps(window, maps, [(t, 2, 0 if fwd[t] >= 0 else -1, 1 if bwd[t] >= 0 else -1)], 1, fill=0x5A)
            out.append(dict(t=t, type=frames[t]["type"], status=int(status[0]), intra=int((info & 4).astype(bool).sum()), moving=int((mv != 0).any(axis=2).sum()),
                            filled=int((via == 0).sum()), differ=int((maps[2, 0] != luma[t]).sum()), odd=int((mv & 1).astype(bool).sum())))
        return out
    (out,) = run_windows(L, data, work, gops_per_window=1, gpu_parser=True, output="ycbcr").values()
    assert len(out) == gop - 1 and {o["type"] for o in out} == {2, 3}
    # the premise: no intra macroblock, full-pel vectors, and macroblocks that move
    assert all(o["status"] == 0 and o["intra"] == 0 and o["filled"] == 0 and o["odd"] == 0 for o in out), out
    assert sum(o["moving"] for o in out) > len(out) * (cw // 16) * (ch // 16) // 2, out
    for o in out:
        print("frame %d (type %d): %d moving macroblocks, %d samples differ" % (o["t"], o["type"], o["moving"], o["differ"]))
    assert all(o["differ"] == 0 for o in out), out
