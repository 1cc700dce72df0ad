"""GPU: the pipeline's ACTIVITY output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_ACTIVITY; k_activity, k_activity_summary) --
every delivered frame's activity record, every window, against leon_ctypes.activity_from_lists of the HOST front end's lists
(leon_vlc_ctypes.Stream), both parts exactly, through both front ends: the GPU front end writes entries with level 0 and reserves more
than it fills, the host one does neither, and the record is the same.  Which pictures are delivered is what
test_pipeline_motion_gpu.expected_motion says (dropped leading B pictures and what an EXACT seek trims have no record).
The streams: 24 macroblocks in one task a row (96 x 64, also as yuva with its A groups behind Cr), 330 in three tasks a row with a
partly filled last chroma group (352 x 240), 74 in five tasks a row (592 x 32: 37 macroblocks, the last luma and chroma groups partly
filled), and 1025 in six tasks a row with the missing luma group 2c + 1 (656 x 400: 41 macroblocks, 11 luma groups)."""
import functools
import os
import threading

import numpy as np
import pytest

from helpers import ROOT
from test_open_gop import open_stream
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import expected_motion

pytestmark = pytest.mark.gpu

STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
PARSERS = pytest.mark.parametrize("gpu_parser", [None, -1], ids=["gpu-parser", "host-parser"])          # the default, and -1
NAMES = ["ibbp_96x64", "leon_synth_352x240", "syntax_escape_ip_592x32", "yuva_ibbp_96x64", "ibbp_656x400"]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def parser_kw(gpu_parser):
    return dict(gpu_parser=None if gpu_parser is None else False)


@functools.lru_cache(maxsize=None)
def stream(name):
    if name == "ibbp_656x400":
        return ibbp_stream(656, 400, [6], 45)
    if name == "open":
        return open_stream(96, 64, 31)[0]
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


def expected_activity(data, first_gop=0):
    """({(gop, display_index): (cells, summary)} of the pictures a run from key-map entry first_gop delivers, (mbw, mbh), the motion
    records of the same pictures): the host front end's lists through activity_from_lists, built once per stream and left unchanged"""
    import leon_ctypes as L_
    import leon_vlc_ctypes as V
    motion, grid = expected_motion(data, first_gop)
    st = V.Stream(data, threads=1)
    out, gop = {}, -1
    while True:
        p = st.next_picture()
        if p is None:
            break
        if p["type"] == 1:
            gop += 1
        key = (gop, p["temporal_reference"])
        if key in motion:
            out[key] = L_.activity_from_lists(grid[0], grid[1], p["grp_off"], p["entries"], p["qscale"])
    st.close()
    assert set(out) == set(motion)
    return out, grid, motion


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_activity(stream(name))


def run_activity(L, data, **kw):
    """{(gop, display_index): (cells, summary)} as the pipeline delivers them, the activity layout, the motion records where asked for"""
    kw.setdefault("parser_threads", 2)
    got, motion = {}, {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        records = pipe.window_activity(window, len(frames))
        for f in frames:
            assert f["activity"] and f["activity"] % 256 == 0 and records[f["_i"]] == f["activity"]
            key = (f["gop"], f["display_index"])
            assert key not in got
            got[key] = pipe.read_activity(window, f["_i"])
            if f["motion"] is not None:
                motion[key] = pipe.read_motion(window, f["_i"])
    pipe = L.Pipeline(data, on_window=on_window, activity=True, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        assert pipe.info.output & L.PIPELINE_OUTPUT_ACTIVITY
        lay = pipe.activity_layout
    finally:
        pipe.close()
    return got, lay, motion


def assert_activity(got, want, what=""):
    assert sorted(got) == sorted(want), "%s: delivered and not expected %s, expected and missing %s" % (
        what, sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for k in sorted(want):
        (cells, s), (wc, ws) = got[k], want[k]
        assert cells.shape == wc.shape and cells.dtype == wc.dtype and s.dtype == np.uint32
        bad = np.argwhere(cells != wc)
        assert not len(bad), "%s: frame %s: cells differ at macroblocks %s: %s, expected %s" % (what, k, bad[:6].tolist(), cells[cells != wc][:6].tolist(), wc[cells != wc][:6].tolist())
        assert s.tolist() == ws.tolist(), "%s: frame %s: summary %s, expected %s" % (what, k, s.tolist(), ws.tolist())


@PARSERS
@pytest.mark.parametrize("name,mbs", list(zip(NAMES, [(6, 4), (22, 15), (37, 2), (6, 4), (41, 25)])))
def test_records_equal_the_definition(L, name, mbs, gpu_parser):
    want, grid, _ = expected(name)
    assert grid == mbs and any(w[1][0] > 0 for w in want.values())
    got, lay, _ = run_activity(L, stream(name), gops_per_window=2, output="both" if name.startswith("yuva") else "rgba", **parser_kw(gpu_parser))
    assert (lay.mb_width, lay.mb_height) == mbs
    assert_activity(got, want, name)


@PARSERS
def test_every_window_and_ring_reuse(L, gpu_parser):
    """one GOP per window, two ring entries, five GOPs: an I picture's dense record lands where a B picture's sparse one was, and
    every record is exact: written whole, nothing left of the window before"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    want, _, _ = expected_activity(data)
    got, _, _ = run_activity(L, data, gops_per_window=1, windows_in_flight=2, **parser_kw(gpu_parser))
    assert len(got) == 30
    assert_activity(got, want, "five windows")


@pytest.mark.parametrize("output", ["rgba", "ycbcr", "tensor"])
def test_beside_motion_and_every_output(L, output):
    """both front ends, each output, MOTION beside it: the activity record is the same and the motion record is untouched"""
    want, _, motion = expected("ibbp_96x64")
    for gpu_parser in (None, -1):
        got, _, got_motion = run_activity(L, stream("ibbp_96x64"), gops_per_window=2, output=output, motion=True, **parser_kw(gpu_parser))
        assert_activity(got, want, "%s beside motion" % output)
        assert sorted(got_motion) == sorted(motion)
        for k, v in got_motion.items():
            assert all(np.array_equal(a, b) for a, b in zip(v, motion[k][:3])), k


def test_activity_view_is_the_record_in_place(L):
    """torch views of device memory equal read_activity, and frame["activity"] is where they lie"""
    want, _, _ = expected("ibbp_96x64")
    seen = {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        for f in frames:
            words, octets, s = pipe.activity_view(window, f["_i"])
            assert words.is_cuda and words.data_ptr() == f["activity"] == octets.data_ptr() and s.data_ptr() == f["activity"] + pipe.activity_layout.summary_offset
            cells, summary = pipe.read_activity(window, f["_i"])
            assert np.array_equal(octets.cpu().numpy().reshape(-1), cells.reshape(-1).view(np.uint8))
            assert np.array_equal(words.cpu().numpy().reshape(-1), cells.reshape(-1).view(np.int16))
            assert np.array_equal(s.cpu().numpy().view(np.uint32), summary)
            seen[(f["gop"], f["display_index"])] = (cells, summary)
    pipe = L.Pipeline(stream("ibbp_96x64"), on_window=on_window, activity=True, gops_per_window=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_activity(seen, want, "views")


@PARSERS
@pytest.mark.parametrize("window", [1, 3])
def test_open_gops(L, window, gpu_parser):
    """leading B pictures without a predecessor are not delivered and have no record; every call's n is the window's n_frames"""
    from test_open_gop import BROKEN, GOPS, OPEN, dropped_positions, gop_entries
    want, _, _ = expected("open")
    every = {(g, disp) for g, n in enumerate(GOPS) for _, disp, _, _ in gop_entries(n)}
    dropped = dropped_positions(GOPS, OPEN, BROKEN)
    assert dropped and set(want) == every - dropped
    got, _, _ = run_activity(L, stream("open"), gops_per_window=window, **parser_kw(gpu_parser))
    assert_activity(got, want, "open GOPs, window %d" % window)


@PARSERS
def test_exact_seek_trims(L, gpu_parser):
    """LEON_PIPELINE_SEEK_EXACT into GOP 3 of the open-GOP stream: trimmed pictures have no record, the delivered ones are exact"""
    import leon_vlc_ctypes as V
    data = stream("open")
    want3, _, _ = expected_activity(data, first_gop=3)
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
    t = (gop_ts[3] + 40.0 * 4 + 1.0) / 1000.0          # display position 4 of GOP 3: a B picture behind the first P
    lock, log = threading.Lock(), []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        with lock:
            assert len(pipe.window_activity(window, len(frames))) >= len(frames)
            for f in frames:
                log.append((window, (f["gop"], f["display_index"]), pipe.read_activity(window, f["_i"])))
    pipe = L.Pipeline(data, on_window=on_window, activity=True, gops_per_window=2, parser_threads=2, **parser_kw(gpu_parser))
    try:
        pipe.wait()
        first = pipe.seek(t, exact=True)
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    got = {k: v for w, k, v in log if w >= first}
    keys = [k for w, k, v in log if w >= first]
    assert keys[0] == (3, 4) and not any(k[0] == 3 and k[1] < 4 for k in keys)
    assert_activity(got, {k: v for k, v in want3.items() if k[0] != 3 or k[1] >= 4}, "EXACT seek")


def test_refusals(L):
    import ctypes as C
    data = stream("ibbp_96x64")
    for alone in (L.PIPELINE_OUTPUT_ACTIVITY, L.PIPELINE_OUTPUT_ACTIVITY | L.PIPELINE_OUTPUT_MOTION):          # the bit alone, and with MOTION only
        with pytest.raises(L.LeonError) as e:
            L.Pipeline(data, output=alone)
        assert e.value.code == L.ERR_INVALID
    for bad in (64, 128 | 4, 128 | 8, 256):          # unknown bits stay refused beside it
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output=bad | 1, activity=True)
    seen = []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        assert frames[0]["activity"] is None
        out = (C.c_void_p * n)()
        seen.append(pipe.lib.leon_pipeline_window_activity(pipe.h, window, out, n))
        seen.append(pipe.lib.leon_pipeline_read_activity(pipe.h, window, 0, None, None))
        lay = L.PipelineActivityLayout()
        seen.append(pipe.lib.leon_pipeline_get_activity_layout(pipe.h, C.byref(lay)))
        with pytest.raises(L.LeonError):
            pipe.activity_view(window, 0)
    pipe = L.Pipeline(data, on_window=on_window, gops_per_window=2, motion=True)          # without the bit (MOTION does not bring it)
    try:
        pipe.wait()
        assert pipe.error is None and pipe.activity_layout is None and not pipe.info.output & L.PIPELINE_OUTPUT_ACTIVITY
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)
    seen = []

    def on_activity_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        assert frames[0]["motion"] is None          # ... nor ACTIVITY MOTION
        out = (C.c_void_p * (n + 1))()
        for bad_n in (n - 1, n + 1, 0, -1):
            seen.append(pipe.lib.leon_pipeline_window_activity(pipe.h, window, out, bad_n))
        seen.append(pipe.lib.leon_pipeline_window_activity(pipe.h, window, None, n))
        seen.append(pipe.lib.leon_pipeline_read_activity(pipe.h, window, n, None, None))
        seen.append(pipe.lib.leon_pipeline_read_activity(pipe.h, window, -1, None, None))
        seen.append(pipe.lib.leon_pipeline_window_activity(pipe.h, window + 1000, out, n))
        assert pipe.lib.leon_pipeline_window_activity(pipe.h, window, out, n) == L.OK
        assert pipe.lib.leon_pipeline_read_activity(pipe.h, window, 0, None, None) == L.OK          # both pointers may be NULL
    pipe = L.Pipeline(data, on_window=on_activity_window, gops_per_window=2, activity=True)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        with pytest.raises(L.LeonError):          # every window has been released by now
            pipe.read_activity(0, 0)
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)


def test_uncoded_still_macroblocks_are_copies_of_their_reference(L):
    """The physical meaning of blocks == 0: a P picture's macroblock that codes nothing (blocks == 0) and predicts forward (info == 1)
    with a zero vector is, in the delivered YCbCr planes, its forward reference's co-located macroblock, byte for byte (clipped to the
    frame: ibbp_96x64.jsv shows 90 x 60 of its 96 x 64)"""
    found = []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        frames = list(frames)
        planes = {(f["gop"], f["display_index"]): pipe.read_planes(f) for f in frames}
        fw, fh = pipe.info.frame_width, pipe.info.frame_height
        for f in frames:
            if f["type"] != 2:
                continue
            cells, _ = pipe.read_activity(window, f["_i"])
            mv, info, _ = pipe.read_motion(window, f["_i"])
            ref = planes[(f["motion"]["fwd_gop"], f["motion"]["fwd_display"])]
            mine = planes[(f["gop"], f["display_index"])]
            for my, mx in np.argwhere((cells["blocks"] == 0) & (info == L.MOTION_FWD) & ~mv.any(axis=2)):
                y0, y1, x0, x1 = 16 * my, min(16 * my + 16, fh), 16 * mx, min(16 * mx + 16, fw)
                assert y1 > y0 and x1 > x0
                assert np.array_equal(mine[0][y0:y1, x0:x1], ref[0][y0:y1, x0:x1]), (f["gop"], f["display_index"], int(mx), int(my))
                for c in (1, 2):
                    assert np.array_equal(mine[c][y0 // 2:(y1 + 1) // 2, x0 // 2:(x1 + 1) // 2], ref[c][y0 // 2:(y1 + 1) // 2, x0 // 2:(x1 + 1) // 2]), (f["gop"], f["display_index"], int(mx), int(my), c)
                found.append((f["gop"], f["display_index"], int(mx), int(my)))
    pipe = L.Pipeline(stream("ibbp_96x64"), on_window=on_window, output="ycbcr", motion=True, activity=True, gops_per_window=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert len(found) >= 1, "ibbp_96x64.jsv has no uncoded, still, forward-predicted macroblock in a P picture"
