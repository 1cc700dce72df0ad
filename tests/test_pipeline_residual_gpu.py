"""GPU: the pipeline's RESIDUAL output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_RESIDUAL; k_residual) -- every delivered frame's
residual record, every window, against the oracle's residual (lo_pass1_plane, then lo_pass2_residual_plane) of the HOST front end's
densified planes, maps and the matrices of the sequence in force, all three planes bit-exact, through both front ends: the GPU front end
writes entries with level 0 and reserves more than it fills, the host one does neither, and the record is the same.  Which pictures
are delivered is what test_pipeline_motion_gpu.expected_motion says (dropped leading B pictures and what an EXACT seek trims have no
record).  The streams: 4 macroblocks with one task per plane row (32 x 32), 24 in one task a row with B pictures (96 x 64), custom
matrices (48 x 32), ten luma groups with two valid blocks in the last (592 x 32) and 330 macroblocks with partly filled last groups of
both kinds (352 x 240).  Two checks need no reference at all: an I picture's delivered planes are clip(res, 0, 255), and a P picture's
forward-predicted macroblock with a zero vector is clip(its reference's co-located samples + res)."""
import ctypes as C
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
NAMES = ["tiny_ip_32x32", "ibbp_96x64", "custom_intra_ip_48x32", "syntax_escape_ip_592x32", "leon_synth_352x240"]
CODED = [(32, 32), (96, 64), (48, 32), (592, 32), (352, 240)]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def parser_kw(gpu_parser):
    return dict(gpu_parser=None if gpu_parser is None else False)


@functools.lru_cache(maxsize=None)
def stream(name):
    if name == "open":
        return open_stream(96, 64, 31)[0]
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


def expected_residual(data, first_gop=0):
    """({(gop, display_index): (y, cb, cr) int32} of the pictures a run from key-map entry first_gop delivers, (coded_width,
    coded_height)): the host front end's densified planes through the oracle's two passes, built once per stream and left unchanged"""
    import leon_vlc_ctypes as V
    from oracle import oracle_py as O
    motion, grid = expected_motion(data, first_gop)
    st = V.Stream(data, threads=1)
    cw, ch = st.info.coded_width, st.info.coded_height
    assert (cw, ch) == (16 * grid[0], 16 * grid[1])
    matrices = lambda i: np.concatenate([np.frombuffer(bytes(i.intra_qm), np.uint8), np.frombuffer(bytes(i.non_intra_qm), np.uint8)])
    qm, pm = matrices(st.info), O.premultiplier()
    out, gop = {}, -1
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        if p["new_sequence"]:
            qm = matrices(st.refresh_info())
        if p["type"] == 1:
            gop += 1
        key = (gop, p["temporal_reference"])
        if key not in motion:
            continue
        planes = []
        for k, (W, H) in enumerate(((cw, ch), (cw // 2, ch // 2), (cw // 2, ch // 2))):
            scratch = np.ascontiguousarray(O.pass1_plane(p[("coef_y", "coef_cb", "coef_cr")[k]], W, H, k > 0, p["qscale"], p["intra"], cw // 16, qm, pm))
            res = np.zeros((H, W), dtype=np.int32)
            O.lib().lo_pass2_residual_plane(scratch.ctypes.data_as(C.c_void_p), W, H, res.ctypes.data_as(C.c_void_p))
            planes.append(res)
        out[key] = tuple(planes)
    st.close()
    assert set(out) == set(motion)
    return out, (cw, ch)


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_residual(stream(name))


def run_residual(L, data, **kw):
    """{(gop, display_index): (y, cb, cr)} as the pipeline delivers them, the residual layout"""
    kw.setdefault("parser_threads", 2)
    got = {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        records = pipe.window_residual(window, len(frames))
        for f in frames:
            assert f["residual"] and f["residual"] % 256 == 0 and records[f["_i"]] == f["residual"]
            key = (f["gop"], f["display_index"])
            assert key not in got
            got[key] = pipe.read_residual(window, f["_i"])
    pipe = L.Pipeline(data, on_window=on_window, residual=True, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        assert pipe.info.output & L.PIPELINE_OUTPUT_RESIDUAL
        lay = pipe.residual_layout
    finally:
        pipe.close()
    return got, lay


def assert_residual(got, want, what=""):
    assert sorted(got) == sorted(want), "%s: delivered and not expected %s, expected and missing %s" % (
        what, sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for k in sorted(want):
        for name, g, w in zip(("Y", "Cb", "Cr"), got[k], want[k]):
            assert g.dtype == np.int16 and g.shape == w.shape
            assert -32768 < w.min() and w.max() < 32767          # (the reference lies inside int16: nothing saturates)
            bad = np.argwhere(g != w)
            assert not len(bad), "%s: frame %s: %s differs in %d elements, first at (y, x) %s: %d, expected %d" % (
                what, k, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@PARSERS
@pytest.mark.parametrize("name,coded", list(zip(NAMES, CODED)))
def test_records_equal_the_oracle(L, name, coded, gpu_parser):
    want, size = expected(name)
    assert size == coded and any(p.any() for w in want.values() for p in w)
    got, lay = run_residual(L, stream(name), gops_per_window=2, **parser_kw(gpu_parser))
    assert (lay.coded_width, lay.coded_height) == coded
    ref = L.residual_layout(*coded)
    assert bytes(lay) == bytes(ref)
    assert_residual(got, want, name)


@PARSERS
def test_every_window_and_ring_reuse(L, gpu_parser):
    """one GOP per window, two ring entries, five GOPs: an I picture's dense record lands where a B picture's sparse one was, and
    every record is exact: written whole, nothing left of the window before"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    want, _ = expected_residual(data)
    got, _ = run_residual(L, data, gops_per_window=1, windows_in_flight=2, **parser_kw(gpu_parser))
    assert len(got) == 30
    assert_residual(got, want, "five windows")


def test_held_window_while_later_windows_reuse_the_ring(L):
    """the first window is kept (the callback returns False) while the windows behind it go through the other ring entries; read
    after the run has ended, its records are still its own"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    want, _ = expected_residual(data)
    held, later, done = [], {}, threading.Event()

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        if window == 0:
            held.append((window, [(f["gop"], f["display_index"], f["_i"]) for f in frames]))
            return False
        for f in frames:
            later[(f["gop"], f["display_index"])] = pipe.read_residual(window, f["_i"])
        if window == 4:
            done.set()
        return None
    pipe = L.Pipeline(data, on_window=on_window, residual=True, gops_per_window=1, windows_in_flight=2, parser_threads=2)
    try:
        assert done.wait(60), "windows 1 .. 4 were not delivered while window 0 was held"
        window, keys = held[0]
        got = {(g, d): pipe.read_residual(window, i) for g, d, i in keys}
        pipe.release_window(window)
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert len(got) == 6 and len(later) == 24
    got.update(later)
    assert_residual(got, want, "a held window")


@pytest.mark.parametrize("output", ["rgba", "ycbcr", "tensor"])
def test_beside_motion_activity_and_every_output(L, output):
    """both front ends, each output, MOTION and ACTIVITY beside it: the residual record is the same and the other two are untouched"""
    from test_pipeline_activity_gpu import expected as expected_activity
    want, _ = expected("ibbp_96x64")
    want_activity, _, want_motion = expected_activity("ibbp_96x64")
    for gpu_parser in (None, -1):
        got, motion, activity = {}, {}, {}

        def on_window(window, frames):
            pipe = frames[0]["_pipe"]
            for f in frames:
                key = (f["gop"], f["display_index"])
                got[key] = pipe.read_residual(window, f["_i"])
                motion[key] = pipe.read_motion(window, f["_i"])
                activity[key] = pipe.read_activity(window, f["_i"])
        pipe = L.Pipeline(stream("ibbp_96x64"), on_window=on_window, residual=True, motion=True, activity=True, output=output, gops_per_window=2, parser_threads=2,
                          **parser_kw(gpu_parser))
        try:
            pipe.wait()
            assert pipe.error is None, pipe.error
        finally:
            pipe.close()
        assert_residual(got, want, "%s beside motion and activity" % output)
        assert sorted(motion) == sorted(want_motion) and sorted(activity) == sorted(want_activity)
        for k in motion:
            assert all(np.array_equal(a, b) for a, b in zip(motion[k], want_motion[k][:3])), k
            assert all(np.array_equal(a, b) for a, b in zip(activity[k], want_activity[k])), k


def test_residual_view_is_the_record_in_place(L):
    """strided torch views of device memory equal read_residual, and frame["residual"] is where they lie"""
    want, _ = expected("ibbp_96x64")
    seen = {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        lay = pipe.residual_layout
        for f in frames:
            y, cb, cr = pipe.residual_view(window, f["_i"])
            assert y.is_cuda and y.data_ptr() == f["residual"] and cb.data_ptr() == f["residual"] + lay.cb_offset and cr.data_ptr() == f["residual"] + lay.cr_offset
            assert y.stride() == (lay.luma_stride, 1) and cb.stride() == (lay.chroma_stride, 1)
            host = pipe.read_residual(window, f["_i"])
            for v, h in zip((y, cb, cr), host):
                assert np.array_equal(v.cpu().numpy(), h)
            seen[(f["gop"], f["display_index"])] = host
    pipe = L.Pipeline(stream("ibbp_96x64"), on_window=on_window, residual=True, gops_per_window=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_residual(seen, want, "views")


@PARSERS
@pytest.mark.parametrize("window", [1, 3])
def test_open_gops(L, window, gpu_parser):
    """leading B pictures without a predecessor are not delivered and have no record"""
    from test_open_gop import BROKEN, GOPS, OPEN, dropped_positions, gop_entries
    want, _ = expected("open")
    every = {(g, disp) for g, n in enumerate(GOPS) for _, disp, _, _ in gop_entries(n)}
    dropped = dropped_positions(GOPS, OPEN, BROKEN)
    assert dropped and set(want) == every - dropped
    got, _ = run_residual(L, stream("open"), gops_per_window=window, **parser_kw(gpu_parser))
    assert_residual(got, want, "open GOPs, window %d" % window)


@PARSERS
def test_exact_seek_trims(L, gpu_parser):
    """LEON_PIPELINE_SEEK_EXACT into GOP 3 of the open-GOP stream: trimmed pictures have no record, the delivered ones are exact"""
    import leon_vlc_ctypes as V
    data = stream("open")
    want3, _ = expected_residual(data, first_gop=3)
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
            assert len(pipe.window_residual(window, len(frames))) >= len(frames)
            for f in frames:
                log.append((window, (f["gop"], f["display_index"]), pipe.read_residual(window, f["_i"])))
    pipe = L.Pipeline(data, on_window=on_window, residual=True, gops_per_window=2, parser_threads=2, **parser_kw(gpu_parser))
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
    assert_residual(got, {k: v for k, v in want3.items() if k[0] != 3 or k[1] >= 4}, "EXACT seek")


def test_refusals(L):
    data = stream("ibbp_96x64")
    R, M, A = L.PIPELINE_OUTPUT_RESIDUAL, L.PIPELINE_OUTPUT_MOTION, L.PIPELINE_OUTPUT_ACTIVITY
    for alone in (R, R | M, R | A, R | M | A):          # the bit alone, and with only the record bits
        with pytest.raises(L.LeonError) as e:
            L.Pipeline(data, output=alone)
        assert e.value.code == L.ERR_INVALID
    for bad in (64, 256, 1024, 512 | 4, 512 | 8):          # unknown bits stay refused beside it
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output=bad | 1, residual=True)
    seen = []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        assert frames[0]["residual"] is None
        out = (C.c_void_p * n)()
        seen.append(pipe.lib.leon_pipeline_window_residual(pipe.h, window, out, n))
        seen.append(pipe.lib.leon_pipeline_read_residual(pipe.h, window, 0, None, None, None))
        lay = L.PipelineResidualLayout()
        seen.append(pipe.lib.leon_pipeline_get_residual_layout(pipe.h, C.byref(lay)))
        with pytest.raises(L.LeonError):
            pipe.residual_view(window, 0)
    pipe = L.Pipeline(data, on_window=on_window, gops_per_window=2, motion=True, activity=True)          # without the bit (the others do not bring it)
    try:
        pipe.wait()
        assert pipe.error is None and pipe.residual_layout is None and not pipe.info.output & R
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)
    seen = []

    def on_residual_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        assert frames[0]["motion"] is None and frames[0]["activity"] is None          # ... nor RESIDUAL the others
        out = (C.c_void_p * (n + 1))()
        for bad_n in (n - 1, n + 1, 0, -1):
            seen.append(pipe.lib.leon_pipeline_window_residual(pipe.h, window, out, bad_n))
        seen.append(pipe.lib.leon_pipeline_window_residual(pipe.h, window, None, n))
        seen.append(pipe.lib.leon_pipeline_read_residual(pipe.h, window, n, None, None, None))
        seen.append(pipe.lib.leon_pipeline_read_residual(pipe.h, window, -1, None, None, None))
        seen.append(pipe.lib.leon_pipeline_window_residual(pipe.h, window + 1000, out, n))
        assert pipe.lib.leon_pipeline_window_residual(pipe.h, window, out, n) == L.OK
        assert pipe.lib.leon_pipeline_read_residual(pipe.h, window, 0, None, None, None) == L.OK          # every pointer may be NULL
    pipe = L.Pipeline(data, on_window=on_residual_window, gops_per_window=2, residual=True)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        with pytest.raises(L.LeonError):          # every window has been released by now
            pipe.read_residual(0, 0)
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)


@pytest.mark.parametrize("name", ["ibbp_96x64", "custom_intra_ip_48x32", "leon_synth_352x240"])
def test_i_pictures_are_their_clipped_residual(L, name):
    """Physical check 1, from delivered data alone: nothing is predicted in an I picture, so its delivered YCbCr planes are
    clip(res, 0, 255) over the frame -- and the record holds what that clamp hides"""
    checked, negative = [], []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        fw, fh = pipe.info.frame_width, pipe.info.frame_height
        for f in frames:
            if f["type"] != 1:
                continue
            planes = pipe.read_planes(f)
            res = pipe.read_residual(window, f["_i"])
            for c, (p, r) in enumerate(zip(planes[:3], res)):
                h, w = (fh, fw) if c == 0 else ((fh + 1) // 2, (fw + 1) // 2)
                assert np.array_equal(p[:h, :w], np.clip(r[:h, :w], 0, 255).astype(np.uint8)), (f["gop"], f["display_index"], c)
                negative.append(int((r < 0).sum()))
            checked.append((f["gop"], f["display_index"]))
    pipe = L.Pipeline(stream(name), on_window=on_window, output="ycbcr", residual=True, gops_per_window=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert checked
    print("%s: %d I pictures, %d negative residual elements" % (name, len(checked), sum(negative)))


def test_still_forward_macroblocks_are_reference_plus_residual(L):
    """Physical check 2, from delivered data alone: a P picture's macroblock that predicts forward (info == 1) with a zero vector is, in
    the delivered YCbCr planes, clip(its forward reference's co-located samples + res, 0, 255) (clipped to the frame: ibbp_96x64.jsv
    shows 90 x 60 of its 96 x 64).  At least the eight such macroblocks the activity test relies on; printed: how many had coded blocks"""
    found, coded = [], []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        frames = list(frames)
        planes = {(f["gop"], f["display_index"]): pipe.read_planes(f) for f in frames}
        fw, fh = pipe.info.frame_width, pipe.info.frame_height
        for f in frames:
            if f["type"] != 2:
                continue
            res = pipe.read_residual(window, f["_i"])
            cells, _ = pipe.read_activity(window, f["_i"])
            mv, info, _ = pipe.read_motion(window, f["_i"])
            ref = planes[(f["motion"]["fwd_gop"], f["motion"]["fwd_display"])]
            mine = planes[(f["gop"], f["display_index"])]
            for my, mx in np.argwhere((info == L.MOTION_FWD) & ~mv.any(axis=2)):
                y0, y1, x0, x1 = 16 * my, min(16 * my + 16, fh), 16 * mx, min(16 * mx + 16, fw)
                assert y1 > y0 and x1 > x0
                for c in range(3):
                    ys, xs = (slice(y0, y1), slice(x0, x1)) if c == 0 else (slice(y0 // 2, (y1 + 1) // 2), slice(x0 // 2, (x1 + 1) // 2))
                    want = np.clip(ref[c][ys, xs].astype(np.int32) + res[c][ys, xs], 0, 255).astype(np.uint8)
                    assert np.array_equal(mine[c][ys, xs], want), (f["gop"], f["display_index"], int(mx), int(my), c)
                found.append((f["gop"], f["display_index"], int(mx), int(my)))
                coded.append(bool(cells["blocks"][my, mx]))
    pipe = L.Pipeline(stream("ibbp_96x64"), on_window=on_window, output="ycbcr", motion=True, activity=True, residual=True, gops_per_window=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    print("ibbp_96x64: %d still forward-predicted P macroblocks checked, %d of them with coded blocks" % (len(found), sum(coded)))
    assert len(found) >= 8, "ibbp_96x64.jsv has fewer than eight still, forward-predicted macroblocks in its P pictures"
