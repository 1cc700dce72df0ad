"""leon_pipeline_config.output = YCbCr (include/leon_pipeline.h): the pipeline delivers every frame's decoded YCbCr 4:2:0
planes, cropped to the frame -- the reference's own frame event, {'ybr': [Y, Cb, Cr], 'ts': ts} (decoders/jsv.js:600, :673).
Every delivered frame's planes must equal the oracle's bit for bit, on the fused road (k_recon_display_out) and the unfused
one (k_planes_crop), with either front end; with output = both the RGBA must equal a default pipeline's byte for byte."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

from test_pipeline_gpu import STREAMS, ibbp_stream, oracle_frames, run_pipeline

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
FIXTURES = ["leon_synth_352x240", "slices5_ip_96x64", "custom_intra_ip_48x32", "tiny_ip_32x32", "ibbp_96x64", "yuva_ibbp_96x64"]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def fixture(name):
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


def oracle_planes(data):
    """{(gop, display_index): (Y, Cb, Cr[, A]) cropped to the frame}: the walk of oracle_frames, the oracle's planes instead
    of its RGBA"""
    import leon_vlc_ctypes as V
    from oracle import oracle_py as O
    st = V.Stream(data, threads=1)
    info = st.info
    cw, ch, fw, fh = info.coded_width, info.coded_height, info.frame_width, info.frame_height
    matrices = lambda i: np.concatenate([np.frombuffer(bytes(i.intra_qm), np.uint8), np.frombuffer(bytes(i.non_intra_qm), np.uint8)])
    qm = matrices(info)
    out, gop, older, newer = {}, -1, None, None
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        if p["new_sequence"]:
            qm = matrices(st.refresh_info())
        if p["type"] == 1:
            gop += 1
            older = newer = None
        fwd = bwd = None
        if p["type"] == 2:
            fwd = newer
        elif p["type"] == 3:
            bwd, fwd = newer, (older if older is not None else newer)
        planes = O.decode_picture(p["type"], cw, ch, p["coef_y"], p["coef_cb"], p["coef_cr"], p["qscale"], p["intra"],
                                  repadd=p.get("repadd"), mb_dir=p.get("mb_dir"), mv_fwd=p.get("mv_fwd"), mv_bwd=p.get("mv_bwd"),
                                  qm=qm, ref_fwd=fwd, ref_bwd=bwd, coef_a=p.get("coef_a"))
        if p["type"] != 3:
            older, newer = newer, planes
        n3 = cw * ch * 3 // 2
        y, cb, cr = O.split_planes(planes[:n3], cw, ch)
        y, cb, cr = y.reshape(ch, cw), cb.reshape(ch // 2, cw // 2), cr.reshape(ch // 2, cw // 2)
        cwid, chh = (fw + 1) // 2, (fh + 1) // 2
        got = [y[:fh, :fw], cb[:chh, :cwid], cr[:chh, :cwid]]
        if p.get("coef_a") is not None:
            got.append(planes[n3:].reshape(ch, cw)[:fh, :fw])
        out[(gop, p["temporal_reference"])] = tuple(np.ascontiguousarray(g) for g in got)
    return out


def run_planes(L, data, output="ycbcr", **kw):
    """({key: planes}, {key: rgba or None}, [(gop, display_index, ts_ms)]) of a whole run"""
    kw.setdefault("gpu_parser", False)
    planes, rgba, order, lock = {}, {}, [], threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                k = (f["gop"], f["display_index"])
                planes[k] = f["_pipe"].read_planes(f)
                rgba[k] = L.read_frame(f) if f["rgba"] else None
                order.append((f["gop"], f["display_index"], f["ts_ms"]))
    pipe = L.Pipeline(data, on_window=on_window, output=output, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None
    finally:
        pipe.close()
    return planes, rgba, order


def assert_planes(got, want, what):
    assert set(got) == set(want), "%s: frames %s" % (what, sorted(set(got) ^ set(want))[:8])
    for k in sorted(want):
        assert len(got[k]) == len(want[k]), "%s %s: %d planes, want %d" % (what, k, len(got[k]), len(want[k]))
        for name, g, w in zip(("Y", "Cb", "Cr", "A"), got[k], want[k]):
            assert g.shape == w.shape and np.array_equal(g, w), "%s %s: plane %s differs in %d samples" % (
                what, k, name, int((g != w).sum()) if g.shape == w.shape else -1)


@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams_ycbcr(L, name, gpu_parser):
    data = fixture(name)
    want = oracle_planes(data)
    got, rgba, order = run_planes(L, data, "ycbcr", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert_planes(got, want, name)
    assert all(v is None for v in rgba.values())             # frame.rgba is NULL in a YCbCr-only pipeline
    assert order == sorted(order)
    if name.startswith("yuva"):
        assert any((w[3] != 255).any() for w in want.values())


@PARSERS
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_streams_both(L, name, gpu_parser):
    data = fixture(name)
    want = oracle_planes(data)
    got, rgba, _ = run_planes(L, data, "both", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert_planes(got, want, name)
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert set(ref) == set(rgba)
    for k in ref:
        assert np.array_equal(rgba[k], ref[k]), "%s %s: RGBA of output=both differs from the default pipeline's" % (name, k)


@PARSERS
@pytest.mark.parametrize("case", ["360x199", "100x60"])
def test_layout_edges(L, case, gpu_parser):
    """360 x 199 (fused road): chroma width 180, so the 8-byte chroma chunks straddle the crop, odd heights.
    100 x 60 (unfused road, width % 8 != 0): k_planes_crop"""
    fw, fh = (360, 199) if case == "360x199" else (100, 60)
    data = ibbp_stream((fw + 15) // 16 * 16, (fh + 15) // 16 * 16, [6, 9], seed=fw + fh, frame=(fw, fh))
    want = oracle_planes(data)
    for output in ("ycbcr", "both"):
        got, rgba, _ = run_planes(L, data, output, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
        assert_planes(got, want, "%s %s" % (case, output))
        if output == "both":          # RGBA byte for byte that of a default (RGBA) pipeline
            ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
            assert set(ref) == set(rgba) and all(np.array_equal(rgba[k], ref[k]) for k in ref)


@PARSERS
def test_gl_flavour_both(L, gpu_parser):
    """display_flavour = GL takes the unfused road: the planes are the oracle's, the RGBA a GL-flavour RGBA pipeline's"""
    data = fixture("leon_synth_352x240")
    want = oracle_planes(data)
    got, rgba, _ = run_planes(L, data, "both", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert_planes(got, want, "GL both")
    ref, _, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert set(ref) == set(rgba) and all(np.array_equal(rgba[k], ref[k]) for k in ref)
    got, rgba, _ = run_planes(L, data, "ycbcr", parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, display_flavour=L.RGB_GL)
    assert_planes(got, want, "GL ycbcr")


class Log:
    def __init__(self):
        self.cv = threading.Condition()
        self.windows = {}

    def on_window(self, window, frames):
        got = {(f["gop"], f["display_index"]): f["_pipe"].read_planes(f) for f in frames}
        with self.cv:
            self.windows[window] = got
            self.cv.notify_all()

    def since(self, first):
        with self.cv:
            out = {}
            for w in sorted(self.windows):
                if w >= first:
                    out.update(self.windows[w])
            return out


def keys_after_seek(L, data, gpu_parser, t, exact, output):
    log = Log()
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=log.on_window, output=output)
    try:
        pipe.wait()
        first = pipe.seek(t, exact=exact)
        pipe.wait()
        assert pipe.error is None
    finally:
        pipe.close()
    return log.since(first)


@PARSERS
@pytest.mark.parametrize("exact", [False, True], ids=["key", "exact"])
def test_seek(L, gpu_parser, exact):
    """after a KEY or EXACT seek the frames are the oracle's planes, and exactly the frames an RGBA pipeline delivers after the
    same seek (EXACT: no picture decoded only for prediction is delivered)"""
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    want = oracle_planes(data)
    import leon_vlc_ctypes as V
    rate = V.Stream(data, threads=1).info.picture_rate or 25.0
    for t in (0.0, 13.5 / rate, 31.2 / rate):
        got = keys_after_seek(L, data, gpu_parser, t, exact, "ycbcr")
        assert got, "nothing delivered after seeking to %.3f s" % t
        assert_planes(got, {k: want[k] for k in got}, "seek %.3f" % t)
        log = Log()

        def rec(window, frames):
            with log.cv:
                log.windows[window] = {(f["gop"], f["display_index"]): None for f in frames}
        pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=rec)
        try:
            pipe.wait()
            first = pipe.seek(t, exact=exact)
            pipe.wait()
        finally:
            pipe.close()
        rgba_keys = set(log.since(first))
        assert set(got) == rgba_keys, "seek %.3f: other frames than the RGBA pipeline's" % t


@PARSERS
def test_held_window_keeps_its_planes(L, gpu_parser):
    """W = 1, R = 2: window 0 is held while the later windows decode through the other ring entry; its planes are unchanged"""
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=99)
    want = oracle_planes(data)
    held, later, cv = [], {}, threading.Condition()

    def on_window(window, frames):
        with cv:
            if not held:
                recs = []
                for f in frames:
                    r = L.PipelineFrame()
                    C.pointer(r)[0] = f["_frames"][f["_i"]]
                    recs.append(((f["gop"], f["display_index"]), r))
                held.append((window, recs))
                cv.notify_all()
                return False
            for f in frames:
                later[(f["gop"], f["display_index"])] = f["_pipe"].read_planes(f)
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, windows_in_flight=2, gpu_parser=gpu_parser, on_window=on_window, output="ycbcr")
    try:
        with cv:
            assert cv.wait_for(lambda: held, 30)
        t0 = time.time()
        while time.time() - t0 < 5 and len(later) < 6:
            time.sleep(0.01)
        window, recs = held[0]
        got = {}
        for k, r in recs:
            f = {"a": r.a, "_frames": [r], "_i": 0}
            got[k] = pipe.read_planes(f)
        assert_planes(got, {k: want[k] for k in got}, "held window")
        pipe.release_window(window)
        pipe.wait()
    finally:
        pipe.close()
    assert len(later) > 0
    assert_planes(later, {k: want[k] for k in later}, "later windows")


@PARSERS
def test_partial_stream(L, gpu_parser):
    import leon_vlc_ctypes as V
    data = ibbp_stream(96, 64, [6, 9, 3, 12, 6], seed=77)
    want = oracle_planes(data)
    offs = V.Stream(data, threads=1).keymap()
    got, lock = {}, threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                got[(f["gop"], f["display_index"])] = f["_pipe"].read_planes(f)
    first = offs[1] + 3
    buf = bytearray(len(data))
    buf[:first] = data[:first]
    pipe = L.Pipeline(bytes(buf), parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=on_window, valid_bytes=first, output="ycbcr")
    try:
        at = first
        for step in (500, 1, 1800, 700, 10 ** 9):
            n = min(step, len(data) - at)
            pipe.feed(at + n, data[at:at + n], at)
            at += n
            if at == len(data):
                break
        pipe.wait()
    finally:
        pipe.close()
    assert_planes(got, want, "partial")


def test_refusals(L):
    data = fixture("ibbp_96x64")
    for bad in (4, -1, 8):
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output=bad)
    seen = {}

    def grab(pipe_kind):
        def on_window(window, frames):
            f = frames[0]
            p = f["_pipe"]
            rec = f["_frames"][f["_i"]]
            buf = np.empty(p.info.frame_width * p.info.frame_height * 4, np.uint8)
            y = np.empty(p.info.frame_width * p.info.frame_height, np.uint8)
            c = np.empty(p.info.chroma_width * p.info.chroma_height, np.uint8)
            seen.setdefault(pipe_kind, (p.lib.leon_pipeline_read_frame(p.h, C.byref(rec), buf.ctypes.data),
                                        p.lib.leon_pipeline_read_frame_planes(p.h, C.byref(rec), y.ctypes.data, c.ctypes.data, c.ctypes.data, None)))
        return on_window
    for kind in ("ycbcr", "rgba"):
        pipe = L.Pipeline(data, gops_per_window=1, gpu_parser=False, on_window=grab(kind), output=kind)
        try:
            pipe.wait()
        finally:
            pipe.close()
    assert seen["ycbcr"] == (L.ERR_INVALID, L.OK)       # read_frame on a frame without RGBA
    assert seen["rgba"] == (L.OK, L.ERR_INVALID)        # read_frame_planes on a frame without planes


def test_info_and_plane_views(L):
    """leon_pipeline_info reports the layout; plane_views wraps the planes in place (torch, no copy) and equals read_planes"""
    data = ibbp_stream(368, 208, [6], seed=5, frame=(360, 199))
    views = []

    def on_window(window, frames):
        p = frames[0]["_pipe"]
        for f in frames:
            v = p.plane_views(f)
            views.append((tuple(x.cpu().numpy() for x in v), p.read_planes(f)))
    pipe = L.Pipeline(data, gops_per_window=1, gpu_parser=True, on_window=on_window, output="both")
    try:
        pipe.wait()
        i = pipe.info
        lay = L.planes_layout(360, 199)
        assert (i.output, i.chroma_width, i.chroma_height, i.luma_stride, i.chroma_stride) == (3, 180, 100, lay["luma_stride"], lay["chroma_stride"])
    finally:
        pipe.close()
    assert views
    for v, r in views:
        assert all(np.array_equal(a, b) for a, b in zip(v, r))


def test_1080p_two_gops(L):
    import stream_1080p
    data = stream_1080p.load()
    want = oracle_planes(data)
    got, _, _ = run_planes(L, data, "ycbcr", gops_per_window=2, gpu_parser=True)
    assert_planes(got, want, "1080p")
