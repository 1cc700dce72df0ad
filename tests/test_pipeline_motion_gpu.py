"""GPU: the pipeline's MOTION output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_MOTION; k_motion) -- every delivered frame's motion
record against leon_ctypes.motion_from_maps of the HOST parser's maps (leon_vlc_ctypes.Stream, walked as
test_pipeline_gpu.oracle_frames walks a stream), all three parts exactly, and the references each record names against the GOP
structure.  tests/test_pipeline_motion_abi.py holds motion_from_maps against the tensors that were written.
The streams are the smallest at which the kernel can go wrong: 24 macroblocks (less than a wave), 74 (no multiple of the four a lane
takes per trip, two waves), 91 (odd in both), 330 (a second, partly filled trip of the 256-lane loop; the fixture of that size has I
and P pictures only, so an IBBP stream of the same grid is written beside it), and a coded grid larger than the frame on the unfused
road."""
import functools
import os
import threading

import numpy as np
import pytest

from helpers import ROOT
from test_open_gop import open_stream
from test_pipeline_gpu import ibbp_stream

pytestmark = pytest.mark.gpu

STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def expected_motion(data, first_gop=0):
    """{(gop, display_index): (mv, info, summary, fwd_gop, fwd_display, bwd_display)} of a run that starts at key-map entry first_gop:
    the host parser's maps through motion_from_maps, and the references by the rules of include/leon_pipeline.h -- a P picture the
    anchor before it, a B picture the two anchors around it; the leading B pictures of a closed GOP its I picture for both, those of an
    open GOP with its predecessor the last anchor of the GOP before, those of an open GOP without are not delivered"""
    import leon_ctypes as L_
    import leon_vlc_ctypes as V
    st = V.Stream(data, threads=1)
    mbw, mbh = st.info.coded_width // 16, st.info.coded_height // 16
    out = {}
    gop, older, newer, dropping, is_open = -1, None, None, False, False
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        if p["type"] == 1:
            gop += 1
            is_open = bool(p["open_gop"])
            has_predecessor = is_open and not p["broken_link"] and gop > first_gop
            before = newer if has_predecessor else None          # (gop, display index) of the last anchor of the GOP before
            older = newer = None
            dropping = is_open and not has_predecessor
        fwd, bwd = None, None
        if p["type"] == 2:
            fwd = newer
        elif p["type"] == 3:
            bwd = newer
            if older is not None:
                fwd = older
            elif not is_open:
                fwd = newer
            elif dropping:
                continue
            else:
                fwd = before
        key = (gop, p["temporal_reference"])
        if p["type"] != 3:
            older, newer = newer, key
        if gop < first_gop:
            continue
        rec = L_.motion_from_maps(p["type"], mbw, mbh, repadd=p.get("repadd"), mb_dir=p.get("mb_dir"), mv_fwd=p.get("mv_fwd"), mv_bwd=p.get("mv_bwd"))
        out[key] = rec + (fwd[0] if fwd else gop, fwd[1] if fwd else -1, bwd[1] if bwd else -1)
    st.close()
    return out, (mbw, mbh)


def run_motion(L, data, **kw):
    """{(gop, display_index): (mv, info, summary, fwd_gop, fwd_display, bwd_display)} as the pipeline delivers them, and the frame order"""
    kw.setdefault("gpu_parser", False)
    kw.setdefault("parser_threads", 2)
    got, order = {}, []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        records = pipe.window_motion(window, len(frames))          # n = the window's n_frames, whatever was dropped or trimmed
        for f in frames:
            m = f["motion"]
            assert m is not None and m["record"] and m["record"] % 256 == 0
            assert records[f["_i"]].record == m["record"]
            got[(f["gop"], f["display_index"])] = pipe.read_motion(window, f["_i"]) + (m["fwd_gop"], m["fwd_display"], m["bwd_display"])
            order.append((f["gop"], f["display_index"], f["type"]))
    pipe = L.Pipeline(data, on_window=on_window, motion=True, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        assert pipe.info.output & L.PIPELINE_OUTPUT_MOTION
        lay = pipe.motion_layout
    finally:
        pipe.close()
    return got, order, lay


def assert_motion(got, want, what=""):
    assert sorted(got) == sorted(want), "%s: delivered and not expected %s, expected and missing %s" % (
        what, sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for k in sorted(want):
        g, w = got[k], want[k]
        assert g[0].shape == w[0].shape and g[0].dtype == np.int16 and g[1].dtype == np.uint8 and g[2].dtype == np.uint32
        assert np.array_equal(g[1], w[1]), "%s: frame %s: info differs at macroblocks %s" % (what, k, np.argwhere(g[1] != w[1])[:6].tolist())
        assert np.array_equal(g[0], w[0]), "%s: frame %s: vectors differ at macroblocks %s" % (what, k, np.argwhere((g[0] != w[0]).any(axis=2))[:6].tolist())
        assert np.array_equal(g[2], w[2]), "%s: frame %s: summary %s, expected %s" % (what, k, g[2].tolist(), w[2].tolist())
        assert tuple(g[3:]) == tuple(w[3:]), "%s: frame %s: references (fwd_gop, fwd_display, bwd_display) %s, expected %s" % (what, k, g[3:], w[3:])


@functools.lru_cache(maxsize=None)
def stream(name):
    """(stream bytes, pipeline keywords): built once per process and left unchanged"""
    import syntax_streams as X
    if name in X.CASES:
        return X.build_case(X.CASES[name])[1], {}
    if name == "ibbp_96x64_coded":
        return ibbp_stream(96, 64, [6, 9], 41), {}
    if name == "cropped_61x45":
        return ibbp_stream(64, 48, [6, 6], 42, frame=(61, 45)), dict(output="rgba")
    if name == "ibbp_352x240":
        return ibbp_stream(352, 240, [6], 44), {}
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read(), {}


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_motion(stream(name)[0])


def gop_structure_refs(order):
    """the references of synth.gop_ibbp for the frames delivered, by (gop, display index): closed GOPs, so a leading B picture (no
    forward entry) names its I picture for both"""
    import synth as S
    sizes = {}
    for g, d, t in order:
        sizes[g] = sizes.get(g, 0) + 1
    out = {}
    for g, n in sizes.items():
        for ptype, disp, f, b in S.gop_ibbp(n):
            if ptype == S.PIC_I:
                out[(g, disp)] = (g, -1, -1)
            else:
                out[(g, disp)] = (g, f if f is not None else b, b if b is not None else -1)
    return out


@PARSERS
@pytest.mark.parametrize("name,mbs", [("ibbp_96x64_coded", (6, 4)), ("escape_592x32", (37, 2)), ("dense_one_slice_208x112", (13, 7)),
                                       ("leon_synth_352x240", (22, 15)), ("ibbp_352x240", (22, 15)), ("cropped_61x45", (4, 3))])
def test_records_equal_the_definition(L, name, mbs, gpu_parser):
    data, kw = stream(name)
    want, grid = expected(name)
    assert grid == mbs
    ip_only = name == "leon_synth_352x240"          # the fixture is I and P pictures; ibbp_352x240 has the same grid with B pictures
    assert any((v[1] == 1).any() for v in want.values()) and (ip_only or any((v[1] == 2).any() for v in want.values()))
    assert ip_only or any((v[1] == 3).any() for v in want.values())
    got, order, lay = run_motion(L, data, gops_per_window=2, gpu_parser=gpu_parser, **kw)
    assert (lay.mb_width, lay.mb_height) == mbs
    assert_motion(got, want, "%s" % name)
    assert {t for _, _, t in order} == ({1, 2} if ip_only else {1, 2, 3})
    if not ip_only:          # written here as closed IBBP GOPs: synth.gop_ibbp says the same as the walk
        refs = gop_structure_refs(order)
        assert set(refs) == set(got)
        for k, v in got.items():
            assert tuple(v[3:]) == refs[k], (name, k, v[3:], refs[k])


@PARSERS
@pytest.mark.parametrize("name", ["f7_f4_fullpel", "per_picture"])
def test_doubled_vectors_and_large_sums(L, name, gpu_parser):
    """full_pel vectors arrive doubled (f_code 7: up to 2048 in magnitude); the summary against numpy on the delivered record itself"""
    data, kw = stream(name)
    want, _ = expected(name)
    got, _, _ = run_motion(L, data, gops_per_window=1, gpu_parser=gpu_parser)
    assert_motion(got, want, name)
    assert max(int(np.abs(v[0].astype(np.int64)).max()) for v in got.values()) >= 1024
    for k, (mv, info, s, *_) in got.items():
        a = np.abs(mv.astype(np.int64)).reshape(-1, 4)
        assert s.tolist() == [int(((info & 1) != 0).sum()), int(((info & 2) != 0).sum()), int(((info & 4) != 0).sum()),
                              int(mv.reshape(-1, 4).any(axis=1).sum())] + a.sum(axis=0).tolist(), k


@pytest.mark.parametrize("output", ["tensor", "ycbcr", "all"])
def test_beside_every_output(L, output):
    data = open(os.path.join(STREAMS, "ibbp_96x64.jsv"), "rb").read()
    want, _ = expected("ibbp_96x64")
    got, _, _ = run_motion(L, data, gops_per_window=2, gpu_parser=True, output=output)
    assert_motion(got, want, output)


@PARSERS
def test_yuva_stream(L, gpu_parser):
    want, _ = expected("yuva_ibbp_96x64")
    got, _, _ = run_motion(L, stream("yuva_ibbp_96x64")[0], gops_per_window=2, gpu_parser=gpu_parser, output="both")
    assert_motion(got, want, "yuva")


def test_motion_view_is_the_record_in_place(L):
    """torch views of device memory equal the host copies, and frame["motion"]["record"] is where they lie"""
    import torch
    data, _ = stream("ibbp_96x64_coded")
    want, _ = expected("ibbp_96x64_coded")
    seen = {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        for f in frames:
            mv, info, s = pipe.motion_view(window, f["_i"])
            assert mv.is_cuda and mv.data_ptr() == f["motion"]["record"] and info.data_ptr() == f["motion"]["record"] + pipe.motion_layout.info_offset
            seen[(f["gop"], f["display_index"])] = (mv.cpu().numpy(), info.cpu().numpy(), s.cpu().numpy().view(np.uint32))
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=2, gpu_parser=True)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert sorted(seen) == sorted(want)
    for k, v in seen.items():
        assert all(np.array_equal(a, b) for a, b in zip(v, want[k][:3])), k
    assert torch.cuda.is_available()


@PARSERS
def test_ring_lifetime_and_reuse(L, gpu_parser):
    """one GOP per window, two ring entries, five GOPs: window 0 is held while windows 1 .. 4 are delivered and released -- they all reuse
    the other ring entry, an I picture's record (all 4 / zeros) lands where a B picture's was -- then window 0's records are read: still
    exact.  Every record of the later windows is exact too: written whole, nothing left of the window before"""
    data = ibbp_stream(96, 64, [6] * 5, 43)
    want, _ = expected_motion(data)
    got, held, done = {}, [], threading.Event()

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        if window == 0:
            held.append((window, [(f["gop"], f["display_index"], f["_i"], f["motion"]) for f in frames]))
            return False
        for f in frames:
            m = f["motion"]
            got[(f["gop"], f["display_index"])] = pipe.read_motion(window, f["_i"]) + (m["fwd_gop"], m["fwd_display"], m["bwd_display"])
        if window == 4:
            done.set()
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=1, windows_in_flight=2, gpu_parser=gpu_parser, parser_threads=2)
    try:
        assert done.wait(60), "windows 1 .. 4 were not delivered while window 0 was held"
        assert len(held) == 1 and len(got) == 24
        window, frames = held[0]
        again = pipe.window_motion(window, len(frames))
        for i, (g, d, idx, m) in enumerate(frames):
            assert again[i].record == m["record"]
            got[(g, d)] = pipe.read_motion(window, idx) + (m["fwd_gop"], m["fwd_display"], m["bwd_display"])
        pipe.release_window(window)
        with pytest.raises(L.LeonError):          # released: no longer out for delivery
            pipe.read_motion(window, 0)
        with pytest.raises(L.LeonError):
            pipe.window_motion(window, len(frames))
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert_motion(got, want, "held window and ring reuse")
    i_pics = [v for v in got.values() if (v[1] == 4).all()]
    assert len(i_pics) >= 5 and all(not v[0].any() and v[2].tolist() == [0, 0, 24, 0, 0, 0, 0, 0] for v in i_pics)


@PARSERS
@pytest.mark.parametrize("window", [1, 2, 3])
def test_open_gops(L, window, gpu_parser):
    """leading B pictures with predecessor have records and name the GOP before (inside a window and across windows: the carried
    anchor); without predecessor they are not delivered and every call's n is the window's n_frames"""
    from test_open_gop import BROKEN, GOPS, OPEN, dropped_positions, gop_entries
    data = open_stream(96, 64, 31)[0]
    want, _ = expected_motion(data)
    every = {(g, disp) for g, n in enumerate(GOPS) for _, disp, _, _ in gop_entries(n)}
    assert set(want) == every - dropped_positions(GOPS, OPEN, BROKEN)
    across = [k for k, v in want.items() if v[3] == k[0] - 1]
    assert across and all(want[k][4] >= 0 and want[k][5] >= 0 for k in across)
    got, order, _ = run_motion(L, data, gops_per_window=window, gpu_parser=gpu_parser)
    assert_motion(got, want, "window %d" % window)
    assert all(got[k][3] == k[0] - 1 for k in across)


@PARSERS
def test_exact_seek_trims(L, gpu_parser):
    """LEON_PIPELINE_SEEK_EXACT into GOP 3 of the open-GOP stream: trimmed frames have no record, the first delivered frame's is exact"""
    data = open_stream(96, 64, 31)[0]
    want3, _ = expected_motion(data, first_gop=3)
    import leon_vlc_ctypes as V
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
            for f in frames:
                m = f["motion"]
                log.append((window, (f["gop"], f["display_index"]), pipe.read_motion(window, f["_i"]) + (m["fwd_gop"], m["fwd_display"], m["bwd_display"])))
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=2, gpu_parser=gpu_parser, parser_threads=2)
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
    assert_motion(got, {k: v for k, v in want3.items() if k[0] != 3 or k[1] >= 4}, "EXACT seek")


def test_refusals(L):
    import ctypes as C
    data = open(os.path.join(STREAMS, "ibbp_96x64.jsv"), "rb").read()
    with pytest.raises(L.LeonError) as e:          # the bit alone
        L.Pipeline(data, output=L.PIPELINE_OUTPUT_MOTION)
    assert e.value.code == L.ERR_INVALID
    for bad in (64, 32 | 4, 32 | 8):               # other unknown bits stay refused beside it
        with pytest.raises(L.LeonError):
            L.Pipeline(data, output=bad | 1)
    seen = []

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        assert frames[0]["motion"] is None
        out = (L.PipelineMotionFrame * n)()
        seen.append(pipe.lib.leon_pipeline_window_motion(pipe.h, window, out, n))
        seen.append(pipe.lib.leon_pipeline_read_motion(pipe.h, window, 0, None, None, None))
        lay = L.PipelineMotionLayout()
        seen.append(pipe.lib.leon_pipeline_get_motion_layout(pipe.h, C.byref(lay)))
    pipe = L.Pipeline(data, on_window=on_window, gops_per_window=2)          # without the bit
    try:
        pipe.wait()
        assert pipe.error is None and pipe.motion_layout is None
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)
    seen = []

    def on_motion_window(window, frames):
        pipe = frames[0]["_pipe"]
        n = len(frames)
        out = (L.PipelineMotionFrame * (n + 1))()
        for bad_n in (n - 1, n + 1, 0, -1):
            seen.append(pipe.lib.leon_pipeline_window_motion(pipe.h, window, out, bad_n))
        seen.append(pipe.lib.leon_pipeline_read_motion(pipe.h, window, n, None, None, None))
        seen.append(pipe.lib.leon_pipeline_read_motion(pipe.h, window, -1, None, None, None))
        seen.append(pipe.lib.leon_pipeline_window_motion(pipe.h, window + 1000, out, n))
        assert pipe.lib.leon_pipeline_window_motion(pipe.h, window, out, n) == L.OK
        assert pipe.lib.leon_pipeline_read_motion(pipe.h, window, 0, None, None, None) == L.OK          # all three pointers may be NULL
    pipe = L.Pipeline(data, on_window=on_motion_window, gops_per_window=2, motion=True)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
        with pytest.raises(L.LeonError):          # every window has been released by now
            pipe.read_motion(0, 0)
    finally:
        pipe.close()
    assert seen and all(rc == L.ERR_INVALID for rc in seen)
