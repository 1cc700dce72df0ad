"""GPU: the pipeline decodes open GOPs (include/leon_pipeline.h "Open GOPs").  The leading B pictures of an open GOP predict
forward from the last anchor of the GOP before it -- inside a window from the lane before, across windows from the carry slot;
an open GOP without its predecessor (first of a run or of a loop pass, the target of a seek, broken_link) delivers from its I
picture on.  Expected frames: test_open_gop.open_gop_frames (held against the writer's tensors there)."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from test_open_gop import BROKEN, GOPS, OPEN, dropped_positions, gop_entries, open_gop_frames, open_stream
from test_pipeline_gpu import oracle_frames, run_pipeline

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


class Case:
    """a stream, its expected frames from the start, and the presentation time of each GOP header"""

    def __init__(self, cw, ch, seed, **kw):
        import leon_vlc_ctypes as V
        self.data, self.pics, self.starts = open_stream(cw, ch, seed, **kw)
        self.rgba, self.planes = open_gop_frames(self.data)
        st = V.Stream(self.data, threads=1)
        self.offs = st.keymap()
        self.gop_ts = []
        while True:
            p = st.next_picture()
            if p is None:
                break
            if p["type"] == 1:
                self.gop_ts.append(p["ts"])
        self._from = {0: self.rgba}

    def frames_from(self, gop):
        if gop not in self._from:
            self._from[gop] = open_gop_frames(self.data, gop)[0]
        return self._from[gop]

    def time_of(self, gop, display_index, plus_ms=1.0):
        """seconds: just behind the start of that display position (25 pictures/s)"""
        return (self.gop_ts[gop] + 40.0 * display_index + plus_ms) / 1000.0


@pytest.fixture(scope="module")
def big():
    return Case(96, 64, 31)


@pytest.fixture(scope="module")
def small():
    return Case(48, 32, 32)


def assert_rgba(got, want, what=""):
    assert sorted(got) == sorted(want), "%s: frames delivered and not expected %s, expected and missing %s" % (
        what, sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for k in sorted(want):
        assert np.array_equal(got[k], want[k]), "%s: frame %s differs from the oracle in %d bytes" % (what, k, int((got[k] != want[k]).sum()))


@PARSERS
@pytest.mark.parametrize("inflight", [2, 3])
@pytest.mark.parametrize("window", [1, 2, 3])
def test_frames_equal_the_oracle(L, big, window, inflight, gpu_parser):
    """GOP borders inside a window (the lane before's slot) and between windows (the carry slot): the key set -- the broken
    link's leading B pictures absent, nothing else missing -- and every pixel"""
    got, order, stats = run_pipeline(L, big.data, parser_threads=2, gops_per_window=window, windows_in_flight=inflight, gpu_parser=gpu_parser)
    every = {(g, disp) for g, n in enumerate(GOPS) for _, disp, _, _ in gop_entries(n)}
    assert set(big.rgba) == every - dropped_positions(GOPS, OPEN, BROKEN) == every - {(6, 0), (6, 1)}
    assert_rgba(got, big.rgba, "window %d" % window)
    assert stats["pictures"] == len(big.rgba) and stats["gops"] == len(GOPS)      # pictures: what was decoded
    assert order == sorted(order)


# whole IBBP-12 GOPs in a row, all open: four anchors each, so a GOP's leading B pictures wait for level 4 (behind a 12) or 3 (behind
# the 9, three anchors) while its own fourth anchor, level 3, reuses the first anchor slot of the lane
LONG_GOPS = (12, 9, 12, 12)


@pytest.fixture(scope="module")
def long_gops():
    return Case(48, 32, 36, gops=LONG_GOPS, open_gops=(0, 1, 2, 3), broken=())


@PARSERS
@pytest.mark.parametrize("window", [1, 2, 3, 4])
def test_long_open_gops_keep_their_i_picture(L, long_gops, window, gpu_parser):
    """the backward reference of a leading B picture is its GOP's I picture, also when the GOP has four anchors and sits behind
    another in one window (windows of 2, 3, 4: lanes 1 .. 3 -- the I picture must outlive the lane's slot rotation) and when
    it is a window's first GOP (window 1: the carry slot)"""
    every = {(g, disp) for g, n in enumerate(LONG_GOPS) for _, disp, _, _ in gop_entries(n)}
    assert set(long_gops.rgba) == every - {(0, 0), (0, 1)}
    got, _, stats = run_pipeline(L, long_gops.data, parser_threads=2, gops_per_window=window, gpu_parser=gpu_parser)
    assert_rgba(got, long_gops.rgba, "window %d" % window)
    assert stats["pictures"] == len(long_gops.rgba)


@PARSERS
def test_the_unfused_road_with_planes(L, gpu_parser):
    """96 x 64 coded, 92 x 64 shown: every picture writes its planes (B pictures into slots of their own), converted and
    cropped by launches of their own"""
    from test_pipeline_planes_gpu import assert_planes, run_planes
    data = open_stream(96, 64, 33, gops=GOPS + (12,), open_gops=OPEN + (7,), frame=(92, 64))[0]       # (GOP 7: a whole open GOP behind a whole one)
    rgba, planes = open_gop_frames(data)
    for window in (2, 3):
        got_planes, got_rgba, _ = run_planes(L, data, "both", parser_threads=2, gops_per_window=window, gpu_parser=gpu_parser)
        assert_planes(got_planes, planes, "window %d" % window)
        assert_rgba(got_rgba, rgba, "window %d" % window)


def test_outputs_follow_the_frames(L, big):
    """YCbCr planes and uint8 HWC tensors of the same stream, through their definitions, against the RGBA run's frames"""
    from oracle import oracle_py as O
    from test_pipeline_planes_gpu import run_planes
    ref, _, _ = run_pipeline(L, big.data, parser_threads=2, gops_per_window=2, gpu_parser=True)
    assert_rgba(ref, big.rgba)
    planes, none, _ = run_planes(L, big.data, "ycbcr", parser_threads=2, gops_per_window=2, gpu_parser=True)
    assert all(v is None for v in none.values())
    assert_rgba({k: O.ycbcr_to_rgba(y, cb, cr, 96, 96, 64, "cpu") for k, (y, cb, cr) in planes.items()}, ref, "ycbcr")
    tensors = {}

    def on_window(window, frames):
        for f in frames:
            tensors[(f["gop"], f["display_index"])] = f["_pipe"].read_tensor(f)
    pipe = L.Pipeline(big.data, parser_threads=2, gops_per_window=2, gpu_parser=True, on_window=on_window, output="tensor", tensor_dtype="uint8", tensor_layout="hwc")
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None
    finally:
        pipe.close()
    assert_rgba(tensors, {k: v[..., :3] for k, v in ref.items()}, "uint8 HWC tensors")


@PARSERS
def test_every_loop_pass_starts_without_predecessor(L, gpu_parser):
    """loop = 2 over a stream whose first GOP is open: both passes drop its leading B pictures (pass two's first GOP does not
    predict from pass one's last), every other frame of pass two equals pass one's; the pass border falls inside a window"""
    gops = (4, 6, 3)
    data = open_stream(48, 32, 34, gops=gops, open_gops=(0, 1, 2), broken=())[0]
    want = open_gop_frames(data)[0]
    assert set(want) == {(g, disp) for g, n in enumerate(gops) for _, disp, _, _ in gop_entries(n)} - {(0, 0), (0, 1)}
    got, _, stats = run_pipeline(L, data, parser_threads=2, gops_per_window=2, loop=2, gpu_parser=gpu_parser)
    assert_rgba(got, {**want, **{(g + len(gops), d): v for (g, d), v in want.items()}})
    assert stats["pictures"] == 2 * len(want) and stats["gops"] == 2 * len(gops)


def seek_and_collect(L, pipe, rec, t, exact=False):
    fw = pipe.seek(t, exact=exact)
    rec.mark(fw)
    pipe.wait()
    assert pipe.ended and pipe.error is None
    return rec.since(fw)


@PARSERS
def test_seeks_onto_an_open_gop(L, small, gpu_parser):
    """KEY and EXACT seeks onto GOP 4 (open; behind GOP 3 in a whole run): its leading B pictures are absent, GOP 5 -- which
    predicts from GOP 4's last anchor -- is complete and correct; an EXACT target inside the dropped pictures starts at the I
    picture; then a seek back to the start gives the whole run again"""
    from test_pipeline_seek_gpu import Recorder, exact_expected
    want4 = small.frames_from(4)
    assert (4, 0) in small.rgba and (4, 0) not in want4 and (4, 1) not in want4 and {(5, 0), (5, 1)} <= set(want4)
    assert all(np.array_equal(small.rgba[k], want4[k]) for k in want4)       # what is still delivered is what a whole run delivers
    kw = dict(parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    rec = Recorder(L)
    pipe = L.Pipeline(small.data, on_window=rec.on_window, **kw)
    try:
        pipe.wait()
        assert_rgba(rec.since(0)[1], small.rgba, "whole run")
        order, got = seek_and_collect(L, pipe, rec, small.time_of(4, 2))                          # KEY, at the I picture
        assert pipe.info.first_gop == 4 and order[0][:2] == (4, 2)
        assert_rgba(got, want4, "KEY seek")
        key_order = order
        order, got = seek_and_collect(L, pipe, rec, small.time_of(4, 1), exact=True)              # EXACT inside the dropped pictures
        assert order == key_order
        assert_rgba(got, want4, "EXACT seek onto a dropped frame")
        order, got = seek_and_collect(L, pipe, rec, small.time_of(4, 4), exact=True)              # EXACT at a B picture behind the I
        assert order == exact_expected(key_order, small.time_of(4, 4)) and order[0][:2] == (4, 4)
        assert_rgba(got, {k: v for k, v in want4.items() if k[0] != 4 or k[1] >= 4}, "EXACT seek")
        order, got = seek_and_collect(L, pipe, rec, 0.0)
        assert_rgba(got, small.rgba, "back to the start")
        rec.check_no_stale()
    finally:
        pipe.close()


@PARSERS
def test_a_seek_while_windows_are_in_flight_starts_clean(L, small, gpu_parser):
    """one GOP per window, three windows in flight, a seek as soon as the first window is out: windows of the old run are
    submitted and drained around the seek, and their last anchors are other pictures than GOP 4's.  GOP 5 of the new run
    predicts from the new run's GOP 4 -- the frames of a fresh pipeline created at that time, and the oracle's"""
    from test_pipeline_seek_gpu import Recorder
    kw = dict(parser_threads=2, gops_per_window=1, windows_in_flight=3, gpu_parser=gpu_parser)
    t = small.time_of(4, 2)
    fresh, fresh_order, _ = run_pipeline(L, small.data, start_seconds=t, **kw)
    assert_rgba(fresh, small.frames_from(4), "fresh pipeline at start_seconds")
    rec = Recorder(L)
    pipe = L.Pipeline(small.data, on_window=rec.on_window, **kw)
    try:
        rec.wait_window(0)
        order, got = seek_and_collect(L, pipe, rec, t)
        assert order == fresh_order
        assert_rgba(got, fresh, "seek in flight")
        rec.check_no_stale()
    finally:
        pipe.close()


@PARSERS
def test_shards_still_refuse_open_gops(L, gpu_parser):
    """a shard never holds a GOP's neighbour: an open GOP with leading B pictures is refused at wait(), not decoded with
    pictures missing; a closed stream is sharded as before"""
    gops = (6, 6, 6, 6)
    data = open_stream(48, 32, 35, gops=gops, open_gops=(1, 2, 3), broken=(3,))[0]
    for si in range(2):
        pipe = L.Pipeline(data, parser_threads=2, gops_per_window=2, shard_index=si, shard_count=2, gpu_parser=gpu_parser)
        try:
            with pytest.raises(L.LeonError) as e:
                pipe.wait()
            assert "is open (closed_gop = 0)" in str(e.value) and "GOP shards must be closed" in str(e.value)
        finally:
            pipe.close()
    closed = open_stream(48, 32, 35, gops=gops, open_gops=(), broken=())[0]
    want, got = oracle_frames(closed), {}
    for si in range(2):
        part, _, _ = run_pipeline(L, closed, parser_threads=2, gops_per_window=2, shard_index=si, shard_count=2, gpu_parser=gpu_parser)
        assert {g % 2 for g, _ in part} == {si} and not set(part) & set(got)
        got.update(part)
    assert_rgba(got, want, "closed stream in two shards")


@PARSERS
def test_a_stream_that_arrives_gop_by_gop(L, small, gpu_parser):
    data, offs = small.data, small.offs
    ends = [min(o + 3, len(data)) for o in offs[1:]] + [len(data)]
    buf = bytearray(len(data))
    buf[:ends[0]] = data[:ends[0]]
    got = {}

    def on_window(window, frames):
        for f in frames:
            got[(f["gop"], f["display_index"])] = L.read_frame(f)
    pipe = L.Pipeline(bytes(buf), parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, on_window=on_window, valid_bytes=ends[0])
    try:
        for a, b in zip(ends, ends[1:]):
            pipe.feed(b, data[a:b], a)
        pipe.wait()
        assert pipe.ended and pipe.error is None
    finally:
        pipe.close()
    assert_rgba(got, small.rgba, "partial stream")


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_delivers_the_same_frames(L, small, tmp_path):
    path = tmp_path / "open.jsv"
    path.write_bytes(small.data)
    out = subprocess.run(["node", os.path.join(ROOT, "tools", "js_pipeline_bench.js"), str(path), "--hash", "--threads", "2", "--window", "2", "--gpu-parser"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    js = json.loads(out.stdout.strip().splitlines()[-1])
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    py, _, _ = run_pipeline(L, small.data, parser_threads=2, gops_per_window=2, gpu_parser=True)
    assert_rgba(py, small.rgba)
    assert js["pictures"] == len(py) == len(js["frames"])
    assert {(f["gop"], f["displayIndex"]): f["sha256"] for f in js["frames"]} == {k: sha(v) for k, v in py.items()}
