"""leon_pipeline_seek (include/leon_pipeline.h): a running pipeline moves to another time without being recreated --
KEY mode against a fresh pipeline created at that start_seconds and against the oracle, EXACT mode from the frame on
screen, held windows, seeks while windows are in flight, shards, partial streams, seeking after the end, refusals."""
import ctypes as C
import math
import os
import threading
import time

import numpy as np
import pytest

from test_pipeline_gpu import STREAMS, ibbp_stream, oracle_frames, run_pipeline

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def stream(name):
    if name == "ibbp8":
        return ibbp_stream(96, 64, [6, 9, 3, 12, 6, 9, 12, 3], seed=1618)
    return open(os.path.join(STREAMS, name + ".jsv"), "rb").read()


class Recorder:
    """what the callback saw, in the order it saw it: ("w", window, [(gop, display_index, ts_ms, rgba)]) entries and
    ("seek", first_window) markers the test appends after each seek returns"""

    def __init__(self, L, hold=0):
        self.L = L
        self.cv = threading.Condition()
        self.log = []
        self.hold = hold              # keep the first `hold` windows (copies of their frame records in self.held)
        self.held = []

    def on_window(self, window, frames):
        got = [(f["gop"], f["display_index"], f["ts_ms"], self.L.read_frame(f)) for f in frames]
        keep = False
        with self.cv:
            if len(self.held) < self.hold:
                recs = []
                for f in frames:
                    r = self.L.PipelineFrame()
                    C.pointer(r)[0] = f["_frames"][f["_i"]]
                    recs.append(r)
                self.held.append((window, recs, [g[3] for g in got]))
                keep = True
            self.log.append(("w", window, got))
            self.cv.notify_all()
        return False if keep else None

    def mark(self, first_window):
        with self.cv:
            self.log.append(("seek", first_window))

    def since(self, first_window):
        """order [(gop, display_index, ts_ms)] and frames {(gop, display_index): rgba} of windows >= first_window"""
        with self.cv:
            ws = sorted((e for e in self.log if e[0] == "w" and e[1] >= first_window), key=lambda e: e[1])
        order = [(g, d, ts) for _, _, fr in ws for g, d, ts, _ in fr]
        return order, {(g, d): px for _, _, fr in ws for g, d, _, px in fr}

    def wait_window(self, first_window, timeout=30):
        with self.cv:
            ok = self.cv.wait_for(lambda: any(e[0] == "w" and e[1] >= first_window for e in self.log), timeout)
        assert ok, "no window >= %d within %d s" % (first_window, timeout)

    def check_no_stale(self):
        """no callback carried an id below the first window of the latest seek that had returned before it"""
        floor = -1
        with self.cv:
            for e in self.log:
                if e[0] == "seek":
                    floor = e[1]
                else:
                    assert e[1] >= floor, "window %d delivered after a seek to first window %d returned" % (e[1], floor)


def read_held(pipe, rec, L):
    out = []
    for _, recs, _ in rec.held:
        for r in recs:
            a = np.empty((pipe.info.frame_height, pipe.info.frame_width, 4), np.uint8)
            assert pipe.lib.leon_pipeline_read_frame(pipe.h, C.byref(r), a.ctypes.data) == L.OK
            out.append(a)
    return out


def gop_times(order):
    """ts_ms of each GOP's first frame, from a full run's order"""
    first = {}
    for g, d, ts in order:
        first.setdefault(g, ts)
    return [first[g] for g in sorted(first)]


def exact_expected(key_order, t):
    """EXACT mode from the KEY order at t: the first GOP from its frame with the largest ts_ms <= t * 1000 on (none:
    all of it), every later GOP whole"""
    g0 = key_order[0][0]
    first = [o for o in key_order if o[0] == g0]
    at = [o for o in first if o[2] <= t * 1000.0]
    target = max(at, key=lambda o: o[2])[1] if at else min(o[1] for o in first)
    return [o for o in key_order if o[0] != g0 or o[1] >= target]


@PARSERS
@pytest.mark.parametrize("name", ["ibbp8", "leon_synth_352x240"])
def test_key_seek_equals_a_fresh_pipeline_and_the_oracle(L, gpu_parser, name):
    data = stream(name)
    want = oracle_frames(data)
    kw = dict(parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    _, full, _ = run_pipeline(L, data, **kw)
    gt = gop_times(full)
    assert len(gt) >= 2
    rec = Recorder(L)
    pipe = L.Pipeline(data, on_window=rec.on_window, **kw)
    try:
        rec.wait_window(0)
        for t in ((gt[-1] + 50.0) / 1000.0, (gt[len(gt) // 3] + 5.0) / 1000.0, 0.0):         # forward, backward, to the start
            fw = pipe.seek(t)
            rec.mark(fw)
            pipe.wait()
            assert pipe.ended and pipe.error is None
            order, got = rec.since(fw)
            f_got, f_order, _ = run_pipeline(L, data, start_seconds=t, **kw)
            assert order == f_order, "t = %.3f s: not the frames of a pipeline created at that time" % t
            assert order and order[0][0] == pipe.info.first_gop
            for k in f_got:
                assert np.array_equal(got[k], f_got[k]), "t = %.3f s: frame %s differs from the fresh pipeline's" % (t, k)
                assert np.array_equal(got[k], want[k]), "t = %.3f s: frame %s differs from the oracle" % (t, k)
        rec.check_no_stale()
        assert pipe.stats()["windows"] >= 4
    finally:
        pipe.close()


def exact_case(L, data, gpu_parser, flavour, times, oracle):
    kw = dict(parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, display_flavour=flavour)
    rec = Recorder(L)
    pipe = L.Pipeline(data, on_window=rec.on_window, **kw)
    try:
        pipe.wait()
        for t in times:
            fw = pipe.seek(t, exact=True)
            rec.mark(fw)
            pipe.wait()
            assert pipe.error is None
            order, got = rec.since(fw)
            k_got, k_order, _ = run_pipeline(L, data, start_seconds=t, **kw)
            exp = exact_expected(k_order, t)
            assert order == exp, "t = %.4f s: %s... instead of %s..." % (t, order[:3], exp[:3])
            g0 = k_order[0][0]
            at = [o[2] for o in k_order if o[0] == g0 and o[2] <= t * 1000.0]
            if at:
                assert order[0][2] == max(at)
            for g, d, _ in order:
                assert np.array_equal(got[(g, d)], k_got[(g, d)]), "t = %.4f s: frame %s differs from KEY mode's" % (t, (g, d))
                if oracle is not None:
                    assert np.array_equal(got[(g, d)], oracle[(g, d)]), "t = %.4f s: frame %s differs from the oracle" % (t, (g, d))
        rec.check_no_stale()
    finally:
        pipe.close()


def exact_times(L, data, gpu_parser):
    _, full, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    ts = sorted(o[2] for o in full)
    mid = len(ts) // 2
    in_b = [o[2] for o in full if o[0] == 2 and o[1] == 2][0]      # IBBP: display positions 1 and 2 are B pictures
    return [ts[mid] / 1000.0,                              # on a frame boundary
            (ts[mid + 1] + ts[mid + 2]) / 2000.0,          # between frames
            in_b / 1000.0 + 1e-4,                          # inside a B run
            ts[-1] / 1000.0 + 5.0,                         # past the last frame
            ts[3] / 1000.0]


@PARSERS
def test_exact_seek_starts_at_the_frame_on_screen(L, gpu_parser):
    data = stream("ibbp8")
    exact_case(L, data, gpu_parser, 0, exact_times(L, data, gpu_parser), oracle_frames(data))


@PARSERS
def test_exact_seek_on_the_unfused_road(L, gpu_parser):
    """a frame width that is no multiple of 8 (planes + a conversion launch per picture), and the GL display flavour
    (the unfused road too; its pixels are the KEY mode's, the oracle is the CPU twin)"""
    data = ibbp_stream(64, 48, [6, 9, 3, 12, 6], seed=62, frame=(61, 45))
    exact_case(L, data, gpu_parser, 0, exact_times(L, data, gpu_parser), oracle_frames(data))
    data = stream("ibbp8")
    exact_case(L, data, gpu_parser, 1, exact_times(L, data, gpu_parser)[:3], None)


@PARSERS
def test_held_windows_survive_a_seek(L, gpu_parser):
    data = stream("ibbp8")
    want = oracle_frames(data)
    rec = Recorder(L, hold=2)
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=1, windows_in_flight=3, gpu_parser=gpu_parser, on_window=rec.on_window)
    try:
        with rec.cv:
            assert rec.cv.wait_for(lambda: len(rec.held) == 2, 30)
        before = read_held(pipe, rec, L)
        assert all(np.array_equal(a, b) for a, b in zip(before, [px for _, _, pxs in rec.held for px in pxs]))
        fw = pipe.seek(0.0)
        rec.mark(fw)
        rec.wait_window(fw)
        after = read_held(pipe, rec, L)
        assert len(after) == len(before) and all(np.array_equal(a, b) for a, b in zip(before, after)), "a held window was overwritten"
        for w, _, _ in rec.held:
            pipe.release_window(w)
        pipe.wait()
        assert pipe.ended and pipe.error is None
        order, got = rec.since(fw)
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    finally:
        pipe.close()


@PARSERS
def test_seeks_while_windows_are_in_flight(L, gpu_parser):
    data = ibbp_stream(96, 64, [6, 9, 3, 12] * 4, seed=2024)
    want = oracle_frames(data)
    kw = dict(parser_threads=3, gops_per_window=2, windows_in_flight=2, gpu_parser=gpu_parser)
    _, full, _ = run_pipeline(L, data, **kw)
    end_s = max(o[2] for o in full) / 1000.0
    rng = np.random.default_rng(20)
    rec = Recorder(L)
    pipe = L.Pipeline(data, on_window=rec.on_window, **kw)
    try:
        rec.wait_window(0)
        fw = 0
        for i in range(20):
            t = float(rng.uniform(0.0, end_s * 1.05))
            fw = pipe.seek(t, exact=bool(i % 3 == 2))
            ends = pipe.ends
            rec.mark(fw)
            rec.wait_window(fw)
        pipe.wait()
        assert pipe.ends - ends == 1, "the last run ended %d times" % (pipe.ends - ends)
        assert pipe.error is None
        rec.check_no_stale()
        order, got = rec.since(fw)
        k_got, k_order, _ = run_pipeline(L, data, start_seconds=t, **kw)
        assert order == (exact_expected(k_order, t) if i % 3 == 2 else k_order)
        for g, d, _ in order:
            assert np.array_equal(got[(g, d)], want[(g, d)]), "frame %s differs from the oracle" % ((g, d),)
    finally:
        pipe.close()


@PARSERS
def test_seek_with_shards(L, gpu_parser):
    data = stream("ibbp8")
    kw = dict(parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    _, full, _ = run_pipeline(L, data, **kw)
    gt = gop_times(full)
    for t, exact in (((gt[3] + 30.0) / 1000.0, False), ((gt[2] + 50.0) / 1000.0, True)):
        union = {}
        for si in range(2):
            rec = Recorder(L)
            pipe = L.Pipeline(data, shard_index=si, shard_count=2, on_window=rec.on_window, **kw)
            try:
                rec.wait_window(0)
                fw = pipe.seek(t, exact=exact)
                rec.mark(fw)
                pipe.wait()
                order, got = rec.since(fw)
                assert all(g % 2 == si for g, _, _ in order), "shard %d delivered %s" % (si, sorted({g for g, _, _ in order}))
                assert not set(got) & set(union)
                union.update(got)
            finally:
                pipe.close()
        u_got, u_order, _ = run_pipeline(L, data, start_seconds=t, **kw)
        exp = exact_expected(u_order, t) if exact else u_order
        assert sorted(union) == sorted((g, d) for g, d, _ in exp)
        for k in union:
            assert np.array_equal(union[k], u_got[k])


@PARSERS
def test_seek_in_a_stream_that_is_still_arriving(L, gpu_parser):
    import leon_vlc_ctypes as V
    data = stream("ibbp8")
    want = oracle_frames(data)
    offs = V.Stream(data, threads=1).keymap()
    first = offs[2] + 3                  # GOPs 0 and 1 complete
    _, full, _ = run_pipeline(L, data, parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser)
    t = (gop_times(full)[5] + 20.0) / 1000.0
    buf = bytearray(len(data))
    buf[:first] = data[:first]
    rec = Recorder(L)
    pipe = L.Pipeline(bytes(buf), parser_threads=2, gops_per_window=1, gpu_parser=gpu_parser, on_window=rec.on_window, valid_bytes=first)
    try:
        rec.wait_window(0)
        fw = pipe.seek(t)
        rec.mark(fw)
        first_gop = pipe.info.first_gop
        assert offs[first_gop] > first
        time.sleep(0.3)
        assert rec.since(fw)[0] == [], "frames of GOPs whose bytes have not arrived"
        pipe.feed(len(data), data[first:], first)
        pipe.wait()
        assert pipe.error is None
        order, got = rec.since(fw)
        assert sorted(got) == sorted(k for k in want if k[0] >= first_gop)
        assert all(np.array_equal(got[k], want[k]) for k in got)
    finally:
        pipe.close()


@PARSERS
def test_seek_after_the_end_and_refusals(L, gpu_parser):
    data = stream("ibbp8")
    want = oracle_frames(data)
    kw = dict(parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    refused = []

    def seek_inside(window, frames):
        if not refused:
            try:
                frames[0]["_pipe"].seek(0.0)
            except L.LeonError as e:
                refused.append(e)
            except Exception as e:           # anything else is a failure, reported below
                refused.append(e)
        rec.on_window(window, frames)

    rec = Recorder(L)
    pipe = L.Pipeline(data, on_window=seek_inside, **kw)
    try:
        pipe.wait()
        assert pipe.ends == 1 and pipe.ended
        assert len(refused) == 1 and isinstance(refused[0], L.LeonError), refused      # from inside the callback
        for bad in (dict(seconds=0.1, mode=7), dict(seconds=math.nan), dict(seconds=math.inf)):
            with pytest.raises(L.LeonError):
                pipe.seek(**bad)
        assert pipe.ended and pipe.ends == 1             # nothing changed
        fw = pipe.seek(0.0)
        rec.mark(fw)
        pipe.wait()
        assert pipe.ends == 2 and pipe.ended and pipe.error is None
        order, got = rec.since(fw)
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
        rec.check_no_stale()
    finally:
        pipe.close()
    # benchmark mode does not seek, and the refusal leaves the run alone
    rec = Recorder(L)
    pipe = L.Pipeline(data, loop=3, on_window=rec.on_window, **kw)
    try:
        with pytest.raises(L.LeonError):
            pipe.seek(0.2)
        pipe.wait()
        assert pipe.ends == 1 and pipe.error is None
        assert len(rec.since(0)[1]) == 3 * len(want)
    finally:
        pipe.close()
