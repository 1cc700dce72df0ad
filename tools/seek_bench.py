#!/usr/bin/env python3
"""Seek-to-first-frame latency of the native pipeline (include/leon_pipeline.h): the time from a seek to the first
callback of the new position, over --seeks seeded random times --

  in place   leon_pipeline_seek on the running pipeline (KEY mode, or EXACT with --exact)
  recreate   leon_pipeline_destroy + leon_pipeline_create at start_seconds = t, what a host had to do before

-- in two geometries:
  player      the player's pipeline (js/leon_player.js): gops_per_window 1, 2 windows in flight, the 352x240 fixture
  throughput  the 1080p --varied stream of tools/stream_1080p.py, W = 128, R = 3, GPU parser

Prints one JSON line per geometry: median and maximum milliseconds of each.  Not bench.py's metric.

  python tools/seek_bench.py [--geometry player|throughput|both] [--seeks 32] [--seed 1648] [--exact]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")]


class Windows:
    """when each window was delivered (the callback's clock), for "the first window with an id >= floor" """

    def __init__(self):
        self.cv = threading.Condition()
        self.seen = []

    def on_window(self, window, frames):
        now = time.perf_counter()
        with self.cv:
            self.seen.append((window, now))
            self.cv.notify_all()

    def first_at_least(self, floor, timeout=60.0):
        def found():
            return next((t for w, t in self.seen if w >= floor), None)
        with self.cv:
            if not self.cv.wait_for(lambda: found() is not None, timeout):
                raise RuntimeError("no window of the new position within %.0f s" % timeout)
            at = found()
            self.seen.clear()
            return at


def geometry(name):
    if name == "player":
        data = open(os.path.join(ROOT, "tests", "golden", "streams", "leon_synth_352x240.jsv"), "rb").read()
        return data, dict(parser_threads=4, gops_per_window=1, windows_in_flight=2)
    import stream_1080p
    return stream_1080p.load_varied(), dict(parser_threads=16, gops_per_window=128, windows_in_flight=3, gpu_parser=True)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def run(name, seeks, seed, exact):
    import numpy as np
    import leon_ctypes as L
    data, kw = geometry(name)
    win = Windows()
    pipe = L.Pipeline(data, on_window=win.on_window, **kw)
    info = pipe.info
    duration = info.duration if info.duration > 0 else info.gops * 12 / max(info.picture_rate, 1.0)
    times = [float(t) for t in np.random.default_rng(seed).uniform(0.0, duration, seeks)]
    inplace, recreate = [], []
    try:
        win.first_at_least(0)
        for t in times:                            # seek the running pipeline
            t0 = time.perf_counter()
            first = pipe.seek(t, exact=exact)
            inplace.append((win.first_at_least(first) - t0) * 1e3)
        for t in times:                            # destroy the running pipeline, create one at t
            t0 = time.perf_counter()
            pipe.close()
            win = Windows()
            pipe = L.Pipeline(data, on_window=win.on_window, start_seconds=t, **kw)
            recreate.append((win.first_at_least(0) - t0) * 1e3)
    finally:
        pipe.close()
    out = {"geometry": name, "mode": "exact" if exact else "key", "seeks": seeks, "seed": seed,
           "frame": "%dx%d" % (info.frame_width, info.frame_height), "kw": kw,
           "in_place": summary(inplace), "recreate": summary(recreate)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["player", "throughput", "both"], default="both")
    ap.add_argument("--seeks", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1648)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    res = [run(g, a.seeks, a.seed, a.exact) for g in (["player", "throughput"] if a.geometry == "both" else [a.geometry])]
    if a.out:
        with open(a.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
