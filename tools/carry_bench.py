#!/usr/bin/env python3
"""Boxes carried along the motion vectors of a delivered 1080p window (include/leon_pipeline.h, leon_pipeline_carry_regions; k_carry):
what one hop and what the whole GOP cost on the device, from the enqueue to the synchronisation of the stream, beside the only road
there was before -- read_motion to the host and the vectors under every box averaged there (leon_ctypes.carry_box).

The stream is the varied 1080p IBBP stream of tools/stream_1080p.py (16 GOPs of 12 pictures), one window, motion=True.  --boxes N
seeded boxes of up to --max-box pixels a side lie on the first GOP's I picture:
  single hop   N records I -> the first P picture, one carry_regions_device call (one k_carry launch)
  gop          carry_regions_gop: the N boxes to all 12 frames of the GOP, one call per level of carry_plan, gathers by torch indexing
  host         read_motion of the P picture's record, then carry_box for the same N records
Prints one JSON line.

  python tools/carry_bench.py [--boxes 4096] [--reps 20] [--max-box 256] [--host-boxes N]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-box", type=int, default=256)
    ap.add_argument("--host-boxes", type=int, default=None, help="boxes of the host yardstick (default: all of --boxes)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import leon_ctypes as L
    import stream_1080p
    data = stream_1080p.load_varied()
    held, delivered = {}, threading.Event()

    def on_window(window, frames):
        if held:
            return None
        held["window"], held["frames"] = window, list(frames)
        delivered.set()
        return False
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=stream_1080p.VARIED_GOPS, gpu_parser=True, parser_threads=16)
    try:
        if not delivered.wait(300):
            raise RuntimeError("no window was delivered: %s" % (pipe.error,))
        window, frames = held["window"], held["frames"]
        fw, fh, n = pipe.info.frame_width, pipe.info.frame_height, len(frames)
        src = [i for i, f in enumerate(frames) if f["type"] == L.PIC_I][0]
        fwd, bwd = pipe.carry_refs(window)
        tgt = [i for i, f in enumerate(frames) if f["type"] == L.PIC_P and fwd[i] == src][0]
        rng = np.random.default_rng(1080)
        w = rng.integers(16, a.max_box + 1, size=a.boxes)
        h = rng.integers(16, a.max_box + 1, size=a.boxes)
        boxes = np.stack([rng.integers(0, fw - w + 1), rng.integers(0, fh - h + 1), w, h], axis=1).astype(np.int32)
        rec = np.zeros((a.boxes, 8), dtype=np.int32)
        rec[:, 0], rec[:, 1:5], rec[:, 5] = src, boxes, tgt
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_rec, d_boxes = torch.tensor(rec, device="cuda"), torch.tensor(boxes, device="cuda")
            out = torch.empty((a.boxes, 8), dtype=torch.int32, device="cuda")
            votes = torch.empty((a.boxes, 4), dtype=torch.int32, device="cuda")
            status = torch.empty((a.boxes,), dtype=torch.int32, device="cuda")
            hop_us, hop_enqueue_us, gop_us, gop_enqueue_us = [], [], [], []
            for i in range(a.reps + 2):          # (the first two: the scratch, the stream and torch's allocator warm up)
                st.synchronize()
                t0 = time.perf_counter()
                pipe.carry_regions_device(window, d_rec, out=out, votes=votes, status=status)
                t1 = time.perf_counter()
                st.synchronize()
                t2 = time.perf_counter()
                if i >= 2:
                    hop_us.append((t2 - t0) * 1e6)
                    hop_enqueue_us.append((t1 - t0) * 1e6)
            hop = (out.cpu().numpy(), votes.cpu().numpy(), status.cpu().numpy())
            for i in range(a.reps + 2):
                st.synchronize()
                t0 = time.perf_counter()
                g_rec, g_votes, g_status = pipe.carry_regions_gop(window, d_boxes, src)
                t1 = time.perf_counter()
                st.synchronize()
                t2 = time.perf_counter()
                if i >= 2:
                    gop_us.append((t2 - t0) * 1e6)
                    gop_enqueue_us.append((t1 - t0) * 1e6)
            gop_frames = [i for i, f in enumerate(frames) if f["gop"] == frames[src]["gop"]]
            gop_ok = int((g_status[gop_frames] == 0).sum().item())
        levels, unreachable = L.carry_plan((fwd, bwd), frames, src)
        # the road there was: the record to the host, the vectors under every box averaged there
        m = a.boxes if a.host_boxes is None else min(a.boxes, a.host_boxes)
        t0 = time.perf_counter()
        mv, info, _ = pipe.read_motion(window, tgt)
        t1 = time.perf_counter()
        records = [None] * n
        records[tgt] = (mv, info)
        same = 0
        for k in range(m):
            s, o, v = L.carry_box(fw, fh, n, fwd, bwd, records, rec[k])
            same += s == hop[2][k] and (s != 0 or (o == hop[0][k].tolist() and v == hop[1][k].tolist()))
        t2 = time.perf_counter()
        if same != m:
            raise RuntimeError("the device and carry_box disagree in %d of %d records" % (m - same, m))
        med = statistics.median
        print(json.dumps({"bench": "carry", "frame": [fw, fh], "window_frames": n, "boxes": a.boxes, "reps": a.reps, "max_box": a.max_box,
                          "single_hop_us": round(med(hop_us), 1), "single_hop_min_us": round(min(hop_us), 1), "single_hop_enqueue_us": round(med(hop_enqueue_us), 1),
                          "gop_levels": len(levels), "gop_hops": sum(len(x) for x in levels), "gop_unreachable": len(unreachable), "gop_records_ok": gop_ok,
                          "gop_us": round(med(gop_us), 1), "gop_min_us": round(min(gop_us), 1), "gop_enqueue_us": round(med(gop_enqueue_us), 1),
                          "host_boxes": m, "host_read_motion_us": round((t1 - t0) * 1e6, 1), "host_carry_box_us": round((t2 - t1) * 1e6, 1),
                          "host_us_per_4096": round(((t1 - t0) + (t2 - t1) * a.boxes / max(1, m)) * 1e6, 1), "device_equals_host": True,
                          "moved": int((hop[1][:, 2:] != 0).any(axis=1).sum())}))
        pipe.release_window(window)
        pipe.wait()
    finally:
        pipe.close()


if __name__ == "__main__":
    main()
