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

--gauge: in the same job, the boxes the single hop moved (its output records, on the P picture) go through gauge_regions_device
(leon_pipeline_gauge_regions; k_gauge) for sources 1 (motion), 2 (activity) and 3 (both): the time of one call beside the single hop's
on the same boxes, and the first --gauge-check records against gauge_box on the records read back.  The pipeline then runs with
activity=True as well.

--maps: dense maps instead (leon_pipeline_propagate_maps; k_propagate): a map on the first GOP's I picture propagated to the GOP's 12
frames by propagate_maps_gop, for three shapes -- a uint8 label mask [1, 1080, 1920] at stride 1, fp16 heatmaps [17, 270, 480] at
stride 4, fp16 features [256, 68, 120] at stride 16 -- from the enqueue to the synchronisation of the stream; the bytes the hops
read and write a second beside the rate of a device-to-device copy of as many bytes measured in the same run; and the road a user
had before: motion_view, a per-cell index grid built with torch ops and a gather, hop by hop in the same order, whose result is
compared with the kernel's byte for byte.  Prints one JSON line.

--propose: boxes proposed instead (leon_pipeline_propose_regions; k_propose): one propose_regions_device call over EVERY frame of the
window with both sources (--mv-min, --ac-min, K = --max-boxes, connectivity 8), from the enqueue to the synchronisation of the
stream; the first --propose-check frames against propose_boxes on the records read back; then the [F, K, 8] result as it is into
gauge_regions_device in the same job (word 0 = w * h for the first count rows, REGION_BOX behind).  The bytes the kernel must read --
F x (8 + 1 + 8) x the macroblocks of a frame -- are set against the time.  Prints one JSON line.

--suppress / --match: boxes compared by overlap instead (leon_pipeline_suppress_regions, leon_pipeline_match_regions; k_suppress,
k_match): for K = 64, 256 and 1024, F sets of K seeded boxes of side 16 .. 160, one set on each of the F frames of the window, in ONE
suppress_regions_device (IOU 0.5 and IOMIN 0.75, seeded scores) or match_regions_device (IOU 0.3, against a second seeded tensor)
call, from the enqueue to the synchronisation of the stream; the first --overlap-check sets against suppress_boxes / match_boxes;
beside it the same call through the host road (suppress_regions / match_regions on numpy arrays: the upload, the launch and the
copies back -- the round trip a user had to make, with a numpy loop in place of the launch).  --match adds the worst case of the
mutual-best rounds: ONE pair of sets of 256 and of 1024 identical boxes, a pair a round.  Both print one JSON line.

--accumulate: motion and residual accumulated instead (leon_pipeline_accumulate; k_accumulate): accumulate_gop from the first GOP's I
picture to the GOP's 12 frames for parts 1 (AX AY AGE), 2 (RY RCb RCr) and 3, from the enqueue to the synchronisation of the stream;
one level of the plan and one hop alone (one accumulate_device call each); the bytes a hop moves from the shapes -- the source planes
read, the target's residual record read, the destination planes written -- beside a device-to-device copy that moves as many bytes,
measured in the same run; one hop of parts 3 against accumulate_hop on the records read back; and the road a user had before for
that hop: three propagate_maps_device calls (AX AY AGE RY at stride 1, RCb RCr at stride 2, a coordinate map to recover the clamped
displacement) with the elementwise torch adds around them -- no saturation, restart cells not rebased: a yardstick of time alone.  Its
first call is k_propagate at stride 1, int16, 4 planes, timed by itself as well.  The pipeline then runs with residual=True.  --parts
names the parts timed (under a profiler one at a time: the launches of parts 1 and 2 have the same grid).

--fields: boxes of the records as a model's tensors instead (leon_pipeline_field_tensors; k_box_tables and k_fields): --boxes seeded
boxes of 16 .. --max-box pixels a side spread over the window's frames to 224 x 224 fp16, once from the motion records (2 channels:
fwd_h, fwd_v at scale 0.5) and once from the residual records (3 channels: Y, Cb, Cr at scale 1 / 128), one call each, from the enqueue
to the synchronisation of the stream; the bytes the call writes; the first --fields-check records against field_tensor on the records
read back; and the road a user has today for --torch-boxes of the same boxes on the same views, box by box: the cells under the box,
repeat_interleave to pixels, the crop, F.interpolate(mode="bilinear", antialias=True), a multiply-add and the cast -- a yardstick of
time alone: its filter is not the pixel tensors' and its values differ.  The pipeline then runs with residual=True.  --fields-source
names the sources timed (under a profiler one at a time: the launches have the same names).

  python tools/carry_bench.py [--boxes 4096] [--reps 20] [--max-box 256] [--host-boxes N] [--gauge [--gauge-check 64]]
  python tools/carry_bench.py --maps [--reps 20]
  python tools/carry_bench.py --propose [--reps 20] [--mv-min 2] [--ac-min 256] [--max-boxes 16] [--propose-check 8]
  python tools/carry_bench.py --suppress | --match [--reps 20] [--overlap-check 2]
  python tools/carry_bench.py --accumulate [--reps 20] [--parts 1,2,3]
  python tools/carry_bench.py --fields [--boxes 4096] [--reps 20] [--max-box 256] [--torch-boxes 256] [--fields-check 4] [--fields-source motion,residual]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")]


MAP_SHAPES = [("uint8 mask", 1, "uint8", 1), ("fp16 heatmaps", 4, "float16", 17), ("fp16 features", 16, "float16", 256)]          # name, stride, dtype, planes


def torch_hop(torch, pipe, window, t, src_f, src_b, s, fill_value):
    """one hop with torch ops alone: the target's record in place (motion_view), a per-cell index grid, a gather per direction"""
    mv, info, _ = pipe.motion_view(window, t)
    planes, mh, mw = (src_f if src_f is not None else src_b).shape
    dev = mv.device
    cy, cx = torch.meshgrid(torch.arange(mh, device=dev), torch.arange(mw, device=dev), indexing="ij")
    kj, ki = (cy * s) >> 4, (cx * s) >> 4
    f, v = info[kj, ki].to(torch.int32), mv[kj, ki].to(torch.int32)
    use_f = ((f & 1) != 0) if src_f is not None else torch.zeros_like(f, dtype=torch.bool)
    use_b = ~use_f & ((f & 2) != 0) if src_b is not None else torch.zeros_like(use_f)
    vh, vv = torch.where(use_f, v[..., 0], v[..., 2]), torch.where(use_f, v[..., 1], v[..., 3])
    sx = (cx + torch.div(vh + s, 2 * s, rounding_mode="floor")).clamp(0, mw - 1)
    sy = (cy + torch.div(vv + s, 2 * s, rounding_mode="floor")).clamp(0, mh - 1)
    at = (sy * mw + sx).reshape(-1)
    out = torch.full((planes, mh * mw), fill_value, dtype=(src_f if src_f is not None else src_b).dtype, device=dev)
    if src_f is not None:
        out = torch.where(use_f.reshape(1, -1), src_f.reshape(planes, -1)[:, at], out)
    if src_b is not None:
        out = torch.where(use_b.reshape(1, -1), src_b.reshape(planes, -1)[:, at], out)
    return out.reshape(planes, mh, mw)


def maps_bench(a, pipe, window, frames):
    import torch
    import leon_ctypes as L
    fw, fh = pipe.info.frame_width, pipe.info.frame_height
    src = [i for i, f in enumerate(frames) if f["type"] == L.PIC_I][0]
    rows = pipe.gop_frames(window, src)
    levels, unreachable = L.propagate_plan(pipe.carry_refs(window), frames, src)
    hops = sum(len(x) for x in levels)
    med = statistics.median
    result = {"bench": "propagate", "frame": [fw, fh], "window_frames": len(frames), "gop_frames": len(rows), "gop_levels": len(levels), "gop_hops": hops,
              "gop_unreachable": len(unreachable), "reps": a.reps, "shapes": []}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for name, s, dtype, planes in MAP_SHAPES:
            lay = L.propagate_layout(fw, fh, s, planes, 1 if dtype == "uint8" else 2)
            bits = torch.uint8 if dtype == "uint8" else torch.int16
            g = torch.Generator(device="cuda").manual_seed(s)
            m = torch.randint(0, 256 if dtype == "uint8" else 32767, (planes, lay.mh, lay.mw), generator=g, device="cuda", dtype=bits)
            m = m if dtype == "uint8" else m.view(torch.float16)
            gop_us, enqueue_us = [], []
            for i in range(a.reps + 2):          # (the first two: the scratch, the stream and torch's allocator warm up)
                st.synchronize()
                t0 = time.perf_counter()
                maps, via, status = pipe.propagate_maps_gop(window, m, src, s, fill=0)
                t1 = time.perf_counter()
                st.synchronize()
                t2 = time.perf_counter()
                if i >= 2:
                    gop_us.append((t2 - t0) * 1e6)
                    enqueue_us.append((t1 - t0) * 1e6)
            # the bytes the hops move: every hop reads a map's worth of source cells and the record, writes a map and its via bytes
            moved = hops * (2 * lay.slot_bytes + lay.mh * lay.mw)
            a_, b_ = torch.empty(hops * lay.slot_bytes, dtype=torch.uint8, device="cuda"), torch.empty(hops * lay.slot_bytes, dtype=torch.uint8, device="cuda")
            copy_us = []
            for i in range(a.reps + 2):
                st.synchronize()
                t0 = time.perf_counter()
                b_.copy_(a_)
                st.synchronize()
                if i >= 2:
                    copy_us.append((time.perf_counter() - t0) * 1e6)
            # the road there was, in the levels' order, and its result against the kernel's
            slot = {f: i for i, f in enumerate(rows)}
            mb = m.view(bits)
            torch_us = []
            for i in range(min(a.reps, 5) + 1):
                st.synchronize()
                t0 = time.perf_counter()
                ref = {src: mb}
                for level in levels:
                    for t, f, b in level:
                        ref[t] = torch_hop(torch, pipe, window, t, ref.get(f) if f >= 0 else None, ref.get(b) if b >= 0 else None, s, 0)
                st.synchronize()
                if i >= 1:
                    torch_us.append((time.perf_counter() - t0) * 1e6)
            got = maps.view(bits)
            same = all(torch.equal(got[slot[t]], ref[t]) for t in ref)
            if not same or int((status != 0).sum().item()) != 0:
                raise RuntimeError("%s: the kernel and the torch road disagree" % name)
            result["shapes"].append({"name": name, "shape": [planes, lay.mh, lay.mw], "stride": s, "dtype": dtype, "fast_path": lay.fast_path,
                                     "planes_per_group": lay.planes_per_group, "slot_bytes": lay.slot_bytes,
                                     "gop_us": round(med(gop_us), 1), "gop_min_us": round(min(gop_us), 1), "gop_enqueue_us": round(med(enqueue_us), 1),
                                     "bytes_moved": moved, "gop_gb_per_s": round(moved / med(gop_us) / 1e3, 1),
                                     "copy_us": round(med(copy_us), 1), "copy_gb_per_s": round(2 * hops * lay.slot_bytes / med(copy_us) / 1e3, 1),
                                     "torch_road_us": round(med(torch_us), 1), "kernel_equals_torch_road": True,
                                     "cells_moved": int((via[[slot[t] for t in ref if t != src]] != 0).sum().item())})
    print(json.dumps(result))


def propose_bench(a, pipe, window, frames):
    import numpy as np
    import torch
    import leon_ctypes as L
    fw, fh, n = pipe.info.frame_width, pipe.info.frame_height, len(frames)
    kw = dict(max_boxes=a.max_boxes, mv_min=a.mv_min, ac_min=a.ac_min, connectivity=8)
    st = torch.cuda.Stream()
    us, enq = [], []
    with torch.cuda.stream(st):
        d_frames = torch.arange(n, dtype=torch.int32, device="cuda")
        for i in range(a.reps + 2):
            st.synchronize()
            t0 = time.perf_counter()
            regions, count, info, status = pipe.propose_regions_device(window, d_frames, **kw)
            t1 = time.perf_counter()
            st.synchronize()
            t2 = time.perf_counter()
            if i >= 2:
                us.append((t2 - t0) * 1e6)
                enq.append((t1 - t0) * 1e6)
        stats, gstatus = pipe.gauge_regions_device(window, regions)
    st.synchronize()
    h_regions, h_count, h_info, h_status = regions.cpu().numpy(), count.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy()
    checked = min(n, a.propose_check)
    motion, activity = [None] * n, [None] * n
    for f in range(checked):
        motion[f], activity[f] = pipe.read_motion(window, f)[:2], pipe.read_activity(window, f)[0]
        s_, r_, i_, c_ = L.propose_boxes(fw, fh, n, motion, activity, f, **kw)
        if s_ != h_status[f] or c_ != h_count[f] or r_ != h_regions[f].tolist() or i_ != h_info[f].tolist():
            raise RuntimeError("the device and propose_boxes disagree in frame %d" % f)
    if (h_status != 0).any():
        raise RuntimeError("a frame of the window was refused")
    used = (np.arange(a.max_boxes)[None, :] < h_count[:, None]).reshape(-1)
    rows, h_stats, h_gstatus = h_regions.reshape(-1, 8), stats.cpu().numpy(), gstatus.cpu().numpy()
    if not ((h_gstatus[used] == 0).all() and (h_gstatus[~used] == L.REGION_BOX).all() and (h_stats[used, 0] == rows[used, 3].astype(np.int64) * rows[used, 4]).all()):
        raise RuntimeError("gauge_regions_device on the proposed rows: word 0 or the status words are not what the rows say")
    mbs = pipe.motion_layout.mb_width * pipe.motion_layout.mb_height
    med = statistics.median(us)
    print(json.dumps({"propose": {"frames": n, "macroblocks": mbs, "config": kw, "us": round(med, 1), "min_us": round(min(us), 1), "enqueue_us": round(statistics.median(enq), 1),
                                  "reps": a.reps, "bytes_read": n * 17 * mbs, "read_GBps_of_the_call": round(n * 17 * mbs / med / 1e3, 1),
                                  "boxes": int(np.minimum(h_count, a.max_boxes).sum()), "components": int(h_count.sum()), "frames_over_K": int((h_count > a.max_boxes).sum()),
                                  "largest_count": int(h_count.max()), "hot_cells_in_boxes": int(h_info[..., 0].sum()), "checked_frames": checked,
                                  "gauged_rows_ok": int(used.sum()), "gauged_rows_region_box": int((~used).sum())}}))


def overlap_sets(np, n, k, fw, fh, seed):
    """[n, k, 8] rows: set f on frame f, sides 16 .. 160"""
    g = np.random.default_rng(seed)
    w, h = g.integers(16, 161, size=(n, k)), g.integers(16, 161, size=(n, k))
    r = np.zeros((n, k, 8), dtype=np.int32)
    r[..., 0] = np.arange(n)[:, None]
    r[..., 1], r[..., 2], r[..., 3], r[..., 4] = g.integers(0, fw - w + 1), g.integers(0, fh - h + 1), w, h
    return r


def timed(torch, st, reps, call):
    """the median and the least of `reps` calls from the enqueue to the synchronisation of the stream, and the median enqueue, in us"""
    us, enq = [], []
    for i in range(reps + 2):          # (the first two: the scratch, the stream and torch's allocator warm up)
        st.synchronize()
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        st.synchronize()
        t2 = time.perf_counter()
        if i >= 2:
            us.append((t2 - t0) * 1e6)
            enq.append((t1 - t0) * 1e6)
    return out, {"us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "enqueue_us": round(statistics.median(enq), 1)}


def overlap_bench(a, pipe, window, frames):
    import numpy as np
    import torch
    import leon_ctypes as L
    fw, fh, n = pipe.info.frame_width, pipe.info.frame_height, len(frames)
    st = torch.cuda.Stream()
    result = {"frames": n, "reps": a.reps, "K": {}}
    with torch.cuda.stream(st):
        for k in (64, 256, 1024):
            rows, other = overlap_sets(np, n, k, fw, fh, k), overlap_sets(np, n, k, fw, fh, k + 1)
            scores = np.random.default_rng(k).integers(0, 1000, size=(n, k)).astype(np.int32)
            d_rows, d_other, d_scores = torch.tensor(rows, device="cuda"), torch.tensor(other, device="cuda"), torch.tensor(scores, device="cuda")
            entry = {}
            if a.suppress:
                for name, t, measure in (("iou_0.5", 32768, L.OVERLAP_IOU), ("iomin_0.75", 49152, L.OVERLAP_IOMIN)):
                    got, e = timed(torch, st, a.reps, lambda: pipe.suppress_regions_device(window, d_rows, d_scores, threshold_q16=t, measure=measure))
                    out, order, by, count, status = (x.cpu().numpy() for x in got)
                    for s_ in range(min(n, a.overlap_check)):
                        o_, ord_, by_, c_, st_ = L.suppress_boxes(fw, fh, n, rows[s_].tolist(), scores[s_].tolist(), t, measure)
                        if (o_, ord_, by_, c_, st_) != (out[s_].tolist(), order[s_].tolist(), by[s_].tolist(), count[s_], status[s_].tolist()):
                            raise RuntimeError("the device and suppress_boxes disagree in set %d" % s_)
                    t0 = time.perf_counter()
                    host = pipe.suppress_regions(window, rows, scores, threshold_q16=t, measure=measure)
                    e["host_road_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                    if not all(np.array_equal(h_, g_) for h_, g_ in zip(host, (out, order, by, count, status))):
                        raise RuntimeError("the host road and the device road disagree")
                    e.update(kept=int(count.sum()), suppressed=int((status == 0).sum() - count.sum()), checked_sets=min(n, a.overlap_check))
                    entry[name] = e
            if a.match:
                got, e = timed(torch, st, a.reps, lambda: pipe.match_regions_device(window, d_rows, d_other, threshold_q16=19661))
                ma, mb, ov, count, sa, sb = (x.cpu().numpy() for x in got)
                for s_ in range(min(n, a.overlap_check) if k <= 256 else 0):          # (the definition sorts exact fractions: not at K = 1024)
                    m_ = L.match_boxes(fw, fh, n, rows[s_].tolist(), other[s_].tolist(), 19661)
                    if m_[:4] != (ma[s_].tolist(), mb[s_].tolist(), ov[s_].tolist(), count[s_]):
                        raise RuntimeError("the device and match_boxes disagree in set %d" % s_)
                t0 = time.perf_counter()
                host = pipe.match_regions(window, rows, other, threshold_q16=19661)
                e["host_road_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                if not all(np.array_equal(h_, g_) for h_, g_ in zip(host, (ma, mb, ov, count, sa, sb))):
                    raise RuntimeError("the host road and the device road disagree")
                e.update(pairs=int(count.sum()), checked_sets=min(n, a.overlap_check) if k <= 256 else 0)
                entry["iou_0.3"] = e
            result["K"][k] = entry
        if a.match:
            result["identical"] = {}
            for k in (256, 1024):
                same = np.zeros((1, k, 8), dtype=np.int32)
                same[..., 1:5] = (100, 100, 50, 40)
                d_same = torch.tensor(same, device="cuda")
                got, e = timed(torch, st, max(3, a.reps // 4), lambda: pipe.match_regions_device(window, d_same, d_same, threshold_q16=65536))
                if got[0].cpu().numpy().tolist() != [list(range(k))] or got[3].cpu().numpy().tolist() != [k]:
                    raise RuntimeError("identical boxes: row i is not matched with row i")
                result["identical"][k] = e
    print(json.dumps({("suppress" if a.suppress else "match"): result}))


def accumulate_bench(a, pipe, window, frames):
    import numpy as np
    import torch
    import leon_ctypes as L
    fw, fh, cw, ch = pipe.info.frame_width, pipe.info.frame_height, pipe.info.coded_width, pipe.info.coded_height
    n = len(frames)
    src = [i for i, f in enumerate(frames) if f["type"] == L.PIC_I][0]
    rows = pipe.gop_frames(window, src)
    slot = {f: i for i, f in enumerate(rows)}
    fwd, bwd = pipe.carry_refs(window)
    levels, unreachable = L.propagate_plan((fwd, bwd), frames, src)
    tgt = [t for t, f, b in levels[0] if frames[t]["type"] == L.PIC_P][0]
    luma, chroma = 2 * cw * ch, 2 * (cw // 2) * (ch // 2)
    result = {"bench": "accumulate", "frame": [fw, fh], "coded": [cw, ch], "window_frames": n, "gop_frames": len(rows), "gop_levels": len(levels) + 1,
              "gop_hops": sum(len(x) for x in levels) + 1, "gop_unreachable": len(unreachable), "reps": a.reps, "parts": []}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for parts in a.parts:
            lay = L.accumulate_layout(cw, ch, parts)
            got, gop = timed(torch, st, a.reps, lambda: pipe.accumulate_gop(window, src, parts))
            if int((got["status"] != 0).sum().item()) != 0:
                raise RuntimeError("parts %d: a hop of the GOP was refused" % parts)
            slots = got["slots"]
            level_hops = torch.tensor([(t, slot[t], slot.get(f, -1), slot.get(b, -1), 0, 0, 0, 0) for t, f, b in levels[0]], dtype=torch.int32, device="cuda")
            one_hop = torch.tensor([(tgt, slot[tgt], slot[src], -1, 0, 0, 0, 0)], dtype=torch.int32, device="cuda")
            via = torch.empty((len(levels[0]), ch // 16, cw // 16), dtype=torch.uint8, device="cuda")
            status = torch.empty(len(levels[0]), dtype=torch.int32, device="cuda")
            _, level = timed(torch, st, a.reps, lambda: pipe.accumulate_device(window, slots, level_hops, parts, via=via, status=status))
            _, hop = timed(torch, st, a.reps, lambda: pipe.accumulate_device(window, slots, one_hop, parts, via=via[:1], status=status[:1]))
            # the bytes a hop moves, from the shapes: its planes read from the source and written, T's residual record read for the residual part
            planes = (3 * luma if parts & 1 else 0) + (luma + 2 * chroma if parts & 2 else 0)
            per_hop = 2 * planes + (luma + 2 * chroma if parts & 2 else 0)
            a_, b_ = torch.empty(per_hop // 2, dtype=torch.uint8, device="cuda"), torch.empty(per_hop // 2, dtype=torch.uint8, device="cuda")
            _, copy = timed(torch, st, a.reps, lambda: b_.copy_(a_))
            result["parts"].append({"parts": parts, "slot_bytes": lay.slot_bytes, "gop": gop, "level": dict(level, hops=len(levels[0])), "hop": hop,
                                    "hop_bytes_moved": per_hop, "hop_gb_per_s": round(per_hop / hop["us"] / 1e3, 1), "hop_min_gb_per_s": round(per_hop / hop["min_us"] / 1e3, 1),
                                    "level_gb_per_s": round(len(levels[0]) * per_hop / level["us"] / 1e3, 1),
                                    "copy_of_as_many_bytes": copy, "copy_gb_per_s": round(per_hop / copy["us"] / 1e3, 1),
                                    "hop_fraction_of_copy_rate": round(copy["us"] / hop["us"], 3)})
        # one hop of parts 3 against the definition, on the records read back
        lay = L.accumulate_layout(cw, ch, 3)
        got = pipe.accumulate_gop(window, src, 3)
        st.synchronize()
        motion, residual = [None] * n, [None] * n
        motion[tgt], residual[tgt] = pipe.read_motion(window, tgt)[:2], pipe.read_residual(window, tgt)
        want = np.zeros((2, lay.slot_bytes), dtype=np.uint8)
        acc = L.accumulate_views(want, lay)
        if L.accumulate_hop(cw, ch, n, motion, residual, (tgt, 1, 0, -1), acc)[0] != 0 or any(not np.array_equal(acc[k][1], got[k][slot[tgt]].cpu().numpy()) for k in acc):
            raise RuntimeError("the device and accumulate_hop disagree on the hop to frame %d" % tgt)
        result["hop_equals_accumulate_hop"] = True
        result["moving_macroblocks_of_the_hop"] = int((motion[tgt][0] != 0).any(axis=2).sum())
        # the road there was for that hop: three propagate calls and the adds around them (maps lie over the FRAME)
        mh2, mw2 = (fh + 1) // 2, (fw + 1) // 2
        m4 = torch.zeros((2, 4, fh, fw), dtype=torch.int16, device="cuda")          # AX AY AGE RY
        m2 = torch.zeros((2, 2, mh2, mw2), dtype=torch.int16, device="cuda")        # RCb RCr
        yy, xx = torch.meshgrid(torch.arange(fh, device="cuda", dtype=torch.int16), torch.arange(fw, device="cuda", dtype=torch.int16), indexing="ij")
        mc = torch.stack([torch.stack([xx, yy]), torch.zeros((2, fh, fw), dtype=torch.int16, device="cuda")])
        hop8 = torch.tensor([(tgt, 1, 0, -1, 0, 0, 0, 0)], dtype=torch.int32, device="cuda")
        ry, rcb, rcr = pipe.residual_view(window, tgt)

        def composed():
            pipe.propagate_maps_device(window, m4, hop8, 1)
            pipe.propagate_maps_device(window, m2, hop8, 2)
            pipe.propagate_maps_device(window, mc, hop8, 1)
            m4[1, 0] += mc[1, 0] - xx
            m4[1, 1] += mc[1, 1] - yy
            m4[1, 2] += 1
            m4[1, 3] += ry[:fh, :fw]
            m2[1, 0] += rcb[:mh2, :mw2]
            m2[1, 1] += rcr[:mh2, :mw2]
        _, road = timed(torch, st, a.reps, composed)
        _, prop4 = timed(torch, st, a.reps, lambda: pipe.propagate_maps_device(window, m4, hop8, 1))
        moved4 = 2 * 4 * 2 * fh * fw          # four int16 planes read and written
        c_, d_ = torch.empty(moved4 // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved4 // 2, dtype=torch.uint8, device="cuda")
        _, copy4 = timed(torch, st, a.reps, lambda: d_.copy_(c_))
        result["composed_road_one_hop_parts_3"] = road
        result["propagate_stride_1_int16_4_planes"] = dict(prop4, bytes_moved=moved4, gb_per_s=round(moved4 / prop4["us"] / 1e3, 1), copy_of_as_many_bytes=copy4,
                                                         fraction_of_copy_rate=round(copy4["us"] / prop4["us"], 3))
    print(json.dumps(result))


def fields_bench(a, pipe, window, frames):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import leon_ctypes as L
    fw, fh, cw, ch, n = pipe.info.frame_width, pipe.info.frame_height, pipe.info.coded_width, pipe.info.coded_height, len(frames)
    rng = np.random.default_rng(224)
    N, size = a.boxes, (224, 224)
    w, h = rng.integers(16, a.max_box + 1, size=N), rng.integers(16, a.max_box + 1, size=N)
    recs = np.zeros((N, 8), dtype=np.int32)
    recs[:, 0] = np.arange(N) % n
    recs[:, 1], recs[:, 2], recs[:, 3], recs[:, 4] = rng.integers(0, fw - w + 1), rng.integers(0, fh - h + 1), w, h
    result = {"bench": "fields", "frame": [fw, fh], "coded": [cw, ch], "window_frames": n, "boxes": N, "box_side": [16, a.max_box], "size": list(size), "dtype": "float16",
              "reps": a.reps, "sources": {}}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dev = torch.from_numpy(recs).cuda()
        for source in a.fields_source:
            C_ = 2 if source == "motion" else 3
            scale = 0.5 if source == "motion" else 1.0 / 128
            out = torch.empty(N * C_ * size[0] * size[1] * 2, dtype=torch.uint8, device="cuda")
            status = torch.empty(N, dtype=torch.int32, device="cuda")
            call = (lambda: pipe.motion_tensors(window, dev, size, scale=scale, out=out, status=status)) if source == "motion" else \
                (lambda: pipe.residual_tensors(window, dev, size, scale=scale, out=out, status=status))
            (batch, _), t = timed(torch, st, a.reps, call)
            if int((status != 0).sum().item()) != 0:
                raise RuntimeError("%s: a record was refused" % source)
            # against the definition, on the records read back
            for k in range(min(a.fields_check, N)):
                f = int(recs[k, 0])
                if source == "motion":
                    item, chans = np.ascontiguousarray(pipe.read_motion(window, f)[0]).reshape(-1), L.field_channels_motion(cw // 16, scale=scale)
                else:
                    item = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in pipe.read_residual(window, f)])
                    chans = [L.field_channel(0, cw, 1, 0, scale), L.field_channel(2 * cw * ch, cw // 2, 1, 1, scale), L.field_channel(2 * cw * ch + 2 * (cw // 2) * (ch // 2), cw // 2, 1, 1, scale)]
                if not np.array_equal(batch[k].cpu().numpy(), L.field_tensor(item, fw, fh, recs[k, 1:5], size, chans)):
                    raise RuntimeError("%s: record %d differs from field_tensor" % (source, k))
            # the road a user has today, box by box on the same views
            M = min(a.torch_boxes, N)
            views = {}
            for f in sorted(set(int(v) for v in recs[:M, 0])):
                views[f] = (pipe.motion_view(window, f)[0][..., :2].permute(2, 0, 1),) if source == "motion" else pipe.residual_view(window, f)
            res = torch.empty((M, C_) + size, dtype=torch.float16, device="cuda")

            def torch_road():
                for k in range(M):
                    f, x, y, bw, bh = (int(v) for v in recs[k, :5])
                    planes = []
                    for q, v in enumerate(views[f]):
                        s = 4 if source == "motion" else (0 if q == 0 else 1)
                        v = v if v.dim() == 3 else v[None]
                        cells = v[:, y >> s:((y + bh - 1) >> s) + 1, x >> s:((x + bw - 1) >> s) + 1]
                        px = cells.repeat_interleave(1 << s, dim=1).repeat_interleave(1 << s, dim=2) if s else cells
                        y0, x0 = y - ((y >> s) << s), x - ((x >> s) << s)
                        planes.append(px[:, y0:y0 + bh, x0:x0 + bw])
                    crop = torch.cat(planes).to(torch.float32)[None]
                    res[k] = (F.interpolate(crop, size=size, mode="bilinear", antialias=True, align_corners=False)[0] * scale + 0.0).to(torch.float16)
                return res
            _, road = timed(torch, st, max(2, a.reps // 4), torch_road)
            written = N * C_ * size[0] * size[1] * 2
            result["sources"][source] = {"channels": C_, "call": t, "us_per_box": round(t["us"] / N, 3), "bytes_written": written, "write_gb_per_s": round(written / t["us"] / 1e3, 1),
                                         "records_checked_against_field_tensor": min(a.fields_check, N),
                                         "torch_road": dict(road, boxes=M, us_per_box=round(road["us"] / M, 2)),
                                         "torch_road_per_box_over_call_per_box": round((road["us"] / M) / (t["us"] / N), 1)}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", action="store_true", help="dense maps (k_propagate) instead of boxes")
    ap.add_argument("--gauge", action="store_true", help="the carried boxes through k_gauge in the same job, sources 1, 2 and 3")
    ap.add_argument("--gauge-check", type=int, default=64, help="records of each gauge call compared with gauge_box")
    ap.add_argument("--propose", action="store_true", help="boxes proposed from the records of every frame (k_propose) instead of boxes carried")
    ap.add_argument("--mv-min", type=int, default=2)
    ap.add_argument("--ac-min", type=int, default=256)
    ap.add_argument("--max-boxes", type=int, default=16)
    ap.add_argument("--propose-check", type=int, default=8, help="frames compared with propose_boxes")
    ap.add_argument("--suppress", action="store_true", help="sets of boxes pruned by overlap (k_suppress) instead of boxes carried")
    ap.add_argument("--match", action="store_true", help="pairs of sets of boxes matched by overlap (k_match) instead of boxes carried")
    ap.add_argument("--overlap-check", type=int, default=2, help="sets compared with suppress_boxes / match_boxes")
    ap.add_argument("--accumulate", action="store_true", help="motion and residual accumulated over the GOP (k_accumulate) instead of boxes carried")
    ap.add_argument("--parts", type=lambda v: [int(x) for x in v.split(",")], default=[1, 2, 3], help="--accumulate: the parts timed, e.g. 3 alone under a profiler")
    ap.add_argument("--fields", action="store_true", help="boxes of the motion and residual records as fp16 tensors (k_fields) instead of boxes carried")
    ap.add_argument("--torch-boxes", type=int, default=256, help="--fields: boxes of the torch yardstick")
    ap.add_argument("--fields-check", type=int, default=4, help="--fields: records compared with field_tensor")
    ap.add_argument("--fields-source", type=lambda v: v.split(","), default=["motion", "residual"], help="--fields: the sources timed")
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
    pipe = L.Pipeline(data, on_window=on_window, motion=True, activity=a.gauge or a.propose, residual=a.accumulate or a.fields, gops_per_window=stream_1080p.VARIED_GOPS, gpu_parser=True, parser_threads=16)
    try:
        if not delivered.wait(300):
            raise RuntimeError("no window was delivered: %s" % (pipe.error,))
        window, frames = held["window"], held["frames"]
        if a.maps or a.propose or a.suppress or a.match or a.accumulate or a.fields:
            (maps_bench if a.maps else propose_bench if a.propose else accumulate_bench if a.accumulate else fields_bench if a.fields else overlap_bench)(a, pipe, window, frames)
            pipe.release_window(window)
            pipe.wait()
            return
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
            gauge = None
            if a.gauge:          # the moved boxes, on the P picture, under its two records
                gauge = {}
                stats = torch.empty((a.boxes, L.GAUGE_WORDS), dtype=torch.int64, device="cuda")
                gstatus = torch.empty((a.boxes,), dtype=torch.int32, device="cuda")
                moved_to = out.clone()
                g_motion, g_cells = pipe.read_motion(window, tgt)[:2], pipe.read_activity(window, tgt)[0]
                g_m, g_a = [None] * n, [None] * n
                g_m[tgt], g_a[tgt] = g_motion, g_cells
                for sources in (1, 2, 3):
                    us, enq = [], []
                    for i in range(a.reps + 2):
                        st.synchronize()
                        t0 = time.perf_counter()
                        pipe.gauge_regions_device(window, moved_to, sources=sources, stats=stats, status=gstatus)
                        t1 = time.perf_counter()
                        st.synchronize()
                        t2 = time.perf_counter()
                        if i >= 2:
                            us.append((t2 - t0) * 1e6)
                            enq.append((t1 - t0) * 1e6)
                    h_stats, h_status, h_rec = stats.cpu().numpy(), gstatus.cpu().numpy(), moved_to.cpu().numpy()
                    for k in range(min(a.boxes, a.gauge_check)):
                        s_, w_ = L.gauge_box(fw, fh, n, g_m, g_a, h_rec[k], sources)
                        if s_ != h_status[k] or (s_ == 0 and w_ != h_stats[k].tolist()):
                            raise RuntimeError("sources %d: the device and gauge_box disagree in record %d" % (sources, k))
                    gauge["sources_%d" % sources] = {"us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "enqueue_us": round(statistics.median(enq), 1),
                                                     "records_ok": int((h_status == 0).sum()), "checked": min(a.boxes, a.gauge_check)}
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
                          "moved": int((hop[1][:, 2:] != 0).any(axis=1).sum()), **({"gauge": gauge} if gauge is not None else {})}))
        pipe.release_window(window)
        pipe.wait()
    finally:
        pipe.close()


if __name__ == "__main__":
    main()
