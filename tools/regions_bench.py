#!/usr/bin/env python3
"""leon_pipeline_resample_regions alone: one window of 1080p frames held, then --calls calls of --regions seeded random boxes (ratio
1 .. --max-ratio on both axes, clipped to the frame, frames drawn at random) resampled to --size, into one caller-owned buffer.
Reports the wall time of a call (it is synchronous: tables built on the host, one upload, one launch, the wait), the host part that
can be timed without a device (leon_pipeline_regions_check: one of the two passes over the tables), the bytes a call requests (the
boxes' Y, Cb and Cr samples) and writes, and the copy rate of the same process.  The kernel's own time comes from running this under
`rocprofv3 --kernel-trace --stats -- python tools/regions_bench.py ...` (k_regions, and k_resample of the pipeline's own --tensor-size
tensors for comparison: one launch per window of --window GOPs).  --device-boxes times the same boxes through
leon_pipeline_resample_regions_device too (k_box_tables + k_regions per chunk -- a trace then holds k_regions launches of both roads; enqueue -> stream synchronisation) and checks that both
paths wrote the same bytes.  --fit letterbox times the SAME seeded boxes letterboxed into --size as well (leon_pipeline_regions_fit:
k_fitted, and k_fit_tables on the device path), in the same process, a stretched and a letterboxed call alternating; the boxes whose
height the frame clips are the ones that get pad.  With --device-boxes it also checks that both paths wrote the same letterboxed bytes.
--warp times leon_pipeline_warp_regions and leon_pipeline_warp_regions_device (k_warp) in the same process on the same seeded boxes'
centres and frames: every region a box of --scale times --size, rotated by --angle degrees about its centre (parts of it may leave
the frame and read the pad), and checks that both paths wrote the same bytes.

  python tools/regions_bench.py [--regions 4096] [--size 224 224] [--calls 5] [--window 128] [--filter triangle] [--device-boxes]
                                [--fit letterbox [--anchor centre|top_left] [--pad-value R G B]] [--warp [--angle A] [--scale S]]"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=4096)
    ap.add_argument("--size", type=int, nargs=2, default=[224, 224], metavar=("H", "W"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--window", type=int, default=128, help="GOPs of the held window (12 pictures each)")
    ap.add_argument("--windows", type=int, default=4, help="windows decoded (each one launch of the pipeline's own resize kernel)")
    ap.add_argument("--max-ratio", type=float, default=8.0)
    ap.add_argument("--filter", choices=["triangle", "bicubic"], default="triangle")
    ap.add_argument("--tensor-dtype", choices=["float16", "bfloat16", "float32", "uint8"], default="float16")
    ap.add_argument("--tensor-layout", choices=["chw", "hwc"], default="chw")
    ap.add_argument("--device-boxes", action="store_true",
                    help="also time leon_pipeline_resample_regions_device: the same boxes uploaded once as a CUDA tensor, the call enqueued on a torch side "
                         "stream; its time runs from the enqueue to that stream's synchronisation")
    ap.add_argument("--fit", choices=["stretch", "letterbox"], default="stretch", help="letterbox: the same boxes letterboxed too, alternating with the stretched calls")
    ap.add_argument("--anchor", choices=["centre", "top_left"], default="centre")
    ap.add_argument("--pad-value", type=int, nargs=3, default=[114, 114, 114], metavar=("R", "G", "B"))
    ap.add_argument("--warp", action="store_true", help="also time the warp calls: boxes of --scale x --size about the same centres, rotated by --angle")
    ap.add_argument("--angle", type=float, default=0.0, help="--warp: degrees")
    ap.add_argument("--scale", type=float, default=1.0, help="--warp: frame pixels per output pixel, at most 4")
    a = ap.parse_args()
    fit = dict(fit="letterbox", anchor=a.anchor, pad_value=tuple(a.pad_value)) if a.fit == "letterbox" else None
    import numpy as np
    import torch
    import leon_ctypes as L
    import stream_1080p
    data = stream_1080p.load()          # two GOPs of 12 pictures
    L.load()
    dec = L.Decoder(96, 64, n_slots=3, device_id=0)
    copy_gbps = dec.measure_copy_bandwidth()
    dec.close()
    oh, ow = a.size
    out, lock = {}, threading.Lock()

    def on_window(window, frames):
        if out:
            return None
        p = frames[0]["_pipe"]
        n_frames, fw, fh = len(frames), p.info.frame_width, p.info.frame_height
        rng = np.random.default_rng(4096)
        r = 1.0 + rng.random(a.regions) * (a.max_ratio - 1.0)
        w = np.minimum(fw, np.rint(ow * r)).astype(np.int64)
        h = np.minimum(fh, np.rint(oh * r)).astype(np.int64)
        x = (rng.random(a.regions) * (fw - w + 1)).astype(np.int64)
        y = (rng.random(a.regions) * (fh - h + 1)).astype(np.int64)
        boxes = np.stack([rng.integers(0, n_frames, a.regions), x, y, w, h], axis=1)
        nbytes, pitch = p.region_bytes((oh, ow))
        buf = torch.empty(a.regions * pitch, dtype=torch.uint8, device="cuda:0")
        t = time.perf_counter()
        L.regions_check(fw, fh, n_frames, boxes, (oh, ow), a.filter)
        check_ms = 1e3 * (time.perf_counter() - t)
        p.resample_regions(window, boxes, (oh, ow), a.filter, out=buf)          # scratch reaches its high-water mark
        fbuf = torch.empty_like(buf) if fit else None
        if fit:
            p.resample_regions(window, boxes, (oh, ow), a.filter, out=fbuf, **fit)
        times, fit_times = [], []
        for _ in range(a.calls):
            t = time.perf_counter()
            p.resample_regions(window, boxes, (oh, ow), a.filter, out=buf)
            times.append(1e3 * (time.perf_counter() - t))
            if fit:
                t = time.perf_counter()
                p.resample_regions(window, boxes, (oh, ow), a.filter, out=fbuf, **fit)
                fit_times.append(1e3 * (time.perf_counter() - t))
        dev_times, dev_enqueue, same = None, None, None
        fit_dev_times, fit_same, padded = None, None, None
        if a.device_boxes:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                dev_boxes = torch.from_numpy(boxes.astype(np.int32)).cuda()
                buf2 = torch.empty_like(buf)
                status = torch.empty(a.regions, dtype=torch.int32, device="cuda:0")
                p.resample_regions_device(window, dev_boxes, (oh, ow), a.filter, out=buf2, status=status)          # scratch reaches its high-water mark
            st.synchronize()
            same = bool(torch.equal(buf, buf2)) and not bool(status.any())
            if fit:
                with torch.cuda.stream(st):
                    fbuf2 = torch.empty_like(buf)
                    _, fstatus, rects = p.resample_regions_device(window, dev_boxes, (oh, ow), a.filter, out=fbuf2, rects=True, **fit)
                st.synchronize()
                fit_same = bool(torch.equal(fbuf, fbuf2)) and not bool(fstatus.any())
                padded = int(((rects[:, 2] < ow) | (rects[:, 3] < oh)).sum())
            dev_times, dev_enqueue, fit_dev_times = [], [], []
            for _ in range(a.calls):
                t = time.perf_counter()
                p.resample_regions_device(window, dev_boxes, (oh, ow), a.filter, out=buf2, status=status, stream=st)
                dev_enqueue.append(1e3 * (time.perf_counter() - t))
                st.synchronize()
                dev_times.append(1e3 * (time.perf_counter() - t))
                if fit:
                    t = time.perf_counter()
                    p.resample_regions_device(window, dev_boxes, (oh, ow), a.filter, out=fbuf2, status=status, stream=st, **fit)
                    st.synchronize()
                    fit_dev_times.append(1e3 * (time.perf_counter() - t))
        warp = None
        if a.warp:
            # leon_pipeline_warp_from_rotated_box's expressions for every region at once
            cs, sn = np.cos(np.deg2rad(a.angle)), np.sin(np.deg2rad(a.angle))
            A = np.array([a.scale * cs, -a.scale * sn, 0.0, a.scale * sn, a.scale * cs, 0.0])
            cx, cy = x + w / 2.0, y + h / 2.0
            rec = np.zeros((a.regions, 8), dtype=np.int32)
            rec[:, 0] = boxes[:, 0]
            rec[:, 1:7] = np.floor(A * 65536.0 + 0.5)
            rec[:, 3] = np.floor((cx - (A[0] * ow / 2.0 + A[1] * oh / 2.0)) * 65536.0 + 0.5)
            rec[:, 6] = np.floor((cy - (A[3] * ow / 2.0 + A[4] * oh / 2.0)) * 65536.0 + 0.5)
            pad = tuple(a.pad_value)
            wbuf, wbuf2 = torch.empty_like(buf), torch.empty_like(buf)
            p.warp_regions(window, rec, (oh, ow), pad, out=wbuf)          # scratch reaches its high-water mark
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                dev_rec = torch.from_numpy(rec).cuda()
                wstatus = torch.empty(a.regions, dtype=torch.int32, device="cuda:0")
                p.warp_regions_device(window, dev_rec, (oh, ow), pad, out=wbuf2, status=wstatus)
            st.synchronize()
            warp = dict(angle=a.angle, scale=a.scale, device_equals_host=bool(torch.equal(wbuf, wbuf2)) and not bool(wstatus.any()), call_ms=[], device_call_ms=[],
                        device_enqueue_ms=[])
            for _ in range(a.calls):
                t = time.perf_counter()
                p.warp_regions(window, rec, (oh, ow), pad, out=wbuf)
                warp["call_ms"].append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                p.warp_regions_device(window, dev_rec, (oh, ow), pad, out=wbuf2, status=wstatus, stream=st)
                warp["device_enqueue_ms"].append(1e3 * (time.perf_counter() - t))
                st.synchronize()
                warp["device_call_ms"].append(1e3 * (time.perf_counter() - t))
            warp["call_ms_mean"] = sum(warp["call_ms"]) / a.calls
            warp["device_call_ms_mean"] = sum(warp["device_call_ms"]) / a.calls
        requested = int((w * h).sum() * 3 // 2)
        with lock:
            out.update(frames=n_frames, call_ms=times, regions_check_ms=check_ms, requested_bytes=requested, written_bytes=a.regions * nbytes,
                       mean_ratio_x=float((w / ow).mean()), mean_ratio_y=float((h / oh).mean()), device_call_ms=dev_times, device_enqueue_ms=dev_enqueue,
                       device_equals_host=same, fit=a.fit, fit_call_ms=fit_times or None, fit_device_call_ms=fit_dev_times or None,
                       fit_device_equals_host=fit_same, fit_regions_with_pad=padded, warp=warp)
    pipe = L.Pipeline(data, parser_threads=16, gops_per_window=a.window, windows_in_flight=2, loop=a.window * a.windows // 2, gpu_parser=True, output="tensor",
                      tensor_dtype=a.tensor_dtype, tensor_layout=a.tensor_layout, tensor_size=(oh, ow), tensor_filter=a.filter, on_window=on_window)
    try:
        pipe.wait()
        if pipe.error is not None:
            raise SystemExit("pipeline: %r" % (pipe.error,))
    finally:
        pipe.close()
    mean = sum(out["call_ms"]) / len(out["call_ms"])
    print(json.dumps(dict(out, metric="leon_pipeline_resample_regions: %d regions of a window of %d 1080p frames -> %d x %d %s %s, %s" % (
        a.regions, out["frames"], oh, ow, a.tensor_dtype, a.tensor_layout, a.filter), regions=a.regions, call_ms_mean=mean, regions_per_s=a.regions / (mean * 1e-3),
        device_call_ms_mean=sum(out["device_call_ms"]) / len(out["device_call_ms"]) if out["device_call_ms"] else None,
        fit_call_ms_mean=sum(out["fit_call_ms"]) / len(out["fit_call_ms"]) if out["fit_call_ms"] else None,
        fit_device_call_ms_mean=sum(out["fit_device_call_ms"]) / len(out["fit_device_call_ms"]) if out["fit_device_call_ms"] else None,
        call_gbps_requested_plus_written=(out["requested_bytes"] + out["written_bytes"]) / (mean * 1e-3) / 1e9, copy_gbps_same_process=copy_gbps,
        windows=pipe.windows, frames_per_window=out["frames"])))


if __name__ == "__main__":
    main()
