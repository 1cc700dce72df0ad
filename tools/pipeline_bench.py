#!/usr/bin/env python3
"""End to end on one GPU through the NATIVE pipeline (include/leon_pipeline.h): pageable stream bytes ->
K parser threads (one libleon_vlc stream per GOP shard, output written straight into pinned memory) ->
one upload per GOP -> one launch per picture type and dependency level across a window of GOPs, display
conversion fused in -> RGBA frames in device memory, delivered by callback.  No interpreter in the loop:
Python only starts the pipeline and waits.

This is NOT the bench.py metric (that one starts with the boundary tensors resident in HBM); it is the
figure DESIGN.md quotes for the whole drop-in path.  The stream is a synthetic 1080p IBBP stream of
--gops GOPs (tools/parse_bench.py writes and caches it; tools/probe/stream_1080p_<n>gop.bin is used when
present) decoded --loop times over.

  python tools/pipeline_bench.py [--gops 2] [--loop 64] [--threads 16] [--window 32]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gops", type=int, default=2)
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--gpu-parser", action="store_true", help="decode the slice layer on the GPU (leon_pipeline_config.gpu_parser)")
    ap.add_argument("--output", choices=["rgba", "ycbcr", "both", "tensor", "rgba+tensor", "ycbcr+tensor", "all"], default="rgba",
                    help="what the frames carry (leon_pipeline_config.output): RGBA, the YCbCr planes, planar float tensors, or a combination")
    ap.add_argument("--tensor-dtype", choices=["float16", "bfloat16", "float32", "uint8"], default="float16", help="element type of --output tensor")
    ap.add_argument("--tensor-layout", choices=["chw", "hwc"], default="chw", help="planar [3, H, W] or channels-last [H, W, 3] tensors (leon_pipeline_tensor_format)")
    ap.add_argument("--tensor-size", type=int, nargs=2, metavar=("H", "W"), help="tensors resampled on the device to H x W (leon_pipeline_tensor_resize)")
    ap.add_argument("--tensor-crop", type=int, nargs=4, metavar=("X", "Y", "W", "H"), help="the crop box --tensor-size resamples (frame pixels; default: the whole frame)")
    ap.add_argument("--tensor-filter", choices=["triangle", "bicubic"], default="triangle", help="the filter of --tensor-size (leon_pipeline_tensor_resize.filter)")
    ap.add_argument("--tensor-canvas", type=int, nargs=2, metavar=("H", "W"), help="with --tensor-size: the resampled image centred in an H x W tensor (leon_pipeline_tensor_canvas)")
    ap.add_argument("--tensor-letterbox", type=int, nargs=2, metavar=("H", "W"),
                    help="the crop box (or the frame) resampled with its aspect ratio kept and centred in an H x W tensor (leon_pipeline_letterbox): instead of --tensor-size")
    ap.add_argument("--tensor-pad-value", type=int, nargs=3, metavar=("R", "G", "B"), help="the 8-bit colour value of the canvas outside the image (default 0 0 0)")
    ap.add_argument("--host-resize", type=int, nargs=2, metavar=("H", "W"),
                    help="the route without --tensor-size, for comparison: full-size tensors, and the callback resizes every window's window_tensor view "
                         "with torch.nn.functional.interpolate(mode='bilinear', antialias=True)")
    ap.add_argument("--regions", type=int, nargs=3, metavar=("N", "H", "W"),
                    help="with a tensor output: after each window is delivered and before it is released, N seeded random boxes per frame (ratio <= 16) of the "
                         "full-resolution frames resampled to H x W in one call (leon_pipeline_resample_regions); reports regions/s and the mean time per call")
    ap.add_argument("--regions-filter", choices=["triangle", "bicubic"], default="triangle", help="the filter of --regions")
    ap.add_argument("--regions-fit", choices=["stretch", "letterbox"], default="stretch",
                    help="with --regions: letterbox keeps every box's aspect ratio inside H x W, centred, the rest grey (leon_pipeline_regions_fit)")
    ap.add_argument("--device-boxes", action="store_true",
                    help="with --regions: the boxes are uploaded as a CUDA tensor and the call is leon_pipeline_resample_regions_device, enqueued on a torch side "
                         "stream (tables built on the device); the callback waits for that stream before it returns, since the window is released then")
    ap.add_argument("--copy-rate", action="store_true", help="measure leon_measure_copy_bandwidth in this process first (the yardstick of a launch's rate)")
    ap.add_argument("--motion", action="store_true", help="every frame carries its motion record too (LEON_PIPELINE_OUTPUT_MOTION: k_motion, one launch per window)")
    ap.add_argument("--activity", action="store_true", help="every frame carries its activity record too (LEON_PIPELINE_OUTPUT_ACTIVITY: k_activity and k_activity_summary, "
                                                            "one launch each per window)")
    ap.add_argument("--residual", action="store_true", help="every frame carries its residual record too (LEON_PIPELINE_OUTPUT_RESIDUAL: k_residual, one launch per window)")
    ap.add_argument("--varied", action="store_true", help="the 16-GOP stream with 16 different contents (tools/stream_1080p.py) instead of --gops GOPs")
    ap.add_argument("--open-gops", action="store_true", help="with --varied: the same recipe written with open GOPs (closed_gop = 0), the leading B pictures "
                                                             "predicting forward (from the GOP before) and bidirectionally")
    a = ap.parse_args()
    if a.device_boxes and not a.regions:
        ap.error("--device-boxes goes with --regions")
    if a.regions_fit != "stretch" and not a.regions:
        ap.error("--regions-fit goes with --regions")
    regions_fit = dict(fit="letterbox", pad_value=(114, 114, 114)) if a.regions_fit == "letterbox" else {}
    if a.open_gops and not a.varied:
        ap.error("--open-gops goes with --varied")
    cached = os.path.join(ROOT, "tools", "probe", "stream_1080p_%dgop.bin" % a.gops)
    if a.varied:
        import stream_1080p
        data = stream_1080p.load_varied(open_gops=a.open_gops)
        a.gops = stream_1080p.VARIED_GOPS
    elif os.path.exists(cached):
        data = open(cached, "rb").read()
    else:
        import parse_bench
        data = parse_bench.make_stream(a.gops, "/tmp/leon_parse_bench_%d.jsv" % a.gops)
    import ctypes
    import leon_ctypes as L
    L.load()

    def free_device_bytes():                      # what the pipeline holds on the device = free before - free after its creation
        hip = ctypes.CDLL("libamdhip64.so")
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        return f.value if hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0 else None
    copy_gbps = None
    if a.copy_rate:
        dec = L.Decoder(96, 64, n_slots=3, device_id=0)
        copy_gbps = dec.measure_copy_bandwidth()
        dec.close()
    on_window = None
    if a.host_resize:
        import torch

        def on_window(window, frames):
            fl = list(frames)
            p = fl[0]["_pipe"]
            t = p.window_tensor(fl)
            parts = [t] if t is not None else [p.tensor_view(f)[None] for f in fl]
            for x in parts:
                torch.nn.functional.interpolate(x, size=tuple(a.host_resize), mode="bilinear", antialias=True, align_corners=False)
            torch.cuda.synchronize()          # the window is released on return: the resize must have read it
    regions_stat = {"calls": 0, "regions": 0, "seconds": 0.0, "out": None}
    if a.regions:
        if a.host_resize:
            ap.error("--regions and --host-resize are two runs")
        import numpy as np
        import torch
        rn, rh, rw = a.regions

        def on_window(window, frames):
            p = frames[0]["_pipe"]
            n_frames, fw, fh = len(frames), p.info.frame_width, p.info.frame_height
            rng = np.random.default_rng(1000 + window)
            n = n_frames * rn
            # boxes of ratio <= 16 inside the frame: sizes first, then an origin that keeps them inside
            w = rng.integers(1, min(fw, 16 * rw) + 1, n)
            h = rng.integers(1, min(fh, 16 * rh) + 1, n)
            x = (rng.random(n) * (fw - w + 1)).astype(np.int64)
            y = (rng.random(n) * (fh - h + 1)).astype(np.int64)
            boxes = np.stack([np.repeat(np.arange(n_frames), rn), x, y, w, h], axis=1)
            nbytes, pitch = p.region_bytes((rh, rw))
            if regions_stat["out"] is None or regions_stat["out"].numel() < n * pitch:          # the caller's batch buffer, allocated once
                regions_stat["out"] = torch.empty(n * pitch, dtype=torch.uint8, device="cuda:0")
                regions_stat["status"] = torch.empty(n, dtype=torch.int32, device="cuda:0")
            t = time.perf_counter()
            if a.device_boxes:
                st = regions_stat.setdefault("stream", torch.cuda.Stream())
                with torch.cuda.stream(st):
                    dev = torch.from_numpy(boxes.astype(np.int32)).to("cuda:0", non_blocking=True)
                    p.resample_regions_device(window, dev, (rh, rw), a.regions_filter, out=regions_stat["out"], status=regions_stat.get("status"), **regions_fit)
                st.synchronize()
            else:
                p.resample_regions(window, boxes, (rh, rw), a.regions_filter, out=regions_stat["out"], **regions_fit)
            regions_stat["seconds"] += time.perf_counter() - t
            regions_stat["calls"] += 1
            regions_stat["regions"] += n
    free0 = free_device_bytes()
    t0 = time.perf_counter()
    pipe = L.Pipeline(data, parser_threads=a.threads, gops_per_window=a.window, windows_in_flight=a.inflight, loop=a.loop, gpu_parser=a.gpu_parser,
                      output=a.output, tensor_dtype=a.tensor_dtype, tensor_size=a.tensor_size, tensor_crop=a.tensor_crop, tensor_layout=a.tensor_layout, tensor_filter=a.tensor_filter,
                      tensor_canvas=a.tensor_canvas, tensor_letterbox=a.tensor_letterbox, tensor_pad_value=a.tensor_pad_value, on_window=on_window, motion=a.motion, activity=a.activity, residual=a.residual)
    free1 = free_device_bytes()
    pool = L.pool_stats()
    pipe.wait()
    wall = time.perf_counter() - t0
    s = pipe.stats()
    canvas = pipe.tensor_canvas_geometry if (a.tensor_canvas or a.tensor_letterbox) else None
    pipe.close()
    mbs = (pipe.info.coded_width // 16) * (pipe.info.coded_height // 16)
    print(json.dumps({
        "metric": "end-to-end %dx%d pictures/s (parse + PCIe + reconstruct + %s in device memory), native pipeline, one GPU"
                  % (pipe.info.frame_width, pipe.info.frame_height, {"rgba": "RGBA", "ycbcr": "YCbCr planes", "both": "RGBA + YCbCr planes", "tensor": "tensors", "rgba+tensor": "RGBA + tensors",
                     "ycbcr+tensor": "YCbCr planes + tensors", "all": "RGBA + YCbCr planes + tensors"}[a.output]),
        "output": a.output, "motion": a.motion, "motion_record_bytes": pipe.motion_layout.record_bytes if pipe.motion_layout is not None else None,
        "activity": a.activity, "activity_record_bytes": pipe.activity_layout.record_bytes if pipe.activity_layout is not None else None,
        "residual": a.residual, "residual_record_bytes": pipe.residual_layout.record_bytes if pipe.residual_layout is not None else None, "tensor_dtype": a.tensor_dtype if pipe.info.tensor_dtype else None, "tensor_layout": a.tensor_layout if pipe.info.tensor_dtype else None,
        "tensor_frame_bytes": pipe.info.tensor_frame_bytes, "tensor_size": a.tensor_size, "tensor_crop": a.tensor_crop, "tensor_filter": a.tensor_filter if (a.tensor_size or a.tensor_letterbox) else None,
        "tensor_canvas": [canvas.height, canvas.width] if canvas else None, "tensor_image": [canvas.x, canvas.y, canvas.image_width, canvas.image_height] if canvas else None,
        "tensor_pad_value": list(canvas.pad) if canvas else None, "host_resize": a.host_resize, "windows_in_flight": a.inflight,
        "value": s["pictures"] / s["seconds"], "macroblocks_per_s": s["pictures"] * mbs / s["seconds"],
        "regions": a.regions, "device_boxes": bool(a.regions and a.device_boxes), "regions_filter": a.regions_filter if a.regions else None, "regions_fit": a.regions_fit if a.regions else None, "regions_calls": regions_stat["calls"] if a.regions else None,
        "regions_per_s": regions_stat["regions"] / s["seconds"] if a.regions else None,
        "regions_ms_per_call": 1e3 * regions_stat["seconds"] / regions_stat["calls"] if regions_stat["calls"] else None,
        "regions_per_call": regions_stat["regions"] / regions_stat["calls"] if regions_stat["calls"] else None,
        "pictures": s["pictures"], "seconds": s["seconds"], "wall_seconds_incl_setup": wall, "windows": s["windows"],
        "slice_layer": "GPU (csrc/leon_vlc_gpu.h)" if a.gpu_parser else "host threads (libleon_vlc.so)",
        "device_gb_held_by_the_pipeline": (free0 - free1) / 1e9 if free0 is not None and free1 is not None else None,
        "pool_held_gb": pool["held_bytes"] / 1e9, "pool_in_use_gb": pool["in_use_bytes"] / 1e9, "copy_gbps_same_process": copy_gbps,
        "parser_threads": pipe.info.parser_threads, "gops_per_window": pipe.info.gops_per_window,
        "parse_seconds_summed_over_threads": s["parse_seconds_sum"],
        "parser_pictures_per_s_per_thread": s["pictures"] / s["parse_seconds_sum"] if s["parse_seconds_sum"] else None,
        "upload_gb": s["upload_bytes"] / 1e9, "upload_gbps": s["upload_bytes"] / 1e9 / s["seconds"],
        "entries_per_picture": s["entries"] / max(1, s["pictures"]), "stream_bytes": s["stream_bytes"],
        "stream_megabit_per_picture": s["stream_bytes"] * 8 / 1e6 / (12 * a.gops), "host_threads": os.cpu_count(),
        "stream": "%d different %sGOPs, looped %d times" % (a.gops, "open " if a.open_gops else "", a.loop)}))


if __name__ == "__main__":
    main()
