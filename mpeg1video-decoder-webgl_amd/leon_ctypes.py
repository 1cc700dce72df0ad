"""ctypes binding of libleon_hip.so (include/leon.h) for the Python-side plumbing:
tests, bench.py and the multi-GPU launcher.  The product's host language is
JavaScript (js/ + the N-API addon); this file only moves pointers around.

Fails loudly when the library is missing or no gfx950 device is usable: there is
no CPU fallback anywhere in this package.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LEON_LIB", os.path.join(_HERE, "lib", "libleon_hip.so"))

OK = 0
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_NO_FREE_SLOT, ERR_NOMEM = -1, -2, -3, -4, -5
PIC_I, PIC_P, PIC_B = 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
RGB_CPU_TWIN, RGB_GL = 0, 1

# every symbol include/leon.h declares (tests check the library exports all of them)
SYMBOLS = [
    "leon_abi_version", "leon_last_error", "leon_create", "leon_destroy", "leon_set_quant_matrices", "leon_add_quant_matrices",
    "leon_acquire_slot", "leon_release_slot", "leon_free_decoded_slots", "leon_submit_picture",
    "leon_submit_batch", "leon_batch_create", "leon_batch_run", "leon_batch_destroy",
    "leon_submit_sparse", "leon_batch_create_sparse",
    "leon_convert_rgba", "leon_convert_rgba_batch", "leon_read_planes", "leon_write_planes",
    "leon_read_alpha_plane", "leon_write_alpha_plane", "leon_slot_device_ptr", "leon_sync", "leon_set_overlap_convert", "leon_timing_enable", "leon_timing_reset", "leon_timing_get",
    "leon_timing_get_launches",
    "leon_measure_copy_bandwidth", "leon_measure_stream_bandwidth", "leon_device_malloc", "leon_device_free", "leon_device_pool_stats",
]
ABI_VERSION = 3        # LEON_ABI_VERSION of include/leon.h
# include/leon_pipeline.h (same library)
PIPELINE_SYMBOLS = [
    "leon_pipeline_create", "leon_pipeline_create_partial", "leon_pipeline_feed", "leon_pipeline_get_info", "leon_pipeline_release_window", "leon_pipeline_wait",
    "leon_pipeline_get_stats", "leon_pipeline_read_frame", "leon_pipeline_error", "leon_pipeline_destroy", "leon_pipeline_seek",
    "leon_pipeline_read_frame_planes",
    "leon_pipeline_create_tensor", "leon_pipeline_tensor_table", "leon_pipeline_window_tensors", "leon_pipeline_read_tensor",
    "leon_pipeline_create_tensor_resized", "leon_pipeline_resize_weights", "leon_pipeline_get_tensor_geometry",
    "leon_pipeline_create_tensor_format", "leon_pipeline_get_tensor_shape",
    "leon_pipeline_create_tensor_canvas", "leon_pipeline_get_tensor_canvas", "leon_pipeline_letterbox",
    "leon_pipeline_regions_check", "leon_pipeline_resample_regions", "leon_pipeline_read_regions",
    "leon_pipeline_resample_regions_device", "leon_pipeline_region_status", "leon_pipeline_resize_weights_device",
    "leon_pipeline_region_fit_rect", "leon_pipeline_regions_fit_check", "leon_pipeline_region_fit_status",
    "leon_pipeline_resample_regions_fit", "leon_pipeline_read_regions_fit", "leon_pipeline_resample_regions_device_fit",
    "leon_pipeline_warp_regions_check", "leon_pipeline_warp_region_status", "leon_pipeline_warp_from_matrix", "leon_pipeline_warp_from_rotated_box",
    "leon_pipeline_warp_regions", "leon_pipeline_read_warp_regions", "leon_pipeline_warp_regions_device",
    "leon_pipeline_motion_layout", "leon_pipeline_motion_record", "leon_pipeline_get_motion_layout", "leon_pipeline_window_motion",
    "leon_pipeline_read_motion", "leon_pipeline_motion_kernel",
    "leon_pipeline_activity_layout", "leon_pipeline_activity_record", "leon_pipeline_activity_kernel", "leon_pipeline_get_activity_layout",
    "leon_pipeline_window_activity", "leon_pipeline_read_activity",
    "leon_pipeline_residual_layout", "leon_pipeline_residual_kernel", "leon_pipeline_get_residual_layout", "leon_pipeline_window_residual",
    "leon_pipeline_read_residual",
    "leon_pipeline_carry_refs", "leon_pipeline_carry_record", "leon_pipeline_get_carry_refs", "leon_pipeline_carry_regions_device",
    "leon_pipeline_carry_regions", "leon_pipeline_carry_device",
    "leon_pipeline_propagate_layout", "leon_pipeline_propagate_record", "leon_pipeline_propagate_maps_device", "leon_pipeline_propagate_maps",
    "leon_pipeline_propagate_kernel",
    "leon_pipeline_accumulate_layout", "leon_pipeline_accumulate_record", "leon_pipeline_accumulate_device", "leon_pipeline_accumulate",
    "leon_pipeline_accumulate_kernel",
    "leon_pipeline_field_tensor_record", "leon_pipeline_field_tensors_device", "leon_pipeline_field_tensors", "leon_pipeline_field_tensors_kernel",
    "leon_pipeline_gauge_record", "leon_pipeline_gauge_regions_device", "leon_pipeline_gauge_regions", "leon_pipeline_gauge_kernel",
    "leon_pipeline_propose_record", "leon_pipeline_propose_regions_device", "leon_pipeline_propose_regions", "leon_pipeline_propose_kernel",
    "leon_pipeline_suppress_record", "leon_pipeline_suppress_regions_device", "leon_pipeline_suppress_regions", "leon_pipeline_suppress_kernel",
    "leon_pipeline_match_record", "leon_pipeline_match_regions_device", "leon_pipeline_match_regions", "leon_pipeline_match_kernel",
]
PIPELINE_SEEK_KEY, PIPELINE_SEEK_EXACT = 0, 1      # leon_pipeline_seek modes
PIPELINE_OUTPUT_RGBA, PIPELINE_OUTPUT_YCBCR = 1, 2  # leon_pipeline_config.output bits
PIPELINE_OUTPUTS = {"rgba": PIPELINE_OUTPUT_RGBA, "ycbcr": PIPELINE_OUTPUT_YCBCR, "both": PIPELINE_OUTPUT_RGBA | PIPELINE_OUTPUT_YCBCR}
# the tensor output (LEON_PIPELINE_OUTPUT_TENSOR) and its combinations: names Pipeline(output=...) takes beside the ones above
PIPELINE_OUTPUT_TENSOR = 16
PIPELINE_TENSOR_OUTPUTS = {"tensor": PIPELINE_OUTPUT_TENSOR, "rgba+tensor": PIPELINE_OUTPUT_RGBA | PIPELINE_OUTPUT_TENSOR,
                           "ycbcr+tensor": PIPELINE_OUTPUT_YCBCR | PIPELINE_OUTPUT_TENSOR,
                           "all": PIPELINE_OUTPUT_RGBA | PIPELINE_OUTPUT_YCBCR | PIPELINE_OUTPUT_TENSOR}
# the motion output (LEON_PIPELINE_OUTPUT_MOTION): Pipeline(motion=True) ORs it into whatever output= resolves to
PIPELINE_OUTPUT_MOTION = 32
MOTION_FWD, MOTION_BWD, MOTION_INTRA = 1, 2, 4      # the bits of a motion record's info bytes
# the activity output (LEON_PIPELINE_OUTPUT_ACTIVITY, bit 7): Pipeline(activity=True) ORs it in the same way; a record's cell
PIPELINE_OUTPUT_ACTIVITY = 128
ACTIVITY_CELL = np.dtype([("ac_count", "<u2"), ("ac_mag", "<u2"), ("dc_mag", "<u2"), ("blocks", "u1"), ("qscale", "u1")])
# the residual output (LEON_PIPELINE_OUTPUT_RESIDUAL, bit 9): Pipeline(residual=True) ORs it in the same way
PIPELINE_OUTPUT_RESIDUAL = 512
TENSOR_F16, TENSOR_BF16, TENSOR_F32 = 1, 2, 3       # LEON_TENSOR_*
TENSOR_DTYPES = {"float16": TENSOR_F16, "bfloat16": TENSOR_BF16, "float32": TENSOR_F32}
TENSOR_U8 = 8                                       # LEON_TENSOR_U8 ("uint8"): the element is the 8-bit colour value
TENSOR_LAYOUT_CHW, TENSOR_LAYOUT_HWC = 0, 1         # LEON_TENSOR_LAYOUT_*
TENSOR_LAYOUTS = {"chw": TENSOR_LAYOUT_CHW, "hwc": TENSOR_LAYOUT_HWC}


def _tensor_dtype_code(dtype):
    if dtype == "uint8":
        return TENSOR_U8
    return TENSOR_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)


def _tensor_layout_code(layout):
    return TENSOR_LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def tensor_table(dtype="float16", scale=None, bias=None):
    """The table T of the tensor output (include/leon_pipeline.h), in numpy and independent of the C code: [3, 256],
    T[c][v] = to_dtype(float32(float64(v) * float64(scale[c]) + float64(bias[c]))); scale and bias default to 1/255 and 0.
    float16 / float32 arrays; bfloat16 as uint16 bit patterns (round to nearest even of the float32 value); "uint8": the identity
    table, T[c][v] = v (a scale or bias other than zero: ValueError)."""
    code = _tensor_dtype_code(dtype)
    sc = np.asarray([0, 0, 0] if scale is None else scale, dtype=np.float32).reshape(3)
    bi = np.asarray([0, 0, 0] if bias is None else bias, dtype=np.float32).reshape(3)
    if code == TENSOR_U8:
        if sc.any() or bi.any():
            raise ValueError("tensor dtype uint8 takes no scale / bias")
        return np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    if not sc.any() and not bi.any():
        sc = np.full(3, np.float32(1.0 / 255.0), dtype=np.float32)
    v = np.arange(256, dtype=np.float64)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = (v * sc.astype(np.float64)[:, None] + bi.astype(np.float64)[:, None]).astype(np.float32)
        if code == TENSOR_F32:
            return f32
        if code == TENSOR_F16:
            return f32.astype(np.float16)
    if code != TENSOR_BF16:
        raise ValueError("tensor dtype %r" % (dtype,))
    x = f32.view(np.uint32).astype(np.uint64)
    return ((x + 0x7fff + ((x >> 16) & 1)) >> 16).astype(np.uint16)


RESIZE_TRIANGLE = 0          # LEON_RESIZE_TRIANGLE
RESIZE_BICUBIC = 3           # LEON_RESIZE_BICUBIC
RESIZE_MAX_TAPS = 33         # LEON_RESIZE_MAX_TAPS
RESIZE_MAX_TAPS_BICUBIC = 65         # LEON_RESIZE_MAX_TAPS_BICUBIC
RESIZE_PRECISION = 22
RESIZE_FILTERS = {"triangle": RESIZE_TRIANGLE, "bicubic": RESIZE_BICUBIC}


def _resize_filter_code(filter):
    """a name of RESIZE_FILTERS or the raw code (what the library does not know it refuses)"""
    return RESIZE_FILTERS[filter] if isinstance(filter, str) else int(filter)


def _triangle(x):
    return max(0.0, 1.0 - abs(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def resize_weights(in_size, crop_start, crop_size, out_size, filter=RESIZE_TRIANGLE):
    """The tables of one axis of the resized tensor output (include/leon_pipeline.h), in numpy / Python floats and independent of
    the C code: (first[out], count[out], weights[out, taps]) with taps = the largest count, weights int32 with 22 fractional bits
    and zero behind count[o].  An antialiased triangle filter (filter=RESIZE_BICUBIC: Keys' cubic with a = -0.5, support 2, signed
    weights) over crop_start .. crop_start + crop_size of an axis of in_size samples: taps may leave the crop box, never the axis.
    ValueError where the library refuses."""
    filter = _resize_filter_code(filter)
    if filter not in (RESIZE_TRIANGLE, RESIZE_BICUBIC):
        raise ValueError("resize filter %d" % filter)
    f, reach = (_bicubic, 2.0) if filter == RESIZE_BICUBIC else (_triangle, 1.0)
    in_size, in0, crop_size, out_size = int(in_size), int(crop_start), int(crop_size), int(out_size)
    if not 1 <= out_size <= 4096:
        raise ValueError("output size %d is outside 1 .. 4096" % out_size)
    if in_size < 1 or crop_size < 1 or in0 < 0 or in0 + crop_size > in_size:
        raise ValueError("the crop (%d, %d) is empty or leaves the axis (%d)" % (in0, crop_size, in_size))
    if crop_size > 16 * out_size:
        raise ValueError("%d -> %d reduces by more than 16" % (crop_size, out_size))
    scale = float(crop_size) / float(out_size)
    fscale = max(scale, 1.0)
    support = reach * fscale
    first, rows = [], []
    for o in range(out_size):
        center = in0 + (o + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        w = [f((lo + k - center + 0.5) / fscale) for k in range(hi - lo)]
        total = 0.0
        for v in w:
            total += v
        first.append(lo)
        q = [(v / total) * float(1 << RESIZE_PRECISION) for v in w]
        rows.append([int(-0.5 + v) if v < 0.0 else int(0.5 + v) for v in q])
    count = np.asarray([len(r) for r in rows], dtype=np.int32)
    weights = np.zeros((out_size, int(count.max())), dtype=np.int32)
    for o, r in enumerate(rows):
        weights[o, :len(r)] = r
    return np.asarray(first, dtype=np.int32), count, weights


def _resize_pass(img, first, count, weights):
    """one pass along axis 1 of img [rows, in, channels] uint8 -> [rows, out, channels] uint8"""
    out = np.empty((img.shape[0], len(first), img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for o in range(len(first)):
        n = int(count[o])
        acc = np.tensordot(src[:, first[o]:first[o] + n, :], weights[o, :n].astype(np.int64), axes=([1], [0]))
        out[:, o, :] = np.clip((acc + (1 << (RESIZE_PRECISION - 1))) >> RESIZE_PRECISION, 0, 255)
    return out


def resize_rgb(rgb, crop, size, filter=RESIZE_TRIANGLE):
    """The resized tensor output's 8-bit colour values, in numpy: rgb [H, W, C] uint8 (the frame), crop = (x, y, width, height) in
    frame pixels (None: the whole frame), size = (out_height, out_width) -> [out_height, out_width, C] uint8.  Horizontal pass first
    with an 8-bit result, then vertical, each clamped to 0 .. 255 (include/leon_pipeline.h has the definition; filter: RESIZE_TRIANGLE or
    RESIZE_BICUBIC)."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    fh, fw = rgb.shape[:2]
    x, y, w, h = (0, 0, fw, fh) if crop is None or not any(crop) else crop
    oh, ow = size
    fx, nx, wx = resize_weights(fw, x, w, ow, filter)
    fy, ny, wy = resize_weights(fh, y, h, oh, filter)
    lo, hi = int(fy.min()), int((fy + ny).max())          # the rows the vertical pass taps
    hz = _resize_pass(rgb[lo:hi], fx, nx, wx)
    return _resize_pass(hz.transpose(1, 0, 2), fy - lo, ny, wy).transpose(1, 0, 2).copy()


def letterbox(src_width, src_height, canvas_width, canvas_height):
    """leon_pipeline_letterbox: the source scaled to fit the canvas with its aspect ratio kept, and centred ->
    (out_width, out_height, x, y).  The library's integers (no device touched)."""
    rz, cv = PipelineTensorResize(), PipelineTensorCanvas()
    _chk(load().leon_pipeline_letterbox(int(src_width), int(src_height), int(canvas_width), int(canvas_height), C.byref(rz), C.byref(cv)))
    return rz.out_width, rz.out_height, cv.x, cv.y


def canvas_rgb(rgb, crop, size, canvas, origin, pad=(0, 0, 0), filter=RESIZE_TRIANGLE):
    """The canvas tensor output's 8-bit colour values, in numpy: resize_rgb(rgb, crop, size, filter) with its top-left pixel at
    origin = (x, y) of a canvas = (height, width) array whose other pixels are pad = (r, g, b) -> [height, width, 3] uint8
    (include/leon_pipeline.h, leon_pipeline_tensor_canvas)."""
    image = resize_rgb(np.asarray(rgb)[..., :3], crop, size, filter)
    (ch, cw), (x, y), (oh, ow) = canvas, origin, size
    if x < 0 or y < 0 or x + ow > cw or y + oh > ch:
        raise ValueError("the image %d x %d at (%d, %d) leaves the canvas %d x %d" % (ow, oh, x, y, cw, ch))
    out = np.empty((ch, cw, 3), dtype=np.uint8)
    out[:] = np.asarray(pad, dtype=np.uint8)
    out[y:y + oh, x:x + ow] = image
    return out


def planes_layout(frame_width, frame_height, alpha=False):
    """the device layout of a frame's planes (include/leon_pipeline.h, leon_pipeline_config.output): rows padded to 64 bytes,
    planes on 256-byte boundaries, [Y | Cb | Cr (| A)].  Offsets are from the Y pointer; `bytes` is one frame's record."""
    up = lambda v, a: (v + a - 1) // a * a
    cw, ch = (frame_width + 1) // 2, (frame_height + 1) // 2
    ls, cs = up(frame_width, 64), up(cw, 64)
    yb, cb = up(ls * frame_height, 256), up(cs * ch, 256)
    return {"luma_stride": ls, "chroma_stride": cs, "chroma_width": cw, "chroma_height": ch,
            "cb_offset": yb, "cr_offset": yb + cb, "a_offset": yb + 2 * cb,
            "bytes": yb + 2 * cb + (up(ls * frame_height, 256) if alpha else 0)}


class LeonError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("leon error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("coded_width", C.c_int32), ("coded_height", C.c_int32), ("frame_width", C.c_int32),
                ("frame_height", C.c_int32), ("n_slots", C.c_int32), ("device_id", C.c_int32),
                ("stream", C.c_void_p), ("alpha", C.c_int32), ("contiguous_slots", C.c_int32)]


class Picture(C.Structure):
    _fields_ = [("type", C.c_int32), ("out_slot", C.c_int32), ("ref_fwd_slot", C.c_int32),
                ("ref_bwd_slot", C.c_int32), ("coef_y", C.c_void_p), ("coef_cb", C.c_void_p),
                ("coef_cr", C.c_void_p), ("qscale", C.c_void_p), ("intra", C.c_void_p),
                ("repadd", C.c_void_p), ("mv_fwd", C.c_void_p), ("mv_bwd", C.c_void_p),
                ("mb_dir", C.c_void_p),
                # ABI 2: fused display conversion (device pointer to the RGBA frame, or NULL)
                ("rgba_out", C.c_void_p), ("no_planes", C.c_int32), ("qm_set", C.c_int32),      # qm_set: ABI 3
                ("coef_a", C.c_void_p)]


class SparsePicture(C.Structure):
    _fields_ = [("type", C.c_int32), ("out_slot", C.c_int32), ("ref_fwd_slot", C.c_int32),
                ("ref_bwd_slot", C.c_int32), ("grp_off", C.c_void_p), ("entries", C.c_void_p),
                ("n_entries", C.c_uint32), ("reserved", C.c_int32), ("qscale", C.c_void_p), ("intra", C.c_void_p),
                ("repadd", C.c_void_p), ("mv_fwd", C.c_void_p), ("mv_bwd", C.c_void_p), ("mb_dir", C.c_void_p),
                ("rgba_out", C.c_void_p), ("no_planes", C.c_int32), ("qm_set", C.c_int32)]


class KernelStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("total_ms", C.c_double), ("algorithmic_bytes", C.c_double),
                ("macroblocks", C.c_uint64)]


class LaunchTime(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pic_type", C.c_int32), ("ms", C.c_double), ("algorithmic_bytes", C.c_double),
                ("macroblocks", C.c_uint64)]


def read_frame(frame):
    """one frame of a window (a dict handed to on_window) as a host array, through the pipeline that delivered it"""
    return frame["_pipe"].read_frame(frame)


class PipelineConfig(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("parser_threads", C.c_int32), ("gops_per_window", C.c_int32),
                ("windows_in_flight", C.c_int32), ("max_gop_pictures", C.c_int32), ("loop", C.c_int32),
                ("shard_index", C.c_int32), ("shard_count", C.c_int32), ("start_seconds", C.c_double),
                ("gpu_parser", C.c_int32), ("display_flavour", C.c_int32), ("output", C.c_int32)]


class PipelineTensorConfig(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class PipelineTensorResize(C.Structure):
    _fields_ = [("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_width", C.c_int32), ("crop_height", C.c_int32),
                ("out_width", C.c_int32), ("out_height", C.c_int32), ("filter", C.c_int32)]


class PipelineTensorGeometry(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("crop_width", C.c_int32),
                ("crop_height", C.c_int32), ("taps_x", C.c_int32), ("taps_y", C.c_int32), ("resized", C.c_int32)]


class PipelineTensorFormat(C.Structure):
    _fields_ = [("layout", C.c_int32), ("reserved", C.c_int32 * 7)]


class PipelineTensorCanvas(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("pad", C.c_int32 * 3),
                ("image_width", C.c_int32), ("image_height", C.c_int32), ("reserved", C.c_int32 * 7)]


class PipelineRegion(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32 * 3)]


class PipelineRegionsConfig(C.Structure):
    _fields_ = [("out_width", C.c_int32), ("out_height", C.c_int32), ("filter", C.c_int32), ("reserved", C.c_int32 * 5)]


class PipelineRegionsDevice(C.Structure):
    _fields_ = [("regions", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("device_out", C.c_void_p), ("out_pitch_bytes", C.c_uint64),
                ("device_status", C.c_void_p), ("stream", C.c_void_p), ("scratch_limit_bytes", C.c_uint64), ("reserved", C.c_uint64 * 1)]


class PipelineRegionsFit(C.Structure):
    _fields_ = [("mode", C.c_int32), ("anchor", C.c_int32), ("pad", C.c_int32 * 3), ("reserved", C.c_int32 * 3)]


REGIONS_FIT_STRETCH, REGIONS_FIT_LETTERBOX = 0, 1           # LEON_REGIONS_FIT_*
REGIONS_ANCHOR_CENTRE, REGIONS_ANCHOR_TOP_LEFT = 0, 1       # LEON_REGIONS_ANCHOR_*
REGIONS_FITS = {"stretch": REGIONS_FIT_STRETCH, "letterbox": REGIONS_FIT_LETTERBOX}
REGIONS_ANCHORS = {"centre": REGIONS_ANCHOR_CENTRE, "center": REGIONS_ANCHOR_CENTRE, "top_left": REGIONS_ANCHOR_TOP_LEFT}


def _regions_fit(fit, anchor, pad_value):
    """The PipelineRegionsFit of the fit keywords -- fit None / "stretch" / "letterbox" (or a PipelineRegionsFit), anchor "centre" /
    "top_left", pad_value (r, g, b) -- or None when none of them is set: the call without a fit.  What the settings may not be is the
    library's to refuse."""
    if isinstance(fit, PipelineRegionsFit):
        return fit
    if fit is None and anchor is None and pad_value is None:
        return None
    f = PipelineRegionsFit()
    f.mode = REGIONS_FITS[fit] if isinstance(fit, str) else int(fit or 0)
    f.anchor = REGIONS_ANCHORS[anchor] if isinstance(anchor, str) else int(anchor or 0)
    if pad_value is not None:
        r, g, b = pad_value
        f.pad[0], f.pad[1], f.pad[2] = int(r), int(g), int(b)
    return f


# LEON_REGION_*: the status word of a region whose box lies in device memory (0: resampled; otherwise skipped, and why)
REGION_OK, REGION_RESERVED, REGION_FRAME, REGION_BOX, REGION_RATIO_X, REGION_RATIO_Y, REGION_TAPS = range(7)
REGIONS_SCRATCH_DEFAULT = 256 << 20          # LEON_REGIONS_SCRATCH_DEFAULT
REGION_SCALE, REGION_OFFSET = 7, 8           # LEON_REGION_SCALE, LEON_REGION_OFFSET: a warp record's two own
REGION_NO_REFERENCE = 9                      # LEON_REGION_NO_REFERENCE: a carry record's own
REGION_SLOT = 10                             # LEON_REGION_SLOT: a propagate record's own
GAUGE_MOTION, GAUGE_ACTIVITY = 1, 2          # LEON_GAUGE_*: the bits of a gauge call's sources
ACCUMULATE_MOTION = 1                        # LEON_ACCUMULATE_MOTION: AX, AY, AGE
ACCUMULATE_RESIDUAL = 2                      # LEON_ACCUMULATE_RESIDUAL: RY, RCb, RCr
ACCUMULATE_PLANES = ("AX", "AY", "AGE", "RY", "RCb", "RCr")          # the planes of an accumulator, in their order in a slot
FIELD_SOURCE_BUFFER, FIELD_SOURCE_MOTION, FIELD_SOURCE_RESIDUAL = 0, 1, 2          # LEON_FIELD_SOURCE_*
FIELD_SOURCES = {"buffer": FIELD_SOURCE_BUFFER, "motion": FIELD_SOURCE_MOTION, "residual": FIELD_SOURCE_RESIDUAL}
FIELD_MAX_CHANNELS = 8                       # LEON_FIELD_MAX_CHANNELS
GAUGE_WORDS = 16                             # int64 words of a gauged record's statistics
PROPOSE_MOTION, PROPOSE_ACTIVITY = 1, 2      # LEON_PROPOSE_*: the bits of a propose call's sources
PROPOSE_INTRA = 1                            # LEON_PROPOSE_INTRA: the bit of its flags
PROPOSE_MAX_BOXES, PROPOSE_MAX_CELLS = 1024, 65536
OVERLAP_IOU, OVERLAP_IOMIN = 0, 1            # LEON_OVERLAP_*: the measure of a suppress or match call
OVERLAP_MAX_ROWS = 1024                      # rows of a set


class PipelineWarpRegion(C.Structure):
    _fields_ = [("frame", C.c_int32), ("m", C.c_int32 * 6), ("reserved", C.c_int32)]


class PipelineWarpConfig(C.Structure):
    _fields_ = [("out_width", C.c_int32), ("out_height", C.c_int32), ("pad", C.c_int32 * 3), ("reserved", C.c_int32 * 3)]


class PipelineWarpRegionsCall(C.Structure):
    _fields_ = [("regions", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("device_out", C.c_void_p), ("out_pitch_bytes", C.c_uint64),
                ("device_status", C.c_void_p), ("stream", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class PipelineCarryRegion(C.Structure):
    _fields_ = [("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("target", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class PipelineCarryRegionsCall(C.Structure):
    _fields_ = [("regions", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("device_out", C.c_void_p), ("device_votes", C.c_void_p),
                ("device_status", C.c_void_p), ("stream", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class PipelineGaugeConfig(C.Structure):
    _fields_ = [("sources", C.c_int32), ("reserved", C.c_int32 * 7)]


class PipelineGaugeRegionsCall(C.Structure):
    _fields_ = [("regions", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("device_stats", C.c_void_p), ("device_status", C.c_void_p), ("stream", C.c_void_p),
                ("reserved", C.c_uint64 * 3)]


class PipelineProposeConfig(C.Structure):
    _fields_ = [("sources", C.c_int32), ("flags", C.c_int32), ("mv_min", C.c_int32), ("ac_min", C.c_int32), ("connectivity", C.c_int32), ("min_cells", C.c_int32),
                ("max_boxes", C.c_int32), ("reserved", C.c_int32)]


class PipelineProposeRegionsCall(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("device_regions", C.c_void_p), ("device_info", C.c_void_p),
                ("device_count", C.c_void_p), ("device_status", C.c_void_p), ("stream", C.c_void_p), ("reserved", C.c_uint64 * 1)]


class PipelineOverlapConfig(C.Structure):
    _fields_ = [("measure", C.c_int32), ("threshold", C.c_int32), ("reserved", C.c_int32 * 2)]


class PipelineSuppressRegionsCall(C.Structure):
    _fields_ = [("regions", C.c_void_p), ("scores", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32), ("score_stride", C.c_int32), ("reserved0", C.c_int32),
                ("device_out", C.c_void_p), ("device_order", C.c_void_p), ("device_by", C.c_void_p), ("device_count", C.c_void_p), ("device_status", C.c_void_p),
                ("stream", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class PipelineMatchRegionsCall(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("n", C.c_int32), ("ka", C.c_int32), ("kb", C.c_int32), ("reserved0", C.c_int32), ("device_match_a", C.c_void_p),
                ("device_match_b", C.c_void_p), ("device_overlap", C.c_void_p), ("device_count", C.c_void_p), ("device_status_a", C.c_void_p),
                ("device_status_b", C.c_void_p), ("stream", C.c_void_p), ("reserved", C.c_uint64 * 1)]


class PipelinePropagateHop(C.Structure):
    _fields_ = [("target", C.c_int32), ("dst_slot", C.c_int32), ("fwd_slot", C.c_int32), ("bwd_slot", C.c_int32), ("reserved", C.c_int32 * 4)]


class PipelinePropagateConfig(C.Structure):
    _fields_ = [("stride", C.c_int32), ("planes", C.c_int32), ("elem_bytes", C.c_int32), ("n_slots", C.c_int32), ("fill", C.c_uint32), ("reserved0", C.c_int32),
                ("slot_pitch_bytes", C.c_uint64), ("maps_bytes", C.c_uint64)]


class PipelinePropagateLayout(C.Structure):
    _fields_ = [("mw", C.c_int32), ("mh", C.c_int32), ("planes_per_group", C.c_int32), ("fast_path", C.c_int32), ("plane_bytes", C.c_uint64), ("slot_bytes", C.c_uint64)]


class PipelinePropagateMapsCall(C.Structure):
    _fields_ = [("hops", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("maps", C.c_void_p), ("device_via", C.c_void_p), ("device_status", C.c_void_p),
                ("stream", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class PipelineAccumulateConfig(C.Structure):
    _fields_ = [("parts", C.c_int32), ("n_slots", C.c_int32), ("reserved", C.c_int32 * 2), ("slot_pitch_bytes", C.c_uint64), ("slots_bytes", C.c_uint64)]


class PipelineAccumulateLayout(C.Structure):
    _fields_ = [("coded_width", C.c_int32), ("coded_height", C.c_int32), ("parts", C.c_int32), ("planes", C.c_int32), ("luma_stride", C.c_int32), ("chroma_stride", C.c_int32),
                ("ax_offset", C.c_uint32), ("ay_offset", C.c_uint32), ("age_offset", C.c_uint32), ("ry_offset", C.c_uint32), ("rcb_offset", C.c_uint32),
                ("rcr_offset", C.c_uint32), ("slot_bytes", C.c_uint32), ("slot_pitch", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PipelineAccumulateCall(C.Structure):
    _fields_ = [("hops", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("slots", C.c_void_p), ("device_via", C.c_void_p), ("device_status", C.c_void_p),
                ("stream", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class PipelineFieldChannel(C.Structure):
    _fields_ = [("offset_bytes", C.c_uint32), ("row_stride", C.c_int32), ("elem_stride", C.c_int32), ("shift", C.c_int32), ("scale", C.c_float), ("bias", C.c_float),
                ("reserved", C.c_int32 * 2)]


class PipelineFieldConfig(C.Structure):
    _fields_ = [("source", C.c_int32), ("dtype", C.c_int32), ("channels", C.c_int32), ("filter", C.c_int32), ("out_width", C.c_int32), ("out_height", C.c_int32),
                ("n_items", C.c_int32), ("reserved", C.c_int32), ("item_pitch_bytes", C.c_uint64), ("source_bytes", C.c_uint64), ("channel", PipelineFieldChannel * 8)]


class PipelineFieldTensorsCall(C.Structure):
    _fields_ = [("records", C.c_void_p), ("n", C.c_int32), ("reserved0", C.c_int32), ("source", C.c_void_p), ("device_out", C.c_void_p), ("out_pitch_bytes", C.c_uint64),
                ("device_status", C.c_void_p), ("stream", C.c_void_p), ("reserved", C.c_uint64)]


class PipelineTensorShape(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("element_bytes", C.c_int32), ("layout", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("stride_c", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64)]


class PipelineMotionLayout(C.Structure):
    _fields_ = [("mb_width", C.c_int32), ("mb_height", C.c_int32), ("mbs", C.c_int32), ("reserved0", C.c_int32), ("info_offset", C.c_uint64),
                ("summary_offset", C.c_uint64), ("record_bytes", C.c_uint64), ("record_pitch", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class PipelineMotionFrame(C.Structure):
    _fields_ = [("record", C.c_void_p), ("fwd_gop", C.c_uint64), ("fwd_display", C.c_int32), ("bwd_display", C.c_int32), ("reserved", C.c_int32 * 2)]


class PipelineMotionPicture(C.Structure):
    _fields_ = [("type", C.c_int32), ("reserved0", C.c_int32), ("repadd", C.c_void_p), ("mb_dir", C.c_void_p), ("mv_fwd", C.c_void_p), ("mv_bwd", C.c_void_p)]


class PipelineActivityLayout(C.Structure):
    _fields_ = [("mb_width", C.c_int32), ("mb_height", C.c_int32), ("mbs", C.c_int32), ("reserved0", C.c_int32), ("summary_offset", C.c_uint64),
                ("record_bytes", C.c_uint64), ("record_pitch", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class PipelineActivityPicture(C.Structure):
    _fields_ = [("grp_off", C.c_void_p), ("entries", C.c_void_p), ("qscale", C.c_void_p), ("n_entries", C.c_uint32), ("reserved0", C.c_int32)]


class PipelineResidualLayout(C.Structure):
    _fields_ = [("coded_width", C.c_int32), ("coded_height", C.c_int32), ("luma_stride", C.c_int32), ("chroma_stride", C.c_int32), ("cb_offset", C.c_uint64),
                ("cr_offset", C.c_uint64), ("record_bytes", C.c_uint64), ("record_pitch", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class PipelineResidualPicture(C.Structure):
    _fields_ = [("grp_off", C.c_void_p), ("entries", C.c_void_p), ("qscale", C.c_void_p), ("intra", C.c_void_p), ("matrices", C.c_void_p),
                ("premultiplier", C.c_void_p), ("n_entries", C.c_uint32), ("reserved0", C.c_int32)]


class PipelineFrame(C.Structure):
    _fields_ = [("gop", C.c_uint64), ("display_index", C.c_int32), ("type", C.c_int32), ("ts_ms", C.c_double),
                ("rgba", C.c_void_p), ("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p), ("a", C.c_void_p)]


class PipelineInfo(C.Structure):
    _fields_ = [("coded_width", C.c_int32), ("coded_height", C.c_int32), ("frame_width", C.c_int32), ("frame_height", C.c_int32),
                ("picture_rate", C.c_double), ("duration", C.c_double), ("gops", C.c_uint32), ("shard_gops", C.c_uint32),
                ("first_gop", C.c_uint32), ("parser_threads", C.c_int32), ("gops_per_window", C.c_int32),
                ("gpu_parser", C.c_int32), ("display_flavour", C.c_int32), ("output", C.c_int32),
                ("chroma_width", C.c_int32), ("chroma_height", C.c_int32), ("luma_stride", C.c_int32), ("chroma_stride", C.c_int32),
                ("tensor_dtype", C.c_int32), ("tensor_element_bytes", C.c_int32), ("tensor_frame_bytes", C.c_uint64),
                ("tensor_frame_pitch", C.c_uint64), ("tensor_gop_pitch", C.c_uint64)]


class PipelineStats(C.Structure):
    _fields_ = [("pictures", C.c_uint64), ("gops", C.c_uint64), ("windows", C.c_uint64), ("stream_bytes", C.c_uint64),
                ("seconds", C.c_double), ("parse_seconds_sum", C.c_double), ("upload_bytes", C.c_double), ("entries", C.c_uint64)]


PIPELINE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.POINTER(PipelineFrame), C.c_int32, C.c_int32)

_lib = None


def load():
    """dlopen the library (no GPU needed for this); raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; two HIP runtimes in one process cannot both
    # own the GPU ("No HIP GPUs are available").  Whichever is loaded first serves both,
    # so when torch is going to be used in this process let it load first.
    if os.environ.get("LEON_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    path = os.environ.get("LEON_DEBUG_LIB") or LIB_PATH      # A/B runs of kernel variants (tools/ab_bench.sh)
    if not os.path.exists(path):
        raise ImportError("libleon_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C mpeg1video-decoder-webgl_amd/csrc` (no CPU fallback exists)")
    lib = C.CDLL(path)
    if lib.leon_abi_version() != ABI_VERSION:
        raise ImportError("libleon_hip.so (%s) speaks ABI %d, this binding ABI %d: rebuild it" % (path, lib.leon_abi_version(), ABI_VERSION))
    lib.leon_last_error.restype = C.c_char_p
    lib.leon_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    lib.leon_destroy.argtypes = [C.c_void_p]
    lib.leon_destroy.restype = None
    lib.leon_set_quant_matrices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.leon_add_quant_matrices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    lib.leon_acquire_slot.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.leon_release_slot.argtypes = [C.c_void_p, C.c_int32]
    lib.leon_free_decoded_slots.argtypes = [C.c_void_p]
    lib.leon_submit_picture.argtypes = [C.c_void_p, C.POINTER(Picture)]
    lib.leon_submit_batch.argtypes = [C.c_void_p, C.POINTER(Picture), C.c_int32, C.c_int32]
    lib.leon_batch_create.argtypes = [C.c_void_p, C.POINTER(Picture), C.c_int32, C.POINTER(C.c_void_p)]
    lib.leon_submit_sparse.argtypes = [C.c_void_p, C.POINTER(SparsePicture), C.c_int32, C.c_int32]
    lib.leon_batch_create_sparse.argtypes = [C.c_void_p, C.POINTER(SparsePicture), C.c_int32, C.POINTER(C.c_void_p)]
    lib.leon_batch_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.leon_batch_destroy.argtypes = [C.c_void_p, C.c_void_p]
    lib.leon_batch_destroy.restype = None
    lib.leon_convert_rgba.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
    lib.leon_convert_rgba_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    lib.leon_read_planes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.leon_write_planes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.leon_read_alpha_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.leon_write_alpha_plane.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.leon_slot_device_ptr.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.leon_sync.argtypes = [C.c_void_p]
    lib.leon_set_overlap_convert.argtypes = [C.c_void_p, C.c_int32]
    lib.leon_timing_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.leon_timing_reset.argtypes = [C.c_void_p]
    lib.leon_timing_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(KernelStats)]
    lib.leon_timing_get_launches.argtypes = [C.c_void_p, C.POINTER(LaunchTime), C.c_int32, C.POINTER(C.c_int32)]
    lib.leon_measure_copy_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_double)]
    lib.leon_measure_stream_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.leon_device_pool_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    lib.leon_device_malloc.argtypes = [C.c_int32, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
    lib.leon_device_free.argtypes = [C.c_void_p]
    lib.leon_pipeline_create.argtypes = [C.POINTER(PipelineConfig), C.c_void_p, C.c_size_t, PIPELINE_CB, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_create_partial.argtypes = [C.POINTER(PipelineConfig), C.c_void_p, C.c_size_t, C.c_size_t, PIPELINE_CB, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_feed.argtypes = [C.c_void_p, C.c_size_t]
    lib.leon_pipeline_get_info.argtypes = [C.c_void_p, C.POINTER(PipelineInfo)]
    lib.leon_pipeline_release_window.argtypes = [C.c_void_p, C.c_int64]
    lib.leon_pipeline_wait.argtypes = [C.c_void_p]
    lib.leon_pipeline_get_stats.argtypes = [C.c_void_p, C.POINTER(PipelineStats)]
    lib.leon_pipeline_read_frame.argtypes = [C.c_void_p, C.POINTER(PipelineFrame), C.c_void_p]
    lib.leon_pipeline_read_frame_planes.argtypes = [C.c_void_p, C.POINTER(PipelineFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.leon_pipeline_create_tensor.argtypes = [C.POINTER(PipelineConfig), C.POINTER(PipelineTensorConfig), C.c_void_p, C.c_size_t, C.c_size_t, PIPELINE_CB,
                                                C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_create_tensor_resized.argtypes = [C.POINTER(PipelineConfig), C.POINTER(PipelineTensorConfig), C.POINTER(PipelineTensorResize), C.c_void_p,
                                                        C.c_size_t, C.c_size_t, PIPELINE_CB, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_resize_weights.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.leon_pipeline_get_tensor_geometry.argtypes = [C.c_void_p, C.POINTER(PipelineTensorGeometry)]
    lib.leon_pipeline_create_tensor_format.argtypes = [C.POINTER(PipelineConfig), C.POINTER(PipelineTensorConfig), C.POINTER(PipelineTensorResize),
                                                       C.POINTER(PipelineTensorFormat), C.c_void_p, C.c_size_t, C.c_size_t, PIPELINE_CB, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_get_tensor_shape.argtypes = [C.c_void_p, C.POINTER(PipelineTensorShape)]
    lib.leon_pipeline_create_tensor_canvas.argtypes = [C.POINTER(PipelineConfig), C.POINTER(PipelineTensorConfig), C.POINTER(PipelineTensorResize),
                                                       C.POINTER(PipelineTensorFormat), C.POINTER(PipelineTensorCanvas), C.c_void_p, C.c_size_t, C.c_size_t,
                                                       PIPELINE_CB, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.leon_pipeline_get_tensor_canvas.argtypes = [C.c_void_p, C.POINTER(PipelineTensorCanvas)]
    lib.leon_pipeline_letterbox.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineTensorResize), C.POINTER(PipelineTensorCanvas)]
    lib.leon_pipeline_tensor_table.argtypes = [C.POINTER(PipelineConfig), C.POINTER(PipelineTensorConfig), C.c_void_p]
    lib.leon_pipeline_window_tensors.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.c_int32]
    lib.leon_pipeline_read_tensor.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    if hasattr(lib, "leon_pipeline_regions_check"):          # (an older build under LEON_DEBUG_LIB, A/B runs against a parent commit, has none of the three)
        lib.leon_pipeline_regions_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineRegion), C.c_int32, C.POINTER(PipelineRegionsConfig), C.POINTER(C.c_int32)]
        lib.leon_pipeline_resample_regions.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PipelineRegion), C.c_int32, C.POINTER(PipelineRegionsConfig), C.c_void_p, C.c_uint64]
        lib.leon_pipeline_read_regions.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PipelineRegion), C.c_int32, C.POINTER(PipelineRegionsConfig), C.c_void_p]
    if hasattr(lib, "leon_pipeline_resample_regions_fit"):
        P = C.POINTER
        lib.leon_pipeline_region_fit_rect.argtypes = [C.c_int32, C.c_int32, P(PipelineRegionsConfig), P(PipelineRegionsFit), P(C.c_int32)]
        lib.leon_pipeline_regions_fit_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(PipelineRegion), C.c_int32, P(PipelineRegionsConfig), P(PipelineRegionsFit),
                                                        P(C.c_int32)]
        lib.leon_pipeline_region_fit_status.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(PipelineRegion), P(PipelineRegionsConfig), P(PipelineRegionsFit)]
        lib.leon_pipeline_region_fit_status.restype = C.c_int32
        lib.leon_pipeline_resample_regions_fit.argtypes = [C.c_void_p, C.c_int64, P(PipelineRegion), C.c_int32, P(PipelineRegionsConfig), P(PipelineRegionsFit), C.c_void_p,
                                                           C.c_uint64]
        lib.leon_pipeline_read_regions_fit.argtypes = [C.c_void_p, C.c_int64, P(PipelineRegion), C.c_int32, P(PipelineRegionsConfig), P(PipelineRegionsFit), C.c_void_p]
        lib.leon_pipeline_resample_regions_device_fit.argtypes = [C.c_void_p, C.c_int64, P(PipelineRegionsConfig), P(PipelineRegionsFit), P(PipelineRegionsDevice), C.c_void_p]
    if hasattr(lib, "leon_pipeline_resample_regions_device"):
        lib.leon_pipeline_resample_regions_device.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PipelineRegionsConfig), C.POINTER(PipelineRegionsDevice)]
        lib.leon_pipeline_region_status.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineRegion), C.POINTER(PipelineRegionsConfig)]
        lib.leon_pipeline_region_status.restype = C.c_int32
        lib.leon_pipeline_resize_weights_device.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_warp_regions"):
        P = C.POINTER
        lib.leon_pipeline_warp_regions_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(PipelineWarpRegion), C.c_int32, P(PipelineWarpConfig), P(C.c_int32)]
        lib.leon_pipeline_warp_region_status.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(PipelineWarpRegion), P(PipelineWarpConfig)]
        lib.leon_pipeline_warp_region_status.restype = C.c_int32
        lib.leon_pipeline_warp_from_matrix.argtypes = [P(C.c_double), P(C.c_int32)]
        lib.leon_pipeline_warp_from_rotated_box.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, P(C.c_int32)]
        lib.leon_pipeline_warp_regions.argtypes = [C.c_void_p, C.c_int64, P(PipelineWarpRegion), C.c_int32, P(PipelineWarpConfig), C.c_void_p, C.c_uint64]
        lib.leon_pipeline_read_warp_regions.argtypes = [C.c_void_p, C.c_int64, P(PipelineWarpRegion), C.c_int32, P(PipelineWarpConfig), C.c_void_p]
        lib.leon_pipeline_warp_regions_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineWarpConfig), P(PipelineWarpRegionsCall)]
    if hasattr(lib, "leon_pipeline_window_motion"):
        lib.leon_pipeline_motion_layout.argtypes = [C.c_int32, C.c_int32, C.POINTER(PipelineMotionLayout)]
        lib.leon_pipeline_motion_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_get_motion_layout.argtypes = [C.c_void_p, C.POINTER(PipelineMotionLayout)]
        lib.leon_pipeline_window_motion.argtypes = [C.c_void_p, C.c_int64, C.POINTER(PipelineMotionFrame), C.c_int32]
        lib.leon_pipeline_read_motion.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_motion_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineMotionPicture), C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_void_p]
    if hasattr(lib, "leon_pipeline_window_activity"):
        lib.leon_pipeline_activity_layout.argtypes = [C.c_int32, C.c_int32, C.POINTER(PipelineActivityLayout)]
        lib.leon_pipeline_activity_record.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_activity_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineActivityPicture), C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                      C.c_int32, C.c_void_p]
        lib.leon_pipeline_get_activity_layout.argtypes = [C.c_void_p, C.POINTER(PipelineActivityLayout)]
        lib.leon_pipeline_window_activity.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.c_int32]
        lib.leon_pipeline_read_activity.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_window_residual"):
        lib.leon_pipeline_residual_layout.argtypes = [C.c_int32, C.c_int32, C.POINTER(PipelineResidualLayout)]
        lib.leon_pipeline_residual_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(PipelineResidualPicture), C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                      C.c_int32, C.c_void_p]
        lib.leon_pipeline_get_residual_layout.argtypes = [C.c_void_p, C.POINTER(PipelineResidualLayout)]
        lib.leon_pipeline_window_residual.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.c_int32]
        lib.leon_pipeline_read_residual.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_carry_regions"):
        P = C.POINTER
        lib.leon_pipeline_carry_refs.argtypes = [P(PipelineFrame), P(PipelineMotionFrame), C.c_int32, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_carry_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, P(C.c_void_p), C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        lib.leon_pipeline_carry_record.restype = C.c_int32
        lib.leon_pipeline_get_carry_refs.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
        lib.leon_pipeline_carry_regions_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineCarryRegionsCall)]
        lib.leon_pipeline_carry_regions.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_carry_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, P(C.c_void_p), C.c_void_p,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_propagate_maps"):
        P = C.POINTER
        lib.leon_pipeline_propagate_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(PipelinePropagateLayout)]
        lib.leon_pipeline_propagate_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(PipelinePropagateConfig), C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
        lib.leon_pipeline_propagate_record.restype = C.c_int32
        lib.leon_pipeline_propagate_maps_device.argtypes = [C.c_void_p, C.c_int64, P(PipelinePropagateConfig), P(PipelinePropagateMapsCall)]
        lib.leon_pipeline_propagate_maps.argtypes = [C.c_void_p, C.c_int64, P(PipelinePropagateConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_propagate_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(PipelinePropagateConfig), C.c_void_p,
                                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_accumulate"):
        P = C.POINTER
        lib.leon_pipeline_accumulate_layout.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(PipelineAccumulateLayout)]
        lib.leon_pipeline_accumulate_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineAccumulateConfig), C.c_void_p, C.c_void_p,
                                                        C.c_void_p]
        lib.leon_pipeline_accumulate_record.restype = C.c_int32
        lib.leon_pipeline_accumulate_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineAccumulateConfig), P(PipelineAccumulateCall)]
        lib.leon_pipeline_accumulate.argtypes = [C.c_void_p, C.c_int64, P(PipelineAccumulateConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_accumulate_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineAccumulateConfig), C.c_void_p,
                                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_field_tensors"):
        P = C.POINTER
        lib.leon_pipeline_field_tensor_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(PipelineFieldConfig), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_field_tensor_record.restype = C.c_int32
        lib.leon_pipeline_field_tensors_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineFieldConfig), P(PipelineFieldTensorsCall)]
        lib.leon_pipeline_field_tensors.argtypes = [C.c_void_p, C.c_int64, P(PipelineFieldConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.leon_pipeline_field_tensors_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(PipelineFieldConfig), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                           C.c_uint64, C.c_void_p, C.c_uint64]
    if hasattr(lib, "leon_pipeline_gauge_regions"):
        P = C.POINTER
        lib.leon_pipeline_gauge_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineGaugeConfig), C.c_void_p,
                                                   C.c_void_p]
        lib.leon_pipeline_gauge_record.restype = C.c_int32
        lib.leon_pipeline_gauge_regions_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineGaugeConfig), P(PipelineGaugeRegionsCall)]
        lib.leon_pipeline_gauge_regions.argtypes = [C.c_void_p, C.c_int64, P(PipelineGaugeConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_gauge_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineGaugeConfig),
                                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_propose_regions"):
        P = C.POINTER
        lib.leon_pipeline_propose_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineProposeConfig), C.c_int32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_propose_record.restype = C.c_int32
        lib.leon_pipeline_propose_regions_device.argtypes = [C.c_void_p, C.c_int64, P(PipelineProposeConfig), P(PipelineProposeRegionsCall)]
        lib.leon_pipeline_propose_regions.argtypes = [C.c_void_p, C.c_int64, P(PipelineProposeConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.leon_pipeline_propose_kernel.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_void_p), P(C.c_void_p), P(PipelineProposeConfig),
                                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "leon_pipeline_suppress_regions"):
        P, i32, vp = C.POINTER, C.c_int32, C.c_void_p
        lib.leon_pipeline_suppress_record.argtypes = [i32, i32, i32, P(PipelineOverlapConfig), vp, i32, vp, i32, vp, vp, vp, vp, vp]
        lib.leon_pipeline_suppress_record.restype = i32
        lib.leon_pipeline_match_record.argtypes = [i32, i32, i32, P(PipelineOverlapConfig), vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
        lib.leon_pipeline_match_record.restype = i32
        lib.leon_pipeline_suppress_regions_device.argtypes = [vp, C.c_int64, P(PipelineOverlapConfig), P(PipelineSuppressRegionsCall)]
        lib.leon_pipeline_match_regions_device.argtypes = [vp, C.c_int64, P(PipelineOverlapConfig), P(PipelineMatchRegionsCall)]
        lib.leon_pipeline_suppress_regions.argtypes = [vp, C.c_int64, P(PipelineOverlapConfig), vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
        lib.leon_pipeline_match_regions.argtypes = [vp, C.c_int64, P(PipelineOverlapConfig), vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        lib.leon_pipeline_suppress_kernel.argtypes = [i32, i32, i32, i32, P(PipelineOverlapConfig), vp, i32, i32, vp, i32, vp, vp, vp, vp, vp]
        lib.leon_pipeline_match_kernel.argtypes = [i32, i32, i32, i32, P(PipelineOverlapConfig), vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.leon_pipeline_error.argtypes = [C.c_void_p]
    lib.leon_pipeline_error.restype = C.c_char_p
    lib.leon_pipeline_seek.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int64)]
    lib.leon_pipeline_destroy.argtypes = [C.c_void_p]
    lib.leon_pipeline_destroy.restype = None
    _lib = lib
    return lib


def _chk(rc):
    if rc != OK:
        raise LeonError(rc, load().leon_last_error().decode("utf-8", "replace"))


def _regions_args(regions, size, filter):
    """(PipelineRegion array, n, PipelineRegionsConfig) of a list of (frame_index, x, y, w, h) -- or PipelineRegion structs, or one
    integer array [n, 5] -- and
    size = (out_height, out_width) -- or a PipelineRegionsConfig"""
    if isinstance(regions, np.ndarray):          # [n, 5] integers: no Python loop over the regions
        full = np.zeros((len(regions), 8), dtype=np.int32)
        full[:, :5] = regions
        arr = (PipelineRegion * max(1, len(full))).from_buffer_copy(full.tobytes() or bytes(32))
        cfg = size if isinstance(size, PipelineRegionsConfig) else PipelineRegionsConfig(int(size[1]), int(size[0]), _resize_filter_code(filter))
        return arr, len(full), cfg
    regions = list(regions)
    arr = (PipelineRegion * max(1, len(regions)))()
    for i, r in enumerate(regions):
        arr[i] = r if isinstance(r, PipelineRegion) else PipelineRegion(*[int(v) for v in r])
    cfg = size if isinstance(size, PipelineRegionsConfig) else PipelineRegionsConfig(int(size[1]), int(size[0]), _resize_filter_code(filter))
    return arr, len(regions), cfg


def regions_check(frame_width, frame_height, n_frames, regions, size, filter="triangle"):
    """leon_pipeline_regions_check: what Pipeline.resample_regions would refuse of these regions (a list of (frame_index, x, y, w, h))
    for a window of n_frames frames of frame_width x frame_height, without a device.  Returns None when they are accepted; raises
    LeonError otherwise, its `bad` the index of the first offending region (-1: size, filter or the number of regions)."""
    arr, n, cfg = _regions_args(regions, size, filter)
    bad = C.c_int32(-2)
    rc = load().leon_pipeline_regions_check(int(frame_width), int(frame_height), int(n_frames), arr, n, C.byref(cfg), C.byref(bad))
    if rc != OK:
        e = LeonError(rc, load().leon_last_error().decode("utf-8", "replace"))
        e.bad = bad.value
        raise e


def region_status(frame_width, frame_height, n_frames, region, size, filter="triangle"):
    """leon_pipeline_region_status: the REGION_* word Pipeline.resample_regions_device writes for region = (frame_index, x, y, w, h) (or a
    PipelineRegion) in a window of n_frames frames of frame_width x frame_height -- 0 exactly where regions_check accepts the region alone.
    No device.  LeonError for a size or filter the library refuses."""
    arr, _, cfg = _regions_args([region], size, filter)
    st = load().leon_pipeline_region_status(int(frame_width), int(frame_height), int(n_frames), arr, C.byref(cfg))
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st


def motion_layout(mbw, mbh):
    """leon_pipeline_motion_layout: where the parts of a motion record of mbw x mbh macroblocks lie (PipelineMotionLayout), no device"""
    out = PipelineMotionLayout()
    _chk(load().leon_pipeline_motion_layout(int(mbw), int(mbh), C.byref(out)))
    return out


def _motion_parts(buf, lay):
    """(mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8, summary [8] uint32): copies of the specified parts of a record buffer"""
    mbs = lay.mbs
    mv = buf[:8 * mbs].view(np.int16).reshape(lay.mb_height, lay.mb_width, 4).copy()
    info = buf[lay.info_offset:lay.info_offset + mbs].reshape(lay.mb_height, lay.mb_width).copy()
    summary = buf[lay.summary_offset:lay.summary_offset + 32].view(np.uint32).copy()
    return mv, info, summary


def motion_record(type, mbw, mbh, repadd=None, mb_dir=None, mv_fwd=None, mv_bwd=None, fill=None):
    """leon_pipeline_motion_record: the library's CPU evaluation of a picture's motion record from its maps (as leon_vlc_ctypes.Stream
    gives them; those the type does not have may be None) -> (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8, summary [8] uint32).
    fill: the byte the record buffer holds beforehand -- the call then returns (mv, info, summary, buffer), the whole record_bytes
    buffer as the library left it (its unspecified bytes still hold the fill)."""
    lay = motion_layout(mbw, mbh)
    buf = np.full(lay.record_bytes, 0 if fill is None else int(fill), dtype=np.uint8)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in ((repadd, np.uint8), (mb_dir, np.uint8), (mv_fwd, np.int16), (mv_bwd, np.int16))]
    _chk(load().leon_pipeline_motion_record(int(type), int(mbw), int(mbh), *[None if a is None else a.ctypes.data for a in keep], buf.ctypes.data))
    parts = _motion_parts(buf, lay)
    return parts if fill is None else parts + (buf,)


def motion_from_maps(type, mbw, mbh, repadd=None, mb_dir=None, mv_fwd=None, mv_bwd=None):
    """The definition of a frame's motion record (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_MOTION) in numpy, written from the
    header's text and independent of the C code: a picture's maps -> (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8, summary [8] uint32).
    The `intra` map plays no part; an unused direction's vector reads as zero."""
    mbs = int(mbw) * int(mbh)
    mv = np.zeros((mbs, 4), dtype=np.int16)
    if type == 1:
        info = np.full(mbs, 4, dtype=np.uint8)
    else:
        intra = np.asarray(repadd).reshape(-1)[:mbs].astype(np.int64) >= 128
        d = np.where(intra, 0, 1 if type == 2 else np.asarray(mb_dir).reshape(-1)[:mbs].astype(np.int64) & 3)
        info = np.where(intra, 4, d).astype(np.uint8)
        fwd = np.asarray(mv_fwd, dtype=np.int16).reshape(-1)[:2 * mbs].reshape(mbs, 2)
        mv[:, 0:2] = np.where((d & 1)[:, None] != 0, fwd, 0)
        if type == 3:
            bwd = np.asarray(mv_bwd, dtype=np.int16).reshape(-1)[:2 * mbs].reshape(mbs, 2)
            mv[:, 2:4] = np.where((d & 2)[:, None] != 0, bwd, 0)
    a = np.abs(mv.astype(np.int64))
    summary = np.array([int(((info & 1) != 0).sum()), int(((info & 2) != 0).sum()), int(((info & 4) != 0).sum()), int(mv.any(axis=1).sum()),
                        int(a[:, 0].sum()), int(a[:, 1].sum()), int(a[:, 2].sum()), int(a[:, 3].sum())], dtype=np.uint32)
    return mv.reshape(int(mbh), int(mbw), 4), info.reshape(int(mbh), int(mbw)), summary


def motion_kernel(mbw, mbh, pictures, frames, ring_frames=None, pad_byte=0, fill=0xA5, ring=None, device_id=0, n_pictures=None, n_frames=None):
    """leon_pipeline_motion_kernel: k_motion on maps the caller supplies.  pictures = [(type, repadd, mb_dir, mv_fwd, mv_bwd), ...] (maps
    as motion_record takes them, None where the type has none); frames = [(picture, ring index), ...] or an integer array [n, 2];
    every map's padding on the device holds pad_byte.  Returns the ring, uint8 [ring_frames, record_pitch], as it came back: it went
    up holding `fill` in every byte -- or is the caller's `ring` (a contiguous uint8 array), written in place.  pictures, frames None:
    a null pointer; n_pictures, n_frames: the counts handed to the library when they are to differ from the lists' lengths."""
    def one(q, pic):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in zip(pic[1:], (np.uint8, np.uint8, np.int16, np.int16))]
        q.type = int(pic[0])
        q.repadd, q.mb_dir, q.mv_fwd, q.mv_bwd = [None if a is None else a.ctypes.data for a in arrs]
        return arrs
    return _record_kernel("leon_pipeline_motion_kernel", motion_layout, PipelineMotionPicture, one, mbw, mbh, pictures, frames, ring_frames, pad_byte, fill, ring, device_id,
                          n_pictures, n_frames)


def _record_kernel(symbol, layout_fn, struct, one, mbw, mbh, pictures, frames, ring_frames, pad_byte, fill, ring, device_id, n_pictures, n_frames):
    """what motion_kernel and activity_kernel share: the ring made where the caller has none, the pictures as an array of `struct`,
    each filled by one(structure, picture) -> the arrays it points into (kept until the call returns), the frames as int32 [n, 2], the
    counts the lists' lengths unless the caller says otherwise, the call `symbol`"""
    if ring is None:
        ring = np.full((int(ring_frames), int(layout_fn(mbw, mbh).record_pitch)), int(fill), dtype=np.uint8)
    assert ring.dtype == np.uint8 and ring.flags.c_contiguous and ring.flags.writeable
    keep, pics = [], None
    if pictures is not None:
        pics = (struct * max(1, len(pictures)))()
        keep.extend(one(pics[i], pic) for i, pic in enumerate(pictures))
    fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32).reshape(-1, 2)
    _chk(getattr(load(), symbol)(int(device_id), int(mbw), int(mbh), pics, (0 if pictures is None else len(pictures)) if n_pictures is None else int(n_pictures),
                                 None if fr is None or not len(fr) else fr.ctypes.data, (0 if fr is None else len(fr)) if n_frames is None else int(n_frames),
                                 len(ring) if ring_frames is None else int(ring_frames), int(pad_byte), ring.ctypes.data))
    return ring


def activity_layout(mbw, mbh):
    """leon_pipeline_activity_layout: where the parts of an activity record of mbw x mbh macroblocks lie (PipelineActivityLayout), no device"""
    out = PipelineActivityLayout()
    _chk(load().leon_pipeline_activity_layout(int(mbw), int(mbh), C.byref(out)))
    return out


def activity_groups(mbw, mbh):
    """(groups_y, groups_c, n_y, n_c) of a picture of mbw x mbh macroblocks (include/leon_vlc.h); an activity record reads groups 0 .. n_y + 2 n_c - 1"""
    gy, gc = -(-int(mbw) // 4), -(-int(mbw) // 8)
    return gy, gc, 2 * int(mbh) * gy, int(mbh) * gc


def _activity_parts(buf, lay):
    """(cells [mbh, mbw] of ACTIVITY_CELL, summary [8] uint32): copies of the specified parts of a record buffer"""
    cells = buf[:8 * lay.mbs].view(ACTIVITY_CELL).reshape(lay.mb_height, lay.mb_width).copy()
    return cells, buf[lay.summary_offset:lay.summary_offset + 32].view(np.uint32).copy()


def _activity_arrays(grp_off, entries, qscale):
    return (None if grp_off is None else np.ascontiguousarray(grp_off, dtype=np.uint32), None if entries is None else np.ascontiguousarray(entries, dtype=np.uint32),
            None if qscale is None else np.ascontiguousarray(qscale, dtype=np.uint8))


def activity_record(mbw, mbh, grp_off, entries, qscale, n_entries=None, fill=None, record=True):
    """leon_pipeline_activity_record: the library's CPU evaluation of a picture's activity record from its group lists (as
    leon_vlc_ctypes.Stream gives them) and its qscale map -> (cells [mbh, mbw] of ACTIVITY_CELL, summary [8] uint32).  n_entries: the
    count handed to the library when it is to differ from len(entries).  fill: the byte the record buffer holds beforehand -- the call
    then returns (cells, summary, buffer), the whole record_bytes buffer as the library left it.  record=False: a null record."""
    lay = activity_layout(mbw, mbh) if 1 <= int(mbw) <= 256 and 1 <= int(mbh) <= 256 else None
    buf = np.full(lay.record_bytes if lay else 64, 0 if fill is None else int(fill), dtype=np.uint8)
    keep = _activity_arrays(grp_off, entries, qscale)
    n = (0 if keep[1] is None else keep[1].size) if n_entries is None else int(n_entries)
    try:
        _chk(load().leon_pipeline_activity_record(int(mbw), int(mbh), None if keep[0] is None else keep[0].ctypes.data, None if keep[1] is None or not keep[1].size else keep[1].ctypes.data,
                                                  n, None if keep[2] is None else keep[2].ctypes.data, buf.ctypes.data if record else None))
    except LeonError as e:
        e.buffer = buf          # (a refusal leaves it as it was: tests look)
        raise
    parts = _activity_parts(buf, lay)
    return parts if fill is None else parts + (buf,)


def activity_from_lists(mbw, mbh, grp_off, entries, qscale):
    """The definition of a frame's activity record (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_ACTIVITY) in numpy, written from the
    header's text and independent of the C code: a picture's group lists and qscale map -> (cells [mbh, mbw] of ACTIVITY_CELL, summary [8]
    uint32).  grp_off is non-decreasing; only the groups of Y, Cb and Cr are read."""
    mbw, mbh = int(mbw), int(mbh)
    mbs = mbw * mbh
    gy, gc, n_y, n_c = activity_groups(mbw, mbh)
    n = n_y + 2 * n_c
    off = np.asarray(grp_off).reshape(-1)[:n + 1].astype(np.int64)
    e = np.asarray(entries, dtype=np.uint32).reshape(-1)[off[0]:off[n]].astype(np.int64)
    gid = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    a = np.abs((e & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64))
    b, dc = (e >> 20) & 7, (((e >> 23) & 7) == 0) & (((e >> 17) & 7) == 0)
    luma, cr = gid < n_y, gid >= n_y + n_c
    q = np.where(luma, gid, gid - n_y - np.where(cr, n_c, 0))
    R, g = q // np.where(luma, gy, gc), q % np.where(luma, gy, gc)
    mx = np.where(luma, 4 * g + (b >> 1), 8 * g + b)
    my = np.where(luma, R >> 1, R)
    j = np.where(luma, 2 * (R & 1) + (b & 1), 4 + cr)
    keep = (a != 0) & (mx < mbw)
    k = (my * mbw + mx)[keep]
    a, dc, j = a[keep], dc[keep], j[keep]
    # exact: ac_count, ac_mag, dc_mag (a float64 sum of integers is exact below 2^53)
    sums = np.stack([np.bincount(k[~dc], minlength=mbs), np.bincount(k[~dc], weights=a[~dc], minlength=mbs).astype(np.int64),
                     np.bincount(k[dc], weights=a[dc], minlength=mbs).astype(np.int64)])
    blocks = sum((np.bincount(k[j == i], minlength=mbs) > 0).astype(np.int64) << i for i in range(6))
    sat = np.minimum(sums, 65535)
    cells = np.zeros(mbs, dtype=ACTIVITY_CELL)
    cells["ac_count"], cells["ac_mag"], cells["dc_mag"], cells["blocks"] = sat[0], sat[1], sat[2], blocks
    cells["qscale"] = np.where(blocks != 0, np.asarray(qscale, dtype=np.uint8).reshape(-1)[:mbs], 0)
    pop = sum((blocks >> i) & 1 for i in range(6))
    summary = np.array([int((blocks != 0).sum()), int(sat[0].sum()), int(sat[1].sum()), int(sat[2].sum()), int(sat[1].max()), int(cells["qscale"].astype(np.int64).sum()),
                        int(pop.sum()), 0], dtype=np.uint32)
    return cells.reshape(mbh, mbw), summary


def activity_kernel(mbw, mbh, pictures, frames, ring_frames=None, pad_byte=0, fill=0xA5, ring=None, device_id=0, n_pictures=None, n_frames=None):
    """leon_pipeline_activity_kernel: k_activity and k_activity_summary on lists the caller supplies.  pictures = [(grp_off, entries, qscale)
    or (grp_off, entries, qscale, n_entries), ...] (n_entries: the capacity handed over, len(entries) by default); frames, the ring and
    the rest as motion_kernel's.  Returns the ring, uint8 [ring_frames, record_pitch], as it came back."""
    def one(q, pic):
        arrs = _activity_arrays(*pic[:3])
        q.grp_off, q.entries, q.qscale = [None if a is None or not a.size else a.ctypes.data for a in arrs]
        q.n_entries = int(pic[3]) if len(pic) > 3 else (0 if arrs[1] is None else arrs[1].size)
        return arrs
    return _record_kernel("leon_pipeline_activity_kernel", activity_layout, PipelineActivityPicture, one, mbw, mbh, pictures, frames, ring_frames, pad_byte, fill, ring,
                          device_id, n_pictures, n_frames)


def residual_layout(cw, ch):
    """leon_pipeline_residual_layout: where the planes of a residual record of a coded picture of cw x ch lie (PipelineResidualLayout), no device"""
    out = PipelineResidualLayout()
    _chk(load().leon_pipeline_residual_layout(int(cw), int(ch), C.byref(out)))
    return out


def residual_planes(buf, lay, pads=False):
    """a record buffer (uint8, at least record_bytes) -> (y [ch, cw], cb, cr [ch / 2, cw / 2]) int16, copies of the specified elements;
    pads=True: the whole rows instead, pad columns included ([ch, luma_stride], [ch / 2, chroma_stride] twice)"""
    cw, ch, ls, cs = lay.coded_width, lay.coded_height, lay.luma_stride, lay.chroma_stride
    y = buf[:2 * ls * ch].view("<i2").reshape(ch, ls)
    cb = buf[lay.cb_offset:lay.cb_offset + 2 * cs * (ch // 2)].view("<i2").reshape(ch // 2, cs)
    cr = buf[lay.cr_offset:lay.cr_offset + 2 * cs * (ch // 2)].view("<i2").reshape(ch // 2, cs)
    if pads:
        return y.copy(), cb.copy(), cr.copy()
    return y[:, :cw].copy(), cb[:, :cw // 2].copy(), cr[:, :cw // 2].copy()


def residual_kernel(cw, ch, pictures, frames, ring_frames=None, pad_byte=0, fill=0xA5, ring=None, device_id=0, n_pictures=None, n_frames=None):
    """leon_pipeline_residual_kernel: k_residual on lists, maps and matrices the caller supplies.  pictures = [(grp_off, entries, qscale, intra,
    matrices [128], premultiplier [64]) or the same with n_entries behind them, ...] (n_entries: the capacity handed over, len(entries) by
    default); frames, the ring and the rest as activity_kernel's.  Returns the ring, uint8 [ring_frames, record_pitch], as it came back
    (residual_planes takes a record of it apart)."""
    def one(q, pic):
        arrs = _activity_arrays(*pic[:3]) + tuple(None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in pic[3:6])
        q.grp_off, q.entries, q.qscale, q.intra, q.matrices, q.premultiplier = [None if a is None or not a.size else a.ctypes.data for a in arrs]
        q.n_entries = int(pic[6]) if len(pic) > 6 else (0 if arrs[1] is None else arrs[1].size)
        return arrs
    return _record_kernel("leon_pipeline_residual_kernel", residual_layout, PipelineResidualPicture, one, cw, ch, pictures, frames, ring_frames, pad_byte, fill, ring,
                          device_id, n_pictures, n_frames)


def _floor_div(a, b):
    return a // b          # Python's integer division floors, also for negatives


def carry_box(frame_width, frame_height, n_frames, fwd, bwd, records, rec):
    """The definition of one hop of leon_pipeline_carry_regions (include/leon_pipeline.h) in Python integers, written from the header's
    text and independent of the C code.  fwd, bwd: what carry_refs gives; records[i] = (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8) of
    window frame i (as read_motion gives them; None where no record is at hand); rec = the 8 words (frame, x, y, w, h, target, 0, 0).
    Returns (status, out, votes): out the 8 words of the moved region and votes [A, I, dh, dv] as lists of Python integers, both None
    where status is not 0."""
    S, x, y, w, h, T, r0, r1 = [int(v) for v in rec]
    fw, fh, n = int(frame_width), int(frame_height), int(n_frames)
    if r0 or r1:
        return REGION_RESERVED, None, None
    if not (0 <= S < n and 0 <= T < n):
        return REGION_FRAME, None, None
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > fw or y + h > fh:
        return REGION_BOX, None, None
    if S == T:
        return REGION_OK, [T, x, y, w, h, 0, 0, 0], [0, 0, 0, 0]
    D = (1 if int(fwd[T]) == S else 0) | (2 if int(bwd[T]) == S else 0)
    M, sense = T, -1
    if not D:
        D = (1 if int(fwd[S]) == T else 0) | (2 if int(bwd[S]) == T else 0)
        M, sense = S, 1
    if not D:
        return REGION_NO_REFERENCE, None, None
    mv, info = records[M][0], records[M][1]
    A = I = SH = SV = 0
    for j in range(y >> 4, ((y + h - 1) >> 4) + 1):
        for i in range(x >> 4, ((x + w - 1) >> 4) + 1):
            a = (min(x + w, 16 * i + 16) - max(x, 16 * i)) * (min(y + h, 16 * j + 16) - max(y, 16 * j))
            f = int(info[j][i])
            for b, k in ((1, 0), (2, 2)):
                if D & b and f & b:
                    A += a
                    SH += a * int(mv[j][i][k])
                    SV += a * int(mv[j][i][k + 1])
            if f & 4:
                I += a
    dh = _floor_div(sense * SH + A, 2 * A) if A else 0
    dv = _floor_div(sense * SV + A, 2 * A) if A else 0
    return REGION_OK, [T, min(max(x + dh, 0), fw - w), min(max(y + dv, 0), fh - h), w, h, 0, 0, 0], [A, I, dh, dv]


def carry_refs(frames, motion):
    """leon_pipeline_carry_refs: (fwd, bwd), int32 arrays -- for each frame of a window the index of the window frame its forward and its
    backward vectors point into, -1: none.  frames: [(gop, display_index), ...] (or dicts with those keys); motion: [(fwd_gop,
    fwd_display, bwd_display), ...] (or the frames' "motion" dicts).  No device."""
    n = len(frames)
    fa, ma = (PipelineFrame * max(1, n))(), (PipelineMotionFrame * max(1, n))()
    for i, (f, m) in enumerate(zip(frames, motion)):
        fa[i].gop, fa[i].display_index = (f["gop"], f["display_index"]) if isinstance(f, dict) else (f[0], f[1])
        ma[i].fwd_gop, ma[i].fwd_display, ma[i].bwd_display = (m["fwd_gop"], m["fwd_display"], m["bwd_display"]) if isinstance(m, dict) else m
    fwd, bwd = np.full(max(1, n), -2, dtype=np.int32), np.full(max(1, n), -2, dtype=np.int32)
    _chk(load().leon_pipeline_carry_refs(fa, ma, n, fwd.ctypes.data, bwd.ctypes.data))
    return fwd[:n], bwd[:n]


def _carry_records(records, mbw, mbh):
    """(pointer array, the buffers it points into) of records[i] = (mv, info) or None, each laid out as motion_layout says"""
    lay = motion_layout(mbw, mbh)
    ptrs, keep = (C.c_void_p * max(1, len(records)))(), []
    for i, r in enumerate(records):
        if r is None:
            continue
        buf = np.zeros(lay.record_bytes, dtype=np.uint8)
        buf[:8 * lay.mbs] = np.ascontiguousarray(r[0], dtype=np.int16).reshape(-1).view(np.uint8)
        buf[lay.info_offset:lay.info_offset + lay.mbs] = np.ascontiguousarray(r[1], dtype=np.uint8).reshape(-1)
        keep.append(buf)
        ptrs[i] = buf.ctypes.data
    return ptrs, keep


def _records_array(rows, words=8):
    """[n, words] int32 of a list of records that may leave their last (reserved) words out, or of an integer array: carry regions
    (frame, x, y, w, h, target[, r0, r1]), propagate hops (target, dst_slot, fwd_slot, bwd_slot[, four reserved words])"""
    a = np.asarray(rows, dtype=np.int64).reshape(len(rows), -1) if len(rows) else np.zeros((0, words), dtype=np.int64)
    full = np.zeros((len(a), words), dtype=np.int32)
    full[:, :a.shape[1]] = a
    return full


def _result_arrays(n, *specs):
    """the host arrays a call writes its n results into, one per (row shape, fill, dtype): pre-filled, of one row at the least (an address); sliced to n by the caller"""
    return [np.full((max(1, n),) + tuple(row), fill, dtype=dtype) for row, fill, dtype in specs]


def _device_records_check(name, t, stacked=False):
    """records (or hops) of a device road: a contiguous CUDA int32 torch tensor [N, 8] -- stacked: or [F, N, 8]"""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() in (2, 2 + stacked) and t.shape[-1] == 8 and t.is_contiguous()):
        raise ValueError("%s: a contiguous CUDA int32 tensor [N, 8]%s" % (name, " or [F, N, 8]" if stacked else ""))


def carry_record(frame_width, frame_height, mbw, mbh, n_frames, fwd, bwd, records, rec, fill=0):
    """leon_pipeline_carry_record: the library's CPU evaluation of one hop; arguments as carry_box's.  Returns (status, out [8], votes [4])
    as int32 arrays that hold `fill` where the library wrote nothing; LeonError where it refuses the call."""
    ptrs, keep = _carry_records(records, mbw, mbh)
    f, b = np.ascontiguousarray(fwd, dtype=np.int32), np.ascontiguousarray(bwd, dtype=np.int32)
    r = _records_array([rec])
    out, votes = np.full(8, fill, dtype=np.int32), np.full(4, fill, dtype=np.int32)
    st = load().leon_pipeline_carry_record(int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), f.ctypes.data, b.ctypes.data, ptrs, r.ctypes.data,
                                           out.ctypes.data, votes.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, out, votes


def carry_device(frame_width, frame_height, mbw, mbh, n_frames, fwd, bwd, records, regions, device_id=0, fill=-1, n=None):
    """leon_pipeline_carry_device: k_carry on motion records the caller supplies (as carry_box's), regions = [(frame, x, y, w, h,
    target), ...] -> (out [m, 8], votes [m, 4], status [m]) int32 arrays pre-filled with `fill`: a refused record keeps it in out and
    votes.  n: the count handed to the library when it is to differ from m = len(regions) (smaller: what lies behind keeps the fill)."""
    ptrs, keep = _carry_records(records, mbw, mbh)
    f, b = np.ascontiguousarray(fwd, dtype=np.int32), np.ascontiguousarray(bwd, dtype=np.int32)
    r = _records_array(regions)
    out, votes, status = _result_arrays(len(r), ((8,), fill, np.int32), ((4,), fill, np.int32), ((), fill, np.int32))
    _chk(load().leon_pipeline_carry_device(int(device_id), int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), f.ctypes.data, b.ctypes.data, ptrs,
                                           r.ctypes.data if len(r) else None, len(r) if n is None else int(n), out.ctypes.data, votes.ctypes.data, status.ctypes.data))
    return out[:len(r)], votes[:len(r)], status[:len(r)]


def gauge_box(frame_width, frame_height, n_frames, motion, activity, rec, sources=GAUGE_MOTION | GAUGE_ACTIVITY):
    """The definition of one record of leon_pipeline_gauge_regions (include/leon_pipeline.h) in Python integers, written from the
    header's text and independent of the C code.  motion[i] = (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8) and activity[i] = cells
    [mbh, mbw] of ACTIVITY_CELL of window frame i (as read_motion and read_activity give them; a list the sources do not ask for may be
    None); rec = the 8 words (frame, x, y, w, h, 0, 0, 0).  Returns (status, stats): the 16 words as a list of Python integers, None
    where status is not 0."""
    f, x, y, w, h, r0, r1, r2 = [int(v) for v in rec]
    fw, fh, n, sources = int(frame_width), int(frame_height), int(n_frames), int(sources)
    if r0 or r1 or r2:
        return REGION_RESERVED, None
    if not 0 <= f < n:
        return REGION_FRAME, None
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > fw or y + h > fh:
        return REGION_BOX, None
    s = [0] * GAUGE_WORDS
    for j in range(y >> 4, ((y + h - 1) >> 4) + 1):
        for i in range(x >> 4, ((x + w - 1) >> 4) + 1):
            a = (min(x + w, 16 * i + 16) - max(x, 16 * i)) * (min(y + h, 16 * j + 16) - max(y, 16 * j))
            s[0] += a
            if sources & GAUGE_ACTIVITY:
                cell = activity[f][j][i]
                blocks, ac_mag = int(cell["blocks"]), int(cell["ac_mag"])
                s[1] += a if blocks else 0
                s[2] += a * int(cell["ac_count"])
                s[3] += a * ac_mag
                s[4] += a * int(cell["dc_mag"])
                s[5] += a * int(cell["qscale"])
                s[6] += a * bin(blocks).count("1")
                s[7] = max(s[7], ac_mag)
            if sources & GAUGE_MOTION:
                mv, info = [int(v) for v in motion[f][0][j][i]], int(motion[f][1][j][i])
                s[8] += a if info & 1 else 0
                s[9] += a if info & 2 else 0
                s[10] += a if info & 4 else 0
                s[11] += a if any(mv) else 0
                for k in range(4):
                    s[12 + k] += a * abs(mv[k])
    return REGION_OK, s


def _gauge_records(motion, activity, mbw, mbh, n_frames):
    """(motion pointer array or None, activity pointer array or None, the buffers they point into): motion[i] = (mv, info) or None laid
    out as motion_layout says, activity[i] = cells or None as activity_layout says, each buffer exactly record_bytes long"""
    keep = []
    mp = None
    if motion is not None:
        mp, k = _carry_records(list(motion) + [None] * (int(n_frames) - len(motion)), mbw, mbh)
        keep += k
    ap = None
    if activity is not None:
        lay = activity_layout(mbw, mbh)
        ap = (C.c_void_p * max(1, int(n_frames), len(activity)))()
        for i, cells in enumerate(activity):
            if cells is None:
                continue
            buf = np.zeros(lay.record_bytes, dtype=np.uint8)
            buf[:8 * lay.mbs] = np.ascontiguousarray(cells, dtype=ACTIVITY_CELL).reshape(-1).view(np.uint8)
            keep.append(buf)
            ap[i] = buf.ctypes.data
    return mp, ap, keep


def gauge_record(frame_width, frame_height, mbw, mbh, n_frames, motion, activity, rec, sources=GAUGE_MOTION | GAUGE_ACTIVITY, fill=0, cfg=None):
    """leon_pipeline_gauge_record: the library's CPU evaluation of one record; arguments as gauge_box's.  Returns (status, stats [16]
    int64) with `fill` where the library wrote nothing; LeonError where it refuses the call.  cfg: a PipelineGaugeConfig in place of
    sources."""
    mp, ap, keep = _gauge_records(motion, activity, mbw, mbh, n_frames)
    r = _records_array([rec])
    stats = np.full(GAUGE_WORDS, fill, dtype=np.int64)
    cfg = PipelineGaugeConfig(int(sources)) if cfg is None else cfg
    st = load().leon_pipeline_gauge_record(int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), mp, ap, C.byref(cfg), r.ctypes.data, stats.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, stats


def gauge_kernel(frame_width, frame_height, mbw, mbh, n_frames, motion, activity, regions, sources=GAUGE_MOTION | GAUGE_ACTIVITY, device_id=0, fill=-1, n=None,
                 cfg=None):
    """leon_pipeline_gauge_kernel: k_gauge on records the caller supplies (as gauge_box's), regions = [(frame, x, y, w, h), ...] ->
    (stats [m, 16] int64, status [m] int32) pre-filled with `fill`: a refused record keeps it in its statistics.  n: the count handed
    to the library when it is to differ from m = len(regions) (smaller: what lies behind keeps the fill)."""
    mp, ap, keep = _gauge_records(motion, activity, mbw, mbh, n_frames)
    r = _records_array(regions)
    stats, status = _result_arrays(len(r), ((GAUGE_WORDS,), fill, np.int64), ((), fill, np.int32))
    cfg = PipelineGaugeConfig(int(sources)) if cfg is None else cfg
    _chk(load().leon_pipeline_gauge_kernel(int(device_id), int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), mp, ap, C.byref(cfg),
                                           r.ctypes.data if len(r) else None, len(r) if n is None else int(n), stats.ctypes.data, status.ctypes.data))
    return stats[:len(r)], status[:len(r)]


def _propose_config(sources, max_boxes, mv_min, ac_min, intra, connectivity, min_cells):
    """the config of a propose call; sources None: the sources a threshold is given for.  A threshold that is None goes down as 0."""
    if sources is None:
        sources = (PROPOSE_MOTION if mv_min is not None else 0) | (PROPOSE_ACTIVITY if ac_min is not None else 0)
    return PipelineProposeConfig(int(sources), PROPOSE_INTRA if intra else 0, int(mv_min or 0), int(ac_min or 0), int(connectivity), int(min_cells), int(max_boxes), 0)


def propose_boxes(frame_width, frame_height, n_frames, motion, activity, frame, max_boxes=16, mv_min=None, ac_min=None, intra=False, connectivity=8, min_cells=1,
                  sources=None):
    """The definition of one request of leon_pipeline_propose_regions (include/leon_pipeline.h), written from the header's text and
    independent of the C code: thresholds on the arrays, then a breadth-first fill in Python integers.  motion[i] = (mv [mbh, mbw, 4]
    int16, info [mbh, mbw] uint8) and activity[i] = cells [mbh, mbw] of ACTIVITY_CELL of window frame i (as read_motion and
    read_activity give them; a list the sources do not ask for may be None).  sources None: the sources a threshold is given for.
    Returns (status, regions, info, count): K rows of 8 words, K rows of [cells, first] (lists of Python integers) and the number of
    selected components, not capped; (REGION_FRAME, None, None, None) for a frame outside the window."""
    fw, fh, f, K = int(frame_width), int(frame_height), int(frame), int(max_boxes)
    if sources is None:
        sources = (PROPOSE_MOTION if mv_min is not None else 0) | (PROPOSE_ACTIVITY if ac_min is not None else 0)
    if not 0 <= f < int(n_frames):
        return REGION_FRAME, None, None, None
    hot = None
    if sources & PROPOSE_MOTION:
        mv, info = np.asarray(motion[f][0]).astype(np.int64), np.asarray(motion[f][1])
        hot = np.abs(mv).max(axis=2) >= int(mv_min)
        if intra:
            hot |= (info & 4) != 0
    if sources & PROPOSE_ACTIVITY:
        a = np.asarray(activity[f])["ac_mag"].astype(np.int64) >= int(ac_min)
        hot = a if hot is None else hot | a
    mbh, mbw = hot.shape
    hot = hot & (16 * np.arange(mbw)[None, :] < fw) & (16 * np.arange(mbh)[:, None] < fh)
    todo = [[bool(v) for v in row] for row in hot]
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (1, -1), (-1, 1), (1, 1)] if int(connectivity) == 8 else [])
    regions, infos, count = [], [], 0
    for j0 in range(mbh):
        for i in range(mbw):
            if not todo[j0][i]:
                continue
            todo[j0][i] = False
            queue, at, lo, hi, j1 = [(i, j0)], 0, i, i, j0
            while at < len(queue):
                ci, cj = queue[at]
                at += 1
                lo, hi, j1 = min(lo, ci), max(hi, ci), max(j1, cj)
                for di, dj in steps:
                    ni, nj = ci + di, cj + dj
                    if 0 <= ni < mbw and 0 <= nj < mbh and todo[nj][ni]:
                        todo[nj][ni] = False
                        queue.append((ni, nj))
            if len(queue) < int(min_cells):
                continue
            if count < K:
                x, y = 16 * lo, 16 * j0
                regions.append([f, x, y, min(16 * (hi + 1), fw) - x, min(16 * (j1 + 1), fh) - y, 0, 0, 0])
                infos.append([len(queue), j0 * mbw + i])
            count += 1
    while len(regions) < K:
        regions.append([f, 0, 0, 0, 0, 0, 0, 0])
        infos.append([0, -1])
    return REGION_OK, regions, infos, count


def propose_record(frame_width, frame_height, mbw, mbh, n_frames, motion, activity, frame, max_boxes=16, mv_min=None, ac_min=None, intra=False, connectivity=8,
                   min_cells=1, sources=None, fill=-1, cfg=None):
    """leon_pipeline_propose_record: the library's CPU evaluation of one request; arguments as propose_boxes's.  Returns (status,
    regions [K, 8] int32, info [K, 2] int32, count) with `fill` where the library wrote nothing; LeonError where it refuses the call.
    cfg: a PipelineProposeConfig in place of the keywords."""
    mp, ap, keep = _gauge_records(motion, activity, mbw, mbh, n_frames)
    cfg = _propose_config(sources, max_boxes, mv_min, ac_min, intra, connectivity, min_cells) if cfg is None else cfg
    K = max(1, min(int(cfg.max_boxes), PROPOSE_MAX_BOXES))
    regions, info, count = np.full((K, 8), fill, dtype=np.int32), np.full((K, 2), fill, dtype=np.int32), np.full(1, fill, dtype=np.int32)
    st = load().leon_pipeline_propose_record(int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), mp, ap, C.byref(cfg), int(frame), regions.ctypes.data,
                                             info.ctypes.data, count.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, regions, info, int(count[0])


def propose_kernel(frame_width, frame_height, mbw, mbh, n_frames, motion, activity, frames, max_boxes=16, mv_min=None, ac_min=None, intra=False, connectivity=8,
                   min_cells=1, sources=None, device_id=0, fill=-1, n=None, cfg=None, with_info=True, with_status=True):
    """leon_pipeline_propose_kernel: k_propose on records the caller supplies (as propose_boxes's), frames = the requests -> (regions
    [m, K, 8], info [m, K, 2], count [m], status [m]) int32, pre-filled with `fill`: a refused request keeps it in its rows and its
    count.  n: the count handed to the library when it is to differ from m = len(frames) (smaller: what lies behind keeps the fill);
    with_info / with_status False: NULL goes down in their place and they come back as the fill."""
    mp, ap, keep = _gauge_records(motion, activity, mbw, mbh, n_frames)
    cfg = _propose_config(sources, max_boxes, mv_min, ac_min, intra, connectivity, min_cells) if cfg is None else cfg
    K = max(1, min(int(cfg.max_boxes), PROPOSE_MAX_BOXES))
    fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
    m = max(1, len(fr))
    regions, info = np.full((m, K, 8), fill, dtype=np.int32), np.full((m, K, 2), fill, dtype=np.int32)
    count, status = np.full(m, fill, dtype=np.int32), np.full(m, fill, dtype=np.int32)
    _chk(load().leon_pipeline_propose_kernel(int(device_id), int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), mp, ap, C.byref(cfg),
                                             fr.ctypes.data if len(fr) else None, len(fr) if n is None else int(n), regions.ctypes.data,
                                             info.ctypes.data if with_info else None, count.ctypes.data, status.ctypes.data if with_status else None))
    return regions[:len(fr)], info[:len(fr)], count[:len(fr)], status[:len(fr)]


def _overlap_config(threshold, measure, threshold_q16=None):
    """the config of a suppress or match call: measure "iou" / "iomin" (or the word itself), the threshold as a float converted with
    round(threshold * 65536) unless threshold_q16 gives the Q16 word"""
    m = {"iou": OVERLAP_IOU, "iomin": OVERLAP_IOMIN}.get(measure, measure)
    return PipelineOverlapConfig(int(m), int(round(float(threshold) * 65536)) if threshold_q16 is None else int(threshold_q16))


def _overlap_ok(row, fw, fh, n_frames):
    """the status word of a row, as the gauge family judges it"""
    f, x, y, w, h, r0, r1, r2 = (int(v) for v in row)
    if r0 or r1 or r2:
        return REGION_RESERVED
    if not 0 <= f < n_frames:
        return REGION_FRAME
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > fw or y + h > fh:
        return REGION_BOX
    return REGION_OK


def _overlap_pair(measure, a, b):
    """(inter, den) of two rows in Python integers"""
    iw = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    ih = min(a[2] + a[4], b[2] + b[4]) - max(a[2], b[2])
    inter = max(iw, 0) * max(ih, 0)
    return inter, (min(a[3] * a[4], b[3] * b[4]) if measure == OVERLAP_IOMIN else a[3] * a[4] + b[3] * b[4] - inter)


def suppress_boxes(frame_width, frame_height, n_frames, rows, scores=None, threshold_q16=32768, measure=OVERLAP_IOU):
    """The definition of one set of leon_pipeline_suppress_regions (include/leon_pipeline.h), written from the header's text in Python
    integers and independent of the C code: rows = K rows of 8 words, scores = K integers (None: all 0).  Returns (out, order, by,
    count, status): K rows of 8 words, K input indices (-1 behind count), K words of by (None for a refused row: not written), the
    kept rows' number and K status words."""
    rows = [[int(v) for v in r] for r in rows]
    K = len(rows)
    status = [_overlap_ok(r, int(frame_width), int(frame_height), int(n_frames)) for r in rows]
    walk = sorted((i for i in range(K) if status[i] == REGION_OK), key=lambda i: (-(int(scores[i]) if scores is not None else 0), i))
    by, kept = [None] * K, []
    for i in walk:
        by[i] = -1
        for k in kept:
            inter, den = _overlap_pair(measure, rows[k], rows[i])
            if inter * 65536 >= int(threshold_q16) * den:
                by[i] = k
                break
        if by[i] == -1:
            kept.append(i)
    out = [rows[i][:5] + [0, 0, 0] for i in kept] + [[0] * 8] * (K - len(kept))
    return out, kept + [-1] * (K - len(kept)), by, len(kept), status


def match_boxes(frame_width, frame_height, n_frames, a, b, threshold_q16=32768, measure=OVERLAP_IOU):
    """The definition of one pair of sets of leon_pipeline_match_regions in Python integers: a = Ka rows, b = Kb rows of 8 words.
    Returns (match_a, match_b, overlap, count, status_a, status_b); the words of a refused row are None (not written).  The candidates
    are sorted with exact fractions."""
    from fractions import Fraction
    a, b = [[int(v) for v in r] for r in a], [[int(v) for v in r] for r in b]
    sa = [_overlap_ok(r, int(frame_width), int(frame_height), int(n_frames)) for r in a]
    sb = [_overlap_ok(r, int(frame_width), int(frame_height), int(n_frames)) for r in b]
    match_a, overlap = [-1 if s == REGION_OK else None for s in sa], [0 if s == REGION_OK else None for s in sa]
    match_b = [-1 if s == REGION_OK else None for s in sb]
    okb = [j for j in range(len(b)) if sb[j] == REGION_OK]
    cand = []
    for i in range(len(a)):
        if sa[i] != REGION_OK:
            continue
        for j in okb:
            if a[i][1] + a[i][3] <= b[j][1] or b[j][1] + b[j][3] <= a[i][1]:          # no common column: inter 0 reaches no threshold
                continue
            inter, den = _overlap_pair(measure, a[i], b[j])
            if inter * 65536 >= int(threshold_q16) * den:
                cand.append((-Fraction(inter, den), i, j, inter * 65536 // den))
    cand.sort()
    count = 0
    for _, i, j, q in cand:
        if match_a[i] == -1 and match_b[j] == -1:
            match_a[i], match_b[j], overlap[i] = j, i, q
            count += 1
    return match_a, match_b, overlap, count, sa, sb


def _overlap_rows(rows, name):
    """rows [K, 8] or [n, K, 8] -> a contiguous int32 array [n, K, 8]"""
    r = np.ascontiguousarray(rows, dtype=np.int32)
    if r.ndim == 2:
        r = r[None]
    if r.ndim != 3 or r.shape[2] != 8:
        raise ValueError("%s: [K, 8] or [n, K, 8] words" % name)
    return r


def _suppress_arrays(rows, scores, score_stride, fill):
    r = _overlap_rows(rows, "regions")
    n, K = r.shape[0], r.shape[1]
    sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.int32).reshape(-1)
    if sc is not None and sc.size < (n * K - 1) * int(score_stride) + 1 and 1 <= int(score_stride) <= 8:
        raise ValueError("scores: at least %d words" % ((n * K - 1) * int(score_stride) + 1))
    if sc is not None and sc.size < n * K * max(1, int(score_stride)):         # the library reads whole strides
        sc = np.concatenate([sc, np.zeros(n * K * max(1, int(score_stride)) - sc.size, dtype=np.int32)])
    m, Kc = max(1, n), max(1, K)
    outs = (np.full((m, Kc, 8), fill, dtype=np.int32), np.full((m, Kc), fill, dtype=np.int32), np.full((m, Kc), fill, dtype=np.int32), np.full(m, fill, dtype=np.int32),
            np.full((m, Kc), fill, dtype=np.int32))
    return r, n, K, sc, outs


def suppress_record(frame_width, frame_height, n_frames, rows, scores=None, threshold=0.5, measure="iou", score_stride=1, threshold_q16=None, fill=-1, cfg=None, k=None,
                    with_out=True, with_order=True, with_status=True):
    """leon_pipeline_suppress_record: the library's CPU evaluation of one set; rows [K, 8].  Returns (out [K, 8], order [K], by [K],
    count, status [K]) int32 with `fill` where the library wrote nothing; LeonError where it refuses the call.  cfg: a
    PipelineOverlapConfig in place of the keywords; k: the count handed down when it is to differ from len(rows)."""
    r, n, K, sc, (out, order, by, count, status) = _suppress_arrays(rows, scores, score_stride, fill)
    cfg = _overlap_config(threshold, measure, threshold_q16) if cfg is None else cfg
    st = load().leon_pipeline_suppress_record(int(frame_width), int(frame_height), int(n_frames), C.byref(cfg), r.ctypes.data if r.size else None, K if k is None else int(k),
                                              None if sc is None else sc.ctypes.data, int(score_stride), out.ctypes.data if with_out else None,
                                              order.ctypes.data if with_order else None, by.ctypes.data, count.ctypes.data, status.ctypes.data if with_status else None)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return out[0], order[0], by[0], int(count[0]), status[0]


def suppress_kernel(frame_width, frame_height, n_frames, rows, scores=None, threshold=0.5, measure="iou", score_stride=1, threshold_q16=None, device_id=0, fill=-1, n=None,
                    cfg=None, with_out=True, with_order=True, with_status=True):
    """leon_pipeline_suppress_kernel: k_suppress on rows the caller supplies, [n, K, 8] (or [K, 8]) -> (out [n, K, 8], order [n, K],
    by [n, K], count [n], status [n, K]) int32, pre-filled with `fill`.  n: the set count handed to the library when it is to differ
    (smaller: what lies behind keeps the fill); with_* False: NULL goes down in its place and it comes back as the fill."""
    r, sets, K, sc, (out, order, by, count, status) = _suppress_arrays(rows, scores, score_stride, fill)
    cfg = _overlap_config(threshold, measure, threshold_q16) if cfg is None else cfg
    _chk(load().leon_pipeline_suppress_kernel(int(device_id), int(frame_width), int(frame_height), int(n_frames), C.byref(cfg), r.ctypes.data if r.size else None,
                                              sets if n is None else int(n), K, None if sc is None else sc.ctypes.data, int(score_stride),
                                              out.ctypes.data if with_out else None, order.ctypes.data if with_order else None, by.ctypes.data, count.ctypes.data,
                                              status.ctypes.data if with_status else None))
    return out, order, by, count, status


def _match_arrays(a, b, fill):
    ra, rb = _overlap_rows(a, "a"), _overlap_rows(b, "b")
    if ra.shape[0] != rb.shape[0]:
        raise ValueError("a and b: as many sets")
    n, Ka, Kb = ra.shape[0], ra.shape[1], rb.shape[1]
    m, A, B = max(1, n), max(1, Ka), max(1, Kb)
    outs = (np.full((m, A), fill, dtype=np.int32), np.full((m, B), fill, dtype=np.int32), np.full((m, A), fill, dtype=np.int32), np.full(m, fill, dtype=np.int32),
            np.full((m, A), fill, dtype=np.int32), np.full((m, B), fill, dtype=np.int32))
    return ra, rb, n, Ka, Kb, outs


def match_record(frame_width, frame_height, n_frames, a, b, threshold=0.5, measure="iou", threshold_q16=None, fill=-1, cfg=None, ka=None, kb=None, with_status=True):
    """leon_pipeline_match_record: the library's CPU evaluation of one pair of sets, a [Ka, 8] and b [Kb, 8].  Returns (match_a [Ka],
    match_b [Kb], overlap [Ka], count, status_a [Ka], status_b [Kb]) int32 with `fill` where the library wrote nothing."""
    ra, rb, n, Ka, Kb, (ma, mb, ov, count, sa, sb) = _match_arrays(a, b, fill)
    cfg = _overlap_config(threshold, measure, threshold_q16) if cfg is None else cfg
    st = load().leon_pipeline_match_record(int(frame_width), int(frame_height), int(n_frames), C.byref(cfg), ra.ctypes.data if ra.size else None, Ka if ka is None else int(ka),
                                           rb.ctypes.data if rb.size else None, Kb if kb is None else int(kb), ma.ctypes.data, mb.ctypes.data, ov.ctypes.data,
                                           count.ctypes.data, sa.ctypes.data if with_status else None, sb.ctypes.data if with_status else None)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return ma[0], mb[0], ov[0], int(count[0]), sa[0], sb[0]


def match_kernel(frame_width, frame_height, n_frames, a, b, threshold=0.5, measure="iou", threshold_q16=None, device_id=0, fill=-1, n=None, cfg=None, with_status_a=True,
                 with_status_b=True):
    """leon_pipeline_match_kernel: k_match on rows the caller supplies, a [n, Ka, 8] and b [n, Kb, 8] -> (match_a [n, Ka], match_b
    [n, Kb], overlap [n, Ka], count [n], status_a [n, Ka], status_b [n, Kb]) int32, pre-filled with `fill`; n and with_* as
    suppress_kernel's."""
    ra, rb, sets, Ka, Kb, (ma, mb, ov, count, sa, sb) = _match_arrays(a, b, fill)
    cfg = _overlap_config(threshold, measure, threshold_q16) if cfg is None else cfg
    _chk(load().leon_pipeline_match_kernel(int(device_id), int(frame_width), int(frame_height), int(n_frames), C.byref(cfg), ra.ctypes.data if ra.size else None, Ka,
                                           rb.ctypes.data if rb.size else None, Kb, sets if n is None else int(n), ma.ctypes.data, mb.ctypes.data, ov.ctypes.data,
                                           count.ctypes.data, sa.ctypes.data if with_status_a else None, sb.ctypes.data if with_status_b else None))
    return ma, mb, ov, count, sa, sb


def carry_plan(refs, frames, src):
    """The hops that carry boxes from window frame `src` to every delivered frame of its GOP in the window: (levels, unreachable) --
    levels = [[(from_index, to_index), ...], ...], every level's sources are `src` or targets of an earlier level; unreachable = the
    frames of the GOP no chain of predictions inside the window reaches.  refs = (fwd, bwd) of carry_refs; frames = the window's frames
    as dicts (or (gop, display_index, type) tuples).  Anchors (I and P pictures) go along the forward chain in both senses, level by
    level; then every B picture goes from the nearer of its carried references (display distance; a tie: the forward one).  Host only."""
    fwd, bwd = [int(v) for v in refs[0]], [int(v) for v in refs[1]]
    info = [(f["gop"], f["display_index"], f["type"]) if isinstance(f, dict) else (int(f[0]), int(f[1]), int(f[2])) for f in frames]
    src = int(src)
    group = [i for i in range(len(info)) if info[i][0] == info[src][0]]
    anchors = [i for i in group if info[i][2] != PIC_B]
    carried, levels, front = {src}, [], [src]
    while front:
        hops = []
        for u in front:
            near = [fwd[u]] + ([bwd[u]] if info[u][2] == PIC_B else []) + [a for a in anchors if fwd[a] == u]
            for a in near:
                if a in anchors and a not in carried:
                    carried.add(a)
                    hops.append((u, a))
        if hops:
            levels.append(hops)
        front = [a for _, a in hops]
    hops, unreachable = [], [a for a in anchors if a not in carried]
    for b in group:
        if info[b][2] != PIC_B or b in carried:
            continue
        cands = [r for r in dict.fromkeys((fwd[b], bwd[b])) if r in carried]
        if not cands:
            unreachable.append(b)
            continue
        hops.append((min(cands, key=lambda r: abs(info[r][1] - info[b][1])), b))
    if hops:
        levels.append(hops)
    return levels, sorted(unreachable)


def propagate_map(frame_width, frame_height, n_frames, records, hop, stride, maps, fill=0):
    """The definition of one hop of leon_pipeline_propagate_maps (include/leon_pipeline.h) in numpy integers, written from the header's
    text and independent of the C code.  records[i] = (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8) of window frame i (None where no
    record is at hand); hop = the 8 words (target, dst_slot, fwd_slot, bwd_slot, 0, 0, 0, 0) (or the first four); maps = an array
    [S, P, mh, mw] of a 1-, 2- or 4-byte dtype, WRITTEN IN PLACE (maps[dst_slot]) where the status is 0.  Returns (status, via): via
    [mh, mw] uint8, None where status is not 0."""
    hop = [int(v) for v in hop] + [0] * (8 - len(hop))
    T, dst, fs, bs = hop[:4]
    fw, fh, s = int(frame_width), int(frame_height), int(stride)
    S, P, mh, mw = maps.shape
    e = maps.dtype.itemsize
    if s not in (1, 2, 4, 8, 16) or e not in (1, 2, 4) or (mh, mw) != (-(-fh // s), -(-fw // s)):
        raise ValueError("propagate_map: stride %d, %d-byte elements, maps of %d x %d cells over a frame of %d x %d" % (s, e, mw, mh, fw, fh))
    if any(hop[4:]):
        return REGION_RESERVED, None
    if not 0 <= T < int(n_frames):
        return REGION_FRAME, None
    if not (0 <= dst < S and -1 <= fs < S and -1 <= bs < S) or dst == fs or dst == bs:
        return REGION_SLOT, None
    mv, info = np.asarray(records[T][0]).astype(np.int64), np.asarray(records[T][1]).astype(np.int64)
    cy, cx = np.mgrid[0:mh, 0:mw]
    kj, ki = (cy * s) >> 4, (cx * s) >> 4
    f, v = info[kj, ki], mv[kj, ki]
    use_f = ((f & 1) != 0) & (fs >= 0)
    use_b = ~use_f & ((f & 2) != 0) & (bs >= 0)
    dx = np.where(use_f, v[..., 0], v[..., 2]) + s
    dy = np.where(use_f, v[..., 1], v[..., 3]) + s
    sx = np.clip(cx + dx // (2 * s), 0, mw - 1)          # (numpy's integer division floors, also for negatives)
    sy = np.clip(cy + dy // (2 * s), 0, mh - 1)
    out = np.empty((P, mh, mw), dtype=maps.dtype)
    out[:] = np.array([int(fill) & 0xffffffff], dtype="<u4").view(np.uint8)[:e].view(maps.dtype)[0]
    if fs >= 0:
        out[:, use_f] = maps[fs][:, sy[use_f], sx[use_f]]
    if bs >= 0:
        out[:, use_b] = maps[bs][:, sy[use_b], sx[use_b]]
    maps[dst] = out
    return REGION_OK, (use_f * 1 + use_b * 2).astype(np.uint8)


def propagate_layout(frame_width, frame_height, stride, planes, elem_bytes):
    """leon_pipeline_propagate_layout: the sizes of a map over a frame (PipelinePropagateLayout: mw, mh, planes_per_group, fast_path,
    plane_bytes, slot_bytes), no device"""
    out = PipelinePropagateLayout()
    _chk(load().leon_pipeline_propagate_layout(int(frame_width), int(frame_height), int(stride), int(planes), int(elem_bytes), C.byref(out)))
    return out


def _propagate_config(maps, stride, fill, over=None):
    """PipelinePropagateConfig of a numpy array [S, P, mh, mw] whose slots may lie further apart than a map (strides[0]); `over`
    replaces fields (the refusals' tests)"""
    S, P, mh, mw = maps.shape
    e = maps.dtype.itemsize
    if maps.strides[1:] != (mh * mw * e, mw * e, e):
        raise ValueError("maps: the planes of a slot are contiguous")
    cfg = PipelinePropagateConfig(int(stride), P, e, S, int(fill) & 0xffffffff, 0, maps.strides[0], S * maps.strides[0])
    for k, v in (over or {}).items():
        setattr(cfg, k, v)
    return cfg


def _fill_element(fill, elem_bytes):
    """the fill word as an element of elem_bytes bytes, a signed integer: its low bytes (propagate_map states the same)"""
    return int(np.array([int(fill) & 0xffffffff], dtype="<u4").view(np.uint8)[:elem_bytes].view({1: np.uint8, 2: np.int16, 4: np.int32}[elem_bytes])[0])


def propagate_record(frame_width, frame_height, mbw, mbh, n_frames, records, hop, stride, maps, fill=0, via_fill=0, **over):
    """leon_pipeline_propagate_record: the library's CPU evaluation of one hop; arguments as propagate_map's, maps written in place.
    Returns (status, via [mh, mw] uint8 that holds `via_fill` where the library wrote nothing); LeonError where it refuses the call."""
    ptrs, keep = _carry_records(records, mbw, mbh)
    h = _records_array([hop])
    via = np.full(maps.shape[2:], via_fill, dtype=np.uint8)
    cfg = _propagate_config(maps, stride, fill, over)
    st = load().leon_pipeline_propagate_record(int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), ptrs, C.byref(cfg), h.ctypes.data, maps.ctypes.data,
                                               via.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, via


def propagate_kernel(frame_width, frame_height, mbw, mbh, n_frames, records, hops, stride, maps, fill=0, via=True, device_id=0, via_fill=0, status_fill=-1, n=None, **over):
    """leon_pipeline_propagate_kernel: k_propagate on motion records the caller supplies (as propagate_map's), hops = [(target,
    dst_slot, fwd_slot, bwd_slot), ...], maps [S, P, mh, mw] written in place -> (via [m, mh, mw] uint8 pre-filled with `via_fill`, or
    None with via=False, status [m] int32 pre-filled with `status_fill`).  n: the count handed to the library when it is to differ
    from m = len(hops)."""
    ptrs, keep = _carry_records(records, mbw, mbh)
    h = _records_array(hops)
    v, status = _result_arrays(len(h), (maps.shape[2:], via_fill, np.uint8), ((), status_fill, np.int32))
    cfg = _propagate_config(maps, stride, fill, over)
    _chk(load().leon_pipeline_propagate_kernel(int(device_id), int(frame_width), int(frame_height), int(mbw), int(mbh), int(n_frames), ptrs, C.byref(cfg),
                                               h.ctypes.data if len(h) else None, len(h) if n is None else int(n), maps.ctypes.data, v.ctypes.data if via else None,
                                               status.ctypes.data))
    return (v[:len(h)] if via else None), status[:len(h)]


def propagate_plan(refs, frames, src):
    """The hops that propagate a map from window frame `src` to every delivered frame of its GOP in the window that a chain of
    predictions reaches: (levels, unreachable) -- levels = [[(target, fwd_ref, bwd_ref), ...], ...] with window frame indices, -1
    for a reference that is not reachable; every level's references are `src` or targets of an earlier level.  First the set of
    reachable frames is closed (T is reachable when fwd[T] or bwd[T] is), then level(T) = 1 + max(level of its reachable
    references): a B picture waits for both anchors.  A hop is a gather through the TARGET's record, so nothing goes from a picture
    back to its reference: from a P picture the GOP's earlier anchors are out of reach.  refs = (fwd, bwd) of carry_refs; frames =
    the window's frames as dicts (or (gop, display_index, type) tuples).  Host only."""
    fwd, bwd = [int(v) for v in refs[0]], [int(v) for v in refs[1]]
    gops = [f["gop"] if isinstance(f, dict) else int(f[0]) for f in frames]
    src = int(src)
    group = [i for i in range(len(gops)) if gops[i] == gops[src]]
    level, grew = {src: 0}, True
    reach = {src}
    while grew:
        grew = False
        for t in group:
            if t not in reach and (fwd[t] in reach or bwd[t] in reach):
                reach.add(t)
                grew = True

    def level_of(t):
        if t not in level:
            level[t] = 1 + max(level_of(r) for r in (fwd[t], bwd[t]) if r in reach)
        return level[t]
    levels = {}
    for t in group:
        if t in reach and t != src:
            levels.setdefault(level_of(t), []).append((t, fwd[t] if fwd[t] in reach else -1, bwd[t] if bwd[t] in reach else -1))
    return [levels[k] for k in sorted(levels)], [t for t in group if t not in reach]


def accumulate_layout(cw, ch, parts=ACCUMULATE_MOTION | ACCUMULATE_RESIDUAL):
    """leon_pipeline_accumulate_layout: where the planes of an accumulator over a coded picture of cw x ch lie (PipelineAccumulateLayout), no device"""
    out = PipelineAccumulateLayout()
    _chk(load().leon_pipeline_accumulate_layout(int(cw), int(ch), int(parts), C.byref(out)))
    return out


def accumulate_names(parts):
    """the planes `parts` asks for, in their order in a slot"""
    return tuple(n for i, n in enumerate(ACCUMULATE_PLANES) if int(parts) & (ACCUMULATE_MOTION if i < 3 else ACCUMULATE_RESIDUAL))


def accumulate_views(buf, lay):
    """a buffer of accumulators (uint8 [S, pitch], pitch at least lay.slot_bytes) -> {name: int16 view [S, h, w]} of the planes the layout
    holds, cropped to the coded size: [S, ch, cw] for AX, AY, AGE, RY and [S, ch / 2, cw / 2] for RCb, RCr.  Views, not copies."""
    S, pitch = buf.shape
    cw, ch = lay.coded_width, lay.coded_height
    out = {}
    for name in accumulate_names(lay.parts):
        chroma = name in ("RCb", "RCr")
        h, w, stride = (ch // 2, cw // 2, lay.chroma_stride) if chroma else (ch, cw, lay.luma_stride)
        off = getattr(lay, name.lower() + "_offset")
        out[name] = np.lib.stride_tricks.as_strided(buf.reshape(-1)[off:].view("<i2"), shape=(S, h, w), strides=(pitch, 2 * stride, 2))
    return out


def accumulate_hop(cw, ch, n_frames, motion, residual, hop, acc):
    """The definition of one hop of leon_pipeline_accumulate (include/leon_pipeline.h) in numpy integers, written from the header's text
    and independent of the C code.  motion[i] = (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8), residual[i] = (y [ch, cw], cb, cr
    [ch / 2, cw / 2]) int16 of window frame i (None where no record is at hand; residual may be None without residual planes); hop =
    the 8 words (target, dst_slot, fwd_slot, bwd_slot, 0, 0, 0, 0) (or the first four); acc = {name: int16 array [S, h, w]} with the
    planes of one or both parts (AX AY AGE | RY RCb RCr), WRITTEN IN PLACE (acc[name][dst_slot]) where the status is 0.  Returns
    (status, via): via [mbh, mbw] uint8, None where the status is not 0."""
    hop = [int(v) for v in hop] + [0] * (8 - len(hop))
    T, dst, fs, bs = hop[:4]
    cw, ch = int(cw), int(ch)
    names = [n for n in ACCUMULATE_PLANES if n in acc]
    if cw % 16 or ch % 16 or set(names) not in ({"AX", "AY", "AGE"}, {"RY", "RCb", "RCr"}, set(ACCUMULATE_PLANES)):
        raise ValueError("accumulate_hop: a coded size of %d x %d, planes %s" % (cw, ch, names))
    S = acc[names[0]].shape[0]
    if any(hop[4:]):
        return REGION_RESERVED, None
    if not 0 <= T < int(n_frames):
        return REGION_FRAME, None
    if not (0 <= dst < S and -1 <= fs < S and -1 <= bs < S) or dst == fs or dst == bs:
        return REGION_SLOT, None
    mv, info = np.asarray(motion[T][0]).astype(np.int64), np.asarray(motion[T][1]).astype(np.int64)
    use_f = ((info & 1) != 0) & (fs >= 0)
    use_b = ~use_f & ((info & 2) != 0) & (bs >= 0)
    res = dict(zip(("RY", "RCb", "RCr"), residual[T])) if "RY" in acc else {}
    for name in names:
        step = 2 if name in ("RCb", "RCr") else 1          # luma pixels an element: the rounding is floor((v + step) / (2 step))
        h, w = ch // step, cw // step
        y, x = np.mgrid[0:h, 0:w]
        kj, ki = (y * step) >> 4, (x * step) >> 4
        f, b, v = use_f[kj, ki], use_b[kj, ki], mv[kj, ki]
        dx = (np.where(f, v[..., 0], v[..., 2]) + step) // (2 * step)          # (numpy's integer division floors, also for negatives)
        dy = (np.where(f, v[..., 1], v[..., 3]) + step) // (2 * step)
        sx, sy = np.clip(x + dx, 0, w - 1), np.clip(y + dy, 0, h - 1)
        own = {"AX": sx - x, "AY": sy - y, "AGE": 1}.get(name)
        if own is None:
            own = np.asarray(res[name]).astype(np.int64)
        plane = acc[name]
        out = np.zeros((h, w), dtype=np.int64)
        for use, slot in ((f, fs), (b, bs)):
            if slot >= 0:
                out[use] = (plane[slot].astype(np.int64)[sy, sx] + own)[use]
        plane[dst] = np.clip(out, -32768, 32767).astype(np.int16)
    return REGION_OK, (use_f * 1 + use_b * 2).astype(np.uint8)


def _residual_records(residual, cw, ch):
    """(pointer array, the buffers it points into) of residual[i] = (y, cb, cr) or None, each laid out as residual_layout says (8-byte aligned)"""
    lay = residual_layout(cw, ch)
    n = 0 if residual is None else len(residual)
    ptrs, keep = (C.c_void_p * max(1, n))(), []
    for i in range(n):
        if residual[i] is None:
            continue
        buf = np.zeros(lay.record_pitch // 8, dtype=np.uint64).view(np.uint8)
        for plane, off, stride in zip(residual[i], (0, lay.cb_offset, lay.cr_offset), (lay.luma_stride, lay.chroma_stride, lay.chroma_stride)):
            plane = np.ascontiguousarray(plane, dtype=np.int16)
            np.lib.stride_tricks.as_strided(buf[off:].view("<i2"), shape=plane.shape, strides=(2 * stride, 2))[...] = plane
        keep.append(buf)
        ptrs[i] = buf.ctypes.data
    return ptrs, keep


def _accumulate_config(buf, parts, over=None):
    """PipelineAccumulateConfig of a numpy buffer uint8 [S, pitch]; `over` replaces fields (the refusals' tests)"""
    if not (isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.ndim == 2 and buf.flags.c_contiguous):
        raise ValueError("slots: a contiguous uint8 array [S, pitch]")
    cfg = PipelineAccumulateConfig(int(parts), buf.shape[0], (C.c_int32 * 2)(0, 0), buf.shape[1], buf.shape[0] * buf.shape[1])
    for k, v in (over or {}).items():
        setattr(cfg, k, (C.c_int32 * 2)(*v) if k == "reserved" else v)
    return cfg


def accumulate_record(cw, ch, n_frames, motion, residual, hop, parts, slots, via_fill=0, **over):
    """leon_pipeline_accumulate_record: the library's CPU evaluation of one hop; motion, residual and hop as accumulate_hop's, slots a
    uint8 array [S, pitch] written in place (accumulate_views takes it apart).  Returns (status, via [mbh, mbw] uint8 that holds
    `via_fill` where the library wrote nothing); LeonError where it refuses the call."""
    mptrs, keep = _carry_records(motion, int(cw) // 16, int(ch) // 16)
    rptrs, rkeep = _residual_records(residual, cw, ch)
    h = _records_array([hop])
    via = np.full((int(ch) // 16, int(cw) // 16), via_fill, dtype=np.uint8)
    cfg = _accumulate_config(slots, parts, over)
    st = load().leon_pipeline_accumulate_record(int(cw), int(ch), int(n_frames), mptrs, rptrs if residual is not None else None, C.byref(cfg), h.ctypes.data, slots.ctypes.data,
                                                via.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, via


def accumulate_kernel(cw, ch, n_frames, motion, residual, hops, parts, slots, via=True, status=True, device_id=0, via_fill=0, status_fill=-1, n=None, **over):
    """leon_pipeline_accumulate_kernel: k_accumulate on records the caller supplies (as accumulate_hop's), hops = [(target, dst_slot,
    fwd_slot, bwd_slot), ...], slots uint8 [S, pitch] written in place -> (via [m, mbh, mbw] uint8 pre-filled with `via_fill`, status [m]
    int32 pre-filled with `status_fill`); via=False / status=False hand the library NULL, and the array comes back as it was filled.
    n: the count handed to the library when it is to differ from m = len(hops)."""
    mptrs, keep = _carry_records(motion, int(cw) // 16, int(ch) // 16)
    rptrs, rkeep = _residual_records(residual, cw, ch)
    h = _records_array(hops)
    v, st = _result_arrays(len(h), ((int(ch) // 16, int(cw) // 16), via_fill, np.uint8), ((), status_fill, np.int32))
    cfg = _accumulate_config(slots, parts, over)
    _chk(load().leon_pipeline_accumulate_kernel(int(device_id), int(cw), int(ch), int(n_frames), mptrs, rptrs if residual is not None else None, C.byref(cfg),
                                                h.ctypes.data if len(h) else None, len(h) if n is None else int(n), slots.ctypes.data, v.ctypes.data if via else None,
                                                st.ctypes.data if status else None))
    return v[:len(h)], st[:len(h)]


FIELD_NP_DTYPES = {"float16": np.float16, "bfloat16": np.uint16, "float32": np.float32}          # bfloat16 as bit patterns, like read_tensor


def field_channel(offset_bytes, row_stride, elem_stride=1, shift=0, scale=1.0, bias=0.0):
    """one channel of a field tensors call: the plane's first element offset_bytes into the item, its value under frame pixel (x, y) at
    element offset_bytes / 2 + (y >> shift) * row_stride + (x >> shift) * elem_stride; the element is fl32(fl32(r * scale) + bias)"""
    return (int(offset_bytes), int(row_stride), int(elem_stride), int(shift), float(scale), float(bias))


def _per_channel(v, n):
    """a scalar for every channel, or one value a channel"""
    v = [float(v)] * n if np.isscalar(v) else [float(x) for x in v]
    if len(v) != n:
        raise ValueError("%d values for %d channels" % (len(v), n))
    return v


MOTION_FIELDS = ("fwd_h", "fwd_v", "bwd_h", "bwd_v")          # a motion record's four interleaved words a macroblock


def field_channels_motion(mbw, names=("fwd_h", "fwd_v"), scale=1.0, bias=0.0):
    """channels of a motion record's vectors (motion_layout: int16 [mbs][4] at 0) over a picture mbw macroblocks wide: cells of 16 frame
    pixels, 4 elements apart.  VECTORS ARE IN HALF-PEL FRAME UNITS: scale = 0.5 * out_size / box_size makes them output pixels (per
    channel: the horizontal words with the widths, the vertical ones with the heights).  scale, bias: one value, or one a channel."""
    sc, bi = _per_channel(scale, len(names)), _per_channel(bias, len(names))
    return [field_channel(2 * MOTION_FIELDS.index(n), 4 * int(mbw), 4, 4, sc[i], bi[i]) for i, n in enumerate(names)]


def field_channels_residual(layout, names=("Y", "Cb", "Cr"), scale=1.0, bias=0.0):
    """channels of a residual record's planes (layout: residual_layout's): Y at the frame's size, Cb and Cr in cells of 2 frame pixels"""
    sc, bi = _per_channel(scale, len(names)), _per_channel(bias, len(names))
    at = {"Y": (0, layout.luma_stride, 0), "Cb": (layout.cb_offset, layout.chroma_stride, 1), "Cr": (layout.cr_offset, layout.chroma_stride, 1)}
    return [field_channel(at[n][0], at[n][1], 1, at[n][2], sc[i], bi[i]) for i, n in enumerate(names)]


def field_channels_accumulate(layout, names=("AX", "AY"), scale=1.0, bias=0.0):
    """channels of an accumulator's planes (layout: accumulate_layout's; names of ACCUMULATE_PLANES the layout holds).  AX and AY are in
    FRAME PIXELS: scale = out_size / box_size makes them output pixels."""
    sc, bi = _per_channel(scale, len(names)), _per_channel(bias, len(names))
    have = accumulate_names(layout.parts)
    out = []
    for i, n in enumerate(names):
        if n not in have:
            raise ValueError("the accumulator has no plane %s (parts %d)" % (n, layout.parts))
        chroma = n in ("RCb", "RCr")
        out.append(field_channel(getattr(layout, n.lower() + "_offset"), layout.chroma_stride if chroma else layout.luma_stride, 1, 1 if chroma else 0, sc[i], bi[i]))
    return out


def field_record_status(fw, fh, n_items, record, size):
    """the status word of one record of a field tensors call (REGION_*), in Python integers from the header's text: the reserved words,
    the frame or item index, then per axis -- x before y -- the box and the ratio"""
    r = [int(v) for v in record] + [0] * (8 - len(record))
    oh, ow = int(size[0]), int(size[1])
    if any(r[5:]):
        return REGION_RESERVED
    if not 0 <= r[0] < int(n_items):
        return REGION_FRAME
    for in_size, start, length, out, ratio in ((int(fw), r[1], r[3], ow, REGION_RATIO_X), (int(fh), r[2], r[4], oh, REGION_RATIO_Y)):
        if in_size < 1 or length < 1 or start < 0 or start > in_size or length > in_size - start:
            return REGION_BOX
        if length > 16 * out:
            return ratio
    return REGION_OK


def _field_pass(p, first, count, weights):
    """one pass along axis 1 of p [rows, in] int64 -> [rows, out] int64: exact integers, saturated to int16"""
    out = np.empty((p.shape[0], len(first)), dtype=np.int64)
    for o in range(len(first)):
        n = int(count[o])
        acc = p[:, first[o]:first[o] + n] @ weights[o, :n].astype(np.int64)
        out[:, o] = np.clip((acc + (1 << (RESIZE_PRECISION - 1))) >> RESIZE_PRECISION, -32768, 32767)
    return out


def field_resample(item, fw, fh, box, size, channel):
    """r of one channel: item a 1-D int16 array of the item's elements, box = (x, y, width, height) in frame pixels, size = (out_height,
    out_width) -> int64 [out_height, out_width], each value inside int16"""
    off, rs, es, shift = channel[:4]
    x, y, w, h = [int(v) for v in box]
    oh, ow = int(size[0]), int(size[1])
    fx, nx, wx = resize_weights(fw, x, w, ow, RESIZE_TRIANGLE)
    fy, ny, wy = resize_weights(fh, y, h, oh, RESIZE_TRIANGLE)
    lo, hi = int(fy.min()), int((fy + ny).max())          # the rows the vertical pass taps
    a = np.asarray(item).reshape(-1)
    idx = off // 2 + (np.arange(lo, hi)[:, None] >> shift) * rs + (np.arange(int(fw))[None, :] >> shift) * es
    hz = _field_pass(a[idx].astype(np.int64), fx, nx, wx)
    return _field_pass(hz.T.copy(), fy - lo, ny, wy).T.copy()


def field_element(r, scale, bias, dtype="float16"):
    """the elements of r (integers): fl32(fl32(r * scale) + bias) in np.float32, two rounded operations, then one rounding to nearest
    even into the element type -- float16 / float32 arrays, bfloat16 as uint16 bit patterns"""
    u = (np.asarray(r).astype(np.float32) * np.float32(scale)).astype(np.float32) + np.float32(bias)
    if dtype == "float32":
        return u.astype(np.float32)
    if dtype == "float16":
        return u.astype(np.float16)
    if dtype != "bfloat16":
        raise ValueError("dtype %r" % (dtype,))
    bits = np.ascontiguousarray(u, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def field_tensor(item, fw, fh, box, size, channels, dtype="float16"):
    """The definition of one record of leon_pipeline_field_tensors (include/leon_pipeline.h) in numpy integers and np.float32, written
    from the header's text and independent of the C code, on the pure-Python resize_weights: item a 1-D int16 array (the item's
    elements from its first byte on), a frame of fw x fh, box = (x, y, width, height) in frame pixels -- one field_record_status accepts
    --, size = (out_height, out_width), channels = [field_channel(...), ...] -> [C, out_height, out_width] of FIELD_NP_DTYPES[dtype]
    (bfloat16 as uint16 bit patterns)."""
    return np.stack([field_element(field_resample(item, fw, fh, box, size, c), c[4], c[5], dtype) for c in channels])


def _field_config(source, dtype, size, channels, n_items=0, item_pitch=0, source_bytes=0, over=None):
    """PipelineFieldConfig; `over` replaces fields, "channelN" = {field: value} those of channel N (the refusals' tests)"""
    source = FIELD_SOURCES[source] if isinstance(source, str) else int(source)
    dtype = TENSOR_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    cfg = PipelineFieldConfig(source, dtype, len(channels), RESIZE_TRIANGLE, int(size[1]), int(size[0]), int(n_items), 0, int(item_pitch), int(source_bytes))
    for i, c in enumerate(channels[:FIELD_MAX_CHANNELS]):
        cfg.channel[i] = PipelineFieldChannel(c[0], c[1], c[2], c[3], c[4], c[5], (C.c_int32 * 2)(0, 0))
    for k, v in (over or {}).items():
        if k.startswith("channel") and k != "channels":
            for f, x in v.items():
                setattr(cfg.channel[int(k[7:])], f, (C.c_int32 * 2)(*x) if f == "reserved" else x)
        else:
            setattr(cfg, k, v)
    return cfg


def _field_items(items):
    if not (isinstance(items, np.ndarray) and items.dtype == np.uint8 and items.ndim == 2 and items.flags.c_contiguous):
        raise ValueError("items: a contiguous uint8 array [n_items, item_pitch]")
    return items


def field_tensor_record(fw, fh, cw, ch, items, record, size, channels, source="buffer", dtype="float16", fill=0, over=None):
    """leon_pipeline_field_tensor_record: the library's CPU evaluation of one record; items a uint8 array [n_items, item_pitch].  Returns
    (status, tensor [C, oh, ow] of FIELD_NP_DTYPES[dtype] that holds the bytes `fill` where the library wrote nothing); LeonError where it
    refuses the call.  over: fields of the config replaced, as _field_config takes them."""
    items = _field_items(items)
    cfg = _field_config(source, dtype, size, channels, items.shape[0], items.shape[1], items.size, over)
    out = np.full((len(channels), int(size[0]), int(size[1])), 0, dtype=FIELD_NP_DTYPES[dtype])
    out.view(np.uint8)[...] = fill
    r = _records_array([record])
    st = load().leon_pipeline_field_tensor_record(int(fw), int(fh), int(cw), int(ch), C.byref(cfg), items.ctypes.data, r.ctypes.data, out.ctypes.data)
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st, out


def field_tensors_kernel(fw, fh, cw, ch, items, records, size, channels, source="buffer", dtype="float16", pitch=None, status=True, device_id=0, fill=0, status_fill=-1,
                         scratch_limit=0, n=None, over=None):
    """leon_pipeline_field_tensors_kernel: k_box_tables and k_fields on items the caller supplies (uint8 [n_items, item_pitch]), records =
    [(frame, x, y, w, h), ...] -> (out uint8 [m, pitch] pre-filled with `fill`, status [m] int32 pre-filled with `status_fill`); pitch:
    None is the default, a region's bytes rounded up to 256; status=False hands the library NULL.  field_batch takes `out` apart."""
    items = _field_items(items)
    cfg = _field_config(source, dtype, size, channels, items.shape[0], items.shape[1], items.size, over)
    r = _records_array(records)
    nbytes = len(channels) * int(size[0]) * int(size[1]) * np.dtype(FIELD_NP_DTYPES[dtype]).itemsize
    step = -(-nbytes // 256) * 256 if pitch is None else int(pitch)
    out = np.full((max(1, len(r)), max(step, 1)), fill, dtype=np.uint8)
    st, = _result_arrays(len(r), ((), status_fill, np.int32))
    _chk(load().leon_pipeline_field_tensors_kernel(int(device_id), int(fw), int(fh), int(cw), int(ch), C.byref(cfg), items.ctypes.data, r.ctypes.data if len(r) else None,
                                                   len(r) if n is None else int(n), out.ctypes.data, 0 if pitch is None else step, st.ctypes.data if status else None,
                                                   int(scratch_limit)))
    return out[:len(r)], st[:len(r)]


def field_batch(out, n_channels, size, dtype="float16"):
    """a host buffer of field tensors, uint8 [n, pitch] -> the view [n, C, oh, ow] of FIELD_NP_DTYPES[dtype] over the tensors' bytes"""
    dt = np.dtype(FIELD_NP_DTYPES[dtype])
    nbytes = int(n_channels) * int(size[0]) * int(size[1]) * dt.itemsize
    return out[:, :nbytes].view(dt).reshape(out.shape[0], int(n_channels), int(size[0]), int(size[1])) if out.shape[1] == nbytes else \
        np.lib.stride_tricks.as_strided(out.view(dt), shape=(out.shape[0], int(n_channels), int(size[0]), int(size[1])),
                                        strides=(out.strides[0], int(size[0]) * int(size[1]) * dt.itemsize, int(size[1]) * dt.itemsize, dt.itemsize))


def warp_rgb(rgb, m, size, pad=(0, 0, 0)):
    """The definition of leon_pipeline_warp_regions in numpy integers (include/leon_pipeline.h), written from the header's text: rgb
    [H, W, 3] uint8 -- the CPU twin's colours of the frame, the fill row of an odd height included -- sampled along the Q16 map
    m = (a00, a01, tx, a10, a11, ty) into size = (out_height, out_width) -> uint8 [oh, ow, 3]; positions outside the frame read pad.
    Raises ValueError for a matrix the library refuses (REGION_SCALE, REGION_OFFSET)."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    oh, ow = int(size[0]), int(size[1])
    a00, a01, tx, a10, a11, ty = (int(v) for v in m)
    s2 = max(a00 * a00 + a10 * a10, a01 * a01 + a11 * a11)
    g = next((k for k in range(3) if s2 <= ((1 << (16 + k)) + 1) ** 2), None)
    if g is None:
        raise ValueError("warp_rgb: the matrix reduces by more than 4")
    if max(abs(tx), abs(ty)) > 1 << 29:
        raise ValueError("warp_rgb: an offset above 2^29")
    S = 1 << g
    # the frame inside a border of the pad value: position (x, y) is padded[y + 1, x + 1], everything further out is the border too
    padded = np.empty((H + 2, W + 2, 3), dtype=np.int64)
    padded[:] = np.asarray(pad, dtype=np.int64)
    padded[1:-1, 1:-1] = rgb[..., :3]

    def p(x, y):
        return padded[np.clip(y + 1, 0, H + 1), np.clip(x + 1, 0, W + 1)]
    ox = np.arange(ow, dtype=np.int64)[None, :]
    oy = np.arange(oh, dtype=np.int64)[:, None]
    acc = np.zeros((oh, ow, 3), dtype=np.int64)
    for j in range(S):
        for i in range(S):
            NX = a00 * (2 * S * ox + 2 * i + 1) + a01 * (2 * S * oy + 2 * j + 1) + 2 * S * (tx - 32768)
            NY = a10 * (2 * S * ox + 2 * i + 1) + a11 * (2 * S * oy + 2 * j + 1) + 2 * S * (ty - 32768)
            qx = ((NX >> (g + 1)) + 128) >> 8
            qy = ((NY >> (g + 1)) + 128) >> 8
            x0, fx, y0, fy = qx >> 8, (qx & 255)[..., None], qy >> 8, (qy & 255)[..., None]
            acc += (256 - fx) * (256 - fy) * p(x0, y0) + fx * (256 - fy) * p(x0 + 1, y0) + (256 - fx) * fy * p(x0, y0 + 1) + fx * fy * p(x0 + 1, y0 + 1)
    return ((acc + (1 << (15 + 2 * g))) >> (16 + 2 * g)).astype(np.uint8)


def warp_matrix(A):
    """leon_pipeline_warp_from_matrix: the Q16 words of A = (a00, a01, tx, a10, a11, ty) (or a 2 x 3 array), floor(v * 65536 + 0.5)"""
    a = (C.c_double * 6)(*[float(v) for v in np.asarray(A, dtype=np.float64).ravel()])
    m = (C.c_int32 * 6)()
    _chk(load().leon_pipeline_warp_from_matrix(a, m))
    return tuple(m)


def warp_matrix_rotated_box(cx, cy, w, h, angle_degrees, size):
    """leon_pipeline_warp_from_rotated_box: the Q16 words that fill size = (out_height, out_width) with the box of w x h frame pixels
    centred at (cx, cy) and rotated by angle_degrees"""
    m = (C.c_int32 * 6)()
    _chk(load().leon_pipeline_warp_from_rotated_box(float(cx), float(cy), float(w), float(h), float(angle_degrees), int(size[1]), int(size[0]), m))
    return tuple(m)


def _warp_args(regions, size, pad_value):
    """(PipelineWarpRegion array, n, PipelineWarpConfig) of a list of (frame_index, m) -- or PipelineWarpRegion structs -- and
    or one int32 array [n, 8] of records -- and size = (out_height, out_width) -- or a PipelineWarpConfig"""
    if isinstance(regions, np.ndarray):          # [n, 8] records: no Python loop over the regions
        full = np.ascontiguousarray(regions, dtype=np.int32).reshape(-1, 8)
        return (PipelineWarpRegion * max(1, len(full))).from_buffer_copy(full.tobytes() or bytes(32)), len(full), _warp_config(size, pad_value)
    regions = list(regions)
    arr = (PipelineWarpRegion * max(1, len(regions)))()
    for i, r in enumerate(regions):
        arr[i] = r if isinstance(r, PipelineWarpRegion) else PipelineWarpRegion(int(r[0]), (C.c_int32 * 6)(*[int(v) for v in r[1]]), 0)
    return arr, len(regions), _warp_config(size, pad_value)


def _warp_config(size, pad_value):
    if isinstance(size, PipelineWarpConfig):
        return size
    cfg = PipelineWarpConfig(int(size[1]), int(size[0]))
    if pad_value is not None:
        r, g, b = pad_value
        cfg.pad[0], cfg.pad[1], cfg.pad[2] = int(r), int(g), int(b)
    return cfg


def warp_regions_check(frame_width, frame_height, n_frames, regions, size, pad_value=None):
    """leon_pipeline_warp_regions_check: what Pipeline.warp_regions would refuse of these regions (a list of (frame_index, m)), without
    a device.  Returns None when they are accepted; raises LeonError otherwise, its `bad` the index of the first offending region."""
    arr, n, cfg = _warp_args(regions, size, pad_value)
    bad = C.c_int32(-2)
    rc = load().leon_pipeline_warp_regions_check(int(frame_width), int(frame_height), int(n_frames), arr, n, C.byref(cfg), C.byref(bad))
    if rc != OK:
        e = LeonError(rc, load().leon_last_error().decode("utf-8", "replace"))
        e.bad = bad.value
        raise e


def warp_region_status(frame_width, frame_height, n_frames, region, size, pad_value=None):
    """leon_pipeline_warp_region_status: the REGION_* word Pipeline.warp_regions_device writes for region = (frame_index, m) (or a
    PipelineWarpRegion).  No device."""
    arr, _, cfg = _warp_args([region], size, pad_value)
    st = load().leon_pipeline_warp_region_status(int(frame_width), int(frame_height), int(n_frames), arr, C.byref(cfg))
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st


def _fit_ref(f):
    return C.byref(f) if f is not None else None


def region_fit_rect(box_width, box_height, size, fit="letterbox", anchor=None, pad_value=None):
    """leon_pipeline_region_fit_rect: (x, y, width, height) of the image of a box of box_width x box_height in its tensor of
    size = (height, width) -- the letterbox integers, at (0, 0) with anchor "top_left"; the tensor itself when stretched.  No device."""
    cfg = size if isinstance(size, PipelineRegionsConfig) else PipelineRegionsConfig(int(size[1]), int(size[0]), RESIZE_TRIANGLE)
    rect = (C.c_int32 * 4)()
    _chk(load().leon_pipeline_region_fit_rect(int(box_width), int(box_height), C.byref(cfg), _fit_ref(_regions_fit(fit, anchor, pad_value)), rect))
    return tuple(rect)


def regions_fit_check(frame_width, frame_height, n_frames, regions, size, filter="triangle", fit="letterbox", anchor=None, pad_value=None):
    """leon_pipeline_regions_fit_check: regions_check with the fit keywords of Pipeline.resample_regions"""
    arr, n, cfg = _regions_args(regions, size, filter)
    bad = C.c_int32(-2)
    rc = load().leon_pipeline_regions_fit_check(int(frame_width), int(frame_height), int(n_frames), arr, n, C.byref(cfg),
                                                _fit_ref(_regions_fit(fit, anchor, pad_value)), C.byref(bad))
    if rc != OK:
        e = LeonError(rc, load().leon_last_error().decode("utf-8", "replace"))
        e.bad = bad.value
        raise e


def region_fit_status(frame_width, frame_height, n_frames, region, size, filter="triangle", fit="letterbox", anchor=None, pad_value=None):
    """leon_pipeline_region_fit_status: region_status with the fit keywords of Pipeline.resample_regions_device"""
    arr, _, cfg = _regions_args([region], size, filter)
    st = load().leon_pipeline_region_fit_status(int(frame_width), int(frame_height), int(n_frames), arr, C.byref(cfg), _fit_ref(_regions_fit(fit, anchor, pad_value)))
    if st < 0:
        raise LeonError(st, load().leon_last_error().decode("utf-8", "replace"))
    return st


def resize_weights_device(axes, filter=RESIZE_TRIANGLE, max_taps=None, device_id=0, fill=-1):
    """leon_pipeline_resize_weights_device: the DEVICE's evaluation of the tables of a batch of axes = [(in_size, crop_start, crop_size,
    out_size), ...], copied back: (first[n, max_out], count[n, max_out], weights[n, max_out, max_taps], status[n]) with max_out the
    largest out_size; rows behind an axis's out_size, and all rows of an axis whose status is not 0, hold `fill`.  To be compared word
    for word with resize_weights / leon_pipeline_resize_weights."""
    filter = _resize_filter_code(filter)
    ax = np.ascontiguousarray(np.asarray(axes, dtype=np.int32).reshape(-1, 4))
    n = len(ax)
    if max_taps is None:
        max_taps = RESIZE_MAX_TAPS_BICUBIC if filter == RESIZE_BICUBIC else RESIZE_MAX_TAPS
    max_out = int(ax[:, 3].max()) if n and 1 <= int(ax[:, 3].max()) <= 4096 else 1
    first = np.full((max(n, 1), max_out), fill, dtype=np.int32)
    count = np.full((max(n, 1), max_out), fill, dtype=np.int32)
    weights = np.full((max(n, 1), max_out, max(1, int(max_taps))), fill, dtype=np.int32)
    status = np.full(max(n, 1), fill, dtype=np.int32)
    _chk(load().leon_pipeline_resize_weights_device(int(device_id), n, ax.ctypes.data, filter, int(max_taps), first.ctypes.data, count.ctypes.data,
                                                    weights.ctypes.data, status.ctypes.data))
    return first, count, weights, status


def _hostptr(a, dtype, keep):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    keep.append(a)
    return a.ctypes.data


def make_picture(ptype, out_slot, coef_y, coef_cb, coef_cr, qscale, intra, repadd=None, mv_fwd=None,
                 mv_bwd=None, mb_dir=None, ref_fwd_slot=-1, ref_bwd_slot=-1, keep=None, device=False,
                 rgba_out=None, no_planes=False, coef_a=None, qm_set=0):
    """Fill a Picture from numpy arrays (host) or raw device addresses (device=True: ints).
    rgba_out: device address of the RGBA frame for the fused display conversion (always a device address);
    coef_a: the A plane's levels for a yuva decoder."""
    p = Picture()
    p.type, p.out_slot, p.ref_fwd_slot, p.ref_bwd_slot = ptype, out_slot, ref_fwd_slot, ref_bwd_slot
    p.rgba_out = None if rgba_out is None else int(rgba_out)
    p.no_planes = 1 if no_planes else 0
    p.qm_set = int(qm_set)
    if device:
        vals = (coef_y, coef_cb, coef_cr, qscale, intra, repadd, mv_fwd, mv_bwd, mb_dir)
        (p.coef_y, p.coef_cb, p.coef_cr, p.qscale, p.intra, p.repadd, p.mv_fwd, p.mv_bwd, p.mb_dir) = \
            [None if v is None else int(v) for v in vals]
        p.coef_a = None if coef_a is None else int(coef_a)
        return p
    keep = keep if keep is not None else []
    p.coef_a = _hostptr(coef_a, np.int16, keep)
    p.coef_y = _hostptr(coef_y, np.int16, keep)
    p.coef_cb = _hostptr(coef_cb, np.int16, keep)
    p.coef_cr = _hostptr(coef_cr, np.int16, keep)
    p.qscale = _hostptr(qscale, np.uint8, keep)
    p.intra = _hostptr(intra, np.uint8, keep)
    p.repadd = _hostptr(repadd, np.uint8, keep)
    p.mv_fwd = _hostptr(mv_fwd, np.int16, keep)
    p.mv_bwd = _hostptr(mv_bwd, np.int16, keep)
    p.mb_dir = _hostptr(mb_dir, np.uint8, keep)
    p._keep = keep
    return p


def make_sparse_picture(ptype, out_slot, grp_off, entries, n_entries, qscale, intra, repadd=None, mv_fwd=None,
                        mv_bwd=None, mb_dir=None, ref_fwd_slot=-1, ref_bwd_slot=-1, keep=None, device=False,
                        rgba_out=None, no_planes=False, qm_set=0):
    """The sparse-boundary twin of make_picture (lists in the format of include/leon_vlc.h)."""
    p = SparsePicture()
    p.qm_set = int(qm_set)
    p.type, p.out_slot, p.ref_fwd_slot, p.ref_bwd_slot = ptype, out_slot, ref_fwd_slot, ref_bwd_slot
    p.rgba_out = None if rgba_out is None else int(rgba_out)
    p.no_planes = 1 if no_planes else 0
    p.n_entries = int(n_entries)
    if device:
        vals = (grp_off, entries, qscale, intra, repadd, mv_fwd, mv_bwd, mb_dir)
        (p.grp_off, p.entries, p.qscale, p.intra, p.repadd, p.mv_fwd, p.mv_bwd, p.mb_dir) = \
            [None if v is None else int(v) for v in vals]
        return p
    keep = keep if keep is not None else []
    p.grp_off = _hostptr(grp_off, np.uint32, keep)
    p.entries = _hostptr(entries, np.uint32, keep)
    p.qscale = _hostptr(qscale, np.uint8, keep)
    p.intra = _hostptr(intra, np.uint8, keep)
    p.repadd = _hostptr(repadd, np.uint8, keep)
    p.mv_fwd = _hostptr(mv_fwd, np.int16, keep)
    p.mv_bwd = _hostptr(mv_bwd, np.int16, keep)
    p.mb_dir = _hostptr(mb_dir, np.uint8, keep)
    p._keep = keep
    return p


class Decoder:
    """Thin object wrapper over the C ABI; method names follow include/leon.h."""

    def __init__(self, coded_w, coded_h, frame_w=None, frame_h=None, n_slots=13, device_id=0, stream=None, alpha=False, contiguous_slots=False):
        self.lib = load()
        cfg = Config(coded_w, coded_h, frame_w or coded_w, frame_h or coded_h, n_slots, device_id, stream, 1 if alpha else 0,
                     1 if contiguous_slots else 0)
        h = C.c_void_p()
        _chk(self.lib.leon_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.cw, self.ch = coded_w, coded_h
        self.fw, self.fh = cfg.frame_width, cfg.frame_height
        self.n_slots = n_slots

    def close(self):
        if self.h:
            self.lib.leon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_quant_matrices(self, intra=None, non_intra=None):
        keep = []
        _chk(self.lib.leon_set_quant_matrices(self.h, _hostptr(intra, np.uint8, keep), _hostptr(non_intra, np.uint8, keep)))

    def add_quant_matrices(self, intra=None, non_intra=None):
        """a further set of matrices beside set 0; returns the id pictures name in qm_set"""
        keep, s = [], C.c_int32()
        _chk(self.lib.leon_add_quant_matrices(self.h, _hostptr(intra, np.uint8, keep), _hostptr(non_intra, np.uint8, keep), C.byref(s)))
        return s.value

    def acquire_slot(self):
        s = C.c_int32()
        _chk(self.lib.leon_acquire_slot(self.h, C.byref(s)))
        return s.value

    def release_slot(self, slot):
        _chk(self.lib.leon_release_slot(self.h, slot))

    def free_decoded_slots(self):
        _chk(self.lib.leon_free_decoded_slots(self.h))

    def submit_picture(self, pic):
        _chk(self.lib.leon_submit_picture(self.h, C.byref(pic)))

    def submit_batch(self, pics, mem=MEM_DEVICE):
        arr = (Picture * len(pics))(*pics)
        _chk(self.lib.leon_submit_batch(self.h, arr, len(pics), mem))

    def batch_create(self, pics):
        arr = (Picture * len(pics))(*pics)
        b = C.c_void_p()
        _chk(self.lib.leon_batch_create(self.h, arr, len(pics), C.byref(b)))
        return b

    def submit_sparse(self, pics, mem=MEM_HOST):
        arr = (SparsePicture * len(pics))(*pics)
        _chk(self.lib.leon_submit_sparse(self.h, arr, len(pics), mem))

    def batch_create_sparse(self, pics):
        arr = (SparsePicture * len(pics))(*pics)
        b = C.c_void_p()
        _chk(self.lib.leon_batch_create_sparse(self.h, arr, len(pics), C.byref(b)))
        return b

    def batch_run(self, b):
        _chk(self.lib.leon_batch_run(self.h, b))

    def batch_destroy(self, b):
        self.lib.leon_batch_destroy(self.h, b)

    def convert_rgba(self, slot, flavour=RGB_CPU_TWIN):
        out = np.empty((self.fh, self.fw, 4), dtype=np.uint8)
        _chk(self.lib.leon_convert_rgba(self.h, slot, out.ctypes.data, MEM_HOST, flavour))
        return out

    def convert_rgba_batch(self, slots, rgba_device_ptr, flavour=RGB_CPU_TWIN):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        _chk(self.lib.leon_convert_rgba_batch(self.h, s.ctypes.data, len(s), int(rgba_device_ptr), flavour))

    def read_planes(self, slot):
        n = self.cw * self.ch
        y = np.empty((self.ch, self.cw), dtype=np.uint8)
        cb = np.empty((self.ch // 2, self.cw // 2), dtype=np.uint8)
        cr = np.empty((self.ch // 2, self.cw // 2), dtype=np.uint8)
        _chk(self.lib.leon_read_planes(self.h, slot, y.ctypes.data, cb.ctypes.data, cr.ctypes.data))
        return y, cb, cr

    def read_alpha_plane(self, slot):
        a = np.empty((self.ch, self.cw), dtype=np.uint8)
        _chk(self.lib.leon_read_alpha_plane(self.h, slot, a.ctypes.data))
        return a

    def write_alpha_plane(self, slot, a):
        keep = []
        _chk(self.lib.leon_write_alpha_plane(self.h, slot, _hostptr(a, np.uint8, keep)))

    def write_planes(self, slot, y, cb, cr):
        keep = []
        _chk(self.lib.leon_write_planes(self.h, slot, _hostptr(y, np.uint8, keep), _hostptr(cb, np.uint8, keep),
                                        _hostptr(cr, np.uint8, keep)))

    def slot_device_ptr(self, slot):
        p, n = C.c_void_p(), C.c_size_t()
        _chk(self.lib.leon_slot_device_ptr(self.h, slot, C.byref(p), C.byref(n)))
        return p.value, n.value

    def sync(self):
        _chk(self.lib.leon_sync(self.h))

    def set_overlap_convert(self, on=True):
        _chk(self.lib.leon_set_overlap_convert(self.h, 1 if on else 0))

    def timing_enable(self, on=True):
        _chk(self.lib.leon_timing_enable(self.h, 1 if on else 0))

    def timing_reset(self):
        _chk(self.lib.leon_timing_reset(self.h))

    def timing_get(self, kind=0):
        s = KernelStats()
        _chk(self.lib.leon_timing_get(self.h, kind, C.byref(s)))
        return {"launches": s.launches, "total_ms": s.total_ms, "algorithmic_bytes": s.algorithmic_bytes,
                "macroblocks": s.macroblocks}

    def timing_launches(self):
        """the timed launches one by one, in submission order"""
        n = C.c_int32()
        _chk(self.lib.leon_timing_get_launches(self.h, None, 0, C.byref(n)))
        arr = (LaunchTime * max(1, n.value))()
        _chk(self.lib.leon_timing_get_launches(self.h, arr, n.value, C.byref(n)))
        return [{"kind": a.kind, "pic_type": a.pic_type, "ms": a.ms, "algorithmic_bytes": a.algorithmic_bytes,
                 "macroblocks": a.macroblocks} for a in arr[:n.value]]

    def measure_copy_bandwidth(self, nbytes=1 << 31, iters=10):
        g = C.c_double()
        _chk(self.lib.leon_measure_copy_bandwidth(self.h, nbytes, iters, C.byref(g)))
        return g.value

    def measure_stream_bandwidth(self, nbytes=1 << 31, iters=10, reads=1, writes=1):
        """GB/s over all streams of the 16-byte-per-lane kernel with `reads` source and `writes` destination streams"""
        g = C.c_double()
        _chk(self.lib.leon_measure_stream_bandwidth(self.h, nbytes, iters, reads, writes, C.byref(g)))
        return g.value


class _Frames:
    """the frames of a delivered window as a read-only sequence of dicts, made when asked for (a 128-GOP window has 1536 of
    them; a callback that looks at a dozen should not pay for the rest on the pipeline's notify thread)"""

    def __init__(self, frames, n, pipe, window=-1, tensors=None, motion=None, activity=None, residual=None):
        self._f, self._n, self._pipe, self._window, self._tensors, self._motion, self._activity = frames, n, pipe, window, tensors, motion, activity
        self._residual = residual

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        f = self._f[i]
        m = self._motion[i] if self._motion is not None else None
        return {"motion": None if m is None else {"record": m.record, "fwd_gop": int(m.fwd_gop), "fwd_display": m.fwd_display, "bwd_display": m.bwd_display},
                "gop": int(f.gop), "display_index": f.display_index, "type": f.type, "ts_ms": f.ts_ms, "rgba": f.rgba,
                "y": f.y, "cb": f.cb, "cr": f.cr, "a": f.a, "tensor": self._tensors[i] if self._tensors is not None else None,
                "activity": self._activity[i] if self._activity is not None else None,
                "residual": self._residual[i] if self._residual is not None else None,
                "_i": i, "_window": self._window, "_frames": self._f, "_pipe": self._pipe}

    def __iter__(self):
        return (self[i] for i in range(self._n))


def _device_tensor_check(name, t, dtype, count, dev, words=False, strided=False):
    """what a device road asks of a tensor argument (None: not supplied): on the pipeline's device and, with a dtype, of that dtype,
    contiguous (strided: left to the caller) and of at least `count` elements (words: the text of the int32 arrays)"""
    if t is None:
        return
    if not t.is_cuda or t.device.index != dev:
        raise ValueError("%s: on %s, the pipeline's device is cuda:%d" % (name, t.device, dev))
    if dtype is not None and (t.dtype != dtype or not (strided or t.is_contiguous()) or t.numel() < count):
        raise ValueError("%s: a contiguous %s tensor of at least %d %s" % ((name, "int32", count, "words") if words else (name, dtype, count, "elements")))


def _need_output(layout, name):          # the layout of a Pipeline's record output ("motion", "activity", "residual"), or the refusal of one made without it
    if layout is None:
        raise LeonError(ERR_INVALID, "the pipeline has no %s output (Pipeline %s=True)" % (name, name))
    return layout


def _empty_where_none(stream, dev, wanted):
    """wanted = [(tensor or None, shape, dtype), ...] -> the tensors, those that were None allocated on `stream` (not initialised)"""
    import torch
    with torch.cuda.stream(stream):
        return [torch.empty(shape, dtype=dtype, device="cuda:%d" % dev) if t is None else t for t, shape, dtype in wanted]


class Pipeline:
    """leon_pipeline_* (include/leon_pipeline.h): stream bytes in, RGBA frames in device memory out.
    on_window(window_id, frames) runs on the pipeline's notify thread with a list of dicts
    (gop, display_index, type, ts_ms, rgba = device address); unless it returns False the window is
    released right after.  read_frame(frame) works until the frame's window is released.
    Open GOPs (closed_gop = 0) are decoded, no option needed: their leading B pictures predict from the GOP before; an open GOP
    without its predecessor (first of a run or of a loop pass, the target of seek(), broken_link) delivers from its I picture on,
    so its first display positions are missing from `frames`.  Only with shard_count > 1 such a GOP makes wait() raise.
    output="ycbcr" / "both": the frames carry their YCbCr 4:2:0 planes too (y, cb, cr, a = device addresses, a for yuva
    streams only; rgba is None with "ycbcr"): read_planes(frame) copies them to the host, plane_views(frame) wraps them.
    output="tensor" / "rgba+tensor" / "ycbcr+tensor" / "all" (PIPELINE_TENSOR_OUTPUTS): the frames carry a planar [3, H, W] tensor
    (tensor = device address) of tensor_dtype "float16" / "bfloat16" / "float32", element = tensor_table(dtype, scale, bias)[c][colour
    value]; tensor_scale / tensor_bias: three floats each (None: 1/255 and 0).  read_tensor(frame) copies it to the host,
    tensor_view(frame) and window_tensor(frames) wrap it in place as torch tensors.
    tensor_size=(out_h, out_w) [, tensor_crop=(x, y, w, h) in frame pixels]: the tensors are that crop box (default: the whole frame)
    resampled on the device to a model's input size -- element = table[c][resize_rgb(rgb, crop, size, filter)] --, and every tensor shape
    above is [3, out_h, out_w] (tensor_geometry has the values in force); tensor_filter="triangle" (the default, antialiased bilinear) or
    "bicubic" (or the RESIZE_* integers).
    tensor_dtype="uint8": the elements are the 8-bit colour values themselves (no scale / bias).  tensor_layout="hwc": channels last
    -- every shape above is [H, W, 3] ([N, H, W, 3] for window_tensor), a packed uint8 HWC frame is 3 bytes per pixel; tensor_shape
    (PipelineTensorShape) has the element type, the layout and the strides in elements.
    tensor_canvas=(H, W) (with tensor_size): the resampled image lies in an H x W tensor, its top-left element at tensor_origin=(x, y)
    (None: centred, the odd pixel right or below), every other element at tensor_pad_value=(r, g, b), 8-bit colour values that go through
    the element table like the image's -- element = table[c][canvas_rgb(rgb, crop, size, canvas, origin, pad, filter)]; every tensor shape
    above is the canvas's, tensor_canvas_geometry (PipelineTensorCanvas) has the image rectangle.  Every element is written every window.
    tensor_letterbox=(H, W): tensor_size, tensor_canvas and tensor_origin derived with letterbox() from the crop box, or the frame:
    the aspect ratio kept, the image centred.
    Regions (any tensor output): resample_regions(window, regions, size, filter) resamples boxes of the window's full-resolution frames
    -- regions = [(frame["_i"], x, y, w, h), ...], a detector's boxes -- to size = (h, w) into one [N, 3, h, w] ("hwc": [N, h, w, 3])
    device batch of the pipeline's element type and table, element = table[c][resize_rgb(rgb of that frame, (x, y, w, h), size, filter)];
    the pipeline's own tensor_size / crop / canvas play no part.  Until the window is released, from the callback or (for a window held
    by returning False) from any thread; read_regions(...) gives the same as a host array.  resample_regions_device(window, boxes, ...)
    takes the boxes from a CUDA tensor and only enqueues, on torch's current stream: no host wait between a detector and its classifier.
    motion=True (beside any output): every frame carries its motion record -- per macroblock of the coded picture the forward and backward
    vectors and an info byte (MOTION_FWD / MOTION_BWD / MOTION_INTRA), and a summary of eight words: motion_from_maps states it.
    frame["motion"] = {"record": device address, "fwd_gop", "fwd_display", "bwd_display": which pictures the vectors point into (-1: none)};
    read_motion(window, i) copies frame i's record to the host, motion_view(window, i) wraps it in place; motion_layout has the offsets.
    activity=True (beside any output, with or without motion): every frame carries its activity record -- per macroblock how much the
    stream coded on top of the prediction (ACTIVITY_CELL: ac_count, ac_mag, dc_mag, blocks, qscale) and a summary of eight words:
    activity_from_lists states it.  frame["activity"] = the record's device address; read_activity(window, i) copies it to the host,
    activity_view(window, i) wraps it in place; activity_layout has the offsets.
    residual=True (beside any output, independent of the two above): every frame carries its residual record -- the int16 planes Y, Cb, Cr
    of the coded picture that the stream's coefficients decode to before any prediction is added and before any clamp (the oracle's
    pass 1 and residual pass 2 state it).  frame["residual"] = the record's device address; read_residual(window, i) copies the three
    planes to the host, residual_view(window, i) wraps them in place; residual_layout has strides and offsets.
    Carrying boxes (motion=True): carry_regions_device(window, records) moves boxes from one frame of the window to another along those
    vectors, on the device and on torch's current stream (carry_box states one hop; carry_regions is the same from host records);
    gauge_regions_device(window, records) returns per box the area-weighted sums of the frame's motion and activity records under it
    (gauge_box states them; gauge_regions is the same from host records): carry_regions_gop's records go in as they are.
    Proposing boxes (motion=True and / or activity=True): propose_regions_device(window) turns every frame's records into region records on
    the device -- the boxes of the connected components of the macroblocks that moved, are intra or were coded anew (propose_boxes states
    them; propose_regions is the same to host arrays) -- which go into gauge_regions_device and resample_regions_device as they are.
    carry_regions_gop(window, boxes, src) carries a detector's boxes on frame `src` to every frame of its GOP, ready for
    resample_regions_device.
    Comparing boxes (any output): suppress_regions_device(window, records, scores) prunes every set of a [n, K, 8] tensor by greedy
    suppression (suppress_boxes states it) and match_regions_device(window, a, b) pairs the rows of two such tensors one to one by
    overlap (match_boxes states it), both on the device: what propose_regions_device and carry_regions_gop return goes in as it is,
    and the `out` rows of a suppression go into the gauge, resample and carry calls.  suppress_regions / match_regions: the same on
    host arrays.
    Propagating dense maps (motion=True): propagate_maps_device(window, maps, hops, stride) writes the map of a frame -- a mask, heatmaps,
    features at 1, 2, 4, 8 or 16 frame pixels a cell -- as a gather from the maps of the pictures it predicts from, through its own motion
    record, on the device (propagate_map states one hop; propagate_maps is the same from host arrays); propagate_maps_gop(window, map,
    src, stride) takes a network's output on frame `src` to every frame of its GOP.
    Accumulating motion and residual (motion=True; residual=True for the residual planes): accumulate_device(window, slots, hops, parts)
    writes the accumulator of a frame -- per sample where it came from in the picture the chain started at (AX, AY, AGE) and the sum of
    the residual records along that path (RY, RCb, RCr), int16 planes over the coded picture -- through its own motion record from the
    accumulators of the pictures it predicts from (accumulate_hop states one hop; accumulate is the same from host arrays);
    accumulate_gop(window, src) traces every frame of `src`'s GOP back to `src`: what a compressed-domain video model reads."""

    def __init__(self, data, device_id=0, parser_threads=0, gops_per_window=0, windows_in_flight=0, max_gop_pictures=0,
                 loop=0, on_window=None, shard_index=0, shard_count=0, start_seconds=0.0, gpu_parser=None, valid_bytes=None, display_flavour=0,
                 output="rgba", tensor_dtype="float16", tensor_scale=None, tensor_bias=None, tensor_size=None, tensor_crop=None, tensor_filter=RESIZE_TRIANGLE,
                 tensor_layout="chw", tensor_canvas=None, tensor_origin=None, tensor_pad_value=None, tensor_letterbox=None, motion=False, activity=False,
                 residual=False):
        self.lib = load()
        if tensor_letterbox is not None:
            if tensor_size is not None or tensor_canvas is not None or tensor_origin is not None:
                raise ValueError("tensor_letterbox derives tensor_size, tensor_canvas and tensor_origin: give it alone")
            if tensor_crop is not None and any(tensor_crop):
                src_w, src_h = tensor_crop[2], tensor_crop[3]
            else:          # the frame's size, from the stream's first sequence header
                import leon_vlc_ctypes as V
                st = V.Stream(bytes(data) if valid_bytes is None else bytes(data[:int(valid_bytes)]), threads=1)
                src_w, src_h = st.info.frame_width, st.info.frame_height
                st.close()
            ow, oh, x, y = letterbox(src_w, src_h, tensor_letterbox[1], tensor_letterbox[0])
            tensor_size, tensor_canvas, tensor_origin = (oh, ow), tuple(tensor_letterbox), (x, y)
        self.device_id = device_id
        # a name of PIPELINE_OUTPUTS, or the raw bit set (anything the library does not know is refused by create)
        out_bits = (PIPELINE_OUTPUTS.get(output) or PIPELINE_TENSOR_OUTPUTS[output]) if isinstance(output, str) else int(output)
        if motion:
            out_bits = (out_bits or PIPELINE_OUTPUT_RGBA) | PIPELINE_OUTPUT_MOTION
        if activity:
            out_bits = (out_bits or PIPELINE_OUTPUT_RGBA) | PIPELINE_OUTPUT_ACTIVITY
        if residual:
            out_bits = (out_bits or PIPELINE_OUTPUT_RGBA) | PIPELINE_OUTPUT_RESIDUAL
        tcfg = None
        if out_bits > 0 and out_bits & PIPELINE_OUTPUT_TENSOR:
            tcfg = PipelineTensorConfig(_tensor_dtype_code(tensor_dtype), (C.c_float * 3)(*([0, 0, 0] if tensor_scale is None else tensor_scale)),
                                        (C.c_float * 3)(*([0, 0, 0] if tensor_bias is None else tensor_bias)))
        rcfg = None
        tensor_filter = _resize_filter_code(tensor_filter)
        if tensor_size is not None or tensor_crop is not None or tensor_filter:      # (the library refuses what does not go together)
            oh, ow = (0, 0) if tensor_size is None else tensor_size
            cx, cy, cw, ch = (0, 0, 0, 0) if tensor_crop is None else tensor_crop
            rcfg = PipelineTensorResize(int(cx), int(cy), int(cw), int(ch), int(ow), int(oh), int(tensor_filter))
        fcfg = None
        if _tensor_layout_code(tensor_layout) != TENSOR_LAYOUT_CHW:      # only a non-default format goes through leon_pipeline_create_tensor_format
            fcfg = PipelineTensorFormat(_tensor_layout_code(tensor_layout))
        ccfg = None
        if tensor_canvas is not None or tensor_origin is not None or tensor_pad_value is not None:      # (the library refuses what does not go together)
            ch_, cw_ = (0, 0) if tensor_canvas is None else tensor_canvas
            if tensor_origin is None:          # centred, as leon_pipeline_letterbox centres
                oh_, ow_ = (0, 0) if tensor_size is None else tensor_size
                tensor_origin = ((int(cw_) - int(ow_)) // 2, (int(ch_) - int(oh_)) // 2) if int(cw_) >= int(ow_) and int(ch_) >= int(oh_) else (0, 0)
            pr, pg, pb = (0, 0, 0) if tensor_pad_value is None else tensor_pad_value
            ccfg = PipelineTensorCanvas(int(cw_), int(ch_), int(tensor_origin[0]), int(tensor_origin[1]), (C.c_int32 * 3)(int(pr), int(pg), int(pb)))
        self._data = (C.c_uint8 * len(data)).from_buffer_copy(data)      # must outlive the pipeline
        self._on_window = on_window
        self.windows = 0
        self.frames = 0
        self.ended = False
        self.ends = 0              # 'ended' callbacks so far (one per run: create's, then one per seek that runs to the end)
        self.error = None

        import threading
        ready = threading.Event()          # set once self.h exists: decoding starts inside leon_pipeline_create

        self._window_n = {}        # frames of the windows that are out for delivery (motion_view asks window_motion for exactly that many)
        self._window_gops = {}

        def _release(window):
            self._window_n.pop(window, None)
            self._window_gops.pop(window, None)
            rc = self.lib.leon_pipeline_release_window(self.h, window)
            if rc != OK and self.error is None:
                self.error = LeonError(rc, "leon_pipeline_release_window(%d): %s" % (window, self.lib.leon_last_error().decode()))

        def _cb(_user, window, frames, n, status):
            try:
                ready.wait()
                if window < 0:
                    self.ends += 1
                    self.ended = True
                    return
                if status != OK:          # a failed window is delivered too and must be given back like any other
                    self.error = status
                    _release(window)
                    return
                self.windows += 1
                self.frames += n
                self._window_n[window] = n
                if self.info.output & PIPELINE_OUTPUT_MOTION and n:          # what carry_regions_gop plans with: the frames' gop, display_index, type
                    self._window_gops[window] = C.string_at(frames, n * C.sizeof(PipelineFrame))          # (one copy; read when asked for)
                keep = None
                if self._on_window is not None:
                    # `_pipe`: a callback may read frames through the dicts alone (read_frame(f) below), without the
                    # variable its caller assigns the pipeline to -- which does not exist yet while the constructor runs
                    tensors = None
                    if self.info.tensor_dtype and n:          # the window's tensor pointers, one call
                        tensors = (C.c_void_p * n)()
                        if self.lib.leon_pipeline_window_tensors(self.h, window, tensors, n) != OK:
                            raise LeonError(ERR_INVALID, self.lib.leon_last_error().decode())
                    motion = None
                    if self.info.output & PIPELINE_OUTPUT_MOTION and n:          # the window's motion records and references, one call
                        motion = (PipelineMotionFrame * n)()
                        if self.lib.leon_pipeline_window_motion(self.h, window, motion, n) != OK:
                            raise LeonError(ERR_INVALID, self.lib.leon_last_error().decode())
                    activity = None
                    if self.info.output & PIPELINE_OUTPUT_ACTIVITY and n:        # ... and its activity records
                        activity = (C.c_void_p * n)()
                        if self.lib.leon_pipeline_window_activity(self.h, window, activity, n) != OK:
                            raise LeonError(ERR_INVALID, self.lib.leon_last_error().decode())
                    residual = None
                    if self.info.output & PIPELINE_OUTPUT_RESIDUAL and n:        # ... and its residual records
                        residual = (C.c_void_p * n)()
                        if self.lib.leon_pipeline_window_residual(self.h, window, residual, n) != OK:
                            raise LeonError(ERR_INVALID, self.lib.leon_last_error().decode())
                    fl = _Frames(frames, n, self, window, tensors, motion, activity, residual)
                    keep = self._on_window(window, fl)
                if keep is not False:
                    _release(window)
            except Exception as e:      # never let an exception cross the C boundary
                self.error = e
        self._cb = PIPELINE_CB(_cb)
        self._ready = ready
        cfg = PipelineConfig(device_id, parser_threads, gops_per_window, windows_in_flight, max_gop_pictures, loop,
                             shard_index, shard_count, float(start_seconds), 0 if gpu_parser is None else (1 if gpu_parser else -1), int(display_flavour),      # None: the library's default (the GPU)
                             out_bits)
        h = C.c_void_p()
        self.h = None
        # valid_bytes: the stream is still arriving (leon_pipeline_create_partial); feed() reports progress
        if ccfg is not None:
            rc = self.lib.leon_pipeline_create_tensor_canvas(C.byref(cfg), None if tcfg is None else C.byref(tcfg), None if rcfg is None else C.byref(rcfg),
                                                             None if fcfg is None else C.byref(fcfg), C.byref(ccfg), self._data, len(data),
                                                             len(data) if valid_bytes is None else int(valid_bytes), self._cb, None, C.byref(h))
        elif fcfg is not None:
            rc = self.lib.leon_pipeline_create_tensor_format(C.byref(cfg), None if tcfg is None else C.byref(tcfg), None if rcfg is None else C.byref(rcfg), C.byref(fcfg),
                                                             self._data, len(data), len(data) if valid_bytes is None else int(valid_bytes), self._cb, None, C.byref(h))
        elif rcfg is not None:
            rc = self.lib.leon_pipeline_create_tensor_resized(C.byref(cfg), None if tcfg is None else C.byref(tcfg), C.byref(rcfg), self._data, len(data),
                                                              len(data) if valid_bytes is None else int(valid_bytes), self._cb, None, C.byref(h))
        elif tcfg is not None:
            rc = self.lib.leon_pipeline_create_tensor(C.byref(cfg), C.byref(tcfg), self._data, len(data), len(data) if valid_bytes is None else int(valid_bytes),
                                                      self._cb, None, C.byref(h))
        elif valid_bytes is None:
            rc = self.lib.leon_pipeline_create(C.byref(cfg), self._data, len(data), self._cb, None, C.byref(h))
        else:
            rc = self.lib.leon_pipeline_create_partial(C.byref(cfg), self._data, len(data), int(valid_bytes), self._cb, None, C.byref(h))
        _chk(rc)
        self.h = h
        info = PipelineInfo()
        rc = self.lib.leon_pipeline_get_info(self.h, C.byref(info))
        self.info = info
        # the tensors' shape: the frame's, or tensor_size (None without tensor output)
        self.tensor_geometry = None
        self.tensor_shape = None
        if rc == OK and info.tensor_dtype:
            geom = PipelineTensorGeometry()
            rc = self.lib.leon_pipeline_get_tensor_geometry(self.h, C.byref(geom))
            self.tensor_geometry = geom
        if rc == OK and info.tensor_dtype:
            shape = PipelineTensorShape()
            rc = self.lib.leon_pipeline_get_tensor_shape(self.h, C.byref(shape))
            self.tensor_shape = shape
        # where the image lies in the tensor (without canvas settings: all of it)
        self.tensor_canvas_geometry = None
        if rc == OK and info.tensor_dtype:
            canvas = PipelineTensorCanvas()
            rc = self.lib.leon_pipeline_get_tensor_canvas(self.h, C.byref(canvas))
            self.tensor_canvas_geometry = canvas
        self.motion_layout = None
        if rc == OK and info.output & PIPELINE_OUTPUT_MOTION:
            lay = PipelineMotionLayout()
            rc = self.lib.leon_pipeline_get_motion_layout(self.h, C.byref(lay))
            self.motion_layout = lay
        self.activity_layout = None
        if rc == OK and info.output & PIPELINE_OUTPUT_ACTIVITY:
            lay = PipelineActivityLayout()
            rc = self.lib.leon_pipeline_get_activity_layout(self.h, C.byref(lay))
            self.activity_layout = lay
        self.residual_layout = None
        if rc == OK and info.output & PIPELINE_OUTPUT_RESIDUAL:
            lay = PipelineResidualLayout()
            rc = self.lib.leon_pipeline_get_residual_layout(self.h, C.byref(lay))
            self.residual_layout = lay
        ready.set()
        _chk(rc)

    def _delivered_n(self, window):
        """the number of frames of a window that is out for delivery"""
        n = self._window_n.get(int(window))
        if n is None:
            raise LeonError(ERR_INVALID, "window %d is not out for delivery" % int(window))
        return n

    def window_motion(self, window, n):
        """leon_pipeline_window_motion: the n motion frames (PipelineMotionFrame array) of a delivered, not yet released window"""
        out = (PipelineMotionFrame * max(1, int(n)))()
        _chk(self.lib.leon_pipeline_window_motion(self.h, int(window), out, int(n)))
        return out

    def read_motion(self, window, index):
        """the motion record of frame `index` of a delivered, not yet released window as host arrays:
        (mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8, summary [8] uint32)"""
        lay = self.motion_layout
        mbw, mbh = (lay.mb_width, lay.mb_height) if lay is not None else (1, 1)      # (without the output the library refuses below)
        mv = np.empty((mbh, mbw, 4), dtype=np.int16)
        info = np.empty((mbh, mbw), dtype=np.uint8)
        summary = np.empty(8, dtype=np.uint32)
        _chk(self.lib.leon_pipeline_read_motion(self.h, int(window), int(index), mv.ctypes.data, info.ctypes.data, summary.ctypes.data))
        return mv, info, summary

    def motion_view(self, window, index, device_id=None):
        """the same three parts where they lie, as torch views of device memory (int16 [mbh, mbw, 4], uint8 [mbh, mbw], int32 [8]: torch
        has no uint32 arithmetic, the words are below 2^31), without copying: valid until the window is released"""
        lay = _need_output(self.motion_layout, "motion")
        ptr = self.window_motion(window, self._delivered_n(window))[int(index)].record
        dev = self.device_id if device_id is None else device_id
        return (_cuda_view(ptr, (lay.mb_height, lay.mb_width, 4), "<i2", (lay.mb_width * 8, 8, 2), dev),
                _cuda_view(ptr + lay.info_offset, (lay.mb_height, lay.mb_width), "|u1", (lay.mb_width, 1), dev),
                _cuda_view(ptr + lay.summary_offset, (8,), "<i4", (4,), dev))

    def window_activity(self, window, n):
        """leon_pipeline_window_activity: the device addresses of the n activity records of a delivered, not yet released window"""
        out = (C.c_void_p * max(1, int(n)))()
        _chk(self.lib.leon_pipeline_window_activity(self.h, int(window), out, int(n)))
        return out

    def read_activity(self, window, index):
        """the activity record of frame `index` of a delivered, not yet released window as host arrays:
        (cells [mbh, mbw] of ACTIVITY_CELL, summary [8] uint32)"""
        lay = self.activity_layout
        mbw, mbh = (lay.mb_width, lay.mb_height) if lay is not None else (1, 1)      # (without the output the library refuses below)
        cells = np.empty((mbh, mbw), dtype=ACTIVITY_CELL)
        summary = np.empty(8, dtype=np.uint32)
        _chk(self.lib.leon_pipeline_read_activity(self.h, int(window), int(index), cells.ctypes.data, summary.ctypes.data))
        return cells, summary

    def activity_view(self, window, index, device_id=None):
        """the same record where it lies, as torch views of device memory, without copying: (words int16 [mbh, mbw, 4] -- ac_count, ac_mag,
        dc_mag and blocks | qscale << 8 as their 16 bits, torch has no uint16 arithmetic --, bytes uint8 [mbh, mbw, 8] over the same
        cells, summary int32 [8], the 32 bits of each word); valid until the window is released"""
        lay = _need_output(self.activity_layout, "activity")
        ptr = self.window_activity(window, self._delivered_n(window))[int(index)]
        dev = self.device_id if device_id is None else device_id
        return (_cuda_view(ptr, (lay.mb_height, lay.mb_width, 4), "<i2", (lay.mb_width * 8, 8, 2), dev),
                _cuda_view(ptr, (lay.mb_height, lay.mb_width, 8), "|u1", (lay.mb_width * 8, 8, 1), dev),
                _cuda_view(ptr + lay.summary_offset, (8,), "<i4", (4,), dev))

    def window_residual(self, window, n):
        """leon_pipeline_window_residual: the device addresses of the n residual records of a delivered, not yet released window"""
        out = (C.c_void_p * max(1, int(n)))()
        _chk(self.lib.leon_pipeline_window_residual(self.h, int(window), out, int(n)))
        return out

    def read_residual(self, window, index):
        """the residual record of frame `index` of a delivered, not yet released window as host arrays, cropped to the coded size:
        (y [ch, cw], cb [ch / 2, cw / 2], cr [ch / 2, cw / 2]) int16"""
        lay = self.residual_layout
        cw, ch = (lay.coded_width, lay.coded_height) if lay is not None else (16, 16)      # (without the output the library refuses below)
        y, cb, cr = np.empty((ch, cw), dtype=np.int16), np.empty((ch // 2, cw // 2), dtype=np.int16), np.empty((ch // 2, cw // 2), dtype=np.int16)
        _chk(self.lib.leon_pipeline_read_residual(self.h, int(window), int(index), y.ctypes.data, cb.ctypes.data, cr.ctypes.data))
        return y, cb, cr

    def residual_view(self, window, index, device_id=None):
        """the same three planes where they lie, as strided torch views of device memory (int16 [ch, cw], [ch / 2, cw / 2] twice), without
        copying: valid until the window is released"""
        lay = _need_output(self.residual_layout, "residual")
        ptr = self.window_residual(window, self._delivered_n(window))[int(index)]
        dev = self.device_id if device_id is None else device_id
        cw, ch = lay.coded_width, lay.coded_height
        return (_cuda_view(ptr, (ch, cw), "<i2", (2 * lay.luma_stride, 2), dev),
                _cuda_view(ptr + lay.cb_offset, (ch // 2, cw // 2), "<i2", (2 * lay.chroma_stride, 2), dev),
                _cuda_view(ptr + lay.cr_offset, (ch // 2, cw // 2), "<i2", (2 * lay.chroma_stride, 2), dev))

    def carry_refs(self, window):
        """leon_pipeline_get_carry_refs: (fwd, bwd) int32 arrays -- for each frame of a delivered, not yet released window the index of
        the window frame its forward and backward vectors point into (-1: none in this window), as the pipeline resolved them"""
        _need_output(self.motion_layout, "motion")
        n = self._delivered_n(window)
        fwd, bwd = np.empty(max(1, n), dtype=np.int32), np.empty(max(1, n), dtype=np.int32)
        _chk(self.lib.leon_pipeline_get_carry_refs(self.h, int(window), fwd.ctypes.data, bwd.ctypes.data, n))
        return fwd[:n], bwd[:n]

    def carry_regions(self, window, records, fill=0):
        """leon_pipeline_carry_regions: records = [(frame, x, y, w, h, target), ...] in host memory, one hop each along the window's
        motion records (carry_box states it) -> (out [n, 8], votes [n, 4], status [n]) int32 host arrays; out[i] is a region record
        (target, x', y', w, h, 0, 0, 0) for resample_regions, votes[i] = (A, I, dh, dv).  A record's fault is its status word
        (REGION_*, REGION_NO_REFERENCE: no prediction joins the two frames), never a LeonError; its out and votes keep `fill`.  Synchronous."""
        r = _records_array(records)
        out, votes, status = _result_arrays(len(r), ((8,), fill, np.int32), ((4,), fill, np.int32), ((), fill, np.int32))
        _chk(self.lib.leon_pipeline_carry_regions(self.h, int(window), r.ctypes.data if len(r) else None, len(r), out.ctypes.data, votes.ctypes.data, status.ctypes.data))
        return out[:len(r)], votes[:len(r)], status[:len(r)]

    def carry_regions_device(self, window, records, out=None, votes=None, status=None, stream=None):
        """leon_pipeline_carry_regions_device: the same hops from records that lie in DEVICE memory -- a contiguous CUDA int32 torch
        tensor [N, 8]: frame, x, y, w, h, target, 0, 0 -- queued on `stream` (a torch.cuda.Stream; None: torch's current stream) with
        warp_regions_device's ordering: NO host synchronisation.  Returns (out [N, 8], votes [N, 4], status [N]) int32 tensors on the
        device (the caller's, or ones the method allocates, not initialised): out[i] and votes[i] are written exactly where status[i]
        is 0.  out can go to resample_regions_device as it is, and -- a new target written into column 5 -- to the next hop."""
        import torch
        _need_output(self.motion_layout, "motion")
        dev = self.device_id
        _device_records_check("records", records)
        n = int(records.shape[0])
        for name, t, words in (("records", records, 8 * n), ("out", out, 8 * n), ("votes", votes, 4 * n), ("status", status, n)):
            _device_tensor_check(name, t, torch.int32, words, dev, words=True)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        out, votes, status = _empty_where_none(stream, dev, [(out, (max(1, n), 8), torch.int32), (votes, (max(1, n), 4), torch.int32), (status, max(1, n), torch.int32)])
        call = PipelineCarryRegionsCall(records.data_ptr() if n else None, n, 0, out.data_ptr(), votes.data_ptr(), status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_carry_regions_device(self.h, int(window), C.byref(call)))
        return out.view(-1)[:8 * n].view(n, 8), votes.view(-1)[:4 * n].view(n, 4), status.view(-1)[:n]

    def carry_regions_gop(self, window, boxes, src, frames=None):
        """Boxes on window frame `src` carried to every delivered frame of its GOP in the window: boxes = a CUDA int32 tensor [N, 4]
        (x, y, w, h).  One carry_regions_device call per level of carry_plan on torch's current stream, each level's inputs gathered from
        the level before by torch indexing: nothing waits for the device.  Returns (records [F, N, 8], votes [F, N, 4], status
        [F, N]) over all F frames of the window, zero-filled beforehand: records[f] are region records on frame f for
        resample_regions_device, and a hop that failed -- or followed one that did -- reads as an empty box there (status REGION_BOX
        downstream of it).  Frames of another GOP, and frames carry_plan cannot reach, have status REGION_NO_REFERENCE.
        frames: the window's frames when the pipeline did not see them delivered (dicts, or (gop, display_index, type))."""
        import torch
        _need_output(self.motion_layout, "motion")
        dev = "cuda:%d" % self.device_id
        if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda and boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 4):
            raise ValueError("boxes: a CUDA int32 tensor [N, 4] (x, y, w, h)")
        info = self._window_keys(window, frames)
        levels, _ = carry_plan(self.carry_refs(window), info, src)
        F, N = len(info), int(boxes.shape[0])
        records = torch.zeros((F, N, 8), dtype=torch.int32, device=dev)
        votes = torch.zeros((F, N, 4), dtype=torch.int32, device=dev)
        status = torch.full((F, N), REGION_NO_REFERENCE, dtype=torch.int32, device=dev)
        records[src, :, 0] = int(src)
        records[src, :, 1:5] = boxes
        status[src] = REGION_OK
        per = max(1, 65535 // max(1, N))          # hops a call takes: 65535 records at the most
        flat = [h for hops in levels for h in hops]
        ends = torch.tensor([[h[0] for h in flat], [h[1] for h in flat]] if flat else [[], []], dtype=torch.int64, device=dev)          # (one upload for all levels)
        ends32, first = ends.to(torch.int32), 0
        for hops in levels:
            for at in range(first, first + len(hops), per):
                stop = min(at + per, first + len(hops))
                frm, to = ends[0, at:stop], ends[1, at:stop]
                rec = records[frm]          # (a copy; a source whose own hop failed is all zeros: an empty box on its frame)
                rec[:, :, 0] = ends32[0, at:stop, None]
                rec[:, :, 5] = ends32[1, at:stop, None]
                out = torch.zeros_like(rec)
                vot = torch.zeros((stop - at, N, 4), dtype=torch.int32, device=dev)
                sta = torch.zeros((stop - at, N), dtype=torch.int32, device=dev)
                if N:
                    self.carry_regions_device(window, rec.view(-1, 8), out=out.view(-1, 8), votes=vot.view(-1, 4), status=sta.view(-1))
                records[to], votes[to], status[to] = out, vot, sta
            first += len(hops)
        return records, votes, status

    def _gauge_sources(self, sources):
        """the sources of a gauge call: None = every record output the pipeline has"""
        if sources is not None:
            return int(sources)
        return (GAUGE_MOTION if self.motion_layout is not None else 0) | (GAUGE_ACTIVITY if self.activity_layout is not None else 0)

    def gauge_regions(self, window, regions, sources=None, fill=0):
        """leon_pipeline_gauge_regions: regions = [(frame, x, y, w, h), ...] in host memory -> (stats [n, 16] int64, status [n] int32)
        host arrays: per box the area-weighted sums over the macroblocks under it of that frame's motion record (GAUGE_MOTION, words
        8 .. 15), its activity record (GAUGE_ACTIVITY, words 1 .. 7) or both (gauge_box states them); sources=None: every record output
        the pipeline has.  A record's fault is its status word (REGION_*), never a LeonError; its statistics keep `fill`.  Synchronous."""
        r = _records_array(regions)
        stats, status = _result_arrays(len(r), ((GAUGE_WORDS,), fill, np.int64), ((), fill, np.int32))
        cfg = PipelineGaugeConfig(self._gauge_sources(sources))
        _chk(self.lib.leon_pipeline_gauge_regions(self.h, int(window), C.byref(cfg), r.ctypes.data if len(r) else None, len(r), stats.ctypes.data, status.ctypes.data))
        return stats[:len(r)], status[:len(r)]

    def gauge_regions_device(self, window, records, sources=None, stats=None, status=None, stream=None):
        """leon_pipeline_gauge_regions_device: the same from records that lie in DEVICE memory -- a contiguous CUDA int32 torch tensor
        [N, 8] (frame, x, y, w, h, 0, 0, 0), or [F, N, 8] as carry_regions_gop returns it, read as [F * N, 8] -- queued on `stream` (a
        torch.cuda.Stream; None: torch's current stream) with carry_regions_device's ordering: NO host synchronisation.  Returns (stats
        [N, 16] int64, status [N] int32) on the device (the caller's, or ones the method allocates, not initialised): stats[i] is
        written exactly where status[i] is 0."""
        import torch
        dev = self.device_id
        _device_records_check("records", records, stacked=True)
        records = records.view(-1, 8)
        n = int(records.shape[0])
        _device_tensor_check("records", records, torch.int32, 8 * n, dev, words=True)
        _device_tensor_check("stats", stats, torch.int64, GAUGE_WORDS * n, dev)
        _device_tensor_check("status", status, torch.int32, n, dev, words=True)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        stats, status = _empty_where_none(stream, dev, [(stats, (max(1, n), GAUGE_WORDS), torch.int64), (status, max(1, n), torch.int32)])
        cfg = PipelineGaugeConfig(self._gauge_sources(sources))
        call = PipelineGaugeRegionsCall(records.data_ptr() if n else None, n, 0, stats.data_ptr(), status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_gauge_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return stats.view(-1)[:GAUGE_WORDS * n].view(n, GAUGE_WORDS), status.view(-1)[:n]

    def _propose_config(self, max_boxes, mv_min, ac_min, intra, connectivity, min_cells, sources):
        """the config of a propose call: sources None = every record output the pipeline has, each with its threshold"""
        if sources is None:
            sources = (PROPOSE_MOTION if self.motion_layout is not None else 0) | (PROPOSE_ACTIVITY if self.activity_layout is not None else 0)
            if (sources & PROPOSE_MOTION and mv_min is None) or (sources & PROPOSE_ACTIVITY and ac_min is None):
                raise ValueError("propose regions: sources=None reads every record output the pipeline has: give %s" %
                                 ("mv_min" if sources & PROPOSE_MOTION and mv_min is None else "ac_min"))
            mv_min, ac_min = (mv_min if sources & PROPOSE_MOTION else None), (ac_min if sources & PROPOSE_ACTIVITY else None)
        return _propose_config(sources, max_boxes, mv_min, ac_min, intra, connectivity, min_cells)

    def propose_regions(self, window, frames=None, max_boxes=16, mv_min=None, ac_min=None, intra=False, connectivity=8, min_cells=1, sources=None, fill=-1):
        """leon_pipeline_propose_regions: frames = window frame indices in host memory (None: every frame of the window) -> (regions
        [F, K, 8], count [F], info [F, K, 2], status [F]) int32 host arrays: per frame the boxes of the connected components of its hot
        macroblocks -- a vector of mv_min half-pels or more (PROPOSE_MOTION), intra where `intra`, an ac_mag of ac_min or more
        (PROPOSE_ACTIVITY) -- in raster order of their first cell (propose_boxes states them); count is not capped at K = max_boxes.
        sources=None: every record output the pipeline has, with a threshold required for each.  A request's fault is its status word
        (REGION_FRAME), never a LeonError; its rows and count keep `fill`.  Synchronous."""
        cfg = self._propose_config(max_boxes, mv_min, ac_min, intra, connectivity, min_cells, sources)
        fr = np.arange(self._delivered_n(window), dtype=np.int32) if frames is None else np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        m, K = max(1, len(fr)), max(1, min(int(cfg.max_boxes), PROPOSE_MAX_BOXES))
        regions, info = np.full((m, K, 8), fill, dtype=np.int32), np.full((m, K, 2), fill, dtype=np.int32)
        count, status = np.full(m, fill, dtype=np.int32), np.full(m, fill, dtype=np.int32)
        _chk(self.lib.leon_pipeline_propose_regions(self.h, int(window), C.byref(cfg), fr.ctypes.data if len(fr) else None, len(fr), regions.ctypes.data, info.ctypes.data,
                                                    count.ctypes.data, status.ctypes.data))
        return regions[:len(fr)], count[:len(fr)], info[:len(fr)], status[:len(fr)]

    def propose_regions_device(self, window, frames=None, max_boxes=16, mv_min=None, ac_min=None, intra=False, connectivity=8, min_cells=1, sources=None, stream=None):
        """leon_pipeline_propose_regions_device: the same with everything in DEVICE memory -- frames: a contiguous CUDA int32 torch
        tensor [F] of window frame indices (None: every frame of the window) -- queued on `stream` (a torch.cuda.Stream; None: torch's
        current stream) with carry_regions_device's ordering: NO host synchronisation.  Returns (regions [F, K, 8], count [F], info
        [F, K, 2], status [F]) int32 CUDA tensors: regions goes into gauge_regions_device / resample_regions_device as it is (the rows
        behind count come back as REGION_BOX); a request whose status is not 0 has nothing of its rows and count written."""
        import torch
        dev = self.device_id
        cfg = self._propose_config(max_boxes, mv_min, ac_min, intra, connectivity, min_cells, sources)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        if frames is None:
            n = self._delivered_n(window)
            with torch.cuda.stream(stream):
                frames = torch.arange(n, dtype=torch.int32, device="cuda:%d" % dev)
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.int32 and frames.dim() == 1 and frames.is_contiguous()):
            raise ValueError("frames: a contiguous CUDA int32 tensor [F]")
        n = int(frames.shape[0])
        _device_tensor_check("frames", frames, torch.int32, n, dev, words=True)
        m, K = max(1, n), max(1, min(int(cfg.max_boxes), PROPOSE_MAX_BOXES))
        regions, count, info, status = _empty_where_none(stream, dev, [(None, (m, K, 8), torch.int32), (None, m, torch.int32), (None, (m, K, 2), torch.int32),
                                                                       (None, m, torch.int32)])
        call = PipelineProposeRegionsCall(frames.data_ptr() if n else None, n, 0, regions.data_ptr(), info.data_ptr(), count.data_ptr(), status.data_ptr(),
                                          self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_propose_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return regions[:n], count[:n], info[:n], status[:n]

    def suppress_regions(self, window, regions, scores=None, threshold=0.5, measure="iou", score_stride=1, threshold_q16=None, fill=-1):
        """leon_pipeline_suppress_regions: regions [n, K, 8] (or [K, 8]) and scores in host memory -> (out [n, K, 8], order [n, K], by
        [n, K], count [n], status [n, K]) int32 host arrays (suppress_boxes states them).  A row's fault is its status word, never a
        LeonError; its `by` keeps `fill`.  Synchronous."""
        r, n, K, sc, (out, order, by, count, status) = _suppress_arrays(regions, scores, score_stride, fill)
        cfg = _overlap_config(threshold, measure, threshold_q16)
        _chk(self.lib.leon_pipeline_suppress_regions(self.h, int(window), C.byref(cfg), r.ctypes.data if r.size else None, n, K, None if sc is None else sc.ctypes.data,
                                                     int(score_stride), out.ctypes.data, order.ctypes.data, by.ctypes.data, count.ctypes.data, status.ctypes.data))
        return out[:n], order[:n], by[:n], count[:n], status[:n]

    def match_regions(self, window, a, b, threshold=0.5, measure="iou", threshold_q16=None, fill=-1):
        """leon_pipeline_match_regions: a [n, Ka, 8] and b [n, Kb, 8] in host memory -> (match_a [n, Ka], match_b [n, Kb], overlap
        [n, Ka], count [n], status_a, status_b) int32 host arrays (match_boxes states them).  Synchronous."""
        ra, rb, n, Ka, Kb, (ma, mb, ov, count, sa, sb) = _match_arrays(a, b, fill)
        cfg = _overlap_config(threshold, measure, threshold_q16)
        _chk(self.lib.leon_pipeline_match_regions(self.h, int(window), C.byref(cfg), ra.ctypes.data if ra.size else None, Ka, rb.ctypes.data if rb.size else None, Kb, n,
                                                  ma.ctypes.data, mb.ctypes.data, ov.ctypes.data, count.ctypes.data, sa.ctypes.data, sb.ctypes.data))
        return ma[:n], mb[:n], ov[:n], count[:n], sa[:n], sb[:n]

    @staticmethod
    def _overlap_sets(name, t):
        """a CUDA int32 tensor [K, 8] or [n, K, 8] of rows -> [n, K, 8]"""
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.dim() in (2, 3) and t.shape[-1] == 8 and t.is_contiguous()):
            raise ValueError("%s: a contiguous CUDA int32 tensor [K, 8] or [n, K, 8]" % name)
        return t.view(1, -1, 8) if t.dim() == 2 else t

    def suppress_regions_device(self, window, records, scores=None, threshold=0.5, measure="iou", score_stride=1, stream=None, threshold_q16=None):
        """leon_pipeline_suppress_regions_device: records = a contiguous CUDA int32 tensor [n, K, 8] ([K, 8]: one set), scores = a
        contiguous CUDA int32 tensor of n * K * score_stride words (propose's info [n, K, 2] with score_stride=2: the cells) or None,
        queued on `stream` (None: torch's current stream) with carry_regions_device's ordering: NO host synchronisation.  Returns
        (out [n, K, 8], order [n, K], by [n, K], count [n], status [n, K]) int32 CUDA tensors: `out` holds the kept rows in walk
        order and zero rows behind count, and goes into gauge_regions_device / resample_regions_device / carry_regions_gop as it is;
        `by` is written for the accepted rows only."""
        import torch
        dev = self.device_id
        records = self._overlap_sets("records", records)
        n, K = int(records.shape[0]), int(records.shape[1])
        _device_tensor_check("records", records, torch.int32, 8 * n * K, dev, words=True)
        _device_tensor_check("scores", scores, torch.int32, n * K * max(1, int(score_stride)), dev, words=True)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        m, Kc = max(1, n), max(1, K)
        out, order, by, count, status = _empty_where_none(stream, dev, [(None, (m, Kc, 8), torch.int32), (None, (m, Kc), torch.int32), (None, (m, Kc), torch.int32),
                                                                        (None, m, torch.int32), (None, (m, Kc), torch.int32)])
        cfg = _overlap_config(threshold, measure, threshold_q16)
        call = PipelineSuppressRegionsCall(records.data_ptr() if n * K else None, None if scores is None else scores.data_ptr(), n, K, int(score_stride), 0, out.data_ptr(),
                                           order.data_ptr(), by.data_ptr(), count.data_ptr(), status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_suppress_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return out[:n], order[:n], by[:n], count[:n], status[:n]

    def match_regions_device(self, window, a, b, threshold=0.5, measure="iou", stream=None, threshold_q16=None):
        """leon_pipeline_match_regions_device: a [n, Ka, 8] and b [n, Kb, 8], contiguous CUDA int32 tensors ([K, 8]: one set), set s
        of a against set s of b, queued like suppress_regions_device.  Returns (match_a [n, Ka], match_b [n, Kb], overlap [n, Ka],
        count [n], status_a [n, Ka], status_b [n, Kb]) int32 CUDA tensors; the words of a refused row are not written."""
        import torch
        dev = self.device_id
        a, b = self._overlap_sets("a", a), self._overlap_sets("b", b)
        if a.shape[0] != b.shape[0]:
            raise ValueError("a and b: as many sets")
        n, Ka, Kb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        _device_tensor_check("a", a, torch.int32, 8 * n * Ka, dev, words=True)
        _device_tensor_check("b", b, torch.int32, 8 * n * Kb, dev, words=True)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        m, A, B = max(1, n), max(1, Ka), max(1, Kb)
        ma, mb, ov, count, sa, sb = _empty_where_none(stream, dev, [(None, (m, A), torch.int32), (None, (m, B), torch.int32), (None, (m, A), torch.int32),
                                                                    (None, m, torch.int32), (None, (m, A), torch.int32), (None, (m, B), torch.int32)])
        cfg = _overlap_config(threshold, measure, threshold_q16)
        call = PipelineMatchRegionsCall(a.data_ptr() if n * Ka else None, b.data_ptr() if n * Kb else None, n, Ka, Kb, 0, ma.data_ptr(), mb.data_ptr(), ov.data_ptr(),
                                        count.data_ptr(), sa.data_ptr(), sb.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_match_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return ma[:n], mb[:n], ov[:n], count[:n], sa[:n], sb[:n]

    def _propagate_check(self, maps, stride):
        lay = propagate_layout(self.info.frame_width, self.info.frame_height, stride, maps.shape[1] if len(maps.shape) == 4 else 0, self._elem_bytes(maps))
        if len(maps.shape) != 4 or tuple(maps.shape[2:]) != (lay.mh, lay.mw):
            raise ValueError("maps: [S, P, %d, %d] at stride %d, not %s" % (lay.mh, lay.mw, int(stride), tuple(maps.shape)))
        return lay

    @staticmethod
    def _elem_bytes(maps):
        return maps.dtype.itemsize if isinstance(maps, np.ndarray) else maps.element_size()

    def propagate_maps(self, window, maps, hops, stride, fill=0, via_fill=0):
        """leon_pipeline_propagate_maps: maps = a numpy array [S, P, mh, mw] of a 1-, 2- or 4-byte dtype in host memory, WRITTEN IN PLACE;
        hops = [(target, dst_slot, fwd_slot, bwd_slot), ...]: each writes maps[dst_slot], the map of window frame `target`, as a gather
        through the target's motion record from maps[fwd_slot] / maps[bwd_slot] (-1: not supplied) -- propagate_map states it.
        Returns (via [n, mh, mw] uint8, status [n] int32); a record's fault is its status word (REGION_*, REGION_SLOT), never a
        LeonError, and its slot and via map keep what they held (`via_fill`).  Synchronous."""
        _need_output(self.motion_layout, "motion")
        self._propagate_check(maps, stride)
        h = _records_array(hops)
        via, status = _result_arrays(len(h), (maps.shape[2:], via_fill, np.uint8), ((), 0, np.int32))
        cfg = _propagate_config(maps, stride, fill)
        _chk(self.lib.leon_pipeline_propagate_maps(self.h, int(window), C.byref(cfg), h.ctypes.data if len(h) else None, len(h), maps.ctypes.data, via.ctypes.data,
                                                   status.ctypes.data))
        return via[:len(h)], status[:len(h)]

    def propagate_maps_device(self, window, maps, hops, stride, fill=0, via=None, status=None, stream=None):
        """leon_pipeline_propagate_maps_device: the same hops with everything in DEVICE memory -- maps a contiguous CUDA tensor
        [S, P, mh, mw] of any 1-, 2- or 4-byte dtype (its slots may lie further apart than a map, stride(0); a map's bytes, or that
        stride's, are a multiple of 4), written in place; hops a contiguous CUDA int32 tensor [N, 8]: target, dst_slot,
        fwd_slot, bwd_slot, 0, 0, 0, 0 -- queued on `stream` (a torch.cuda.Stream; None: torch's current stream) with
        carry_regions_device's ordering: NO host synchronisation.  Returns (via [N, mh, mw] uint8, status [N] int32) on the device
        (the caller's, or ones the method allocates, not initialised): a slot and its via map are written exactly where status is 0.
        Hops of one call must not name another hop's dst_slot: chain the levels of propagate_plan in calls of their own."""
        import torch
        _need_output(self.motion_layout, "motion")
        dev = self.device_id
        if not (isinstance(maps, torch.Tensor) and maps.is_cuda and maps.dim() == 4 and maps[0].is_contiguous() and maps.element_size() in (1, 2, 4)
                and (maps.shape[0] == 1 or maps.stride(0) >= maps[0].numel())):
            raise ValueError("maps: a CUDA tensor [S, P, mh, mw] of a 1-, 2- or 4-byte dtype, contiguous (or with its slots further apart: stride(0))")
        _device_records_check("hops", hops)
        lay = self._propagate_check(maps, stride)
        n, cells = int(hops.shape[0]), lay.mh * lay.mw
        for name, t, dtype, count in (("maps", maps, maps.dtype, 0), ("hops", hops, torch.int32, 0), ("via", via, torch.uint8, n * cells), ("status", status, torch.int32, n)):
            _device_tensor_check(name, t, dtype, count, dev, strided=t is maps)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        via, status = _empty_where_none(stream, dev, [(via, (max(1, n), lay.mh, lay.mw), torch.uint8), (status, max(1, n), torch.int32)])
        S, P, e = int(maps.shape[0]), int(maps.shape[1]), maps.element_size()
        pitch = (maps.stride(0) if S > 1 else P * cells) * e          # (the library refuses one that is no multiple of 4: pad the slots apart)
        cfg = PipelinePropagateConfig(int(stride), P, e, S, int(fill) & 0xffffffff, 0, pitch, S * pitch)
        call = PipelinePropagateMapsCall(hops.data_ptr() if n else None, n, 0, maps.data_ptr(), via.data_ptr(), status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_propagate_maps_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return via.view(-1)[:n * cells].view(n, lay.mh, lay.mw), status.view(-1)[:n]

    def _window_keys(self, window, frames=None):
        """(gop, display_index, type) of the frames of a window that is out for delivery"""
        if frames is not None:
            return [(f["gop"], f["display_index"], f["type"]) if isinstance(f, dict) else tuple(int(v) for v in f[:3]) for f in frames]
        raw = self._window_gops.get(int(window))
        if raw is None:
            raise LeonError(ERR_INVALID, "window %d is not out for delivery" % int(window))
        fa = np.frombuffer(raw, dtype=np.dtype([("gop", "<u8"), ("display_index", "<i4"), ("type", "<i4"), ("rest", "V48")]))
        return list(zip(fa["gop"].tolist(), fa["display_index"].tolist(), fa["type"].tolist()))

    def gop_frames(self, window, src, frames=None):
        """the window frames of `src`'s GOP, in the window's order: what the rows of propagate_maps_gop's results stand for"""
        keys = self._window_keys(window, frames)
        return [i for i, k in enumerate(keys) if k[0] == keys[int(src)][0]]

    def propagate_maps_gop(self, window, map, src, stride, fill=0, frames=None):
        """A map on window frame `src` propagated to every delivered frame of its GOP in the window: map = a CUDA tensor [P, mh, mw] of a
        1-, 2- or 4-byte dtype (a mask, heatmaps, features).  One propagate_maps_device call per level of propagate_plan on torch's
        current stream; all levels' hop records go up in one upload from pinned memory in front of the first launch, queued like the launches: nothing
        waits for the device.
        Returns (maps [F, P, mh, mw], via [F, mh, mw] uint8, status [F] int32) over the F frames gop_frames(window, src) lists: `src`'s
        row is a copy of `map` with via 3; a frame no chain of predictions reaches from `src` is all fill, via 0, status
        REGION_NO_REFERENCE.  frames: the window's frames when the pipeline did not see them delivered."""
        import torch
        _need_output(self.motion_layout, "motion")
        dev = "cuda:%d" % self.device_id
        if not (isinstance(map, torch.Tensor) and map.is_cuda and map.dim() == 3 and map.element_size() in (1, 2, 4)):
            raise ValueError("map: a CUDA tensor [P, mh, mw] of a 1-, 2- or 4-byte dtype")
        keys = self._window_keys(window, frames)
        src = int(src)
        group = [i for i, k in enumerate(keys) if k[0] == keys[src][0]]
        slot = {f: i for i, f in enumerate(group)}
        levels, unreachable = propagate_plan(self.carry_refs(window), keys, src)
        F, e = len(group), map.element_size()
        per = int(map.numel())
        pitch = (per * e + 3) // 4 * 4 // e          # elements from slot to slot: a map's bytes rounded up to a multiple of 4
        maps = torch.empty((F, pitch), dtype=map.dtype, device=dev)[:, :per].view((F,) + tuple(map.shape))          # (contiguous where per * e is one)
        self._propagate_check(maps, stride)
        via = torch.zeros((F,) + tuple(map.shape[1:]), dtype=torch.uint8, device=dev)
        status = torch.zeros(F, dtype=torch.int32, device=dev)
        maps[slot[src]] = map
        via[slot[src]] = 3
        if unreachable:          # (fills by value: nothing goes up)
            word = _fill_element(fill, e)
            bits = maps.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[e])          # (the same element size: the strides stay)
            for u in unreachable:
                bits[slot[u]].fill_(word)
                status[slot[u]].fill_(REGION_NO_REFERENCE)
        flat = [(t, slot[t], slot.get(f, -1), slot.get(b, -1), 0, 0, 0, 0) for hops in levels for (t, f, b) in hops]
        if not flat:
            return maps, via, status
        hops_dev = torch.tensor(flat, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)          # (one upload for all levels, from pinned memory: queued, not waited for)
        rows = hops_dev[:, 1].to(torch.int64)
        status_hops = torch.empty(len(flat), dtype=torch.int32, device=dev)
        cells = int(map.shape[1]) * int(map.shape[2])
        starts, total = [], 0          # each level's via maps start on a 4-byte boundary of one buffer
        for hops in levels:
            starts.append(total)
            total += (len(hops) * cells + 3) // 4 * 4
        via_hops = torch.empty(total, dtype=torch.uint8, device=dev)
        first = 0
        for hops, at in zip(levels, starts):
            stop = first + len(hops)
            v = via_hops[at:at + len(hops) * cells]
            self.propagate_maps_device(window, maps, hops_dev[first:stop], stride, fill=fill, via=v, status=status_hops[first:stop])
            via[rows[first:stop]] = v.view((len(hops),) + tuple(map.shape[1:]))
            first = stop
        status[rows] = status_hops
        return maps, via, status

    def _accumulate_parts(self, parts):
        """the parts of a call: None is every part the pipeline's outputs allow"""
        _need_output(self.motion_layout, "motion")
        if parts is None:
            return ACCUMULATE_MOTION | (ACCUMULATE_RESIDUAL if self.residual_layout is not None else 0)
        return int(parts)

    def accumulate_layout(self, parts=None):
        """accumulate_layout of the pipeline's coded size"""
        return accumulate_layout(self.info.coded_width, self.info.coded_height, self._accumulate_parts(parts))

    def accumulate(self, window, slots, hops, parts=None, via_fill=0):
        """leon_pipeline_accumulate: slots = a uint8 numpy array [S, pitch] of accumulators in host memory (accumulate_layout says where
        the planes lie, accumulate_views takes it apart), WRITTEN IN PLACE; hops = [(target, dst_slot, fwd_slot, bwd_slot), ...]: each
        writes slot dst_slot, the accumulator of window frame `target`, as a gather through the target's motion record from the slots
        fwd_slot / bwd_slot (-1: not supplied) plus what the hop itself adds -- accumulate_hop states it.  Returns (via [n, mbh, mbw] uint8,
        status [n] int32); a hop's fault is its status word, never a LeonError, and its slot and via keep what they held.  Synchronous."""
        parts = self._accumulate_parts(parts)
        h = _records_array(hops)
        mbw, mbh = self.info.coded_width // 16, self.info.coded_height // 16
        via, status = _result_arrays(len(h), ((mbh, mbw), via_fill, np.uint8), ((), 0, np.int32))
        cfg = _accumulate_config(slots, parts)
        _chk(self.lib.leon_pipeline_accumulate(self.h, int(window), C.byref(cfg), h.ctypes.data if len(h) else None, len(h), slots.ctypes.data, via.ctypes.data,
                                               status.ctypes.data))
        return via[:len(h)], status[:len(h)]

    def accumulate_device(self, window, slots, hops, parts=None, via=None, status=None, stream=None):
        """leon_pipeline_accumulate_device: the same hops with everything in DEVICE memory -- slots a contiguous CUDA uint8 tensor [S, pitch]
        (pitch a multiple of 4 not below the layout's slot_bytes), written in place; hops a contiguous
        CUDA int32 tensor [N, 8] -- queued on `stream` (a torch.cuda.Stream; None: torch's current stream) with
        propagate_maps_device's ordering: NO host synchronisation.  Returns (via [N, mbh, mbw] uint8, status [N] int32) on the device
        (the caller's, or ones the method allocates, not initialised).  Hops of one call must not name another hop's dst_slot: chain
        the levels of propagate_plan in calls of their own."""
        import torch
        parts = self._accumulate_parts(parts)
        dev = self.device_id
        if not (isinstance(slots, torch.Tensor) and slots.is_cuda and slots.dtype == torch.uint8 and slots.dim() == 2 and slots.is_contiguous()):
            raise ValueError("slots: a contiguous CUDA uint8 tensor [S, pitch]")
        _device_records_check("hops", hops)
        mbw, mbh = self.info.coded_width // 16, self.info.coded_height // 16
        n, cells = int(hops.shape[0]), mbw * mbh
        for name, t, dtype, count in (("slots", slots, torch.uint8, 0), ("hops", hops, torch.int32, 0), ("via", via, torch.uint8, n * cells), ("status", status, torch.int32, n)):
            _device_tensor_check(name, t, dtype, count, dev)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        via, status = _empty_where_none(stream, dev, [(via, (max(1, n), mbh, mbw), torch.uint8), (status, max(1, n), torch.int32)])
        S, pitch = int(slots.shape[0]), int(slots.shape[1])
        cfg = PipelineAccumulateConfig(parts, S, (C.c_int32 * 2)(0, 0), pitch, S * pitch)
        call = PipelineAccumulateCall(hops.data_ptr() if n else None, n, 0, slots.data_ptr(), via.data_ptr(), status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_accumulate_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return via.view(-1)[:n * cells].view(n, mbh, mbw), status.view(-1)[:n]

    def accumulate_gop(self, window, src, parts=None, frames=None):
        """Motion and residual accumulated from window frame `src` to every delivered frame of its GOP in the window: `src` is written
        as a restart (a hop with both sources -1: all zero), then one accumulate_device call per level of propagate_plan on torch's
        current stream; all levels' hop records go up in one upload from pinned memory in front of the first launch, queued like the
        launches: nothing waits for the device.  parts: None is every part the pipeline's outputs allow.
        Returns a dict of strided int16 CUDA views over the F frames gop_frames(window, src) lists -- AX, AY, AGE, RY [F, ch, cw], RCb, RCr
        [F, ch / 2, cw / 2], whichever the parts hold --, "via" [F, mbh, mbw] uint8 and "status" [F] int32, with "slots" (the uint8
        [F, slot_pitch] buffer the views lie in, as accumulate_device takes it) and "layout" (accumulate_layout's).  A frame no chain of
        predictions reaches from `src` is all zero, via 0, status REGION_NO_REFERENCE.  frames: the window's frames when the pipeline
        did not see them delivered."""
        import torch
        parts = self._accumulate_parts(parts)
        dev = "cuda:%d" % self.device_id
        lay = accumulate_layout(self.info.coded_width, self.info.coded_height, parts)
        keys = self._window_keys(window, frames)
        src = int(src)
        group = [i for i, k in enumerate(keys) if k[0] == keys[src][0]]
        slot = {f: i for i, f in enumerate(group)}
        levels, unreachable = propagate_plan(self.carry_refs(window), keys, src)
        F, mbw, mbh = len(group), lay.coded_width // 16, lay.coded_height // 16
        slots = torch.empty((F, lay.slot_pitch), dtype=torch.uint8, device=dev)
        for u in unreachable:
            slots[slot[u]].zero_()
        levels = [[(src, -1, -1)]] + levels          # the chain's start: a restart
        flat = [(t, slot[t], slot.get(f, -1), slot.get(b, -1), 0, 0, 0, 0) for hops in levels for (t, f, b) in hops]
        hops_dev = torch.tensor(flat, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)          # (one upload for all levels, from pinned memory: queued, not waited for)
        rows = hops_dev[:, 1].to(torch.int64)
        via = torch.zeros((F, mbh, mbw), dtype=torch.uint8, device=dev)
        status = torch.zeros(F, dtype=torch.int32, device=dev)
        if unreachable:
            status[torch.tensor([slot[u] for u in unreachable], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)] = REGION_NO_REFERENCE
        via_hops = torch.empty((len(flat), mbh, mbw), dtype=torch.uint8, device=dev)
        status_hops = torch.empty(len(flat), dtype=torch.int32, device=dev)
        first = 0
        for hops in levels:
            stop = first + len(hops)
            self.accumulate_device(window, slots, hops_dev[first:stop], parts, via=via_hops[first:stop], status=status_hops[first:stop])
            first = stop
        via[rows] = via_hops
        status[rows] = status_hops
        out = {"via": via, "status": status, "slots": slots, "layout": lay}
        flat16 = slots.view(torch.int16)          # [F, slot_pitch / 2]
        cw, ch = lay.coded_width, lay.coded_height
        for name in accumulate_names(parts):
            chroma = name in ("RCb", "RCr")
            h, w, stride = (ch // 2, cw // 2, lay.chroma_stride) if chroma else (ch, cw, lay.luma_stride)
            off = getattr(lay, name.lower() + "_offset") // 2
            out[name] = flat16[:, off:off + h * stride].view(F, h, stride)[:, :, :w]
        return out

    def _field_source(self, source, buffer):
        """(source code, n_items, item_pitch, source_bytes) of a field tensors call; buffer: a uint8 array or CUDA tensor [n_items, item_pitch]"""
        source = FIELD_SOURCES[source] if isinstance(source, str) else int(source)
        if source == FIELD_SOURCE_MOTION:
            _need_output(self.motion_layout, "motion")
        if source == FIELD_SOURCE_RESIDUAL:
            _need_output(self.residual_layout, "residual")
        if (source == FIELD_SOURCE_BUFFER) != (buffer is not None):
            raise ValueError("buffer: the items of source=\"buffer\", and of no other source")
        if buffer is None:
            return source, 0, 0, 0
        if buffer.dtype != (np.uint8 if isinstance(buffer, np.ndarray) else __import__("torch").uint8) or len(buffer.shape) != 2:
            raise ValueError("buffer: uint8 [n_items, item_pitch]")
        return source, int(buffer.shape[0]), int(buffer.shape[1]), int(buffer.shape[0]) * int(buffer.shape[1])

    @staticmethod
    def _field_bytes(channels, size, dtype, pitch):
        nbytes = len(channels) * int(size[0]) * int(size[1]) * np.dtype(FIELD_NP_DTYPES[dtype]).itemsize
        return nbytes, (-(-nbytes // 256) * 256 if pitch is None else int(pitch))

    def field_tensors_device(self, window, records, size, channels, source="buffer", buffer=None, dtype="float16", out=None, status=None, stream=None, pitch=None):
        """leon_pipeline_field_tensors_device: boxes of int16 fields resampled into one [N, C, h, w] batch of `dtype` ("float16",
        "bfloat16", "float32"), cropped by the same records and through the same tables as resample_regions_device's pixel tensors, so
        the two line up sample for sample.  records: a contiguous CUDA int32 tensor [N, 8] (leon_pipeline_region records: frame, x, y, w,
        h, 0, 0, 0) or stacked [F, N, 8], as carry_regions_gop and propose_regions_device write them; size = (h, w); channels =
        [field_channel(...), ...] (field_channels_motion / _residual / _accumulate build them); source: "motion" / "residual" -- the
        window frame's record -- or "buffer" with buffer = a contiguous CUDA uint8 tensor [n_items, item_pitch], a record's `frame`
        word being the item index (the window is not consulted then).  Queued on `stream` (None: torch's current stream) with
        resample_regions_device's ordering: NO host synchronisation.  Returns (batch [N, C, h, w] view over `out` -- a uint8 tensor,
        256-byte aligned, regions `pitch` bytes apart (None: a region's bytes rounded up to 256), or one the method allocates, not
        initialised --, status [N] int32: REGION_* per record; a refused record's tensor is untouched)."""
        import torch
        dev = self.device_id
        src, n_items, item_pitch, source_bytes = self._field_source(source, buffer)
        _device_records_check("records", records, stacked=True)
        records = records.view(-1, 8)
        n = int(records.shape[0])
        if buffer is not None and not (isinstance(buffer, torch.Tensor) and buffer.is_contiguous()):
            raise ValueError("buffer: a contiguous CUDA uint8 tensor [n_items, item_pitch]")
        nbytes, step = self._field_bytes(channels, size, dtype, pitch)
        for name, t, dt, count in (("records", records, torch.int32, 0), ("buffer", buffer, torch.uint8, 0), ("out", out, torch.uint8, (n - 1) * step + nbytes),
                                   ("status", status, torch.int32, n)):
            _device_tensor_check(name, t, dt, count, dev)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        out, status = _empty_where_none(stream, dev, [(out, max(1, n) * max(step, 1), torch.uint8), (status, max(1, n), torch.int32)])
        cfg = _field_config(src, dtype, size, channels, n_items, item_pitch, source_bytes)
        call = PipelineFieldTensorsCall(records.data_ptr() if n else None, n, 0, buffer.data_ptr() if buffer is not None else None, out.data_ptr(), 0 if pitch is None else step,
                                        status.data_ptr(), self._stream_handle(stream), 0)
        _chk(self.lib.leon_pipeline_field_tensors_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        tdt = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[dtype]
        oh, ow = int(size[0]), int(size[1])
        e = nbytes // max(1, len(channels) * oh * ow)
        batch = torch.as_strided(out.view(tdt), (n, len(channels), oh, ow), (step // e, oh * ow, ow, 1))
        return batch, status.view(-1)[:n]

    def field_tensors(self, window, records, size, channels, source="buffer", buffer=None, dtype="float16", pitch=None, fill=0, status_fill=0):
        """leon_pipeline_field_tensors: the same call from host arrays, synchronous -- records = [(frame, x, y, w, h), ...], buffer a uint8
        numpy array [n_items, item_pitch].  Returns (batch [N, C, h, w] of FIELD_NP_DTYPES[dtype] -- bfloat16 as uint16 bit patterns --
        over a buffer pre-filled with the byte `fill`, which a refused record's tensor still holds, status [N] int32)."""
        src, n_items, item_pitch, source_bytes = self._field_source(source, buffer)
        r = _records_array(records)
        nbytes, step = self._field_bytes(channels, size, dtype, pitch)
        out = np.full((max(1, len(r)), max(step, 1)), fill, dtype=np.uint8)
        st, = _result_arrays(len(r), ((), status_fill, np.int32))
        cfg = _field_config(src, dtype, size, channels, n_items, item_pitch, source_bytes)
        _chk(self.lib.leon_pipeline_field_tensors(self.h, int(window), C.byref(cfg), r.ctypes.data if len(r) else None, len(r),
                                                  _field_items(buffer).ctypes.data if buffer is not None else None, out.ctypes.data, 0 if pitch is None else step, st.ctypes.data))
        return field_batch(out[:len(r)], len(channels), size, dtype), st[:len(r)]

    def motion_tensors(self, window, records, size, channels=("fwd_h", "fwd_v"), scale=1.0, bias=0.0, **kw):
        """field_tensors_device on the window frames' motion records: the vectors named (MOTION_FIELDS) as [N, C, h, w].  Vectors are in
        HALF-PEL FRAME units and the call does not rescale them by the resize ratio: scale = 0.5 * out_size / box_size gives output
        pixels for boxes of one size (one value, or one a channel)."""
        return self.field_tensors_device(window, records, size, field_channels_motion(self.info.coded_width // 16, channels, scale, bias), source="motion", **kw)

    def residual_tensors(self, window, records, size, channels=("Y", "Cb", "Cr"), scale=1.0, bias=0.0, **kw):
        """field_tensors_device on the window frames' residual records: Y, Cb, Cr (chroma replicated to the frame's size) as [N, C, h, w];
        they stay YCbCr differences"""
        return self.field_tensors_device(window, records, size, field_channels_residual(_need_output(self.residual_layout, "residual"), channels, scale, bias),
                                         source="residual", **kw)

    def accumulate_tensors(self, acc, records, size, names=("AX", "AY"), scale=1.0, bias=0.0, **kw):
        """field_tensors_device on accumulate_gop's dict `acc`: the planes named as [N, C, h, w].  A record's `frame` word is the position
        in gop_frames(window, src), the row of acc's planes.  AX and AY are in FRAME PIXELS: scale = out_size / box_size gives output
        pixels."""
        return self.field_tensors_device(-1, records, size, field_channels_accumulate(acc["layout"], names, scale, bias), source="buffer", buffer=acc["slots"], **kw)

    def read_frame(self, frame):
        out = np.empty((self.info.frame_height, self.info.frame_width, 4), dtype=np.uint8)
        _chk(self.lib.leon_pipeline_read_frame(self.h, C.byref(frame["_frames"][frame["_i"]]), out.ctypes.data))
        return out

    def read_planes(self, frame):
        """the frame's planes as packed host arrays: (y, cb, cr), and a for a yuva stream"""
        i = self.info
        y = np.empty((i.frame_height, i.frame_width), dtype=np.uint8)
        cb = np.empty((i.chroma_height, i.chroma_width), dtype=np.uint8)
        cr = np.empty_like(cb)
        a = np.empty_like(y) if frame["a"] else None
        _chk(self.lib.leon_pipeline_read_frame_planes(self.h, C.byref(frame["_frames"][frame["_i"]]), y.ctypes.data, cb.ctypes.data,
                                                      cr.ctypes.data, None if a is None else a.ctypes.data))
        return (y, cb, cr) if a is None else (y, cb, cr, a)

    def _tensor_np_dtype(self):
        return {TENSOR_F16: np.float16, TENSOR_BF16: np.uint16, TENSOR_F32: np.float32, TENSOR_U8: np.uint8}[self.info.tensor_dtype]

    def _tensor_dims(self):
        """(shape, strides in bytes) of one tensor in the pipeline's layout: [3, H, W] or [H, W, 3]"""
        t = self.tensor_shape
        e = t.element_bytes
        if t.layout == TENSOR_LAYOUT_HWC:
            return (t.height, t.width, t.channels), (t.stride_y * e, t.stride_x * e, t.stride_c * e)
        return (t.channels, t.height, t.width), (t.stride_c * e, t.stride_y * e, t.stride_x * e)

    def read_tensor(self, frame):
        """the frame's tensor as a host array [3, height, width] ([height, width, 3] with tensor_layout "hwc"; tensor_geometry: the
        frame's size, or tensor_size): float16 / float32 / uint8, bfloat16 as uint16 bit patterns"""
        if not frame.get("tensor"):
            raise LeonError(ERR_INVALID, "the frame has no tensor (Pipeline output)")
        out = np.empty(self._tensor_dims()[0], dtype=self._tensor_np_dtype())
        _chk(self.lib.leon_pipeline_read_tensor(self.h, frame["_window"], frame["_i"], out.ctypes.data))
        return out

    def region_bytes(self, size):
        """(bytes of one region's tensor, the default pitch between regions: the bytes rounded up to 256)"""
        n = 3 * int(size[0]) * int(size[1]) * self.info.tensor_element_bytes
        return n, (n + 255) // 256 * 256

    def _region_dims(self, size):
        """(shape, strides in bytes) of one region's tensor in the pipeline's layout"""
        h, w, e = int(size[0]), int(size[1]), self.info.tensor_element_bytes
        if self.tensor_shape.layout == TENSOR_LAYOUT_HWC:
            return (h, w, 3), (3 * w * e, 3 * e, e)
        return (3, h, w), (h * w * e, w * e, e)

    def _need_tensors(self):
        if not self.info.tensor_dtype:
            raise LeonError(ERR_INVALID, "the pipeline has no tensor output (Pipeline output)")

    def _regions_out(self, out, n, size, pitch, dev):
        """(out, step): the caller's uint8 buffer, checked, or one allocated for n regions of `size` every `step` = pitch bytes (None: the default)"""
        import torch
        nbytes, dflt = self.region_bytes(size)
        step = dflt if pitch is None else int(pitch)
        if out is None:
            out = torch.empty(max(1, n) * max(step, 1), dtype=torch.uint8, device="cuda:%d" % dev)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < (n - 1) * step + nbytes:
            raise ValueError("out: a contiguous uint8 tensor of at least %d bytes" % ((n - 1) * step + nbytes))
        return out, step

    def _regions_status(self, status, n, dev):
        """the caller's int32 status tensor, checked, or one allocated for n regions"""
        import torch
        if status is None:
            return torch.empty(max(1, n), dtype=torch.int32, device="cuda:%d" % dev)
        if status.dtype != torch.int32 or not status.is_contiguous() or status.numel() < n:
            raise ValueError("status: a contiguous int32 tensor of at least %d words" % n)
        return status

    @staticmethod
    def _stream_handle(stream):
        """the handle the library queues on; torch's legacy default stream has none: waited for here, and the call then waits for its work"""
        handle = int(stream.cuda_stream)
        if not handle:
            stream.synchronize()
        return handle or None

    def _regions_batch(self, out, n, size, step, dev):
        """the view [N, 3, h, w] ("hwc": [N, h, w, 3]) over `out`, regions `step` bytes apart"""
        shape, strides = self._region_dims(size)
        return self._tensor_at(out.data_ptr(), (n,) + shape, (step,) + strides, dev, owner=out)

    def resample_regions(self, window, regions, size, filter="triangle", out=None, pitch=None, device_id=None, fit=None, anchor=None, pad_value=None):
        """leon_pipeline_resample_regions: regions = [(frame_index, x, y, w, h), ...] of the delivered, not yet released `window`
        (frame["_i"] is the index) resampled to size = (h, w) -> a torch view [N, 3, h, w] ("hwc": [N, h, w, 3]) of the pipeline's
        element type, regions `pitch` bytes apart (None: the region's bytes rounded up to 256 -- dense when they are a multiple of
        256, as 224 x 224 is in every element type).  The view lies over a uint8 buffer the method allocates, or over `out`: a torch
        uint8 tensor on the device, 256-byte aligned, of at least (N - 1) * pitch + the region's bytes.  Synchronous: the batch is
        complete when the method returns.  Raises LeonError where the library refuses; nothing is written then.
        fit="letterbox": every box keeps its aspect ratio inside the (h, w) tensor -- centred, or at the top left with
        anchor="top_left" -- and the rest is pad_value = (r, g, b) through the element table (leon_pipeline_regions_fit;
        region_fit_rect says where the image lies).  Without the three keywords the call is the one it always was."""
        import torch
        self._need_tensors()
        arr, n, cfg = _regions_args(regions, size, filter)
        dev = self.device_id if device_id is None else device_id
        out, step = self._regions_out(out, n, size, pitch, dev)
        # the library writes on a stream of its own: what torch has queued for this memory (a fill, an earlier owner's kernels) goes first
        torch.cuda.current_stream(dev).synchronize()
        f = _regions_fit(fit, anchor, pad_value)
        if f is None:
            _chk(self.lib.leon_pipeline_resample_regions(self.h, int(window), arr, n, C.byref(cfg), out.data_ptr(), 0 if pitch is None else step))
        else:
            _chk(self.lib.leon_pipeline_resample_regions_fit(self.h, int(window), arr, n, C.byref(cfg), C.byref(f), out.data_ptr(), 0 if pitch is None else step))
        return self._regions_batch(out, n, size, step, dev)

    def resample_regions_device(self, window, boxes, size, filter="triangle", out=None, pitch=None, status=None, stream=None, scratch_limit=None,
                                fit=None, anchor=None, pad_value=None, rects=None):
        """leon_pipeline_resample_regions_device: the same batch from boxes that lie in DEVICE memory -- a CUDA int32 torch tensor,
        [N, 8] contiguous (leon_pipeline_region records) or [N, 5] (frame_index, x, y, w, h; padded to records on the device) -- queued on
        `stream` (a torch.cuda.Stream; None: torch's current stream of the pipeline's device, where boxes, out and status must lie) behind whatever made the boxes there and in front of
        whatever reads the result there: NO host synchronisation, the batch and the status words are complete when the stream gets
        there.  Returns (the batch view as resample_regions builds it, status): status an int32 tensor [N] on the device (`status`, or
        one the method allocates), REGION_* per box -- 0: resampled; otherwise the region was skipped and its bytes of `out` are
        untouched (the method's own buffer is not initialised).  The window must stay unreleased and the pipeline open until the
        stream has run the work.  scratch_limit: bytes of table scratch a chunk of regions may take (None: 256 MiB).  torch's legacy
        default stream has no handle the library could queue on: there the method waits for the stream, and the call for its work.
        fit / anchor / pad_value: as resample_regions; a box that is refused letterboxed has nothing written, pad included.  rects
        (letterbox only): an int32 tensor of at least [N, 4] words on the device, or True for one the method allocates -- the call
        then returns (batch, status, rects), rects[i] = (x, y, width, height) of region i's image for every status-0 region, the
        others' words untouched."""
        import torch
        self._need_tensors()
        dev = self.device_id
        if not (isinstance(boxes, torch.Tensor) and boxes.is_cuda and boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] in (5, 8)):
            raise ValueError("boxes: a CUDA int32 tensor [N, 8] (records) or [N, 5] (frame, x, y, w, h)")
        want_rects = rects is not None and rects is not False
        if rects is True:
            rects = None
        for name, t in (("boxes", boxes), ("out", out), ("status", status), ("rects", rects)):
            _device_tensor_check(name, t, None, 0, dev)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        n = int(boxes.shape[0])
        cfg = size if isinstance(size, PipelineRegionsConfig) else PipelineRegionsConfig(int(size[1]), int(size[0]), _resize_filter_code(filter))
        with torch.cuda.stream(stream):
            if boxes.shape[1] == 5:
                boxes = torch.nn.functional.pad(boxes, (0, 3))
            elif not boxes.is_contiguous():
                raise ValueError("boxes: [N, 8] records must be contiguous")
            out, step = self._regions_out(out, n, (cfg.out_height, cfg.out_width), pitch, dev)
            status = self._regions_status(status, n, dev)
            if want_rects:
                _device_tensor_check("rects", rects, torch.int32, 4 * n, dev, words=True)
                rects, = _empty_where_none(stream, dev, [(rects, (max(1, n), 4), torch.int32)])
        call = PipelineRegionsDevice(boxes.data_ptr() if n else None, n, 0, out.data_ptr(), 0 if pitch is None else step, status.data_ptr(), self._stream_handle(stream),
                                     0 if scratch_limit is None else int(scratch_limit))
        f = _regions_fit(fit, anchor, pad_value)
        if f is None and not want_rects:
            _chk(self.lib.leon_pipeline_resample_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        else:
            _chk(self.lib.leon_pipeline_resample_regions_device_fit(self.h, int(window), C.byref(cfg), _fit_ref(f), C.byref(call), rects.data_ptr() if want_rects else None))
        batch = self._regions_batch(out, n, (cfg.out_height, cfg.out_width), step, dev)
        return (batch, status[:n], rects.view(-1)[:4 * n].view(n, 4)) if want_rects else (batch, status[:n])

    def read_regions(self, window, regions, size, filter="triangle", fit=None, anchor=None, pad_value=None):
        """leon_pipeline_read_regions: the same regions as a host array [N, 3, h, w] ("hwc": [N, h, w, 3]), packed: float16 / float32 /
        uint8, bfloat16 as uint16 bit patterns like read_tensor; fit, anchor, pad_value as resample_regions"""
        self._need_tensors()
        arr, n, cfg = _regions_args(regions, size, filter)
        out = np.empty((max(1, n),) + self._region_dims(size)[0], dtype=self._tensor_np_dtype())
        f = _regions_fit(fit, anchor, pad_value)
        if f is None:
            _chk(self.lib.leon_pipeline_read_regions(self.h, int(window), arr, n, C.byref(cfg), out.ctypes.data))
        else:
            _chk(self.lib.leon_pipeline_read_regions_fit(self.h, int(window), arr, n, C.byref(cfg), C.byref(f), out.ctypes.data))
        return out[:n]

    def warp_regions(self, window, regions, size, pad_value=None, out=None, pitch=None):
        """leon_pipeline_warp_regions: regions = [(frame_index, m), ...], m the six Q16 words of warp_matrix / warp_matrix_rotated_box,
        of the delivered, not yet released `window` sampled along their affine maps into size = (h, w) -> a torch view [N, 3, h, w]
        ("hwc": [N, h, w, 3]) as resample_regions builds it; out and pitch as there.  Positions outside the frame read pad_value =
        (r, g, b) through the element table.  Synchronous.  Raises LeonError where the library refuses; nothing is written then."""
        import torch
        self._need_tensors()
        arr, n, cfg = _warp_args(regions, size, pad_value)
        dev = self.device_id
        out, step = self._regions_out(out, n, (cfg.out_height, cfg.out_width), pitch, dev)
        torch.cuda.current_stream(dev).synchronize()          # (the library writes on a stream of its own: resample_regions)
        _chk(self.lib.leon_pipeline_warp_regions(self.h, int(window), arr, n, C.byref(cfg), out.data_ptr(), 0 if pitch is None else step))
        return self._regions_batch(out, n, (cfg.out_height, cfg.out_width), step, dev)

    def read_warp_regions(self, window, regions, size, pad_value=None):
        """leon_pipeline_read_warp_regions: the same regions as a host array [N, 3, h, w] ("hwc": [N, h, w, 3]), packed, as read_regions"""
        self._need_tensors()
        arr, n, cfg = _warp_args(regions, size, pad_value)
        out = np.empty((max(1, n),) + self._region_dims((cfg.out_height, cfg.out_width))[0], dtype=self._tensor_np_dtype())
        _chk(self.lib.leon_pipeline_read_warp_regions(self.h, int(window), arr, n, C.byref(cfg), out.ctypes.data))
        return out[:n]

    def warp_regions_device(self, window, records, size, pad_value=None, out=None, pitch=None, status=None, stream=None):
        """leon_pipeline_warp_regions_device: the same batch from records that lie in DEVICE memory -- a contiguous CUDA int32 torch
        tensor [N, 8]: frame, a00, a01, tx, a10, a11, ty (Q16), 0 -- queued on `stream` (a torch.cuda.Stream; None: torch's current
        stream) with resample_regions_device's ordering: NO host synchronisation.  Returns (batch, status): status an int32 tensor [N]
        on the device, REGION_* per record -- 0: written; otherwise the region was skipped and its bytes of `out` are untouched."""
        import torch
        self._need_tensors()
        dev = self.device_id
        _device_records_check("records", records)
        for name, t in (("records", records), ("out", out), ("status", status)):
            _device_tensor_check(name, t, None, 0, dev)
        stream = torch.cuda.current_stream(dev) if stream is None else stream
        n = int(records.shape[0])
        cfg = _warp_config(size, pad_value)
        with torch.cuda.stream(stream):
            out, step = self._regions_out(out, n, (cfg.out_height, cfg.out_width), pitch, dev)
            status = self._regions_status(status, n, dev)
        call = PipelineWarpRegionsCall(records.data_ptr() if n else None, n, 0, out.data_ptr(), 0 if pitch is None else step, status.data_ptr(), self._stream_handle(stream))
        _chk(self.lib.leon_pipeline_warp_regions_device(self.h, int(window), C.byref(cfg), C.byref(call)))
        return self._regions_batch(out, n, (cfg.out_height, cfg.out_width), step, dev), status[:n]

    def _tensor_at(self, ptr, shape, strides, device_id=None, owner=None):
        import torch
        dt = self.info.tensor_dtype
        t = _cuda_view(ptr, shape, {TENSOR_F32: "<f4", TENSOR_F16: "<f2", TENSOR_BF16: "<i2", TENSOR_U8: "|u1"}[dt], strides,
                       self.device_id if device_id is None else device_id, owner)
        return t.view(torch.bfloat16) if dt == TENSOR_BF16 else t

    def tensor_view(self, frame, device_id=None):
        """the frame's tensor where it lies, as a torch [3, H, W] ("hwc": [H, W, 3]) tensor of the pipeline's element type, without
        copying: valid until the frame's window is released"""
        if not frame.get("tensor"):
            raise ValueError("the frame has no tensor (Pipeline output)")
        shape, strides = self._tensor_dims()
        return self._tensor_at(frame["tensor"], shape, strides, device_id)

    def window_tensor(self, frames, device_id=None):
        """frames of one window (in order) as ONE strided torch view [N, 3, H, W] ("hwc": [N, H, W, 3]) when their tensors are evenly spaced in the
        ring -- consecutive display positions of a GOP are tensor_frame_pitch apart --, else None"""
        ptrs = [f.get("tensor") for f in frames]
        if not ptrs or not all(ptrs):
            return None
        step = ptrs[1] - ptrs[0] if len(ptrs) > 1 else self.info.tensor_frame_pitch
        i = self.info
        e = i.tensor_element_bytes
        if step <= 0 or step % e or step < i.tensor_frame_bytes or any(b - a != step for a, b in zip(ptrs, ptrs[1:])):
            return None
        shape, strides = self._tensor_dims()
        return self._tensor_at(ptrs[0], (len(ptrs),) + shape, (step,) + strides, device_id)

    def plane_views(self, frame, device_id=None):
        """the frame's planes where they lie, as torch uint8 tensors (height x width, row stride = the plane's padded stride),
        without copying: valid until the frame's window is released"""
        i = self.info
        dev = self.device_id if device_id is None else device_id
        views = [plane_view(frame["y"], i.frame_height, i.frame_width, i.luma_stride, dev),
                 plane_view(frame["cb"], i.chroma_height, i.chroma_width, i.chroma_stride, dev),
                 plane_view(frame["cr"], i.chroma_height, i.chroma_width, i.chroma_stride, dev)]
        if frame["a"]:
            views.append(plane_view(frame["a"], i.frame_height, i.frame_width, i.luma_stride, dev))
        return tuple(views)

    def feed(self, valid_bytes, chunk=None, offset=None):
        """more of the stream has arrived: optionally copy `chunk` to `offset` of the pipeline's buffer first"""
        if chunk is not None:
            if offset is None:
                raise ValueError("feed(chunk=...) needs the offset the chunk belongs at")
            offset, chunk = int(offset), bytes(chunk)
            if offset < 0 or offset + len(chunk) > len(self._data):
                raise ValueError("chunk of %d bytes at offset %d does not fit the stream buffer of %d bytes" % (len(chunk), offset, len(self._data)))
            C.memmove(C.addressof(self._data) + offset, chunk, len(chunk))
        _chk(self.lib.leon_pipeline_feed(self.h, int(valid_bytes)))

    def release_window(self, window):
        self._window_n.pop(window, None)
        _chk(self.lib.leon_pipeline_release_window(self.h, window))

    def seek(self, seconds, exact=False, mode=None):
        """leon_pipeline_seek: move the running pipeline to `seconds` (the key-map entry at or before it; exact: from
        the frame on screen at it).  Returns the id of the new position's first window: no callback starts for a
        window below it once this returns.  Restarts a run that has ended; `ended` / wait() describe the new run.
        `mode` overrides `exact` with a raw mode value.  Raises LeonError when the pipeline refuses."""
        if mode is None:
            mode = PIPELINE_SEEK_EXACT if exact else PIPELINE_SEEK_KEY
        first = C.c_int64()
        was = self.ended
        self.ended = False
        rc = self.lib.leon_pipeline_seek(self.h, float(seconds), int(mode), C.byref(first))
        if rc != OK:
            self.ended = was
            raise LeonError(rc, self.lib.leon_last_error().decode())
        info = PipelineInfo()
        _chk(self.lib.leon_pipeline_get_info(self.h, C.byref(info)))      # first_gop / shard_gops of the new position
        self.info = info
        return first.value

    def wait(self):
        _chk(self.lib.leon_pipeline_wait(self.h))
        if isinstance(self.error, Exception):
            raise self.error

    def stats(self):
        s = PipelineStats()
        _chk(self.lib.leon_pipeline_get_stats(self.h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in PipelineStats._fields_}

    def close(self):
        if self.h:
            self._ready.set()
            self.lib.leon_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pool_stats():
    """leon_device_pool_stats: contiguous memory this process holds (never returned to the driver), how much is handed out"""
    held, used, seg = C.c_uint64(), C.c_uint64(), C.c_int32()
    _chk(load().leon_device_pool_stats(C.byref(held), C.byref(used), C.byref(seg)))
    return {"held_bytes": held.value, "in_use_bytes": used.value, "segments": seg.value}


def _cuda_view(ptr, shape, typestr, strides, device_id, owner=None):
    """device memory at `ptr` as a torch tensor of `shape` and `typestr` with byte `strides`, without copying (Pipeline.motion_view,
    activity_view and the tensor views).  owner: an object the tensor keeps alive, and with it the memory"""
    import torch

    class _View:
        pass
    v = _View()
    v.owner = owner          # torch.as_tensor keeps this object alive
    v.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "strides": tuple(int(x) for x in strides), "version": 2}
    return torch.as_tensor(v, device="cuda:%d" % device_id)


def device_view(ptr, nbytes, device_id=0):
    """`nbytes` of device memory at `ptr` as a torch uint8 tensor, without copying (the memory must outlive the tensor):
    how bench.py and the tests checksum the pipeline's frames where they lie"""
    import torch

    class _View:
        pass
    v = _View()
    v.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(v, device="cuda:%d" % device_id)


def plane_view(ptr, height, width, stride, device_id=0):
    """a height x width uint8 plane with rows `stride` bytes apart at device address `ptr`, as a torch tensor without copying"""
    import torch

    if not ptr:
        raise ValueError("the frame has no such plane (Pipeline output)")

    class _View:
        pass
    v = _View()
    v.__cuda_array_interface__ = {"shape": (int(height), int(width)), "typestr": "|u1", "data": (int(ptr), False),
                                  "strides": (int(stride), 1), "version": 2}
    return torch.as_tensor(v, device="cuda:%d" % device_id)


class DeviceBuffer:
    """leon_device_malloc / leon_device_free: device memory allocated the way the library allocates its own large buffers
    (physically contiguous where the device grants it).  `ptr` is the device address; `contiguous` says which it got.
    as_tensor(dtype, shape) wraps (a part of) it as a torch tensor without copying -- the buffer must outlive the tensor
    (the tensor keeps a reference to it)."""

    def __init__(self, nbytes, device_id=0):
        self.lib = load()
        p, c = C.c_void_p(), C.c_int32(0)
        _chk(self.lib.leon_device_malloc(device_id, nbytes, C.byref(p), C.byref(c)))
        self.ptr, self.nbytes, self.contiguous, self.device_id = p.value, nbytes, bool(c.value), device_id

    def as_tensor(self, dtype, shape, offset=0):
        import numpy as np
        import torch
        typestr = {torch.uint8: "|u1", torch.int8: "|i1", torch.int16: "<i2", torch.int32: "<i4", torch.int64: "<i8",
                   torch.float32: "<f4", torch.float64: "<f8"}[dtype]
        n = int(np.prod(shape)) * int(typestr[2:])
        if offset < 0 or offset + n > self.nbytes:
            raise ValueError("tensor does not fit in the buffer")

        class _View:          # __cuda_array_interface__: torch.as_tensor wraps the memory and keeps this object (and the buffer) alive
            pass
        v = _View()
        v.owner = self
        v.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": typestr, "data": (self.ptr + offset, False), "version": 2}
        return torch.as_tensor(v, device="cuda:%d" % self.device_id)

    def free(self):
        if self.ptr:
            _chk(self.lib.leon_device_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
