/*
 * leon_pipeline.h -- native decode pipeline over libleon_vlc + libleon_hip (exported by libleon_hip.so).
 *
 * What it replaces in the reference: the page's decode loop -- decodeFrame() pulling one picture at
 * a time through the bit-serial parser and one IDCT_GL per picture, on the page's only thread
 * (decoders/jsv.js:426-469, :1593-1599, :1177-1336; player/easybits.player.js:2310-2324, :2543-2617).
 * Here the same stream bytes go through
 *     K parser threads   one libleon_vlc stream per GOP shard (cut at the key map, decoders/jsv.js:264-350;
 *                        GOPs share nothing but an open GOP's forward reference, see below), lists and maps written
 *                        straight into pinned memory
 *     one submit thread  a window of W consecutive GOPs at a time: one asynchronous upload per GOP, then ONE
 *                        kernel launch per picture type and dependency level ACROSS the window's GOPs, the
 *                        display conversion fused in (leon_picture.rgba_out); B pictures write no planes
 *     one notify thread  waits on the window's HIP event and calls back with the frames (RGBA8 in device
 *                        memory, display order) -- no caller thread ever blocks on the GPU
 * No interpreter is in the loop; a Node host learns of frames through a napi_threadsafe_function
 * (mpeg1video-decoder-webgl_amd/napi/leon_napi.cc), the MI355X-side of the reference's 'frame' event
 * (decoders/jsv.js:673).
 *
 * Requirements on the stream: JSV with a key map (or a raw elementary stream: one shard), ONE picture size
 * (a sequence header that changes the size ends the run with an error; one that changes the quantiser matrices -- the
 * reference reloads them at every header, decoders/jsv.js:540-558 -- is honoured per picture, round 4).  Any frame width:
 * widths that are no multiple of 8 take an unfused road inside (planes + one conversion launch per picture).
 *
 * Open GOPs.  A B picture in front of its GOP's second anchor (coded order) is a LEADING B picture.
 *   - In a GOP whose header says closed_gop = 1 both its references are the GOP's I picture (it predicts backward only).
 *   - In an open GOP (closed_gop = 0) its forward reference is the last anchor, in coded order, of the key-map GOP directly
 *     before it; its backward reference is its own GOP's I picture.
 *   - A GOP HAS ITS PREDECESSOR when the run decodes the key-map entry directly before it, in the same pass of `loop`, and
 *     the GOP's header does not set broken_link.  It has not when it is the first GOP of a run (the stream's start,
 *     start_seconds, the target of a KEY or EXACT seek), the first GOP of each further pass of `loop`, or a GOP with
 *     broken_link = 1.
 *   - The leading B pictures of an open GOP without its predecessor are NOT DECODED AND NOT DELIVERED: never launched, and
 *     with the GPU parser not parsed either (the host parser has read them with the rest of the GOP by then; what it
 *     wrote is uploaded with the GOP and not used).  The GOP's frames start at its I picture's display_index.  ISO 11172-2 prescribes that for broken_link,
 *     and it is what a player does after random access.  The host sees missing display positions, as with a GOP the
 *     encoder cut short; leon_pipeline_stats.pictures counts what was decoded.  LEON_PIPELINE_SEEK_EXACT drops them first
 *     and trims then: a target time on a dropped frame delivers from the I picture.
 *   - shard_count > 1: a shard never holds a GOP's neighbour, so an open GOP WITH leading B pictures ends the run with an
 *     error ("GOP shards must be closed"); nothing is dropped silently there.  Open GOPs without leading B pictures, and
 *     closed streams, shard as before.
 * (The reference ignores closed_gop and drops every B picture.)
 */
#ifndef LEON_PIPELINE_H
#define LEON_PIPELINE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct leon_pipeline leon_pipeline;

#define LEON_PIPELINE_PARSER_DEFAULT 0
#define LEON_PIPELINE_PARSER_GPU 1
#define LEON_PIPELINE_PARSER_HOST (-1)

/* leon_pipeline_config.output: a bit set; 0 = RGBA */
#define LEON_PIPELINE_OUTPUT_RGBA  1
#define LEON_PIPELINE_OUTPUT_YCBCR 2
/* Bit 4, not 2 or 3: create goes on refusing output = 4 and 8 (tests/test_pipeline_planes_gpu.py::test_refusals).  Written as a
 * shift: the decimal defines of this family are the RGBA / YCBCR pair tests/test_pipeline_planes_abi.py compares with its binding. */
#define LEON_PIPELINE_OUTPUT_TENSOR (1 << 4)
/* Bit 5: 4 and 8 stay refused as above, and so does every other unknown bit (-1 among them).  Only beside RGBA, YCBCR or TENSOR: a
 * pipeline that parses and reconstructs nothing is a later step, so the bit on its own (output = 32) is refused at create. */
#define LEON_PIPELINE_OUTPUT_MOTION (1 << 5)
/* Bit 7, not 6: create goes on refusing output = 64 | 1 (tests/test_pipeline_motion_gpu.py::test_refusals), as it does every other
 * unknown bit.  Only beside RGBA, YCBCR or TENSOR, like MOTION and independent of it: on its own (output = 128) it is refused at create. */
#define LEON_PIPELINE_OUTPUT_ACTIVITY (1 << 7)
/* Bit 9, not 6 or 8: create goes on refusing 64 and 256 (tests/test_pipeline_motion_gpu.py, tests/test_pipeline_activity_gpu.py::
 * test_refusals).  Only beside RGBA, YCBCR or TENSOR and independent of MOTION and ACTIVITY: alone, or with only those two, it is
 * refused at create like them. */
#define LEON_PIPELINE_OUTPUT_RESIDUAL (1 << 9)

/* element type of the tensor output (leon_pipeline_tensor_config.dtype) */
#define LEON_TENSOR_F16  1
#define LEON_TENSOR_BF16 2
#define LEON_TENSOR_F32  3
/* 8, not 4: create and leon_pipeline_tensor_table go on refusing dtype 4 (tests/test_pipeline_tensor_abi.py::test_refusals,
 * tests/test_pipeline_tensor_gpu.py::test_refusals); 4 .. 7 and everything above 8 stay refused */
#define LEON_TENSOR_U8   8

/* order of a tensor's elements in memory (leon_pipeline_tensor_format.layout) */
#define LEON_TENSOR_LAYOUT_CHW 0
#define LEON_TENSOR_LAYOUT_HWC 1

typedef struct leon_pipeline_config {
    int32_t device_id;
    int32_t parser_threads;     /* K; <= 0: one per hardware thread, at most 16 */
    int32_t gops_per_window;    /* W: independent GOPs decoded together = pictures per launch and type; <= 0: 32 */
    int32_t windows_in_flight;  /* RGBA / staging rings; <= 0: 2 (3 with gpu_parser) */
    int32_t max_gop_pictures;   /* frames reserved per GOP in a window; <= 0: the longest GOP of the stream (counted at create) */
    int32_t loop;               /* benchmarking: decode the stream this many times over (GOP ids keep counting); <= 0: once */
    /* Frame-parallel GOP shards across the GPUs of a node: this pipeline decodes the key-map GOPs
     * g with g % shard_count == shard_index only -- one process (or pipeline) per GPU, each with its device_id,
     * all given the same stream; nothing is exchanged between them (closed GOPs share nothing, the key map is
     * the stream's own index, decoders/jsv.js:264-350; an open GOP with leading B pictures is refused, see "Open GOPs"
     * above).  shard_count <= 1: everything. */
    int32_t shard_index, shard_count;
    /* = jsv.prototype.seek (decoders/jsv.js:1618-1648) at start-up: begin with the key-map entry at or before this
     * time (seconds) instead of the first one; 0 = from the start.  A running pipeline moves with leon_pipeline_seek. */
    double start_seconds;
    /* Where the slice layer is decoded (everything below a slice start code: macroblock headers, vectors, coefficients
     * -- decodeSlice .. decodeBlockGL, decoders/jsv.js:683-1525):
     *   LEON_PIPELINE_PARSER_DEFAULT (0) and LEON_PIPELINE_PARSER_GPU (1): on the GPU, one lane per slice
     *     (csrc/leon_vlc_gpu.h); the parser threads only read the picture layer and upload the stream bytes.  Errors of
     *     a slice surface when its window completes.  The default since round 3: six times the host front end.
     *     A stream beyond the GPU parser's limits (a picture of more than ~40 k block groups -- larger than 4096 x 2304 --,
     *     a GOP shard of 2^28 bytes) is decoded on the parser threads under DEFAULT and refused under an explicit GPU
     *     (leon_pipeline_info.gpu_parser says which it is).  A picture whose slices OVERLAP (MPEG-1 forbids it; the
     *     reference decodes them one after the other, the later one wins) is refused by the GPU parser, which decodes a
     *     picture's slices side by side, when its window completes: the host parser decodes such a stream.
     *   LEON_PIPELINE_PARSER_HOST (-1): on the parser threads (libleon_vlc.so).
     * Same frames either way. */
    int32_t gpu_parser;
    /* Arithmetic of the frames' colour conversion, leon.h's LEON_RGB_*:
     *   LEON_RGB_CPU_TWIN (0): the integer-exact twin of the reference's CPU conversion, fused into the reconstruction launches
     *     (what every other path of this library delivers; bit-exact to the oracle).
     *   LEON_RGB_GL (1): the fp32 arithmetic of the reference's LIVE display -- renderFrameGL drawing with
     *     SHADER_FRAGMENT_YCBCRTORGBA (player/easybits.player.js:2787-2858, player/parts/end.js:77-156) -- for a host that
     *     wants the pixels the page shows (within 1 LSB of the executed reference's canvas, tests/test_pipeline_gl_flavour_gpu.py).
     *     Takes the unfused road: every picture writes its planes, one k_rgba_gl launch per picture.  Not with yuva streams. */
    int32_t display_flavour;
    /* What a frame carries, a bit set (0 = LEON_PIPELINE_OUTPUT_RGBA, what every caller got before the field existed; other bits
     * are refused at create; LEON_PIPELINE_OUTPUT_TENSOR and LEON_PIPELINE_OUTPUT_MOTION are described further down):
     *   LEON_PIPELINE_OUTPUT_RGBA   frame.rgba, RGBA8 in the display flavour above
     *   LEON_PIPELINE_OUTPUT_YCBCR  frame.y / cb / cr (+ a for yuva streams): the decoded YCbCr 4:2:0 planes, cropped to the frame --
     *                               the reference's own frame event, this['go']('frame', {'ybr': [Y, Cb, Cr], 'ts': ts})
     *                               (decoders/jsv.js:600, :673; a yuva stream's fourth plane as in its 4-plane ring, :59-73), which its
     *                               display converts in a shader (renderFrameGL, player/easybits.player.js:2787-2858).  The planes do
     *                               not depend on display_flavour; with YCBCR alone no RGBA is written nor allocated.
     * Plane layout in device memory (leon_pipeline_info reports it): Y and A frame_width x frame_height, Cb and Cr
     * ((frame_width + 1) / 2) x ((frame_height + 1) / 2); a row takes its plane's width rounded up to 64 bytes (luma_stride,
     * chroma_stride; the bytes behind the width are unspecified), every plane starts on a 256-byte boundary; rows past the plane
     * height are not written.  leon_pipeline_read_frame_planes copies them packed. */
    int32_t output;
} leon_pipeline_config;

/* One decoded picture.  rgba and the planes stay valid until leon_pipeline_release_window(window); a pointer whose output
 * was not asked for (leon_pipeline_config.output) is NULL, and so is `a` but for yuva streams */
typedef struct leon_pipeline_frame {
    uint64_t gop;               /* GOP id (key-map index, counting on across loops) */
    int32_t  display_index;     /* temporal reference inside its GOP */
    int32_t  type;              /* LEON_PIC_I / _P / _B */
    double   ts_ms;             /* presentation time: GOP time code + display_index / picture rate */
    void*    rgba;              /* DEVICE pointer: frame_width * frame_height * 4 bytes */
    void    *y, *cb, *cr, *a;   /* DEVICE pointers to the frame's planes (LEON_PIPELINE_OUTPUT_YCBCR; layout: leon_pipeline_config.output) */
} leon_pipeline_frame;

/* Called on the pipeline's notify thread once per window, frames in display order (GOP-major).
 * n_frames == 0 with window < 0 signals the end of the stream ('ended', decoders/jsv.js:437);
 * status != 0 an error (leon_pipeline_error() has the text).
 * Lifetimes: the `frames` ARRAY belongs to the window -- it is valid until the callback returns or the window is
 * released, whichever comes first (a callback that releases the window must have read frames[] before; copy what is
 * kept); the device memory `rgba` points to stays valid until leon_pipeline_release_window(window).  A window
 * delivered with status != 0 (n_frames may be 0) holds its ring entry and staging like any other and must be
 * released too. */
/* LEON_PIPELINE_OUTPUT_TENSOR: a frame as [3][frame_height][frame_width] elements -- planar R, G, B, dense (row stride = frame_width
 * elements), fp16 / bf16 / fp32 (8-bit elements and the channels-last layout: leon_pipeline_tensor_format below), each element a per-channel affine function of the 8-bit colour value:
 *     tensor[c][y][x] = T[c][ rgba[y][x][c] ]        c = 0, 1, 2; rgba = the bytes an RGBA pipeline with display_flavour
 *                                                    LEON_RGB_CPU_TWIN delivers for the frame (the A byte is not used)
 *     T[c][v] = to_dtype( (float) ( (double)v * (double)scale[c] + (double)bias[c] ) )        v = 0 .. 255
 * -- the double expression rounded once to binary32 (to nearest even), that value once to the element type (to nearest even;
 * identity for fp32).  T is built on the host at create (leon_pipeline_tensor_table gives the same 768 values without a device)
 * and looked up by one kernel per window (k_tensor) that reads the frame's YCbCr planes.  The tensor never depends on
 * display_flavour (that field governs frame.rgba only); a yuva stream's alpha is not in it (ask for YCBCR beside it); an odd
 * frame height leaves the last row at the CPU twin's fill value, T[c][255]; an odd frame width is refused at create.
 * dtype: 0 = LEON_TENSOR_F16; scale and bias all zero = scale 1/255, bias 0 (values in [0, 1]).  Refused: another dtype, a
 * non-finite scale or bias, a table entry that is not finite in the element type, a config with a dtype and without the bit.
 * leon_pipeline_config and leon_pipeline_frame keep their layout (existing hosts and tests pin it): the tensor's settings travel in
 * this struct of their own through leon_pipeline_create_tensor, the frames' tensor pointers through leon_pipeline_window_tensors.
 * leon_pipeline_create / _create_partial with the TENSOR bit set take the defaults (fp16, [0, 1]). */
typedef struct leon_pipeline_tensor_config {
    int32_t dtype;              /* LEON_TENSOR_*; 0 = F16 */
    float   scale[3], bias[3];  /* per channel R, G, B */
} leon_pipeline_tensor_config;

/* The tensor at a model's input size: a crop box of the frame resampled to out_width x out_height on the device, from the frame's
 * planes straight to the small tensor (one kernel per window, k_resample; the full-size tensor is never written).  The definition is
 * integer and built from host tables, P = 22:
 *     one axis (in_size = the FRAME's size, in0 = crop start, in1 = crop start + crop size):
 *         scale = (in1 - in0) / out_size (double); fscale = support = max(scale, 1.0)
 *         center = in0 + (o + 0.5) * scale; first = max(0, (int)(center - support + 0.5)); end = min(in_size, (int)(center + support + 0.5))
 *         w[k] = max(0, 1 - |(first + k - center + 0.5) / fscale|), k = 0 .. end - first - 1; w[k] /= sum(w) (index order, doubles)
 *         W[o][k] = (int)(0.5 + w[k] * 2^P)                                  -- leon_pipeline_resize_weights gives first, count, W
 *     h[y][o][c]  = min(255, (2^(P-1) + sum_k Wx[o][k] * rgb[y][first_x[o] + k][c]) >> P)         horizontal pass first, 8-bit result
 *     r[oy][o][c] = min(255, (2^(P-1) + sum_k Wy[oy][k] * h[first_y[oy] + k][o][c]) >> P)         then vertical
 *     tensor[c][oy][ox] = T[c][ r[oy][ox][c] ]                                                    T: the table above
 * with rgb = the bytes an RGBA pipeline with LEON_RGB_CPU_TWIN delivers (the row of 255 in the last row of an odd frame height
 * included).  Taps may reach outside the crop box, never outside the frame.  This is the arithmetic of an 8-bit antialiased
 * triangle ("bilinear") resize: a triangle filter widened by the ratio when reducing, plain bilinear when enlarging.
 * filter = LEON_RESIZE_BICUBIC is the same definition with another filter function f and support S (triangle: f(x) = max(0, 1 - |x|),
 * S = 1) -- the 8-bit bicubic resize of the published CLIP / SigLIP / DINOv2 preprocessing:
 *         support = S * fscale; w[k] = f((first + k - center + 0.5) / fscale); w[k] /= sum(w)
 *         W[o][k] = w[k] < 0 ? (int)(-0.5 + w[k] * 2^P) : (int)(0.5 + w[k] * 2^P)
 *         bicubic: a = -0.5, S = 2;  f(x) = ((a + 2)|x| - (a + 3)) x^2 + 1           for |x| < 1
 *                                         = (((|x| - 5)|x| + 8)|x| - 4) a             for 1 <= |x| < 2,   0 otherwise
 *     h and r = clamp((2^(P-1) + sum) >> P, 0, 255) with an arithmetic shift (floor): weights are negative too, so the sums overshoot on
 *     both sides.  count <= LEON_RESIZE_MAX_TAPS_BICUBIC.  Per row of a table 2^(P-1) + 255 * (sum of the positive W) and 255 * (sum of
 *     |negative W|) stay below 2^31 and every |W| below 2^23 (checked when the tables are built; with these filters it always holds).
 * All fields zero (or no struct) = the full-size tensor above; a crop box of all zeros = the whole frame.  Refused at create:
 * out_width / out_height outside 1 .. 4096, an empty crop box or one that leaves the frame, crop / out > 16 on an axis, another
 * filter (1, 2 and everything above 3), resize settings without the TENSOR bit. */
#define LEON_RESIZE_TRIANGLE 0
#define LEON_RESIZE_BICUBIC 3                /* (the number image libraries give this filter) */
#define LEON_RESIZE_MAX_TAPS 33              /* triangle: count <= 2 * 16 + 1 */
#define LEON_RESIZE_MAX_TAPS_BICUBIC 65      /* bicubic: count <= 4 * 16 + 1 */
typedef struct leon_pipeline_tensor_resize {
    int32_t crop_x, crop_y, crop_width, crop_height;    /* frame pixels */
    int32_t out_width, out_height;
    int32_t filter;                                     /* LEON_RESIZE_TRIANGLE or LEON_RESIZE_BICUBIC */
} leon_pipeline_tensor_resize;

/* what a pipeline's tensors are (leon_pipeline_get_tensor_geometry): width and height of the tensor, the crop box in force, the
 * largest tap count of an output column / row (1 and 1 without resize settings), resized = 1 when k_resample makes them */
typedef struct leon_pipeline_tensor_geometry {
    int32_t width, height;
    int32_t crop_x, crop_y, crop_width, crop_height;
    int32_t taps_x, taps_y;
    int32_t resized;
} leon_pipeline_tensor_geometry;

/* 8-bit elements and the channels-last layout.
 * LEON_TENSOR_U8: the element IS the 8-bit colour value -- T[c][v] = v, one byte; scale and bias must all be zero (anything else is
 * refused at create and by leon_pipeline_tensor_table, which writes the 768-byte identity table).  Everything else of the
 * definitions above holds: the CPU twin's bytes, the resize arithmetic, the row of 255 in the last row of an odd frame height.
 * layout (leon_pipeline_create_tensor_format), for all four element types, with and without resize settings:
 *   LEON_TENSOR_LAYOUT_CHW (0)  tensor[c][y][x], planar, as above
 *   LEON_TENSOR_LAYOUT_HWC (1)  tensor[y][x][c], dense: pixel stride 3 elements, row stride 3 * width elements -- the same values,
 *                               only the addressing differs (a packed uint8 HWC frame is the RGBA frame without its A bytes)
 * The frame's bytes (tensor_frame_bytes = 3 * height * width * element size) and the ring pitches do not depend on the layout; a
 * window of equally long GOPs is one strided [gops, pictures, H, W, 3] view.  A yuva stream's alpha is in neither layout.
 * Every combination is written by k_tensor<element bytes, layout> at the frame's size and by k_resample<element bytes, layout, filter> at
 * a model's input size.
 * Refused at create: a format without the TENSOR bit, another layout, a non-zero reserved word. */
typedef struct leon_pipeline_tensor_format {
    int32_t layout;             /* LEON_TENSOR_LAYOUT_* */
    int32_t reserved[7];        /* must be 0: room for the next tensor setting */
} leon_pipeline_tensor_format;  /* 32 bytes */

/* what a pipeline's tensors look like in memory (leon_pipeline_get_tensor_shape; leon_pipeline_info and
 * leon_pipeline_tensor_geometry keep their sizes): element type and size, layout, and for the logical index [c][y][x] the
 * strides IN ELEMENTS -- CHW: {height * width, width, 1}, HWC: {1, 3 * width, 3} */
typedef struct leon_pipeline_tensor_shape {
    int32_t dtype, element_bytes;
    int32_t layout;
    int32_t channels;           /* 3 */
    int32_t height, width;
    int64_t stride_c, stride_y, stride_x;
} leon_pipeline_tensor_shape;

/* The resampled image in a padded canvas: detection, segmentation and pose models, and any batch with a fixed input shape, take the
 * frame resized with its aspect ratio kept and padded to a fixed size (1920 x 1080 -> 640 x 360, centred in 640 x 640 of grey).
 * With r[oy][ox][c] the 8-bit result of the resize definition above for `resize` (either filter, unchanged; out_height x out_width)
 * and T the element table, the tensor is width x height:
 *     tensor[c][Y][X] = T[c][ r[Y - y][X - x][c] ]      for x <= X < x + out_width and y <= Y < y + out_height
 *                     = T[c][ pad[c] ]                   everywhere else
 * laid out as CHW or HWC exactly as above with width and height in place of out_width and out_height: tensor_frame_bytes, the ring
 * pitches, leon_pipeline_tensor_shape, leon_pipeline_tensor_geometry.width / height and leon_pipeline_read_tensor are the canvas's; the
 * geometry's crop and tap fields still describe the resampling; leon_pipeline_get_tensor_canvas reports the image rectangle.
 * Every element of a frame's tensor is written by its window's launch, every window.  Pad elements are not written once at create
 * and then relied upon: a consumer may overwrite a delivered tensor in place until it releases the window, and the next window that
 * reuses the ring entry is whole again.  It is still one launch per window (k_letterbox<element bytes, layout, filter>: the image's
 * tiles as k_resample's, further workgroups of the same launch for the pad).
 * A canvas equal to the image (x = y = 0, same size) gives exactly the tensors of the same pipeline without a canvas; an identity resize
 * (out size = crop size, triangle filter) with a larger canvas is the padded full frame.  All fields zero (or no struct) =
 * leon_pipeline_create_tensor_format.
 * Refused at create (LEON_ERR_INVALID, no device touched): a canvas without the TENSOR bit, a canvas without resize settings (no
 * out_width / out_height), width or height outside 1 .. 4096, a negative x or y, x + out_width > width or y + out_height > height, a
 * pad value outside 0 .. 255, image_width / image_height non-zero and different from the out size, a non-zero reserved word. */
typedef struct leon_pipeline_tensor_canvas {
    int32_t width, height;               /* the TENSOR's size; 1 .. 4096 each */
    int32_t x, y;                        /* where the resampled image's top-left element lies in it; >= 0 */
    int32_t pad[3];                      /* 8-bit R, G, B of every element outside the image; 0 .. 255 */
    int32_t image_width, image_height;   /* create: 0, or equal to resize->out_width / out_height; get: the values in force */
    int32_t reserved[7];                 /* must be 0 */
} leon_pipeline_tensor_canvas;           /* 64 bytes */

/* LEON_PIPELINE_OUTPUT_MOTION: what the stream says about motion, per delivered frame -- the block-motion field a compressed-domain
 * model reads, the vectors that carry a detector's boxes from an anchor across the B pictures between, what `-flags2 +export_mvs` gives.
 * A delivered frame of a picture of type t gets one MOTION RECORD.  Its macroblocks are in raster order of the CODED picture:
 * mbw = coded_width / 16, mbh = coded_height / 16, mbs = mbw * mbh.  For macroblock k, with the picture's maps as include/leon.h
 * defines them (integers only):
 *     I picture:  info = 4;  mv = (0, 0, 0, 0)
 *     P picture:  intra = repadd[k] >= 128
 *                 info  = intra ? 4 : 1
 *                 mv    = intra ? 0 : (mv_fwd[2k], mv_fwd[2k+1], 0, 0)
 *     B picture:  intra = repadd[k] >= 128;  d = intra ? 0 : (mb_dir[k] & 3)
 *                 info  = intra ? 4 : d
 *                 mv    = (d&1 ? mv_fwd[2k] : 0, d&1 ? mv_fwd[2k+1] : 0,
 *                          d&2 ? mv_bwd[2k] : 0, d&2 ? mv_bwd[2k+1] : 0)
 * info bits: 1 forward, 2 backward, 4 intra; the other bits are 0.  Vectors are in half-pel luma units as the maps hold them (full_pel
 * vectors are already doubled); positive means right / down, from the macroblock to where it reads in the reference.
 * This is exactly the stream-carried part of the maps: the maps also hold parser state -- the entry of a direction a B macroblock does
 * not use holds the predictor, a skipped macroblock keeps the intra flag of the picture before -- which the record leaves out, so two
 * sets of maps that agree in what the stream carries give the same record, whichever parser wrote them.  The `intra` map is not used.
 * The record in memory, the same on the device and on the host (pad256 = rounding up to 256):
 *     mv       int16 [mbs][4]   fwd_h, fwd_v, bwd_h, bwd_v      at 0
 *     info     uint8 [mbs]                                      at info_offset    = pad256(8 * mbs)
 *     summary  uint32[8]                                        at summary_offset = info_offset + pad256(mbs)
 *     record_bytes = summary_offset + 32;   record_pitch = pad256(record_bytes)
 * Summary words, over the RECORD's values: [0] macroblocks with info & 1, [1] with info & 2, [2] with info & 4, [3] macroblocks with any
 * non-zero vector word, [4..7] the sums of |fwd_h|, |fwd_v|, |bwd_h|, |bwd_v|.  A vector word is at most 2048 in magnitude (f_code 7,
 * full_pel doubled) and a picture has at most 256 x 256 macroblocks: a sum is at most 2^27 and fits its word with room.
 * The bytes between the parts, and up to the pitch, are unspecified.  Every specified byte of every delivered frame's record is
 * written by its window's launch (k_motion: one launch per window on the decoder's stream behind the reconstruction, one workgroup per
 * frame), every window; nothing relies on an earlier clear.  A window delivered with an error has unspecified records.  Pictures that
 * are not delivered (dropped leading B pictures, what an EXACT seek trims) have no record. */
/* (a struct tag only, no typedef: the host call that fills it has the same name, so it is written `struct leon_pipeline_motion_layout`) */
struct leon_pipeline_motion_layout {
    int32_t  mb_width, mb_height, mbs;
    int32_t  reserved0;                 /* 0 */
    uint64_t info_offset, summary_offset, record_bytes, record_pitch;
    uint64_t reserved[2];               /* 0 */
};                                      /* 64 bytes */

typedef struct leon_pipeline_motion_frame {
    void*    record;        /* DEVICE pointer, 256-byte aligned, valid until release_window */
    uint64_t fwd_gop;       /* GOP id of the forward reference (an open GOP's leading B pictures: the GOP before) */
    int32_t  fwd_display;   /* display_index of the picture the forward vectors point into; -1: none (I pictures) */
    int32_t  bwd_display;   /* the same for backward vectors, always in the frame's own GOP; -1: none (I, P) */
    int32_t  reserved[2];
} leon_pipeline_motion_frame;           /* 32 bytes */

/* LEON_PIPELINE_OUTPUT_ACTIVITY: how much the stream coded on top of each prediction, per delivered frame -- where a carried box or a
 * propagated map stops being trustworthy, what a "run the detector again here" gate reads, the residual branch of a compressed-domain
 * model.  A delivered frame gets one ACTIVITY RECORD, made from the picture's sparse group lists and its qscale map as
 * include/leon_vlc.h defines them (integers only).  Geometry: mbw = coded_width / 16, mbh = coded_height / 16, mbs = mbw * mbh,
 * groups_y = ceil(mbw / 4), groups_c = ceil(mbw / 8), n_y = 2 * mbh * groups_y, n_c = mbh * groups_c.  Only the n_y + 2 * n_c groups
 * of Y, Cb and Cr are read (grp_off[0 .. n_y + 2 n_c]); the A groups of a yuva stream are not.
 * An entry e of group G:  level = (int16)(e & 0xffff), a = |level| (0 .. 32768); an entry with level == 0 counts nothing (one front
 * end writes such entries, the other does not: the record is the same).  b = (e >> 20) & 7 is its block in the group, r = (e >> 23) & 7
 * its row and c = (e >> 17) & 7 its column in the block; it is DC when r == 0 and c == 0.  Its macroblock (mx, my) and block j:
 *     luma, block row R, group g   G = R * groups_y + g               mx = 4 g + (b >> 1)   my = R >> 1   j = 2 (R & 1) + (b & 1)
 *     Cb,   block row R, group g   G = n_y + R * groups_c + g         mx = 8 g + b          my = R        j = 4
 *     Cr,   block row R, group g   G = n_y + n_c + R * groups_c + g   mx = 8 g + b          my = R        j = 5
 * An entry whose mx >= mbw counts nothing.  Per macroblock k = my * mbw + mx, over its entries with level != 0:
 *     ac_count  the number of entries that are not DC          ac_mag  the sum of a over those entries
 *     dc_mag    the sum of a over the DC entries                blocks  bit j set when block j has at least one such entry (the
 *                                                                       effective coded block pattern)
 * The three sums are taken exactly and then each saturated at 65535.  qscale = blocks ? qscale_map[k] : 0: the map keeps stale parser
 * state at macroblocks that code nothing, which the record does not show.  DC is kept apart because an intra macroblock's DC entry is
 * in the 0 .. 255 predictor domain (leon_vlc.h), a sample level and not a correction; the motion record's info, or the picture type,
 * tells the two apart.
 * The record in memory, the same on the device and on the host, little endian (pad256 = rounding up to 256):
 *     cell     [mbs] of 8 bytes: uint16 ac_count, uint16 ac_mag, uint16 dc_mag, uint8 blocks, uint8 qscale     at 0
 *     summary  uint32[8]                                                              at summary_offset = pad256(8 * mbs)
 *     record_bytes = summary_offset + 32;   record_pitch = pad256(record_bytes)
 * Summary words, over the RECORD's values: [0] macroblocks with blocks != 0, [1] the sum of ac_count, [2] of ac_mag, [3] of dc_mag,
 * [4] the maximum of ac_mag, [5] the sum of qscale, [6] of popcount(blocks), [7] 0.  A picture has at most 256 x 256 macroblocks and
 * every word fits: the largest, [2], is at most 65536 * 65535 < 2^32.
 * The bytes between the parts, and up to the pitch, are unspecified.  Every specified byte of every delivered frame's record is
 * written by its window's launches (k_activity and k_activity_summary, one launch each per window on the decoder's stream behind the
 * reconstruction), every window; nothing relies on an earlier clear.  A window delivered with an error has unspecified records.
 * Pictures that are not delivered (dropped leading B pictures, what an EXACT seek trims) have no record. */
/* (a struct tag only, as leon_pipeline_motion_layout) */
struct leon_pipeline_activity_layout {
    int32_t  mb_width, mb_height, mbs;
    int32_t  reserved0;                 /* 0 */
    uint64_t summary_offset, record_bytes, record_pitch;
    uint64_t reserved[3];               /* 0 */
};                                      /* 64 bytes */

/* LEON_PIPELINE_OUTPUT_RESIDUAL: the decoded residual picture of each delivered frame -- the correction the stream adds to its own
 * prediction, sample by sample: the third modality of a compressed-domain model beside the I-picture pixels and the motion vectors.
 * It is neither frame - reference (motion compensation lies between them) nor a function of the activity cells.
 * For every delivered frame and every plane Y, Cb, Cr of the CODED picture (coded_width x coded_height, chroma half each), element
 * (y, x) is
 *     res(y, x) = (t + 128) / 256          (C division, truncating toward zero)
 * taken before any prediction is added and before any clamp, t being the output of the reference's two-pass integer IDCT of the
 * dequantised levels (integers only once pass 1 has run), with the picture's qscale and intra maps and the quantiser matrices of its
 * sequence: exactly what lo_pass1_plane followed by lo_pass2_residual_plane of the oracle give for the picture's dense coefficient
 * planes.  Stored as int16, saturated to -32768 .. 32767.  Nobody has proven a bound on the value; a CPU probe with the oracle (4000
 * random 16x16 planes, all levels +-32768, +-2047 or +-255 and sparse extremes, qscale 1 and 31, intra and non-intra) found
 * -3016 .. 3084, so the saturation is a guard and not a tested case (a saturating pack costs no more than a plain one).
 * Consequences: a block without coefficients is all 0.  An intra macroblock's "residual" is its sample levels (the motion record's
 * info & 4 says which macroblocks those are).  Every picture type obeys planes = clamp(prediction + res, 0, 255), with prediction 0
 * where nothing is predicted.  The truncation holds for I pictures too, where the planes' clamp hides it: the record shows negative
 * values.
 * Only the n_y + 2 n_c groups of Y, Cb and Cr are read (a yuva stream's A groups are not part of the record), as in ACTIVITY.  An
 * entry with level 0 contributes nothing.  An entry of a block at or behind the plane's block width (a partly filled last group) is
 * not shown.
 * The record in memory (pad64, pad256 = rounding up):
 *     [ Y: coded_height rows | Cb: coded_height / 2 rows | Cr: coded_height / 2 rows ]   int16, little endian
 *     luma_stride = pad64(coded_width), chroma_stride = pad64(coded_width / 2)   ELEMENTS a row
 *     cb_offset = pad256(2 * luma_stride * coded_height), cr_offset = cb_offset + pad256(2 * chroma_stride * coded_height / 2)   bytes
 *     record_bytes = cr_offset + 2 * chroma_stride * coded_height / 2;   record_pitch = pad256(record_bytes)
 * The pad columns behind coded_width (coded_width / 2 for chroma) are unspecified, and so are the bytes up to the pitch; no byte outside
 * record_bytes is ever written.  Every specified element of every delivered frame's record is written by its window's launch
 * (k_residual, on the decoder's stream behind the reconstruction), every window; nothing is cleared beforehand and nothing is added to
 * atomically.  A frame of frame_width x frame_height is the top-left frame_height x frame_width of the record, as the planes output
 * crops.  A window delivered with an error has unspecified records; pictures that are not delivered have none. */
/* (a struct tag only, as leon_pipeline_activity_layout) */
struct leon_pipeline_residual_layout {
    int32_t  coded_width, coded_height;
    int32_t  luma_stride, chroma_stride;        /* elements */
    uint64_t cb_offset, cr_offset, record_bytes, record_pitch;   /* bytes */
    uint64_t reserved[2];               /* 0 */
};                                      /* 64 bytes */

typedef void (*leon_pipeline_callback)(void* user, int64_t window, const leon_pipeline_frame* frames, int32_t n_frames, int32_t status);

typedef struct leon_pipeline_info {
    int32_t coded_width, coded_height, frame_width, frame_height;
    double  picture_rate, duration;
    uint32_t gops;              /* key-map entries (1 for a stream without key map) */
    uint32_t shard_gops;        /* how many of them this pipeline decodes (per pass over the stream) */
    uint32_t first_gop;         /* key-map entry the run starts with (start_seconds) */
    int32_t parser_threads, gops_per_window;
    int32_t gpu_parser;         /* 1: the slice layer is decoded on the GPU, 0: on the parser threads (what LEON_PIPELINE_PARSER_DEFAULT chose) */
    int32_t display_flavour;    /* LEON_RGB_CPU_TWIN / LEON_RGB_GL, as configured */
    int32_t output;             /* LEON_PIPELINE_OUTPUT_* bits in force (0 configured = RGBA) */
    int32_t chroma_width, chroma_height;   /* of Cb and Cr: (frame_width + 1) / 2, (frame_height + 1) / 2 */
    int32_t luma_stride, chroma_stride;    /* bytes per row of Y (and A), of Cb and Cr: the plane width rounded up to 64 */
    /* LEON_PIPELINE_OUTPUT_TENSOR (all 0 without it): element type and size, 3 * height * width * element size (the frame's, or
     * out_height and out_width of leon_pipeline_tensor_resize), and the
     * bytes between the tensors of consecutive display positions of one GOP and ring entry (= tensor_frame_bytes rounded up to 256)
     * and between the GOP lanes of a window: a window whose GOPs are equally long is one strided [gops, pictures, 3, H, W] view */
    int32_t tensor_dtype, tensor_element_bytes;
    uint64_t tensor_frame_bytes, tensor_frame_pitch, tensor_gop_pitch;
} leon_pipeline_info;

typedef struct leon_pipeline_stats {
    uint64_t pictures, gops, windows, stream_bytes;
    double   seconds;           /* first parser start -> last window completed (so far) */
    double   parse_seconds_sum; /* summed over the parser threads */
    double   upload_bytes;      /* what crossed PCIe */
    uint64_t entries;           /* non-zero coefficients decoded (host front end; 0 with gpu_parser: they stay on the device) */
} leon_pipeline_stats;

/* Copies nothing: `stream` must stay valid until leon_pipeline_destroy.  Starts decoding at once. */
int leon_pipeline_create(const leon_pipeline_config* cfg, const uint8_t* stream, size_t bytes,
                         leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* The same for a stream that is still arriving -- the reference's decoder consumes a growing buffer, stalls when it runs
 * dry and resumes when a chunk is appended (features/bitreader.js:332-430 addBuffer, :135-189 has; decoders/jsv.js
 * :426-469): `stream` is the buffer for the WHOLE file (`bytes` = its final size, known from the HTTP headers as in the
 * reference's {data, start, end, total} chunks), of which the first `valid_bytes` are there -- enough for the container
 * header, the key map and the first sequence header.  The loader writes on into the same buffer and reports progress
 * with leon_pipeline_feed(p, valid_bytes_now); a GOP is parsed once the bytes up to the next key-map entry have
 * arrived, windows are delivered as they complete.  With max_gop_pictures <= 0 a partial stream reserves 16 frames per GOP. */
int leon_pipeline_create_partial(const leon_pipeline_config* cfg, const uint8_t* stream, size_t bytes, size_t valid_bytes,
                                 leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* leon_pipeline_create_partial with the tensor output's settings (valid_bytes = bytes: a complete stream); `tensor` NULL = the defaults */
int leon_pipeline_create_tensor(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const uint8_t* stream, size_t bytes,
                                size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* the table T (3 x 256 elements of the element type, [channel][value]) a pipeline created with these settings looks up: computed on
 * the host, no device touched -- and refused as create refuses (cfg->output must have the TENSOR bit) */
int leon_pipeline_tensor_table(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, void* out768);
/* leon_pipeline_create_tensor with the tensors resampled to a model's input size; `resize` NULL (or all zero) = leon_pipeline_create_tensor */
int leon_pipeline_create_tensor_resized(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                        const uint8_t* stream, size_t bytes, size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* the tables of one axis of that resampling: first[o], count[o] and weights[o * max_taps + k] (k >= count[o]: 0) for o = 0 .. out_size - 1.
 * Computed on the host, no device touched, refused as create refuses (and when a count exceeds max_taps; LEON_RESIZE_MAX_TAPS always fits the
 * triangle filter, LEON_RESIZE_MAX_TAPS_BICUBIC both) */
int leon_pipeline_resize_weights(int32_t in_size, int32_t crop_start, int32_t crop_size, int32_t out_size, int32_t filter,
                                 int32_t* first, int32_t* count, int32_t* weights, int32_t max_taps);
int leon_pipeline_get_tensor_geometry(leon_pipeline* p, leon_pipeline_tensor_geometry* out);
/* leon_pipeline_create_tensor_resized with the tensors' layout; `format` NULL (or all zero) = leon_pipeline_create_tensor_resized */
int leon_pipeline_create_tensor_format(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                       const leon_pipeline_tensor_format* format, const uint8_t* stream, size_t bytes, size_t valid_bytes,
                                       leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* LEON_ERR_INVALID for a pipeline without tensor output, as leon_pipeline_get_tensor_geometry */
int leon_pipeline_get_tensor_shape(leon_pipeline* p, leon_pipeline_tensor_shape* out);
/* leon_pipeline_create_tensor_format with the image placed in a padded canvas; `canvas` NULL (or all zero) = leon_pipeline_create_tensor_format */
int leon_pipeline_create_tensor_canvas(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                       const leon_pipeline_tensor_format* format, const leon_pipeline_tensor_canvas* canvas, const uint8_t* stream,
                                       size_t bytes, size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out);
/* the canvas in force: its size, the image rectangle (x, y, image_width, image_height) and the pad values; without canvas settings the
 * tensor itself (x = y = 0, image = tensor, pad 0).  LEON_ERR_INVALID for a pipeline without tensor output */
int leon_pipeline_get_tensor_canvas(leon_pipeline* p, leon_pipeline_tensor_canvas* out);
/* The usual placement: a source of src_width x src_height scaled to fit canvas_width x canvas_height with its aspect ratio kept, and
 * centred.  Host only, no device; 64-bit integers only, so that every binding agrees on every input:
 *     canvas_width * src_height <= canvas_height * src_width:
 *         out_width = canvas_width,   out_height = max(1, (2 * src_height * canvas_width + src_width) / (2 * src_width))
 *     otherwise:
 *         out_height = canvas_height, out_width = max(1, (2 * src_width * canvas_height + src_height) / (2 * src_height))
 *     x = (canvas_width - out_width) / 2, y = (canvas_height - out_height) / 2          (the odd pixel goes right or below)
 * Fills resize->out_width / out_height (crop and filter are left alone) and canvas->width / height / x / y (pad, image_* and reserved are
 * left alone); src_* is the crop box's size, or the frame's.  1920 x 1080 into 640 x 640 is 640 x 360 at (0, 140).  Refuses a size below 1;
 * the ratio limit of 16 is create's to judge. */
int leon_pipeline_letterbox(int32_t src_width, int32_t src_height, int32_t canvas_width, int32_t canvas_height,
                            leon_pipeline_tensor_resize* resize, leon_pipeline_tensor_canvas* canvas);
int leon_pipeline_feed(leon_pipeline* p, size_t valid_bytes);
int leon_pipeline_get_info(leon_pipeline* p, leon_pipeline_info* out);
/* the consumer is done with a window's frames: its ring entries (RGBA, planes, tensors) and staging may be reused */
int leon_pipeline_release_window(leon_pipeline* p, int64_t window);
/* blocks until every window has been delivered and the final callback (window -1) has returned; returns the
 * first error.  Not to be called from inside the callback. */
int leon_pipeline_wait(leon_pipeline* p);
int leon_pipeline_get_stats(leon_pipeline* p, leon_pipeline_stats* out);

/* Repositioning a running pipeline = jsv.prototype.seek (decoders/jsv.js:1618-1648), without the allocations of create:
 *   LEON_PIPELINE_SEEK_KEY    from the key-map entry start_seconds = `seconds` would start with: the frames from
 *                             *first_window on are those of a pipeline created with that start_seconds (shards honoured)
 *   LEON_PIPELINE_SEEK_EXACT  from the same entry, but the first frame delivered is the one on screen at `seconds` (the
 *                             largest ts_ms <= seconds * 1000 of that GOP, or its first frame): earlier I and P pictures
 *                             are reconstructed for what predicts from them but not delivered, earlier B pictures are not
 *                             decoded.  With shard_count > 1 only the shard that owns the entry trims.
 * *first_window = the id of the first window of the new position (window ids count on across seeks).  Once seek returns
 * no callback starts for a window below it (a callback under way has returned); windows submitted for the old position
 * are drained and never delivered; windows delivered and not released stay valid until released.  After 'ended' a seek
 * starts a new run with its own 'ended'; leon_pipeline_wait waits for the current run; stats accumulate.  A partial
 * stream may be seeked past what has arrived.  Refused (LEON_ERR_INVALID, nothing changes): loop > 1, a failed
 * pipeline, a call from inside the callback, another mode, a non-finite time.  Any host thread but the callback's,
 * not concurrently with leon_pipeline_destroy. */
#define LEON_PIPELINE_SEEK_KEY   0
#define LEON_PIPELINE_SEEK_EXACT 1
int leon_pipeline_seek(leon_pipeline* p, double seconds, int32_t mode, int64_t* first_window);
/* copy one frame of a delivered, not yet released window to host memory (tests, thumbnails); LEON_ERR_INVALID for a frame
 * without RGBA */
int leon_pipeline_read_frame(leon_pipeline* p, const leon_pipeline_frame* f, uint8_t* rgba_host);
/* the same for its planes, packed (row stride = plane width): y frame_width x frame_height, cb and cr chroma_width x chroma_height,
 * a (may be NULL; yuva streams) like y.  LEON_ERR_INVALID for a frame without planes */
int leon_pipeline_read_frame_planes(leon_pipeline* p, const leon_pipeline_frame* f, uint8_t* y, uint8_t* cb, uint8_t* cr, uint8_t* a);
/* the tensors of a delivered, not yet released window: out[i] = DEVICE pointer of frames[i]'s tensor (256-byte aligned, valid until the
 * window is released, like rgba), n = the window's n_frames.  May be called from inside the callback.  LEON_ERR_INVALID for a
 * pipeline without tensor output, a window that is not out for delivery, another n */
int leon_pipeline_window_tensors(leon_pipeline* p, int64_t window, void** out, int32_t n);
/* copy the tensor of frame `index` of such a window to host memory, packed (tensor_frame_bytes: [3][height][width] of the geometry, or
 * [height][width][3] with LEON_TENSOR_LAYOUT_HWC) */
int leon_pipeline_read_tensor(leon_pipeline* p, int64_t window, int32_t index, void* host);
/* host only, no device: the record's layout for a picture of mb_width x mb_height macroblocks; refuses sizes outside 1 .. 256 */
int leon_pipeline_motion_layout(int32_t mb_width, int32_t mb_height, struct leon_pipeline_motion_layout* out);
/* host only: the definition above on the CPU (the per-macroblock text the kernel compiles too, csrc/leon_motion.h), from a picture's
 * maps in host memory into a buffer of record_bytes.  Unspecified bytes are left alone.  Maps the type does not have may be NULL
 * (I: all four; P: mb_dir and mv_bwd); refuses another type, a size outside 1 .. 256, a missing map, a null record */
int leon_pipeline_motion_record(int32_t type, int32_t mb_width, int32_t mb_height, const uint8_t* repadd, const uint8_t* mb_dir,
                                const int16_t* mv_fwd, const int16_t* mv_bwd, void* record);
/* A diagnostic in the manner of leon_pipeline_carry_device: k_motion on maps the CALLER supplies, with memory of its own on device_id's
 * null stream, synchronous, everything in host memory.  pictures[i] is a picture of mb_width x mb_height macroblocks: its type and its
 * maps as leon_pipeline_motion_record takes them (those the type does not have are not read and may be NULL).  On the device every map
 * lies in a piece of its own, padded to a multiple of 256 bytes as the pipeline's arenas pad it (a byte a macroblock: pad256(mbs); a
 * vector map: pad256(4 * mbs)), every padding byte = pad_byte.  Frame i is a record of pictures[frames[i].picture], written to
 * ring + frames[i].ring * record_pitch; several frames may name one picture, no two one record.  `ring` is ring_frames * record_pitch
 * bytes (leon_pipeline_motion_layout), goes up and comes back whole: every byte the kernel leaves alone is still the caller's.  The
 * frames go through the pipeline's own launch, more than 65535 of them in more than one.
 * Refused (LEON_ERR_INVALID, nothing launched, `ring` untouched): a null pictures, frames or ring, a size outside 1 .. 256, n_pictures
 * or ring_frames outside 1 .. LEON_MOTION_KERNEL_MAX_FRAMES, n_frames outside 1 .. ring_frames, pad_byte outside 0 .. 255, a type
 * outside LEON_PIC_I / _P / _B, a non-zero reserved word, a missing map of a type that has it, a picture index outside
 * 0 .. n_pictures - 1, a ring index outside 0 .. ring_frames - 1, two frames with one ring index. */
#define LEON_MOTION_KERNEL_MAX_FRAMES (1 << 20)
typedef struct leon_pipeline_motion_picture {
    int32_t type;               /* LEON_PIC_I / _P / _B */
    int32_t reserved0;          /* 0 */
    const uint8_t* repadd;      /* [mbs]; P, B */
    const uint8_t* mb_dir;      /* [mbs]; B */
    const int16_t* mv_fwd;      /* [mbs][2]; P, B */
    const int16_t* mv_bwd;      /* [mbs][2]; B */
} leon_pipeline_motion_picture;         /* 40 bytes */
typedef struct leon_pipeline_motion_kernel_frame {
    int32_t picture;            /* index into pictures */
    int32_t ring;               /* index of the frame's record in the ring */
} leon_pipeline_motion_kernel_frame;    /* 8 bytes */
int leon_pipeline_motion_kernel(int32_t device_id, int32_t mb_width, int32_t mb_height, const leon_pipeline_motion_picture* pictures, int32_t n_pictures,
                                const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring);
/* the layout of this pipeline's records; LEON_ERR_INVALID for a pipeline without LEON_PIPELINE_OUTPUT_MOTION */
int leon_pipeline_get_motion_layout(leon_pipeline* p, struct leon_pipeline_motion_layout* out);
/* the motion records of a delivered, not yet released window: out[i] belongs to frames[i], n = the window's n_frames.  May be called
 * from inside the callback.  The references are the ones the picture's launch predicted from: a closed GOP's leading B picture names
 * its I picture for both.  LEON_ERR_INVALID for a pipeline without the bit, a window that is not out for delivery, another n */
int leon_pipeline_window_motion(leon_pipeline* p, int64_t window, leon_pipeline_motion_frame* out, int32_t n);
/* copy the record of frame `index` of such a window to host memory, packed: mv [mbs][4], info [mbs], summary [8]; each may be NULL */
int leon_pipeline_read_motion(leon_pipeline* p, int64_t window, int32_t index, int16_t* mv, uint8_t* info, uint32_t* summary);

/* The ACTIVITY family, shaped like the MOTION one. */
/* host only, no device: the record's layout for a picture of mb_width x mb_height macroblocks; refuses sizes outside 1 .. 256 */
int leon_pipeline_activity_layout(int32_t mb_width, int32_t mb_height, struct leon_pipeline_activity_layout* out);
/* host only: the definition above on the CPU (the per-entry and per-macroblock text the kernels compile too, csrc/leon_activity.h),
 * from a picture's lists and qscale map in host memory into a buffer of record_bytes.  grp_off has n_y + 2 n_c + 1 values at least,
 * entries n_entries (NULL only with n_entries = 0), qscale mbs.  Unspecified bytes are left alone.  Refused, the record untouched: a
 * size outside 1 .. 256, a null grp_off, qscale or record, null entries with n_entries > 0, a grp_off that decreases anywhere in
 * 0 .. n_y + 2 n_c, a grp_off[n_y + 2 n_c] above n_entries */
int leon_pipeline_activity_record(int32_t mb_width, int32_t mb_height, const uint32_t* grp_off, const uint32_t* entries, uint32_t n_entries,
                                  const uint8_t* qscale, void* record);
/* A diagnostic in the manner of leon_pipeline_motion_kernel: k_activity and k_activity_summary on lists the CALLER supplies, with
 * memory of its own on device_id's null stream, synchronous, everything in host memory.  pictures[i] is a picture of mb_width x
 * mb_height macroblocks as leon_pipeline_activity_record takes it; n_entries is its list's CAPACITY, which the kernel clamps every
 * offset to.  On the device every array lies in a piece of its own, padded as the pipeline's arenas pad it (grp_off: pad256(4 (n_y +
 * 2 n_c + 1)), entries: pad256(4 n_entries + 4), qscale: pad256(mbs)), every padding byte = pad_byte.  Frames, ring and the launch are
 * leon_pipeline_motion_kernel's: frame i is a record of pictures[frames[i].picture] at ring + frames[i].ring * record_pitch
 * (leon_pipeline_activity_layout), the ring goes up and comes back whole, more than 65535 frames go in more than one launch.
 * Refused (LEON_ERR_INVALID, nothing launched, `ring` untouched): what leon_pipeline_motion_kernel refuses of sizes, counts, pad_byte,
 * indices and null arguments, a non-zero reserved word, and what leon_pipeline_activity_record refuses of a picture (a grp_off that is
 * not monotonic, a grp_off[last] above n_entries among them), n_entries above 2^30. */
typedef struct leon_pipeline_activity_picture {
    const uint32_t* grp_off;    /* [n_y + 2 n_c + 1] */
    const uint32_t* entries;    /* [n_entries] */
    const uint8_t* qscale;      /* [mbs] */
    uint32_t n_entries;
    int32_t reserved0;          /* 0 */
} leon_pipeline_activity_picture;       /* 32 bytes */
int leon_pipeline_activity_kernel(int32_t device_id, int32_t mb_width, int32_t mb_height, const leon_pipeline_activity_picture* pictures, int32_t n_pictures,
                                  const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring);
/* the layout of this pipeline's records; LEON_ERR_INVALID for a pipeline without LEON_PIPELINE_OUTPUT_ACTIVITY */
int leon_pipeline_get_activity_layout(leon_pipeline* p, struct leon_pipeline_activity_layout* out);
/* the activity records of a delivered, not yet released window: out[i] is the DEVICE pointer (256-byte aligned, valid until
 * release_window) of frames[i]'s record, n = the window's n_frames.  May be called from inside the callback.  LEON_ERR_INVALID for a
 * pipeline without the bit, a window that is not out for delivery, another n */
int leon_pipeline_window_activity(leon_pipeline* p, int64_t window, void** out, int32_t n);
/* copy the record of frame `index` of such a window to host memory, packed: cells [mbs] of 8 bytes, summary [8]; each may be NULL */
int leon_pipeline_read_activity(leon_pipeline* p, int64_t window, int32_t index, void* cells, uint32_t* summary);

/* The RESIDUAL family, shaped like the ACTIVITY one.  There is no host restatement of the arithmetic in the library: its definition on
 * the CPU is the oracle. */
/* host only, no device: the record's layout for a coded picture; refuses (`out` untouched) a null `out`, a size that is not a multiple
 * of 16 and a size outside 1 .. 256 macroblocks an axis */
int leon_pipeline_residual_layout(int32_t coded_width, int32_t coded_height, struct leon_pipeline_residual_layout* out);
/* A diagnostic in the manner of leon_pipeline_activity_kernel: k_residual on lists, maps and matrices the CALLER supplies, with memory
 * of its own on device_id's null stream, synchronous, everything in host memory.  pictures[i] is a coded picture of coded_width x
 * coded_height: grp_off, entries and n_entries (the list's CAPACITY) as leon_pipeline_activity_record takes them, the qscale and
 * intra maps, 128 bytes of quantiser matrices (intra, then non-intra, natural order) and the 64-byte premultiplier; the kernel's
 * tables are built from them by the function the decoder uses.  Padding, frames, ring and the launch chunks are
 * leon_pipeline_activity_kernel's (the intra map padded like qscale, the tables in 256 bytes of their own); record_pitch is
 * leon_pipeline_residual_layout's.
 * Refused (LEON_ERR_INVALID, nothing launched, `ring` untouched): what leon_pipeline_residual_layout refuses of the size, what
 * leon_pipeline_activity_kernel refuses of counts, pad_byte, indices, null arguments, a reserved word and a picture's lists, a null
 * intra, matrices or premultiplier, n_entries above 2^29. */
typedef struct leon_pipeline_residual_picture {
    const uint32_t* grp_off;    /* [n_y + 2 n_c + 1] */
    const uint32_t* entries;    /* [n_entries] */
    const uint8_t* qscale;      /* [mbs] */
    const uint8_t* intra;       /* [mbs] */
    const uint8_t* matrices;    /* [128] */
    const uint8_t* premultiplier;       /* [64] */
    uint32_t n_entries;
    int32_t reserved0;          /* 0 */
} leon_pipeline_residual_picture;       /* 56 bytes */
int leon_pipeline_residual_kernel(int32_t device_id, int32_t coded_width, int32_t coded_height, const leon_pipeline_residual_picture* pictures,
                                  int32_t n_pictures, const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames,
                                  int32_t pad_byte, void* ring);
/* the layout of this pipeline's records; LEON_ERR_INVALID for a pipeline without LEON_PIPELINE_OUTPUT_RESIDUAL */
int leon_pipeline_get_residual_layout(leon_pipeline* p, struct leon_pipeline_residual_layout* out);
/* the residual records of a delivered, not yet released window: out[i] is the DEVICE pointer (256-byte aligned, valid until
 * release_window) of frames[i]'s record, n = the window's n_frames.  May be called from inside the callback.  LEON_ERR_INVALID for a
 * pipeline without the bit, a window that is not out for delivery, another n */
int leon_pipeline_window_residual(leon_pipeline* p, int64_t window, void** out, int32_t n);
/* copy the record of frame `index` of such a window to host memory, packed (no row padding): y [coded_height][coded_width], cb and cr
 * [coded_height / 2][coded_width / 2] int16; each may be NULL */
int leon_pipeline_read_residual(leon_pipeline* p, int64_t window, int32_t index, int16_t* y, int16_t* cb, int16_t* cr);

/* Regions of delivered frames as a tensor batch: what runs behind a detector.  The detector's boxes are cut out of the FULL-RESOLUTION
 * frames of a delivered window and resampled to a second-stage model's input size, any number of them in one call, into memory of the
 * caller's -- from the frames' planes, which a pipeline with LEON_PIPELINE_OUTPUT_TENSOR keeps in its ring until the window is released
 * (no second, full-size tensor output is needed for it).
 * Region i is r of the resize definition above (leon_pipeline_tensor_resize) with crop = (x, y, width, height) of frames[frame],
 * in_size the frame's size and out = the config's out_width x out_height; its tensor is T[c][ r[oy][ox][c] ] with the PIPELINE's
 * element table, element type and layout (CHW or HWC), at device_out + i * out_pitch_bytes.  The pipeline's own resize, crop and
 * canvas settings play no part.  The fill row of 255 of an odd frame height is in the source as before; taps may leave the box, never
 * the frame; a yuva stream's alpha is not in it.  It equals, bit for bit, what a pipeline created with crop = the box, out size and
 * filter = the config's delivers for that frame.
 * Placement: region_bytes = 3 * out_height * out_width * element bytes; out_pitch_bytes = 0 means region_bytes rounded up to 256,
 * otherwise it must be a multiple of 256 and >= region_bytes; device_out must be 256-byte aligned.  Exactly the region_bytes of each
 * region are written: the bytes between region_bytes and the pitch are not touched, nor is anything behind region n - 1.
 * The call is synchronous: when it returns LEON_OK the tensors are complete in device memory.  It runs on a non-blocking stream of the
 * pipeline's own (created at first use), not on the decoder's: a window in flight is not ordered behind it.  It may be called from any
 * host thread, from inside the callback too, any number of times on a window that is out for delivery and not released; concurrent
 * calls are serialised.  Releasing the window, or destroying the pipeline, while a call on it is in flight is the caller's error.  A
 * window delivered before a seek and still held stays usable.  One kernel launch per call (k_regions<element bytes, layout, filter>:
 * blockIdx.z = the region); every region has tables of its own, built on the host per call and uploaded with the regions'
 * descriptors; the scratch for them grows to its high-water mark and stays with the pipeline.
 * Refused (LEON_ERR_INVALID, nothing launched, nothing written; the message names the region): a pipeline without the TENSOR bit, a
 * window that is not out for delivery or was delivered with an error, n outside 1 .. 65535, a frame outside the window's frames, an
 * empty box or one that leaves the frame, width / out_width or height / out_height above 16, an out size outside 1 .. 4096, another
 * filter, a non-zero reserved word, a null or misaligned device_out, a bad pitch. */
typedef struct leon_pipeline_region {
    int32_t frame;                 /* index into the window's frames[] as delivered to the callback */
    int32_t x, y, width, height;   /* the box, frame pixels; non-empty, inside the frame */
    int32_t reserved[3];           /* must be 0 */
} leon_pipeline_region;            /* 32 bytes */

typedef struct leon_pipeline_regions_config {
    int32_t out_width, out_height; /* 1 .. 4096, the same for every region of a call */
    int32_t filter;                /* LEON_RESIZE_TRIANGLE or LEON_RESIZE_BICUBIC */
    int32_t reserved[5];           /* must be 0 */
} leon_pipeline_regions_config;    /* 32 bytes */

/* host only, no device: what resample_regions would refuse of a window of n_frames frames of frame_width x frame_height;
 * *bad (may be NULL) = index of the first offending region (-1: the config, or n) */
int leon_pipeline_regions_check(int32_t frame_width, int32_t frame_height, int32_t n_frames,
                                const leon_pipeline_region* regions, int32_t n,
                                const leon_pipeline_regions_config* cfg, int32_t* bad);
int leon_pipeline_resample_regions(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                                   const leon_pipeline_regions_config* cfg, void* device_out, uint64_t out_pitch_bytes);
/* the same into pooled device scratch, then copied to the host packed (n * region_bytes): tests, Node, thumbnails */
int leon_pipeline_read_regions(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                               const leon_pipeline_regions_config* cfg, void* host);
/* Regions whose boxes lie in DEVICE memory: the detector ran on the GPU, its boxes never visit the host, and the crops are queued on the
 * caller's stream behind the detector and in front of the second-stage model.  The tensors are those of leon_pipeline_resample_regions,
 * bit for bit (same definition, same placement rules, same kernels behind a status test); what differs is who judges a region and when.
 * The host knows nothing about a box any more, so the regions' tables are built on the device (k_box_tables: the row expressions of
 * leon_pipeline_tensor_resize in IEEE binary64, the same operations in the same order as the host's builder -- one text compiled for both)
 * and a region's faults are not an error of the call: region i gets a status word,
 *     0 (LEON_REGION_OK)      exactly when leon_pipeline_regions_check accepts the region alone in that window,
 *     otherwise the first failing check in regions_check's order: LEON_REGION_RESERVED (a reserved word), LEON_REGION_FRAME (the frame
 *     index), then for x and after it for y: LEON_REGION_BOX (empty, or leaves the frame), LEON_REGION_RATIO_X / _Y (above 16),
 *     LEON_REGION_TAPS (a row's tap count outside 1 .. the filter's maximum; unreachable inside the other limits)
 * written to device_status[i] when that is given.  A region with a non-zero status is skipped: not one byte of its tensor is written.
 * leon_pipeline_region_status is the same judgement on the host, no device involved (tests; hosts that want to name a fault).
 * Ordering.  With `stream` given the call ONLY ENQUEUES and returns LEON_OK once the work is queued there: what wrote the boxes earlier
 * on that stream has run before they are read, what is queued on it later sees the tensors and the status words, and the host learns
 * nothing until it synchronises that stream itself.  With stream NULL the work runs on the pipeline's regions stream and the call waits
 * for it (the boxes must be complete in memory when it is made).  Either way the window must stay unreleased, the pipeline alive and
 * `regions`, `device_out` and `device_status` valid until the work has run: that is the caller's duty, as the host call's.
 * Scratch.  The regions are taken in chunks of as many as fit scratch_limit_bytes -- per region a 64-byte descriptor and a table slot
 * of the filter's worst case for the out size, 4 * (2 * ow + ow * T + 2 * oh + oh * T) bytes with T = 33 (triangle) or 65 (bicubic);
 * the limit bounds a chunk's descriptors and slots, beside which the allocation holds the window's frame ids (4 bytes a frame), each of
 * the three parts rounded up to 256 bytes, and is never smaller than 1 MiB --
 * one k_box_tables and one k_regions<element bytes, layout, filter> launch per chunk, in stream order over the same memory: the scratch is
 * bounded whatever n is (no 4 GiB rule here).  It belongs to the pipeline and grows to its high-water mark.  Every call records an event
 * behind its last launch and the next call's stream waits for that event on the device before its first, so calls on different
 * streams never share the scratch at once; growing it, and leon_pipeline_destroy, wait for the event on the host.  Concurrent calls are
 * serialised while they enqueue.  Any host thread, inside the callback too.
 * Refused (LEON_ERR_INVALID, nothing enqueued, nothing written): what leon_pipeline_regions_check says about the config and n, a pipeline
 * without the TENSOR bit, a window that is not out for delivery or was delivered with an error, a null call, `regions` or `device_out`,
 * `regions` (or device_status) not 4-byte aligned, device_out not 256-byte aligned, a bad pitch, a scratch limit below one region's slot
 * and descriptor, a non-zero reserved word. */
#define LEON_REGION_OK       0
#define LEON_REGION_RESERVED 1
#define LEON_REGION_FRAME    2
#define LEON_REGION_BOX      3
#define LEON_REGION_RATIO_X  4
#define LEON_REGION_RATIO_Y  5
#define LEON_REGION_TAPS     6
#define LEON_REGION_SCALE    7   /* warp regions only (leon_pipeline_warp_regions below): the matrix reduces by more than 4 */
#define LEON_REGION_OFFSET   8   /* warp regions only: |tx| or |ty| above 2^29 */
#define LEON_REGIONS_SCRATCH_DEFAULT ((uint64_t)256 << 20)   /* scratch_limit_bytes = 0 */
typedef struct leon_pipeline_regions_device {
    const leon_pipeline_region* regions;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    void*    device_out;                   /* 256-byte aligned */
    uint64_t out_pitch_bytes;              /* as resample_regions */
    int32_t* device_status;                /* DEVICE memory, n words, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t scratch_limit_bytes;          /* 0: LEON_REGIONS_SCRATCH_DEFAULT; otherwise >= one region's slot + descriptor */
    uint64_t reserved[1];                  /* must be 0 */
} leon_pipeline_regions_device;            /* 64 bytes */
int leon_pipeline_resample_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_regions_config* cfg,
                                          const leon_pipeline_regions_device* call);
/* host only, no device: the status word the device writes for this one region (cfg as judged by leon_pipeline_regions_check; a null
 * argument or a config that check refuses: LEON_ERR_INVALID, which is negative and no status) */
int32_t leon_pipeline_region_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* region,
                                    const leon_pipeline_regions_config* cfg);
/* Regions letterboxed into the batch's input size: what top-down pose, re-identification, text recognition and most classifiers take
 * behind a detector -- the box with its ASPECT RATIO KEPT, padded to the model's fixed input, instead of stretched to it.  A call
 * with a fit whose mode is LEON_REGIONS_FIT_LETTERBOX reads cfg->out_width x out_height as the size of every region's TENSOR, the
 * canvas cw x ch; region_bytes, the pitch rules and the alignment rules are resample_regions', word for word.  Region i with box
 * (x, y, w, h) gets
 *     (ow_i, oh_i, X_i, Y_i) = the integers of leon_pipeline_letterbox(w, h, cw, ch), the same 64-bit expressions; with
 *                              LEON_REGIONS_ANCHOR_TOP_LEFT X_i = Y_i = 0 (text lines, tiles: padded to the right and below),
 *     r_i                    = the 8-bit result of the resize definition (leon_pipeline_tensor_resize) for crop = the box,
 *                              out = ow_i x oh_i, the config's filter,
 *     tensor                 = T[c][ r_i[Y - Y_i][X - X_i][c] ] inside the rectangle, T[c][pad[c]] everywhere else, CHW or HWC as the
 *                              pipeline's: leon_pipeline_tensor_canvas's definition with a rectangle per region.
 * Every one of a valid region's region_bytes is written by the call, and nothing behind them.  It equals, bit for bit, what a
 * pipeline created with crop = the box, that out size and filter, and a canvas of cw x ch with the image at (X_i, Y_i) delivers.
 * The ratio limit of 16 and the tap limits are judged on w / ow_i and h / oh_i, so a box may pass stretched and fail letterboxed
 * (608 x 57 frame, 592 x 52 into 37 x 13: the image is 37 x 3, 52 / 3 > 16); never the other way round, since ow_i <= cw and
 * oh_i <= ch.  The checks, their order and the status words are leon_pipeline_regions_check's and LEON_REGION_*; a box without a width or a height has
 * no letterbox and is judged against the canvas (LEON_REGION_BOX on the axis that has none).  On the device path a refused region
 * has not one byte written, pad included.
 * One launch per call (chunk): k_fitted<element bytes, layout, filter>, blockIdx.z = the region, x / y = the tiles of the canvas --
 * of which a region runs its own image's -- and behind them the pad workgroups; tables per region for ow_i x oh_i, built on the host,
 * or by k_fit_tables on the device in slots of the unchanged worst-case size for out = the canvas (scratch_limit_bytes means what it
 * meant).
 * Refused with LEON_ERR_INVALID: another mode or anchor, a pad value outside 0 .. 255, a non-zero reserved word, a non-zero anchor or
 * pad under LEON_REGIONS_FIT_STRETCH.  fit NULL or all zero is the call without a fit: the same tensors from the same kernels
 * (k_regions on both roads), the rectangle of every region (0, 0, cw, ch). */
#define LEON_REGIONS_FIT_STRETCH      0
#define LEON_REGIONS_FIT_LETTERBOX    1
#define LEON_REGIONS_ANCHOR_CENTRE    0
#define LEON_REGIONS_ANCHOR_TOP_LEFT  1
typedef struct leon_pipeline_regions_fit {
    int32_t mode;                  /* LEON_REGIONS_FIT_* */
    int32_t anchor;                /* LEON_REGIONS_ANCHOR_* */
    int32_t pad[3];                /* the 8-bit R, G, B of every element outside the image, 0 .. 255 */
    int32_t reserved[3];           /* must be 0 */
} leon_pipeline_regions_fit;       /* 32 bytes */
/* host only, no device: rect = (X, Y, ow, oh), where the image of a box of box_width x box_height lies in its tensor -- what maps a
 * keypoint back to the frame.  Refuses what regions_check refuses of the config, a bad fit, a box size below 1. */
int leon_pipeline_region_fit_rect(int32_t box_width, int32_t box_height, const leon_pipeline_regions_config* cfg,
                                  const leon_pipeline_regions_fit* fit, int32_t rect[4]);
/* leon_pipeline_regions_check and leon_pipeline_region_status with the fit */
int leon_pipeline_regions_fit_check(int32_t frame_width, int32_t frame_height, int32_t n_frames,
                                    const leon_pipeline_region* regions, int32_t n,
                                    const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit, int32_t* bad);
int32_t leon_pipeline_region_fit_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* region,
                                        const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit);
/* leon_pipeline_resample_regions / read_regions / resample_regions_device with the fit.  device_rects (may be NULL; letterbox only):
 * DEVICE memory, n x 4 words (X, Y, ow, oh), 4-byte aligned, written for the regions whose status is 0 and left alone for the others,
 * in stream order with the status words. */
int leon_pipeline_resample_regions_fit(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                                       const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit,
                                       void* device_out, uint64_t out_pitch_bytes);
int leon_pipeline_read_regions_fit(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                                   const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit, void* host);
int leon_pipeline_resample_regions_device_fit(leon_pipeline* p, int64_t window, const leon_pipeline_regions_config* cfg,
                                              const leon_pipeline_regions_fit* fit, const leon_pipeline_regions_device* call,
                                              int32_t* device_rects);
/* Rotated boxes and affine crops of delivered frames as a tensor batch: what OCR on oriented text lines, face recognition after
 * landmark alignment, top-down pose on a rotated person box and oriented-object detectors take behind their first stage.  A family of
 * its own beside the regions calls above, which keep their kernels and their bytes: those resample separably, one table per axis, and
 * cannot express a rotation.  All arithmetic below is integer, so that every binding and the device agree on every byte.
 * A warp region is a frame index and six words m = (a00, a01, tx, a10, a11, ty) in Q16: the map
 *     X = a00 * u + a01 * v + tx,   Y = a10 * u + a11 * v + ty
 * takes continuous OUTPUT coordinates (u, v) to continuous FRAME coordinates; pixel (ox, oy) has its centre at (ox + 0.5, oy + 0.5) on
 * both sides.  Supersampling: s2 = max(a00^2 + a10^2, a01^2 + a11^2) in 64 bits; g = 0 if s2 <= (2^16 + 1)^2, 1 if s2 <= (2^17 + 1)^2,
 * 2 if s2 <= (2^18 + 1)^2, anything above is refused; S = 1 << g, and an output pixel is the mean of S x S bilinear samples, which keeps
 * a reduction of up to 4 from aliasing (the + 1 is slack for the quantiser: a rotation at exactly scale 1, 2 or 4 gets S = 1, 2, 4).
 * Sub-sample (i, j), i, j < S, of pixel (ox, oy):
 *     NX = a00 * (2S * ox + 2i + 1) + a01 * (2S * oy + 2j + 1) + 2S * (tx - 32768)          (int64; NY with a10, a11, ty)
 *     qx = ((NX >> (g + 1)) + 128) >> 8          (arithmetic shifts),          x0 = qx >> 8, fx = qx & 255          (the same for y)
 *     acc[c] += (256 - fx)(256 - fy) p(x0, y0) + fx (256 - fy) p(x0 + 1, y0) + (256 - fx) fy p(x0, y0 + 1) + fx fy p(x0 + 1, y0 + 1)
 * and r[c] = (acc[c] + (1 << (15 + 2g))) >> (16 + 2g): one rounding, acc < 2^28.  p(x, y) is the CPU twin's 8-bit colour of the frame,
 * the fill row of 255 of an odd height included; for every position outside the frame p(x, y) = pad[c], so a region may lie partly or
 * wholly outside the frame and is then part or all pad.  The element is T[c][r[c]] with the pipeline's table, element type and layout;
 * region_bytes, the pitch rules and the alignment rules are resample_regions', word for word, and exactly the region_bytes of each
 * region are written.  The identity map is the crop byte for byte, rotations by multiples of 90 degrees are its rotations, a = 2 and
 * a = 4 at integer offsets are the 2 x 2 and 4 x 4 box means (sum + 2) >> 2 and (sum + 8) >> 4; with S = 1 a pixel lies within
 * 255 * 2 * 2^-9 + 0.5 = 1.5 of the float64 bilinear value at the same Q16 coordinates.
 * A record is judged in this order (one text for host and device, csrc/leon_warp.h): LEON_REGION_RESERVED (the reserved word),
 * LEON_REGION_FRAME (the frame index), LEON_REGION_SCALE (s2 above the last threshold), LEON_REGION_OFFSET (|tx| or |ty| above 2^29).
 * leon_pipeline_warp_regions is synchronous on the pipeline's regions stream and refuses the whole call with LEON_ERR_INVALID, naming
 * the region, as resample_regions does (nothing launched, nothing written); the refusals of the window, the pipeline, n, device_out
 * and the pitch are resample_regions'.  leon_pipeline_warp_regions_device takes the records from DEVICE memory and ONLY ENQUEUES on
 * the caller's stream (stream NULL: the regions stream, and the call waits), with resample_regions_device's ordering rules and its
 * scratch event; region i gets its status word in device_status[i] when that is given, and a region whose status is not 0 has not one
 * byte written, pad included.  One launch per call, k_warp<element bytes, layout>: blockIdx.z = the region, x / y = 32 x 8 output
 * tiles.  There are no tables, hence no pre-pass kernel and no chunking: the kernel judges its own record, and the scratch holds the
 * window's frame ids (on the host path also the uploaded records). */
typedef struct leon_pipeline_warp_region {
    int32_t frame;                 /* index into the window's frames[] as delivered to the callback */
    int32_t m[6];                  /* a00, a01, tx, a10, a11, ty in Q16: output coordinates -> frame coordinates */
    int32_t reserved;              /* must be 0 */
} leon_pipeline_warp_region;       /* 32 bytes */
typedef struct leon_pipeline_warp_config {
    int32_t out_width, out_height; /* 1 .. 4096, the same for every region of a call */
    int32_t pad[3];                /* the 8-bit R, G, B of every position outside the frame, 0 .. 255 */
    int32_t reserved[3];           /* must be 0 */
} leon_pipeline_warp_config;       /* 32 bytes */
typedef struct leon_pipeline_warp_regions_call {
    const leon_pipeline_warp_region* regions;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    void*    device_out;                   /* 256-byte aligned */
    uint64_t out_pitch_bytes;              /* as resample_regions */
    int32_t* device_status;                /* DEVICE memory, n words, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[2];                  /* must be 0 */
} leon_pipeline_warp_regions_call;         /* 64 bytes */
/* host only, no device: what warp_regions would refuse of a window of n_frames frames; *bad (may be NULL) = index of the first
 * offending region (-1: the config, or n) */
int leon_pipeline_warp_regions_check(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_warp_region* regions,
                                     int32_t n, const leon_pipeline_warp_config* cfg, int32_t* bad);
/* host only: the status word the device writes for this one region (a null argument or a config that check refuses: LEON_ERR_INVALID,
 * which is negative and no status) */
int32_t leon_pipeline_warp_region_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_warp_region* region,
                                         const leon_pipeline_warp_config* cfg);
/* host only: m[k] = floor(A[k] * 65536 + 0.5) for A = (a00, a01, tx, a10, a11, ty); refuses non-finite values and values outside int32 */
int leon_pipeline_warp_from_matrix(const double A[6], int32_t m[6]);
/* host only: the box of w x h frame pixels centred at (cx, cy) and rotated by angle_degrees (clockwise on the screen: y points down),
 * filling out_width x out_height: a00 = w / ow * cos, a01 = -h / oh * sin, a10 = w / ow * sin, a11 = h / oh * cos,
 * t = centre - A * (ow / 2, oh / 2); quantised as leon_pipeline_warp_from_matrix does */
int leon_pipeline_warp_from_rotated_box(double cx, double cy, double w, double h, double angle_degrees, int32_t out_width, int32_t out_height,
                                        int32_t m[6]);
int leon_pipeline_warp_regions(leon_pipeline* p, int64_t window, const leon_pipeline_warp_region* regions, int32_t n,
                               const leon_pipeline_warp_config* cfg, void* device_out, uint64_t out_pitch_bytes);
/* the same into pooled device scratch, then copied to the host packed (n * region_bytes): tests, Node, thumbnails */
int leon_pipeline_read_warp_regions(leon_pipeline* p, int64_t window, const leon_pipeline_warp_region* regions, int32_t n,
                                    const leon_pipeline_warp_config* cfg, void* host);
int leon_pipeline_warp_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_warp_config* cfg,
                                      const leon_pipeline_warp_regions_call* call);
/* Boxes carried along the stream's motion vectors: a detector runs on an anchor, and its boxes follow the motion records
 * (LEON_PIPELINE_OUTPUT_MOTION) to the other pictures of the GOP, on the device, between the detector and resample_regions_device.
 * One HOP carries a box between two delivered frames of one window that are joined by a prediction.  Integers only.
 * Records.  The input record is 32 bytes, the layout of leon_pipeline_region with its first reserved word in use
 * (leon_pipeline_carry_region below: frame, the box, target, two reserved words that must be 0).  The output record is a
 * leon_pipeline_region with frame = target, the moved box and all three reserved words 0: it can be handed to resample_regions_device
 * as it is, and, once the caller has written a new target into word 5, to the next hop.
 * References inside a window.  For window frame i, fwd[i] is the index of the window frame whose (gop, display_index) equals
 * (motion[i].fwd_gop, motion[i].fwd_display); -1 when fwd_display is -1 or when no delivered frame of this window is that picture (an
 * open GOP's predecessor in an earlier window, an anchor that an EXACT seek reconstructed but did not deliver).  bwd[i] is the same
 * with (frames[i].gop, motion[i].bwd_display).
 * Which record votes, and in which sense.  With S = frame and T = target:
 *     S == T                                  : the box is returned as it is, votes all 0 (status 0)
 *     else M = T, sense = -1, D = (fwd[T] == S ? 1 : 0) | (bwd[T] == S ? 2 : 0)        if that D != 0
 *     else M = S, sense = +1, D = (fwd[S] == T ? 1 : 0) | (bwd[S] == T ? 2 : 0)        if that D != 0
 *     else status LEON_REGION_NO_REFERENCE
 * D = 3 happens: a closed GOP's leading B picture names its I picture for both directions.  A vector points from a macroblock of M
 * to where it reads in the reference: an object at p in the reference is at p - v/2 in M (sense -1: from the reference to the picture
 * that predicts from it), an object at p in M came from p + v/2 in the reference (sense +1).
 * Votes.  Macroblock (i, j) of M's record covers frame pixels [16i, 16i+16) x [16j, 16j+16); its weight is the pixel area it shares
 * with the box (x, y, w, h),
 *     a = (min(x+w, 16i+16) - max(x, 16i)) * (min(y+h, 16j+16) - max(y, 16j))          1 .. 256
 * over i = x>>4 .. (x+w-1)>>4 and the same range for j (a box inside the frame never leaves the coded grid).  For each direction
 * bit b of D, a macroblock with info & b adds a to A, a * mv_h(b) to SH and a * mv_v(b) to SV: a bidirectional macroblock under
 * D = 3 votes twice.  Macroblocks with info & 4 add a to I.  All sums are int64 (2^16 macroblocks, weight 2^8, |int16| up to 2^15,
 * two directions: 2^40).
 * The moved box.
 *     dh = A ? floor((sense * SH + A) / (2 * A)) : 0          half-pel -> pixels, to nearest, ties up; FLOOR division, also for negatives
 *     dv likewise with SV
 *     x' = clamp(x + dh, 0, frame_width - w),  y' = clamp(y + dv, 0, frame_height - h);  w, h unchanged
 *     votes[4] = { A, I, dh, dv }                              dh, dv before the clamp; A <= 2wh and I <= wh fit int32
 * Order of judgement, regions_check's, one text for host and device (csrc/leon_carry.h): LEON_REGION_RESERVED, LEON_REGION_FRAME
 * (either frame or target outside the window), LEON_REGION_BOX (empty, or leaves the frame), LEON_REGION_NO_REFERENCE.  A record
 * whose status is not 0 has not one byte of its output record or votes written.
 * ON BOTH ROADS A RECORD'S FAULT IS A STATUS WORD, NEVER AN ERROR OF THE CALL -- the host roads of the other families refuse the
 * whole call instead.  A pair of frames with no prediction between them is a property of the stream and the seek, not a caller's bug.
 * One launch per call (k_carry: a 64-lane wave per record, four records per workgroup); the window's table (ring id, fwd, bwd per
 * frame) is the scratch it needs. */
#define LEON_REGION_NO_REFERENCE 9   /* carry regions only: no prediction joins frame and target inside the window */
typedef struct leon_pipeline_carry_region {
    int32_t frame;                 /* the frame the box is on (index into the window's frames[]) */
    int32_t x, y, width, height;   /* the box, frame pixels; non-empty, inside the frame */
    int32_t target;                /* the frame to carry it to */
    int32_t reserved[2];           /* must be 0 */
} leon_pipeline_carry_region;      /* 32 bytes */
typedef struct leon_pipeline_carry_regions_call {
    const leon_pipeline_carry_region* regions;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    leon_pipeline_region* device_out;      /* DEVICE memory, n records, 4-byte aligned */
    int32_t* device_votes;                 /* DEVICE memory, n x 4 words {A, I, dh, dv}, 4-byte aligned, may be NULL */
    int32_t* device_status;                /* DEVICE memory, n words, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[2];                  /* must be 0 */
} leon_pipeline_carry_regions_call;        /* 64 bytes */
/* host only: the resolution rule above for the n_frames frames of a window and their motion frames (leon_pipeline_window_motion) */
int leon_pipeline_carry_refs(const leon_pipeline_frame* frames, const leon_pipeline_motion_frame* motion, int32_t n_frames,
                             int32_t* fwd, int32_t* bwd);
/* host only: the definition on the CPU (the text the kernel compiles too) for one record, from motion records in host memory laid out
 * as leon_pipeline_motion_layout(mb_width, mb_height) says: records[i] is window frame i's, NULL allowed for frames that are not M.
 * Returns the record's status word (>= 0; out and votes, 8 and 4 words, are written exactly when it is 0; votes may be NULL), or
 * LEON_ERR_INVALID (negative) for a null argument, a grid outside 1 .. 256, a frame larger than the grid or below 1, n_frames < 0, a
 * NULL record where M's is needed. */
int32_t leon_pipeline_carry_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                   const int32_t* fwd, const int32_t* bwd, const void* const* records, const leon_pipeline_carry_region* rec,
                                   leon_pipeline_region* out, int32_t* votes);
/* what the pipeline resolved for a delivered, not yet released window (n = its n_frames); LEON_ERR_INVALID as leon_pipeline_window_motion */
int leon_pipeline_get_carry_refs(leon_pipeline* p, int64_t window, int32_t* fwd, int32_t* bwd, int32_t n);
/* Records in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits), with
 * leon_pipeline_warp_regions_device's ordering rules and its scratch event, word for word.  It needs the MOTION bit only, not TENSOR.
 * Refused (LEON_ERR_INVALID, nothing enqueued): a pipeline without the MOTION bit, a window that is not out for delivery or was
 * delivered with an error, a null call, `regions` or `device_out`, a pointer that is not 4-byte aligned, n outside 1 .. 65535, a
 * non-zero reserved word of the call. */
int leon_pipeline_carry_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_carry_regions_call* call);
/* Records in host memory, results to host memory, synchronous: the device road between an upload and three copies.  out (n records),
 * votes (n x 4 words, may be NULL) and status (n words, may be NULL) go up and come back whole, so a refused record's words stay as
 * the caller had them.  The call-level refusals are the device road's. */
int leon_pipeline_carry_regions(leon_pipeline* p, int64_t window, const leon_pipeline_carry_region* regions, int32_t n,
                                leon_pipeline_region* out, int32_t* votes, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_resize_weights_device: k_carry on motion records the CALLER supplies (host memory,
 * records_host[i] of window frame i, laid out as leon_pipeline_motion_layout says; NULL for frames whose record no region of the call
 * votes with), with memory of its own on device_id's null stream, synchronous; regions, out, votes (may be NULL) and status (may be
 * NULL) in host memory, going up and coming back whole.  Refused (LEON_ERR_INVALID): what leon_pipeline_carry_record refuses, n
 * outside 1 .. 65535, a fwd or bwd entry outside -1 .. n_frames - 1. */
int leon_pipeline_carry_device(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                               const int32_t* fwd, const int32_t* bwd, const void* const* records_host, const leon_pipeline_carry_region* regions,
                               int32_t n, leon_pipeline_region* out, int32_t* votes, int32_t* status);
/* Dense maps propagated along the stream's motion vectors: the models beside a detector give a label mask, keypoint heatmaps or a
 * feature map, not boxes.  The network runs on the anchors, and its output is warped to the P and B pictures along the motion records
 * (LEON_PIPELINE_OUTPUT_MOTION), on the device.  The dense counterpart of the carry family above.  Integers only, and NO arithmetic
 * on a map's elements: they are opaque bytes, so uint8 labels, fp16 heatmaps and fp32 features are all exact.
 * Maps.  A map lies over the FRAME (not the coded picture) at `stride` s = 1, 2, 4, 8 or 16 frame pixels a cell:
 *     mw = ceil(frame_width / s), mh = ceil(frame_height / s)
 * It has `planes` planes (1 .. 4096), each [mh][mw], of elements of `elem_bytes` e = 1, 2 or 4.  The caller's buffer `maps` holds
 * n_slots maps (1 .. 65535) at slot_pitch_bytes, a multiple of 4 that is at least planes * mh * mw * e; a contiguous tensor
 * [n_slots][planes][mh][mw] is the normal case.  maps_bytes is what the caller vouches for; it is at least n_slots * slot_pitch_bytes.
 * A HOP writes the map of window frame `target` T from the maps of the pictures T predicts from: a GATHER THROUGH T'S OWN MOTION
 * RECORD.  That is the one direction in which a block-motion field defines every output cell exactly once; there is no scatter and no
 * sense +1.  The record is 32 bytes (leon_pipeline_propagate_hop below): target, dst_slot, fwd_slot, bwd_slot and four reserved words
 * that must be 0.  fwd_slot / bwd_slot hold the maps of the pictures T's forward and backward vectors point into, -1: not supplied.
 * THE CALLER VOUCHES FOR WHICH PICTURE A SLOT HOLDS; the kernel needs T's record alone, so a map kept from an earlier window serves an
 * open GOP's leading B pictures.
 * Per cell (cx, cy) of T, with info and mv of macroblock k = ((cy * s) >> 4) * mb_width + ((cx * s) >> 4) of T's record:
 *     info & 1 and fwd_slot >= 0            : forward:  source = the fwd slot, v = (fwd_h, fwd_v), via = 1
 *     else info & 2 and bwd_slot >= 0       : backward: source = the bwd slot, v = (bwd_h, bwd_v), via = 2
 *     else                                  : via = 0, and every plane of the cell gets `fill` (its low e bytes)
 * A bidirectional macroblock takes the forward map when both are supplied: no averaging, elements are opaque.  Where via != 0,
 *     dx = (v_h + s) >> (1 + log2 s)   = floor((v_h + s) / (2 s))    half-pel luma units to cells, to nearest, ties up; floor also
 *     dy likewise with v_v                                            below zero (the shift is arithmetic)
 *     sx = clamp(cx + dx, 0, mw - 1),  sy = clamp(cy + dy, 0, mh - 1)
 *     dst[pl][cy][cx] = src[pl][sy][sx]                               for every plane pl
 * via[cy][cx], one byte a cell, goes to an optional output [n][mh][mw] (record i's map at i * mh * mw).  Every cell of every plane of
 * dst_slot and every byte of the record's via map are written; an I picture as target is all fill, status 0.
 * Order of judgement: LEON_REGION_RESERVED, LEON_REGION_FRAME (target outside the window), LEON_REGION_SLOT (dst_slot outside
 * 0 .. n_slots - 1, a source outside -1 .. n_slots - 1, or dst_slot equal to a supplied source).  A refused record has not one byte
 * of its slot or via map written.  As in the carry family A RECORD'S FAULT IS A STATUS WORD ON BOTH ROADS, NEVER AN ERROR OF THE CALL.
 * Records of one call must not name another record's dst_slot, as destination or as source (chain the levels of a GOP in calls of
 * their own: leon_ctypes.propagate_plan).  This is not checked; the result is unspecified, but every address stays in bounds.
 * One launch per call (k_propagate; one text for host and device: csrc/leon_propagate.h).  No load touches a byte outside
 * [maps, maps + maps_bytes), no store falls outside dst_slot's planes * mh * mw * e bytes.
 * NOT in this definition: averaging of bidirectional macroblocks, intra cells filled from the co-located source cell, chroma-style
 * scaling of the vectors, interpolation between cells. */
#define LEON_REGION_SLOT 10          /* propagate records only: a slot outside the buffer, or the destination among the sources */
typedef struct leon_pipeline_propagate_hop {
    int32_t target;                /* the frame whose map is written (index into the window's frames[]) */
    int32_t dst_slot;              /* the map that is written */
    int32_t fwd_slot, bwd_slot;    /* the maps of the pictures T's forward / backward vectors point into; -1: not supplied */
    int32_t reserved[4];           /* must be 0 */
} leon_pipeline_propagate_hop;     /* 32 bytes */
typedef struct leon_pipeline_propagate_config {
    int32_t  stride;               /* 1, 2, 4, 8, 16 */
    int32_t  planes;               /* 1 .. 4096 */
    int32_t  elem_bytes;           /* 1, 2, 4 */
    int32_t  n_slots;              /* 1 .. 65535 */
    uint32_t fill;                 /* its low elem_bytes bytes fill the cells with via 0 */
    int32_t  reserved0;            /* must be 0 */
    uint64_t slot_pitch_bytes;     /* a multiple of 4, at least planes * mh * mw * elem_bytes */
    uint64_t maps_bytes;           /* what the caller vouches for behind `maps`: at least n_slots * slot_pitch_bytes */
} leon_pipeline_propagate_config;  /* 40 bytes */
/* (a struct tag only, as leon_pipeline_motion_layout: the host call that fills it has the same name) */
struct leon_pipeline_propagate_layout {
    int32_t  mw, mh;               /* cells of a map */
    int32_t  planes_per_group;     /* planes one lane of k_propagate loops over (grid y = ceil(planes / planes_per_group)) */
    int32_t  fast_path;            /* 1: a work unit is a destination dword (mw * e and (16 / s) * e multiples of 4), 0: a cell */
    uint64_t plane_bytes;          /* mh * mw * elem_bytes */
    uint64_t slot_bytes;           /* planes * plane_bytes: the least slot_pitch_bytes (always a multiple of 4 on the fast path) */
};                                 /* 32 bytes */
typedef struct leon_pipeline_propagate_maps_call {
    const leon_pipeline_propagate_hop* hops;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    void*    maps;                         /* DEVICE memory, cfg->maps_bytes bytes, 4-byte aligned; written in place */
    uint8_t* device_via;                   /* DEVICE memory, n x mh x mw bytes, 4-byte aligned, may be NULL */
    int32_t* device_status;                /* DEVICE memory, n words, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[2];                  /* must be 0 */
} leon_pipeline_propagate_maps_call;       /* 64 bytes */
/* host only: the sizes of a map.  LEON_ERR_INVALID: a null `out`, a frame outside 1 .. 4096 an axis, a stride, plane count or element
 * size outside the above. */
int leon_pipeline_propagate_layout(int32_t frame_width, int32_t frame_height, int32_t stride, int32_t planes, int32_t elem_bytes,
                                   struct leon_pipeline_propagate_layout* out);
/* host only: the definition on the CPU (the text the kernel compiles too) for one record, everything in host memory: records[i] is
 * window frame i's motion record laid out as leon_pipeline_motion_layout(mb_width, mb_height) says (only records[target] is read),
 * maps the buffer of cfg->maps_bytes bytes, via this record's [mh][mw] bytes (may be NULL).  Returns the record's status word (>= 0;
 * the slot and via are written exactly when it is 0), or LEON_ERR_INVALID (negative) for a null argument, a grid outside 1 .. 256, a
 * frame larger than the grid or below 1, n_frames < 0, a cfg the device road refuses, maps not 4-byte aligned, a NULL record of the
 * target's. */
int32_t leon_pipeline_propagate_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                       const void* const* records, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hop,
                                       void* maps, uint8_t* via);
/* Everything in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits),
 * with leon_pipeline_carry_regions_device's ordering rules and scratch, word for word.  It needs the MOTION bit only.
 * Refused (LEON_ERR_INVALID, nothing enqueued): what leon_pipeline_carry_regions_device refuses (no MOTION bit, a window that is not
 * out for delivery or was delivered with an error, a null call, `hops` or `maps`, a pointer that is not 4-byte aligned, n outside
 * 1 .. 65535, a non-zero reserved word of the call), a null cfg, a stride, element size, plane count, n_slots or slot_pitch_bytes
 * outside the above, maps_bytes below n_slots * slot_pitch_bytes, a non-zero reserved word of cfg. */
int leon_pipeline_propagate_maps_device(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg,
                                        const leon_pipeline_propagate_maps_call* call);
/* Records and maps in host memory, synchronous: the device road between an upload and the copies back.  maps (cfg->maps_bytes bytes),
 * via (n x mh x mw bytes, may be NULL) and status (n words, may be NULL) go up and come back whole, so bytes the kernel leaves alone
 * stay the caller's.  The call-level refusals are the device road's. */
int leon_pipeline_propagate_maps(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops,
                                 int32_t n, void* maps, uint8_t* via, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_carry_device: k_propagate on motion records the CALLER supplies (host memory,
 * records_host[i] of window frame i; NULL for frames no hop of the call targets), with memory of its own on device_id's null stream,
 * synchronous; hops, maps, via (may be NULL) and status (may be NULL) in host memory, going up and coming back whole.  Refused
 * (LEON_ERR_INVALID): what leon_pipeline_propagate_record refuses, n outside 1 .. 65535, a valid hop whose target has no record. */
int leon_pipeline_propagate_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                   const void* const* records_host, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops,
                                   int32_t n, void* maps, uint8_t* via, int32_t* status);
/* Motion and residual accumulated along a GOP's chain: what the compressed-domain video networks (CoViAR and its successors) read.  A
 * P picture's vectors and residual (LEON_PIPELINE_OUTPUT_MOTION, LEON_PIPELINE_OUTPUT_RESIDUAL) are relative to the picture before it,
 * which is itself a prediction; they mean something once they are traced back to a picture the model has seen.  For every sample of
 * a P or B picture an accumulator says where the sample came from in the picture the chain started at and the sum of everything the
 * stream added along that path.  The arithmetic counterpart of the propagate family above, on the device.  Integers only.
 * Accumulator.  An accumulator lies over the CODED picture (cw x ch, as the residual record does) and consists of int16 planes chosen
 * by `parts`:
 *     LEON_ACCUMULATE_MOTION (1)   : AX, AY, AGE, each [ch][luma_stride]
 *     LEON_ACCUMULATE_RESIDUAL (2) : RY [ch][luma_stride], RCb and RCr [ch / 2][chroma_stride]
 * Strides follow leon_pipeline_residual_layout: luma_stride = pad64(cw), chroma_stride = pad64(cw / 2), in elements.  Every plane starts
 * on a 256-byte boundary, in the order above, and absent parts take no room: with parts = 2 the three planes lie exactly as a residual
 * record's do, at the same offsets.  The caller's buffer `slots` holds n_slots accumulators (1 .. 65535) at slot_pitch_bytes, a multiple
 * of 4 that is at least slot_bytes.  slots_bytes is what the caller vouches for; it is at least n_slots * slot_pitch_bytes.
 * A HOP is the propagate family's 32-byte record as it is (leon_pipeline_propagate_hop: target, dst_slot, fwd_slot, bwd_slot, four
 * reserved words), judged as there and in the same order: LEON_REGION_RESERVED, LEON_REGION_FRAME, LEON_REGION_SLOT.  What
 * leon_ctypes.propagate_plan makes feeds the call unchanged.  It writes the accumulator of window frame `target` T from those of the
 * pictures T predicts from: a gather through T's own motion record.  THE CALLER VOUCHES FOR WHICH PICTURE A SLOT HOLDS.
 * The pick, per macroblock k of T's motion record, is the propagate family's word for word: forward where info & 1 and fwd_slot >= 0
 * (via = 1), else backward where info & 2 and bwd_slot >= 0 (via = 2), else a restart (via = 0).  via, one byte per MACROBLOCK, goes to
 * an optional output [n][mbh][mbw].  A bidirectional macroblock takes the forward source: no averaging.
 * A restart macroblock (via = 0): every element of every plane asked for under the macroblock is 0 -- the sample is its own origin.
 * An I picture as target is all zero with status 0: that is how a chain's start is written (a hop with both sources -1 does the same).
 * Luma.  For luma element (x, y) under a macroblock with vector v and source slot S:
 *     dx = (v_h + 1) >> 1,  dy = (v_v + 1) >> 1                    the propagate rule at stride 1: arithmetic shift, ties up
 *     sx = clamp(x + dx, 0, cw - 1),  sy = clamp(y + dy, 0, ch - 1)
 *     AX[y][x]  = sat16(S.AX[sy][sx]  + (sx - x))                   the own term is the displacement AFTER the clamp, so
 *     AY[y][x]  = sat16(S.AY[sy][sx]  + (sy - y))                   0 <= x + AX <= cw - 1 whenever the sources obey it (AY likewise)
 *     AGE[y][x] = sat16(S.AGE[sy][sx] + 1)
 *     RY[y][x]  = sat16(S.RY[sy][sx]  + res_T.Y[y][x])              res_T: T's residual record; sat16: saturation to -32768 .. 32767
 * Chroma.  For element (x, y) of the cw / 2 x ch / 2 planes, with macroblock (y >> 3) * mb_width + (x >> 3):
 *     dx = (v_h + 2) >> 2,  dy likewise                             the propagate rule at stride 2; the clamp is to the chroma plane
 *     R[y][x] = sat16(S.R[sy][sx] + res_T[y][x])                    for RCb and RCr
 * Meaning.  With O the picture reached after AGE hops, frame_T(p) ~ O(p + A_T(p)) + R_T(p); exactly so for luma where every vector
 * on the chain is full-pel and no clamp to 0 .. 255 acted.
 * A refused hop has not one byte of its slot or via written; A RECORD'S FAULT IS A STATUS WORD ON BOTH ROADS, NEVER AN ERROR OF THE
 * CALL.  Pad columns behind cw (cw / 2) of a destination are unspecified.  No store falls outside the destination's slot_bytes, no
 * load outside [slots, slots + slots_bytes).  Hops of one call must not name another hop's dst_slot, as destination or as source;
 * this is not checked, the result is unspecified, but every address stays in bounds.  One launch per call (k_accumulate; one text for
 * host and device: csrc/leon_accumulate.h).
 * Outputs.  MOTION is always needed, RESIDUAL when parts & 2; a pipeline lacking one is refused as the gauge family refuses.
 * NOT in this definition: half-pel interpolation of accumulators, averaging of both references, rebasing a restart cell against the
 * I picture, the decoder's own chroma vector derivation. */
#define LEON_ACCUMULATE_MOTION   1
#define LEON_ACCUMULATE_RESIDUAL 2
typedef struct leon_pipeline_accumulate_config {
    int32_t  parts;                /* LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3 */
    int32_t  n_slots;              /* 1 .. 65535 */
    int32_t  reserved[2];          /* must be 0 */
    uint64_t slot_pitch_bytes;     /* a multiple of 4, at least the layout's slot_bytes */
    uint64_t slots_bytes;          /* what the caller vouches for behind `slots`: at least n_slots * slot_pitch_bytes */
} leon_pipeline_accumulate_config; /* 32 bytes */
/* (a struct tag only, as leon_pipeline_propagate_layout: the host call that fills it has the same name) */
struct leon_pipeline_accumulate_layout {
    int32_t  coded_width, coded_height;
    int32_t  parts;
    int32_t  planes;               /* planes asked for: 3 or 6 (k_accumulate's grid y) */
    int32_t  luma_stride, chroma_stride;   /* elements a row */
    uint32_t ax_offset, ay_offset, age_offset, ry_offset, rcb_offset, rcr_offset;   /* bytes into a slot; 0 for an absent plane */
    uint32_t slot_bytes;           /* the least slot_pitch_bytes */
    uint32_t slot_pitch;           /* pad256(slot_bytes) */
    uint32_t reserved[2];
};                                 /* 64 bytes */
typedef struct leon_pipeline_accumulate_call {
    const leon_pipeline_propagate_hop* hops;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    void*    slots;                        /* DEVICE memory, cfg->slots_bytes bytes, 4-byte aligned; written in place */
    uint8_t* device_via;                   /* DEVICE memory, n x mbh x mbw bytes, may be NULL */
    int32_t* device_status;                /* DEVICE memory, n words, 4-byte aligned, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[2];                  /* must be 0 */
} leon_pipeline_accumulate_call;           /* 64 bytes */
/* host only: where the planes of an accumulator lie.  LEON_ERR_INVALID: a null `out`, a coded size the residual layout refuses, parts
 * outside 1 .. 3. */
int leon_pipeline_accumulate_layout(int32_t coded_width, int32_t coded_height, int32_t parts, struct leon_pipeline_accumulate_layout* out);
/* host only: the definition on the CPU (the text the kernel compiles too) for one hop, everything in host memory: motion_records[i] and
 * residual_records[i] are window frame i's records laid out as leon_pipeline_motion_layout(coded_width / 16, coded_height / 16) and
 * leon_pipeline_residual_layout say (only the target's are read; residual_records may be NULL without LEON_ACCUMULATE_RESIDUAL), slots
 * the buffer of cfg->slots_bytes bytes, via this hop's [mbh][mbw] bytes (may be NULL).  Returns the hop's status word (>= 0; the slot and
 * via are written exactly when it is 0), or LEON_ERR_INVALID (negative) for a null argument, a coded size or cfg the device road
 * refuses, n_frames < 0, slots not 4-byte aligned, a missing or misaligned record of the target's. */
int32_t leon_pipeline_accumulate_record(int32_t coded_width, int32_t coded_height, int32_t n_frames, const void* const* motion_records,
                                        const void* const* residual_records, const leon_pipeline_accumulate_config* cfg,
                                        const leon_pipeline_propagate_hop* hop, void* slots, uint8_t* via);
/* Everything in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits),
 * with leon_pipeline_propagate_maps_device's ordering rules and scratch, word for word.
 * Refused (LEON_ERR_INVALID, nothing enqueued): a null cfg, parts outside 1 .. 3, a non-zero reserved word of cfg, a pipeline without
 * the outputs the parts need, a window that is not out for delivery or was delivered with an error, a null call, `hops` or `slots`,
 * hops, slots or device_status not 4-byte aligned, n outside 1 .. 65535, a non-zero reserved word of the call, n_slots or
 * slot_pitch_bytes outside the above, slots_bytes below n_slots * slot_pitch_bytes. */
int leon_pipeline_accumulate_device(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_accumulate_call* call);
/* Hops and accumulators in host memory, synchronous: the device road between an upload and the copies back.  slots (cfg->slots_bytes
 * bytes), via (n x mbh x mbw bytes, may be NULL) and status (n words, may be NULL) go up and come back whole, so bytes the kernel
 * leaves alone stay the caller's.  The call-level refusals are the device road's. */
int leon_pipeline_accumulate(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hops,
                             int32_t n, void* slots, uint8_t* via, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_propagate_kernel: k_accumulate on motion and residual records the CALLER supplies (host
 * memory, records of window frame i; NULL for frames no hop of the call targets), with memory of its own on device_id's null stream,
 * synchronous; hops, slots, via (may be NULL) and status (may be NULL) in host memory, going up and coming back whole.  Refused
 * (LEON_ERR_INVALID): what leon_pipeline_accumulate_record refuses, n outside 1 .. 65535, a valid hop whose target lacks a record. */
int leon_pipeline_accumulate_kernel(int32_t device_id, int32_t coded_width, int32_t coded_height, int32_t n_frames, const void* const* motion_records_host,
                                    const void* const* residual_records_host, const leon_pipeline_accumulate_config* cfg,
                                    const leon_pipeline_propagate_hop* hops, int32_t n, void* slots, uint8_t* via, int32_t* status);
/* Field tensors: boxes of the record side's int16 planes -- a motion record's vectors, a residual record's planes, the accumulators
 * above -- resampled into one [N, C, h, w] batch of a model's element type, cropped by the same box records and through the same tables
 * as the pixel tensors of leon_pipeline_resample_regions, on the caller's stream.  What a CoViAR-style network takes as its motion
 * input [2, 224, 224] and residual input [3, 224, 224] beside its RGB input.
 * Field.  A field is a plane of int16 that lies over the frame at a power-of-two cell size.  Channel c of a call is described by
 * offset_bytes (into the item, a multiple of 2), row_stride (elements, >= 0), elem_stride (1 .. 4 elements), shift (0 .. 4) and scale,
 * bias (float).  Its value at frame pixel (x, y), 0 <= x < frame_width, 0 <= y < frame_height, is
 *     p_c[y][x] = item[offset_bytes / 2 + (y >> shift) * row_stride + (x >> shift) * elem_stride]
 * -- nearest-neighbour replication of the cell, as the compressed-domain models lay a macroblock's vector over its 16 x 16 pixels:
 *     luma-sized planes (AX, AY, AGE, RY, a residual record's Y):  shift 0, elem_stride 1, row_stride the plane's stride
 *     chroma planes:                                               shift 1, elem_stride 1, row_stride the chroma stride
 *     a motion record's fwd_h, fwd_v, bwd_h, bwd_v:                shift 4, elem_stride 4, row_stride 4 * mb_width, offsets 0 / 2 / 4 / 6
 * Source.  One kind per call: LEON_FIELD_SOURCE_BUFFER (0), the caller's device memory holding n_items items (1 .. 65535) at
 * item_pitch_bytes (a multiple of 2), of which the caller vouches for source_bytes; a record's `frame` word is the item index, and the
 * window of the call is not consulted.  LEON_FIELD_SOURCE_MOTION (1): the window frame's motion record (needs
 * LEON_PIPELINE_OUTPUT_MOTION).  LEON_FIELD_SOURCE_RESIDUAL (2): the window frame's residual record (needs the RESIDUAL bit).  A
 * pipeline lacking the output is refused as the gauge family refuses.  For the two record sources the pipeline roads read neither
 * n_items, item_pitch_bytes nor source_bytes, and the call's `source` pointer must be NULL.
 * Records.  A record is a leon_pipeline_region as it is (frame, x, y, width, height, three reserved words), the box in frame pixels,
 * judged by leon_pipeline_regions_check's text in its order against the FRAME size: LEON_REGION_RESERVED, _FRAME (for a BUFFER source:
 * an item index outside n_items), _BOX, _RATIO_X, _RATIO_Y, _TAPS.  What leon_pipeline_carry_regions_device and
 * leon_pipeline_propose_regions_device write goes in unchanged for the two record sources.  A RECORD'S FAULT IS A STATUS WORD ON BOTH
 * ROADS, NEVER AN ERROR OF THE CALL; a refused record has not one byte of its tensor written.
 * Resampling.  The pixel road's tables, unchanged: leon_pipeline_resize_weights(frame_size, box_start, box_size, out_size,
 * LEON_RESIZE_TRIANGLE), 22 fractional bits, for each axis; taps may leave the box, never the frame.  Exact integers:
 *     h[y][o]  = sat16((2^21 + sum_k Wx[o][k]  * p_c[y][first_x[o] + k]) >> 22)       horizontal first; an arithmetic shift
 *     r[oy][o] = sat16((2^21 + sum_k Wy[oy][k] * h[first_y[oy] + k][o]) >> 22)        then vertical
 * (the sums need more than 32 bits; an implementation may split p or use 64-bit multiply-adds as long as the result is the exact
 * integer).  For the same box and size a field tensor is aligned sample for sample with the pixel tensor leon_pipeline_resample_regions
 * gives.
 * Element.  out[i][c][oy][ox] = to_dtype(u), u = fl32(fl32((float)r * scale_c) + bias_c): two separately rounded binary32 operations,
 * no contraction, then one rounding to nearest even to fp16 / bf16 (the identity for fp32).  dtype: LEON_TENSOR_F16 / _BF16 / _F32.
 * Layout CHW, dense, C = 1 .. LEON_FIELD_MAX_CHANNELS.  Region i lies at i * out_pitch_bytes; a pitch of 0 means C * oh * ow * element
 * bytes rounded up to 256.
 * Refused at the call (LEON_ERR_INVALID, nothing enqueued): a non-finite scale or bias; a channel for which
 * fl32(fl32(32768 * |scale|) + |bias|) is not finite in the element type (so every stored element is finite); C outside 1 .. 8; shift,
 * elem_stride, row_stride or offset_bytes outside the above; out sizes outside 1 .. 4096; another filter, dtype or source; a non-zero
 * reserved word; misaligned pointers (records and device_status 4 bytes, source 2, device_out 256; out_pitch_bytes a multiple of 256);
 * a channel whose last element lies outside the item -- offset_bytes + 2 * (((fh - 1) >> shift) * row_stride + ((fw - 1) >> shift) *
 * elem_stride) + 2 above item_pitch_bytes, or for the record sources above the record's bytes --; source_bytes < n_items *
 * item_pitch_bytes.  No load falls outside the source, no store outside a valid region's tensor bytes.
 * One text for host and device: csrc/leon_fields.h.  Per chunk of regions k_box_tables (as leon_pipeline_resample_regions_device runs
 * it, the tables in the pipeline's bounded regions scratch) and k_fields.
 * NOT in this definition: bicubic; uint8 elements and HWC; letterbox fit; converting a YCbCr residual to RGB differences; rescaling
 * vectors by the resize ratio -- vectors are in half-pel FRAME units, and scale = 0.5 * out_size / box_size makes them output pixels. */
#define LEON_FIELD_SOURCE_BUFFER   0
#define LEON_FIELD_SOURCE_MOTION   1
#define LEON_FIELD_SOURCE_RESIDUAL 2
#define LEON_FIELD_MAX_CHANNELS    8
typedef struct leon_pipeline_field_channel {
    uint32_t offset_bytes;         /* into the item, a multiple of 2 */
    int32_t  row_stride;           /* elements, >= 0 */
    int32_t  elem_stride;          /* 1 .. 4 elements */
    int32_t  shift;                /* 0 .. 4: the cell is 1 << shift frame pixels */
    float    scale, bias;
    int32_t  reserved[2];          /* must be 0 */
} leon_pipeline_field_channel;     /* 32 bytes */
typedef struct leon_pipeline_field_config {
    int32_t  source;               /* LEON_FIELD_SOURCE_* */
    int32_t  dtype;                /* LEON_TENSOR_F16 / _BF16 / _F32 */
    int32_t  channels;             /* 1 .. LEON_FIELD_MAX_CHANNELS */
    int32_t  filter;               /* LEON_RESIZE_TRIANGLE */
    int32_t  out_width, out_height;/* 1 .. 4096 */
    int32_t  n_items;              /* 1 .. 65535 */
    int32_t  reserved;             /* must be 0 */
    uint64_t item_pitch_bytes;     /* a multiple of 2 */
    uint64_t source_bytes;         /* at least n_items * item_pitch_bytes */
    leon_pipeline_field_channel channel[LEON_FIELD_MAX_CHANNELS];
} leon_pipeline_field_config;      /* 304 bytes */
typedef struct leon_pipeline_field_tensors_call {
    const leon_pipeline_region* records;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    const void* source;                    /* DEVICE memory, cfg->source_bytes bytes, 2-byte aligned; NULL for the record sources */
    void*    device_out;                   /* DEVICE memory, 256-byte aligned, (n - 1) * pitch + a region's bytes */
    uint64_t out_pitch_bytes;              /* 0, or a multiple of 256 not below a region's bytes */
    int32_t* device_status;                /* DEVICE memory, n words, 4-byte aligned, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved;                     /* must be 0 */
} leon_pipeline_field_tensors_call;        /* 64 bytes */
/* host only: the definition on the CPU (the text the kernel compiles too) for one record, everything in host memory.  items: n_items
 * items at item_pitch_bytes, for every source -- a record source's items are records laid out as leon_pipeline_motion_layout(
 * coded_width / 16, coded_height / 16) or leon_pipeline_residual_layout(coded_width, coded_height) say, at an item_pitch_bytes not
 * below the record's bytes, which are then the channels' limit.  out: the record's dense tensor, C * oh * ow elements, aligned to its
 * element.  Returns the record's status word (>= 0; the tensor is written exactly when it is 0), or LEON_ERR_INVALID (negative) for a
 * null argument, a frame size outside 1 .. 4096, a coded size the record's layout refuses, or a cfg the device road refuses. */
int32_t leon_pipeline_field_tensor_record(int32_t frame_width, int32_t frame_height, int32_t coded_width, int32_t coded_height,
                                          const leon_pipeline_field_config* cfg, const void* items, const leon_pipeline_region* record, void* out);
/* Everything in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits),
 * with leon_pipeline_resample_regions_device's ordering rules and scratch; the window's records are reached through the table the
 * carry, gauge and propagate calls read them through.  Refused (LEON_ERR_INVALID, nothing enqueued): the list above, a null cfg or
 * call, a pipeline without the source's output, a window (record sources) that is not out for delivery or was delivered with an
 * error, n outside 1 .. 65535, a null records or device_out, a null source with LEON_FIELD_SOURCE_BUFFER and a non-null one without. */
int leon_pipeline_field_tensors_device(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_field_tensors_call* call);
/* Records, source (BUFFER only; NULL otherwise), tensors and status in host memory, synchronous: the device road between an upload and
 * the copies back.  out (n regions out_pitch_bytes apart; 0: the default pitch) and status (n words, may be NULL) go up and come back
 * whole, so bytes the kernel leaves alone -- a refused record's tensor, the gap behind a tensor -- stay the caller's. */
int leon_pipeline_field_tensors(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_region* records, int32_t n,
                                const void* source, void* out, uint64_t out_pitch_bytes, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_accumulate_kernel: k_box_tables and k_fields on items the CALLER supplies (host memory,
 * as leon_pipeline_field_tensor_record takes them), with explicit frame and coded sizes and no pipeline, memory of its own on
 * device_id's null stream, synchronous; records, out and status (may be NULL) in host memory, going up and coming back whole.
 * scratch_limit_bytes: the bytes of table scratch a chunk of regions may take (0: 256 MiB), so that a test can make a call of
 * several chunks.  Refused: what leon_pipeline_field_tensor_record refuses, n outside 1 .. 65535, a limit below one region's tables. */
int leon_pipeline_field_tensors_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t coded_width, int32_t coded_height,
                                       const leon_pipeline_field_config* cfg, const void* items, const leon_pipeline_region* records, int32_t n, void* out,
                                       uint64_t out_pitch_bytes, int32_t* status, uint64_t scratch_limit_bytes);
/* Boxes gauged: what a frame's motion record (LEON_PIPELINE_OUTPUT_MOTION) and activity record (LEON_PIPELINE_OUTPUT_ACTIVITY) say
 * under each box, on the device -- what a "run the detector again here" gate reads of a box that the carry family moved.  Integers only.
 * Records.  A record is a leon_pipeline_region (frame, the box, three reserved words that must be 0): exactly what
 * leon_pipeline_carry_regions_device writes, so its output goes in as it is.  Judged in regions_check's order, one text for host and
 * device (csrc/leon_gauge.h): LEON_REGION_RESERVED (a non-zero reserved word), LEON_REGION_FRAME (frame outside the window),
 * LEON_REGION_BOX (empty, or leaves the frame: the carry family's expression).  As in the carry and propagate families A RECORD'S FAULT
 * IS A STATUS WORD ON BOTH ROADS, NEVER AN ERROR OF THE CALL: the boxes come from k_carry, whose refused records hold unspecified bytes.
 * A record whose status is not 0 has not one byte of its statistics written.
 * Cover and weight, the carry family's: macroblocks (i, j) over i = x>>4 .. (x+w-1)>>4 and the same range for j, each with the pixel
 * area a it shares with the box, 1 .. 256 (the formula under "Votes" above).
 * Sources.  cfg->sources is a bit set of the call: LEON_GAUGE_MOTION (1) the frame's motion record, LEON_GAUGE_ACTIVITY (2) its
 * activity record.  The words of a source that was not asked for are written as 0.
 * Statistics: 16 int64 words (128 bytes) a record.  With cell = the macroblock's activity cell and info, mv = its motion entry:
 *     [0]        the sum of a: equals w * h for every accepted box; always written
 *     [1]        the sum of a over cells with blocks != 0                                             (activity)
 *     [2 .. 6]   the sums of a * ac_count, a * ac_mag, a * dc_mag, a * qscale, a * popcount(blocks)   (activity)
 *     [7]        the maximum of ac_mag over the cover, unweighted                                     (activity)
 *     [8 .. 10]  the sums of a over macroblocks with info & 1, info & 2, info & 4                     (motion)
 *     [11]       the sum of a over macroblocks with any non-zero vector word                          (motion)
 *     [12 .. 15] the sums of a * |fwd_h|, a * |fwd_v|, a * |bwd_h|, a * |bwd_v|                       (motion)
 * Bounds.  The sum of a is at most 4096^2 = 2^24; a value is at most 65535, a vector's magnitude at most 32768: the largest word is
 * below 2^41 (and every word below 2^53, exact in a double).
 * Two identities.  Word 0 = w * h.  For a frame whose size is its coded size (a multiple of 16 an axis), the whole-frame box gives
 * 256 x the records' own summary words: activity summary [0], [1], [2], [3], [5], [6] in words 1, 2, 3, 4, 5, 6, activity summary [4]
 * itself in word 7, motion summary [0 .. 7] in words 8 .. 15.
 * One launch per call (k_gauge: a 64-lane wave per record, four records per workgroup); the window's table of ring ids is the
 * scratch it needs.  Nothing is launched on the decoder's stream. */
#define LEON_GAUGE_MOTION   1
#define LEON_GAUGE_ACTIVITY 2
typedef struct leon_pipeline_gauge_config {
    int32_t sources;                       /* LEON_GAUGE_* bits, 1 .. 3 */
    int32_t reserved[7];                   /* must be 0 */
} leon_pipeline_gauge_config;              /* 32 bytes */
typedef struct leon_pipeline_gauge_regions_call {
    const leon_pipeline_region* regions;   /* DEVICE memory, n records, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    int64_t* device_stats;                 /* DEVICE memory, n x 16 words, 8-byte aligned */
    int32_t* device_status;                /* DEVICE memory, n words, 4-byte aligned, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[3];                  /* must be 0 */
} leon_pipeline_gauge_regions_call;        /* 64 bytes */
/* host only: the definition on the CPU (the text the kernel compiles too) for one record, from records in host memory laid out as
 * leon_pipeline_motion_layout / leon_pipeline_activity_layout (mb_width, mb_height) say: motion_records[i] and activity_records[i]
 * are window frame i's; an array the sources do not ask for may be NULL, and so may the entries of frames other than rec->frame.
 * Returns the record's status word (>= 0; stats, 16 words, is written exactly when it is 0), or LEON_ERR_INVALID (negative) for a null
 * argument, a grid outside 1 .. 256, a frame larger than the grid or below 1, n_frames < 0, sources outside 1 .. 3, a non-zero
 * reserved word of cfg, a NULL record where the frame's is needed. */
int32_t leon_pipeline_gauge_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                   const void* const* motion_records, const void* const* activity_records, const leon_pipeline_gauge_config* cfg,
                                   const leon_pipeline_region* rec, int64_t* stats);
/* Records in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits), with
 * leon_pipeline_carry_regions_device's ordering rules and its scratch event, word for word.  Refused (LEON_ERR_INVALID, nothing
 * enqueued): a null cfg or call, sources outside 1 .. 3, a source whose output the pipeline was created without, a window that is not
 * out for delivery or was delivered with an error, a null `regions` or `device_stats`, regions or device_status not 4-byte aligned,
 * device_stats not 8-byte aligned, n outside 1 .. 65535, a non-zero reserved word of cfg or of the call. */
int leon_pipeline_gauge_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg,
                                       const leon_pipeline_gauge_regions_call* call);
/* Records in host memory, results to host memory, synchronous: the device road between an upload and the copies back.  stats
 * (n x 16 words) and status (n words, may be NULL) go up and come back whole, so a refused record's words stay as the caller had them.
 * The call-level refusals are the device road's. */
int leon_pipeline_gauge_regions(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* regions,
                                int32_t n, int64_t* stats, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_carry_device: k_gauge on records the CALLER supplies (host memory, as
 * leon_pipeline_gauge_record takes them; NULL for frames no valid record of the call names), with memory of its own on device_id's
 * null stream, synchronous; regions, stats and status (may be NULL) in host memory, going up and coming back whole.  Refused
 * (LEON_ERR_INVALID): what leon_pipeline_gauge_record refuses, n outside 1 .. 65535, a valid record that names a frame without the
 * record it needs. */
int leon_pipeline_gauge_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                               const void* const* motion_records_host, const void* const* activity_records_host, const leon_pipeline_gauge_config* cfg,
                               const leon_pipeline_region* regions, int32_t n, int64_t* stats, int32_t* status);
/* Boxes proposed: WHERE a frame's motion record (LEON_PIPELINE_OUTPUT_MOTION) and activity record (LEON_PIPELINE_OUTPUT_ACTIVITY) say
 * that something moved or was coded anew, as leon_pipeline_region rows on the device -- what the resample, warp, carry and gauge calls
 * take as they are, so that a detector or a resample runs only there and no record visits the host.  Integers only; one text for host
 * and device (csrc/leon_propose.h).
 * Requests.  A request is a window frame index f.  With the coded grid mbw x mbh, the frame fw x fh and the config cfg:
 * 1. Hot cells.  Macroblock (i, j) is hot iff 16 i < fw, 16 j < fh and at least one term holds:
 *     motion    cfg.sources & LEON_PROPOSE_MOTION, and max(|fwd_h|, |fwd_v|, |bwd_h|, |bwd_v|) >= cfg.mv_min, the entries the frame's
 *               motion record's, |-32768| = 32768; mv_min 1 .. 32768
 *     intra     cfg.sources & LEON_PROPOSE_MOTION, cfg.flags & LEON_PROPOSE_INTRA, and info & 4 (on an I picture: the whole frame)
 *     activity  cfg.sources & LEON_PROPOSE_ACTIVITY, and the cell's ac_mag >= cfg.ac_min; ac_min 1 .. 65535
 *    A cell of the grid that lies wholly outside the frame is never hot (the grid may be larger than ceil(frame / 16)).
 * 2. Components: the connected components of the hot cells under cfg.connectivity -- 4: edge neighbours, 8: edge and corner
 *    neighbours; neighbours by (i, j), never by raster index (the last cell of a row and the first of the next are none).  A component's
 *    `first` is the smallest raster index j * mbw + i among its cells, its `cells` their number, 1 .. 65536.
 * 3. Selection and order.  The components with cells >= cfg.min_cells (1 .. 65536), in ascending order of `first`.  count is their
 *    number, NOT capped: the caller sees an overflow.  The first K = cfg.max_boxes (1 .. 1024) of them are written.
 * 4. Box.  With i0 .. i1 and j0 .. j1 the extent of the component's cells: x = 16 i0, y = 16 j0, w = min(16 (i1 + 1), fw) - x,
 *    h = min(16 (j1 + 1), fh) - y: always a box regions_check accepts.
 * 5. Outputs per request: regions[K] = {f, x, y, w, h, 0, 0, 0}; info[K][2] = {cells, first}; count; status.  Rows min(count, K) ..
 *    K - 1 are written as {f, 0, 0, 0, 0, 0, 0, 0} with info {0, -1}: a [n, K, 8] result goes into the gauge and resample calls as it
 *    is and the unused rows come back as LEON_REGION_BOX.  Every byte of an accepted request's outputs is written by every call.
 * 6. Status.  LEON_REGION_FRAME: f outside the window; nothing else is judged.  As in the carry, propagate and gauge families A
 *    REQUEST'S FAULT IS A STATUS WORD ON BOTH ROADS, NEVER AN ERROR OF THE CALL; a refused request has not one byte of its regions,
 *    info or count written.
 * One launch per call (k_propose: a workgroup per request; labels of 16 bits a cell, two bit masks and the rows in LDS: 2.25 bytes a
 * cell of the grid and 8 a row, 155680 bytes at 256 x 256 and K = 1024); the window's table of ring ids is the scratch it needs.
 * Nothing is launched on the decoder's stream. */
#define LEON_PROPOSE_MOTION   1
#define LEON_PROPOSE_ACTIVITY 2
#define LEON_PROPOSE_INTRA    1           /* flags: an intra macroblock is hot (needs LEON_PROPOSE_MOTION) */
typedef struct leon_pipeline_propose_config {
    int32_t sources;                       /* LEON_PROPOSE_MOTION | LEON_PROPOSE_ACTIVITY, 1 .. 3 */
    int32_t flags;                         /* 0 or LEON_PROPOSE_INTRA */
    int32_t mv_min;                        /* 1 .. 32768 with the motion source, 0 without */
    int32_t ac_min;                        /* 1 .. 65535 with the activity source, 0 without */
    int32_t connectivity;                  /* 4 or 8 */
    int32_t min_cells;                     /* 1 .. 65536 */
    int32_t max_boxes;                     /* K, 1 .. 1024 */
    int32_t reserved;                      /* must be 0 */
} leon_pipeline_propose_config;            /* 32 bytes */
typedef struct leon_pipeline_propose_regions_call {
    const int32_t* frames;                 /* DEVICE memory, n requests, 4-byte aligned */
    int32_t  n;                            /* 1 .. 65535 */
    int32_t  reserved0;                    /* must be 0 */
    leon_pipeline_region* device_regions;  /* DEVICE memory, n x K records, 4-byte aligned */
    int32_t* device_info;                  /* DEVICE memory, n x K x 2 words, 4-byte aligned, may be NULL */
    int32_t* device_count;                 /* DEVICE memory, n words, 4-byte aligned */
    int32_t* device_status;                /* DEVICE memory, n words, 4-byte aligned, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[1];                  /* must be 0 */
} leon_pipeline_propose_regions_call;      /* 64 bytes */
/* host only: the definition on the CPU for one request, from records in host memory laid out as leon_pipeline_motion_layout /
 * leon_pipeline_activity_layout (mb_width, mb_height) say: motion_records[i] and activity_records[i] are window frame i's; an array
 * the sources do not ask for may be NULL, and so may the entries of frames other than `frame`.  The components are found by a flood
 * fill that shares no text with the kernel's search.  Returns the request's status word (>= 0; regions (K records), info (K x 2 words,
 * may be NULL) and *count are written exactly when it is 0), or LEON_ERR_INVALID (negative) for a null argument, a grid outside
 * 1 .. 256, a frame larger than the grid or below 1, n_frames < 0, what the config refuses (below), a NULL record where the frame's
 * is needed. */
int32_t leon_pipeline_propose_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                     const void* const* motion_records, const void* const* activity_records, const leon_pipeline_propose_config* cfg,
                                     int32_t frame, leon_pipeline_region* regions, int32_t* info, int32_t* count);
/* Requests in DEVICE memory: the call ONLY ENQUEUES on the caller's stream (stream NULL: the regions stream, and the call waits), with
 * leon_pipeline_carry_regions_device's ordering rules and its scratch event, word for word.  Refused (LEON_ERR_INVALID, nothing
 * enqueued), in this order: a null cfg, sources outside 1 .. 3, LEON_PROPOSE_INTRA without the motion source or another bit in flags,
 * mv_min or ac_min outside its range for a source asked for or not 0 for one that is not, connectivity not 4 or 8, min_cells outside
 * 1 .. 65536, max_boxes outside 1 .. 1024, a non-zero reserved word of cfg; a source whose output the pipeline was created without;
 * a null call; a window that is not out for delivery or was delivered with an error; a non-zero reserved word of the call; n outside
 * 1 .. 65535; a null `frames`, `device_regions` or `device_count`; a pointer that is not 4-byte aligned. */
int leon_pipeline_propose_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg,
                                         const leon_pipeline_propose_regions_call* call);
/* Requests in host memory, results to host memory, synchronous: the device road between an upload and the copies back.  regions
 * (n x K records), info (n x K x 2 words, may be NULL), count (n words) and status (n words, may be NULL) go up and come back whole,
 * so a refused request's words stay as the caller had them.  The call-level refusals are the device road's. */
int leon_pipeline_propose_regions(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg, const int32_t* frames, int32_t n,
                                  leon_pipeline_region* regions, int32_t* info, int32_t* count, int32_t* status);
/* A diagnostic in the manner of leon_pipeline_gauge_kernel: k_propose on records the CALLER supplies (host memory, as
 * leon_pipeline_propose_record takes them; NULL for frames no valid request of the call names), with memory of its own on device_id's
 * null stream, synchronous; frames, regions, info (may be NULL), count and status (may be NULL) in host memory, the outputs going up
 * and coming back whole.  Refused (LEON_ERR_INVALID): what leon_pipeline_propose_record refuses, n outside 1 .. 65535, a valid
 * request that names a frame without the record it needs. */
int leon_pipeline_propose_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                 const void* const* motion_records_host, const void* const* activity_records_host, const leon_pipeline_propose_config* cfg,
                                 const int32_t* frames, int32_t n, leon_pipeline_region* regions, int32_t* info, int32_t* count, int32_t* status);
/* Boxes compared with each other: the two steps of a detection loop that the calls above leave out -- PRUNING a set of boxes that
 * overlap (leon_pipeline_suppress_regions: greedy suppression, what a detector's raw output and the nested boxes of
 * leon_pipeline_propose_regions want before they are resampled or carried) and ASSOCIATING two sets (leon_pipeline_match_regions:
 * greedy one-to-one matching, e.g. the boxes carried to the end of a GOP with the detections on the next I picture) -- on
 * leon_pipeline_region rows in device memory, so that no box visits the host.  Integers only, everything in int64; one text for host
 * and device (csrc/leon_overlap.h).  The calls read no record and no frame: a pipeline of any output takes them; of the window they
 * use the frame count, of the pipeline the frame size.
 * Rows and sets.  A set is K consecutive rows (1 .. 1024); a call has n sets (1 .. 65535): the [n, K, 8] arrays that the propose and
 * carry calls write go in as they are.  Every row is judged as leon_pipeline_gauge_regions judges it, in that order:
 * LEON_REGION_RESERVED (a non-zero reserved word), LEON_REGION_FRAME (frame outside the window), LEON_REGION_BOX (an empty box, or one
 * that leaves the frame).  A refused row takes no part: it suppresses and matches nothing and none of its per-row outputs is written
 * (the status word apart) -- the filler rows of propose and the refused rows of carry drop out by themselves.  A ROW'S FAULT IS A
 * STATUS WORD ON BOTH ROADS, NEVER AN ERROR OF THE CALL.  The frame word is judged and otherwise ignored: overlap is a matter of pixel
 * coordinates, so rows on different frames of the window compare like rows on one.
 * Overlap of two accepted rows a and b: iw = min(ax + aw, bx + bw) - max(ax, bx), ih likewise, inter = max(iw, 0) * max(ih, 0);
 *     LEON_OVERLAP_IOU    den = aw * ah + bw * bh - inter
 *     LEON_OVERLAP_IOMIN  den = min(aw * ah, bw * bh)           (a nested box overlaps in full)
 * The pair REACHES the threshold iff inter * 65536 >= cfg.threshold * den; threshold is Q16, 1 .. 65536, so boxes that only touch
 * never reach it.  Frames are at most 4096 x 4096: inter <= 2^24, den <= 2^25, every product below 2^50.
 * Suppress, per set.  Row i's score is scores[(set * K + i) * score_stride] (int32; score_stride 1 .. 8 words; scores NULL: every
 * score 0).  The accepted rows are walked by descending score, ties by ascending row index; a row is KEPT iff no row kept before it
 * reaches the threshold with it.  by[n][K]: -1 for a kept row, else the row index of the first kept row in walk order that reaches
 * the threshold with it; count[n]: the kept rows; out[n][K] (may be NULL): the kept rows in walk order as {frame, x, y, w, h, 0, 0,
 * 0}, rows count .. K - 1 eight zero words (which the sibling calls refuse as LEON_REGION_BOX: out goes into them as it is);
 * order[n][K] (may be NULL): the input row index of each row of out, -1 behind count; status[n][K] (may be NULL).  Every byte of
 * count, out and order is written for every set, by for every accepted row.
 * Match, per pair of sets: set s of a ([n][ka]) against set s of b ([n][kb]), ka and kb each 1 .. 1024.  The candidates are the pairs
 * (i, j) of accepted rows that reach the threshold, in the order of inter / den descending -- compared exactly, inter1 * den2
 * against inter2 * den1 --, ties by the smaller i, then the smaller j; walking that order a pair is TAKEN iff neither of its rows
 * has been.  match_a[n][ka]: j or -1; match_b[n][kb]: i or -1; overlap[n][ka]: floor(inter * 65536 / den) of the taken pair, else 0;
 * count[n]: the pairs taken; status_a, status_b (may be NULL).  The words of a refused row are not written.
 * One launch per call (k_suppress / k_match: a workgroup of 256 threads a set or pair, everything in LDS -- suppress: 16 bytes a row
 * of boxes, a 64-bit key (score, index) for each of K rounded up to a power of two, sorted bitonically, two dwords a row: 32768
 * bytes at K = 1024; match: 24 bytes a row of either set and a dword: 49156 bytes at 1024 and 1024).  k_match repeats "every free row
 * finds its best free partner, mutual best pairs are taken", which gives the greedy result; sets of IDENTICAL boxes are its worst
 * case, one pair a round.  Nothing is launched on the decoder's stream. */
#define LEON_OVERLAP_IOU   0
#define LEON_OVERLAP_IOMIN 1
typedef struct leon_pipeline_overlap_config {
    int32_t measure;                       /* LEON_OVERLAP_IOU or LEON_OVERLAP_IOMIN */
    int32_t threshold;                     /* Q16, 1 .. 65536 */
    int32_t reserved[2];                   /* must be 0 */
} leon_pipeline_overlap_config;            /* 16 bytes */
typedef struct leon_pipeline_suppress_regions_call {
    const leon_pipeline_region* regions;   /* DEVICE memory, n x k records, 4-byte aligned */
    const int32_t* scores;                 /* DEVICE memory, n x k x score_stride words, 4-byte aligned, may be NULL */
    int32_t  n;                            /* sets, 1 .. 65535 */
    int32_t  k;                            /* rows of a set, 1 .. 1024 */
    int32_t  score_stride;                 /* words from one row's score to the next, 1 .. 8 (also with scores NULL) */
    int32_t  reserved0;                    /* must be 0 */
    leon_pipeline_region* device_out;      /* DEVICE memory, n x k records, 4-byte aligned, may be NULL */
    int32_t* device_order;                 /* DEVICE memory, n x k words, 4-byte aligned, may be NULL */
    int32_t* device_by;                    /* DEVICE memory, n x k words, 4-byte aligned */
    int32_t* device_count;                 /* DEVICE memory, n words, 4-byte aligned */
    int32_t* device_status;                /* DEVICE memory, n x k words, 4-byte aligned, may be NULL */
    void*    stream;                       /* hipStream_t of the caller's; NULL: the pipeline's regions stream, and the call waits */
    uint64_t reserved[2];                  /* must be 0 */
} leon_pipeline_suppress_regions_call;     /* 96 bytes */
typedef struct leon_pipeline_match_regions_call {
    const leon_pipeline_region* a;         /* DEVICE memory, n x ka records, 4-byte aligned */
    const leon_pipeline_region* b;         /* DEVICE memory, n x kb records, 4-byte aligned */
    int32_t  n;                            /* pairs of sets, 1 .. 65535 */
    int32_t  ka, kb;                       /* rows of a set of a and of b, each 1 .. 1024 */
    int32_t  reserved0;                    /* must be 0 */
    int32_t* device_match_a;               /* DEVICE memory, n x ka words, 4-byte aligned */
    int32_t* device_match_b;               /* DEVICE memory, n x kb words, 4-byte aligned */
    int32_t* device_overlap;               /* DEVICE memory, n x ka words, 4-byte aligned */
    int32_t* device_count;                 /* DEVICE memory, n words, 4-byte aligned */
    int32_t* device_status_a;              /* DEVICE memory, n x ka words, 4-byte aligned, may be NULL */
    int32_t* device_status_b;              /* DEVICE memory, n x kb words, 4-byte aligned, may be NULL */
    void*    stream;                       /* as above */
    uint64_t reserved[1];                  /* must be 0 */
} leon_pipeline_match_regions_call;        /* 96 bytes */
/* host only: the definitions on the CPU for ONE set (pair of sets) in host memory -- a stable sort and a walk that share no text with
 * the kernels' steps.  Return LEON_OK, or LEON_ERR_INVALID (nothing written) for, in this order: a null cfg, a measure outside 0 ..
 * 1, a threshold outside 1 .. 65536, a non-zero reserved word of cfg; a frame outside 1 .. 4096 on an axis, n_frames < 0; k (ka, kb)
 * outside 1 .. 1024; score_stride outside 1 .. 8; a null regions, by or count (a, b, match_a, match_b, overlap or count). */
int32_t leon_pipeline_suppress_record(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                                      const leon_pipeline_region* regions, int32_t k, const int32_t* scores, int32_t score_stride, leon_pipeline_region* out,
                                      int32_t* order, int32_t* by, int32_t* count, int32_t* status);
int32_t leon_pipeline_match_record(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a,
                                   int32_t ka, const leon_pipeline_region* b, int32_t kb, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count,
                                   int32_t* status_a, int32_t* status_b);
/* Sets in DEVICE memory: the calls ONLY ENQUEUE on the caller's stream (stream NULL: the regions stream, and the call waits), with
 * leon_pipeline_carry_regions_device's ordering rules and its scratch event, word for word.  Refused (LEON_ERR_INVALID, nothing
 * enqueued), in this order: a null cfg, a measure outside 0 .. 1, a threshold outside 1 .. 65536, a non-zero reserved word of cfg; a
 * null call; a window that is not out for delivery or was delivered with an error; a non-zero reserved word of the call; n outside
 * 1 .. 65535, k (ka, kb) outside 1 .. 1024; score_stride outside 1 .. 8; a null regions, device_by or device_count (a, b,
 * device_match_a, device_match_b, device_overlap or device_count); a pointer that is not 4-byte aligned. */
int leon_pipeline_suppress_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_suppress_regions_call* call);
int leon_pipeline_match_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_match_regions_call* call);
/* Sets in host memory, results to host memory, synchronous: the device road between an upload and the copies back.  Every output
 * goes up and comes back whole, so a refused row's words stay as the caller had them.  The call-level refusals are the device
 * road's. */
int leon_pipeline_suppress_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* regions, int32_t n, int32_t k,
                                   const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status);
int leon_pipeline_match_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a, int32_t ka,
                                const leon_pipeline_region* b, int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count,
                                int32_t* status_a, int32_t* status_b);
/* Diagnostics in the manner of leon_pipeline_gauge_kernel: k_suppress / k_match on rows the CALLER supplies (host memory) for a frame
 * size and a frame count the caller names, with memory of their own on device_id's null stream, synchronous; the outputs go up and
 * come back whole.  Refused (LEON_ERR_INVALID): what the record calls refuse, n outside 1 .. 65535. */
int leon_pipeline_suppress_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                                  const leon_pipeline_region* regions, int32_t n, int32_t k, const int32_t* scores, int32_t score_stride, leon_pipeline_region* out,
                                  int32_t* order, int32_t* by, int32_t* count, int32_t* status);
int leon_pipeline_match_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                               const leon_pipeline_region* a, int32_t ka, const leon_pipeline_region* b, int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b,
                               int32_t* overlap, int32_t* count, int32_t* status_a, int32_t* status_b);
/* A diagnostic: the DEVICE's evaluation of the tables of n_axes single axes, copied back, to be compared word for word with
 * leon_pipeline_resize_weights (pixels would hide a weight that is one unit off).  axes = n_axes x {in_size, crop_start, crop_size,
 * out_size}; with max_out the largest out_size of the batch, axis a's tables lie at a fixed pitch: first[a * max_out + o],
 * count[a * max_out + o] and weights[(a * max_out + o) * max_taps + k] (k >= count: 0) for o < its out_size -- the caller provides
 * n_axes * max_out words for first and count, n_axes * max_out * max_taps for weights, n_axes for status; what lies behind an axis's
 * out_size, and everything of an axis whose status is not 0, is left as it was.  status[a]: 0, LEON_REGION_BOX, LEON_REGION_RATIO_X
 * (there is one axis), LEON_REGION_TAPS (also: a count above max_taps).  Synchronous, on device_id's null stream, memory of its own.
 * Refused (LEON_ERR_INVALID): a null pointer, n_axes < 1, max_taps < 1, another filter, an in_size or out_size outside 1 .. 4096. */
int leon_pipeline_resize_weights_device(int32_t device_id, int32_t n_axes, const int32_t* axes, int32_t filter, int32_t max_taps,
                                        int32_t* first, int32_t* count, int32_t* weights, int32_t* status);
const char* leon_pipeline_error(leon_pipeline* p);
void leon_pipeline_destroy(leon_pipeline* p);

#ifdef __cplusplus
}
#endif
#endif
