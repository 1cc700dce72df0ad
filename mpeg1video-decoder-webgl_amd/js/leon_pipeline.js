'use strict';
/*
 * leon_pipeline.js -- the native decode pipeline (include/leon_pipeline.h) for a JavaScript host.
 *
 * The reference's page pulls pictures one at a time on its only thread: decodeFrame() -> bit-serial
 * parse -> IDCT_GL, frame by frame, paced by the display timer (decoders/jsv.js:426-469,
 * player/easybits.player.js:2310-2324, :2543-2617).  Here the whole loop runs in native threads (GOP-shard
 * parsers, one submit thread, one notify thread) and the host only receives events, through a
 * napi_threadsafe_function -- the JavaScript thread never waits for the parser or the GPU.
 *
 *   const { LeonPipeline } = require('./leon_pipeline');
 *   const p = new LeonPipeline(fs.readFileSync('clip.jsv'), { parserThreads: 16, gopsPerWindow: 32 });
 *   p.on('frame', (f) => ...)      // {gop, displayIndex, type, ts, window, index}: same event name as the
 *                                  // reference decoder's (decoders/jsv.js:673); frames arrive in display order
 *   p.on('frames', (window, frames) => ...)   // one call per window; keep it with {autoRelease: false}
 *   p.on('ended', () => ...)       // decoders/jsv.js:437
 *   p.on('error', (err) => ...)
 *   p.seek(seconds, {exact}) -> first window id of the new position (leon_pipeline_seek; jsv.prototype.seek,
 *                                  decoders/jsv.js:1618-1648): nothing is recreated; windows of the old position
 *                                  never arrive, 'seeked' (frame) comes with the first frame of the new one, and
 *                                  after 'ended' a seek starts a new run with its own 'ended'
 *   p.readFrame(window, index) -> Uint8Array RGBA (copies to the host: tests, thumbnails)
 *   p.readPlanes(window, index) -> {y, cb, cr[, a]} packed Uint8Arrays: the frame's YCbCr 4:2:0 planes, with
 *                                  opts.output 'ycbcr' (no RGBA at all) or 'both' -- the reference's frame payload
 *                                  {ybr: [Y, Cb, Cr]} (decoders/jsv.js:600, :673); default 'rgba'
 *   p.readTensor(window, index) -> Uint16Array (fp16 / bf16 bit patterns), Float32Array or Uint8Array, [3][H][W] packed: the frame as a planar,
 *                                  normalised R, G, B tensor for a model, with opts.output 'tensor' (no RGBA at all),
 *                                  'rgba+tensor', 'ycbcr+tensor' or 'all'; opts.tensorDtype 'float16' (default) / 'bfloat16' /
 *                                  'float32', opts.tensorScale / tensorBias [r, g, b] (default 1/255 and 0: values in [0, 1]);
 *                                  element = to_dtype(float32(v * scale[c] + bias[c])) of the CPU-twin colour value v;
 *                                  stats() reports tensorDtype, tensorElementBytes, tensorFrameBytes, tensorFramePitch, tensorGopPitch
 *                                  opts.tensorSize [h, w] (and opts.tensorCrop [x, y, w, h], frame pixels; default the whole frame):
 *                                  that crop box resampled on the device to h x w (antialiased triangle filter, include/leon_pipeline.h)
 *                                  -- readTensor then returns [3][h][w]; stats() reports tensorWidth, tensorHeight;
 *                                  opts.tensorFilter 'triangle' (default) or 'bicubic' (LEON_RESIZE_BICUBIC: signed taps, clamped on both sides)
 *                                  opts.tensorDtype 'uint8': the elements are the 8-bit colour values themselves (no tensorScale /
 *                                  tensorBias), readTensor returns a Uint8Array; opts.tensorLayout 'chw' (default) or 'hwc': channels
 *                                  last, [H][W][3] -- uint8 hwc is the packed RGB frame, 3 bytes per pixel; stats() reports tensorLayout
 *                                  opts.tensorCanvas [h, w] (with tensorSize): the resampled image lies in an h x w tensor, its top-left
 *                                  element at opts.tensorOrigin [x, y] (default: centred), every other element at opts.tensorPadValue
 *                                  [r, g, b] (8-bit colour values through the element table; default 0) -- every element is written every
 *                                  window; readTensor returns the canvas; stats() reports tensorWidth / tensorHeight (the canvas's) and the
 *                                  image rectangle tensorImageX, tensorImageY, tensorImageWidth, tensorImageHeight.
 *                                  opts.tensorLetterbox [h, w]: tensorSize, tensorCanvas and tensorOrigin derived from the crop box or the
 *                                  frame with the aspect ratio kept (LeonPipeline.letterbox = leon_pipeline_letterbox)
 *   p.readMotion(window, index) -> {mv: Int16Array [mbs][4] (fwd_h, fwd_v, bwd_h, bwd_v in half-pel luma units), info: Uint8Array [mbs] (bits: 1
 *                                  forward, 2 backward, 4 intra), summary: Uint32Array [8], fwdGop, fwdDisplay, bwdDisplay (the pictures the
 *                                  vectors point into, -1: none), mbWidth, mbHeight}: the frame's motion record, macroblocks in raster order of
 *                                  the coded picture, with opts.motion true beside any output (include/leon_pipeline.h
 *                                  LEON_PIPELINE_OUTPUT_MOTION); read only, until the window is released
 *   p.readActivity(window, index) -> {acCount, acMag, dcMag: Uint16Array [mbs], blocks, qscale: Uint8Array [mbs], summary: Uint32Array [8],
 *                                  mbWidth, mbHeight}: the frame's activity record -- per macroblock how much the stream coded on top of its
 *                                  prediction (non-DC entries, the sum of their magnitudes, the DC magnitudes, the coded block bits, the
 *                                  quantiser scale where something is coded), with opts.activity true beside any output (include/leon_pipeline.h
 *                                  LEON_PIPELINE_OUTPUT_ACTIVITY); until the window is released
 *   p.readResidual(window, index) -> {y: Int16Array [codedHeight][codedWidth], cb, cr: Int16Array [codedHeight / 2][codedWidth / 2],
 *                                  codedWidth, codedHeight}: the frame's residual record -- what the stream's coefficients decode to before
 *                                  any prediction is added and before any clamp, for the coded picture (the frame is its top-left corner),
 *                                  with opts.residual true beside any output (include/leon_pipeline.h LEON_PIPELINE_OUTPUT_RESIDUAL);
 *                                  until the window is released
 *   p.readRegions(window, regions, {size: [h, w], filter}) -> Buffer of n * 3 * h * w elements, packed: regions = [[frameIndex, x, y,
 *                                  width, height], ...], boxes of the window's FULL-RESOLUTION frames (a detector's boxes) each resampled to
 *                                  h x w with the pipeline's element type, table and layout (leon_pipeline_read_regions) -- any tensor
 *                                  output, whatever its tensorSize / tensorCanvas; until the window is released; filter 'triangle'
 *                                  (default) or 'bicubic'.  fit: 'letterbox' keeps every box's aspect ratio inside h x w -- centred, or
 *                                  with anchor: 'top_left' at the top left -- and fills the rest with padValue [r, g, b] through the
 *                                  element table (leon_pipeline_read_regions_fit); without fit, anchor and padValue the boxes are stretched
 *   p.readWarpRegions(window, regions, {size: [h, w], padValue}) -> Buffer like readRegions': regions = [[frameIndex, [a00, a01, tx, a10,
 *                                  a11, ty]], ...], the Q16 affine map from output to frame coordinates of a rotated box or an aligned
 *                                  crop (leon_pipeline_read_warp_regions); positions outside the frame read padValue [r, g, b]
 *   p.carryRegions(window, records) -> {out: Int32Array [n][8], votes: Int32Array [n][4] (A, I, dh, dv), status: Int32Array [n]}: records =
 *                                  [[frameIndex, x, y, width, height, targetFrameIndex], ...], boxes carried along the motion vectors
 *                                  between two frames of the window that a prediction joins (leon_pipeline_carry_regions, opts.motion);
 *                                  out[i] = [target, x', y', width, height, 0, 0, 0] where status[i] is 0, a region record for
 *                                  readRegions; a record's fault is its status word (9: no prediction joins the two frames), not a throw
 *   p.gaugeRegions(window, regions, {sources}) -> {stats: Float64Array [n][16], status: Int32Array [n]}: regions = [[frameIndex, x, y, width,
 *                                  height], ...], per box the area-weighted sums over the macroblocks under it of its frame's motion record
 *                                  (sources 1: words 8 .. 15), its activity record (sources 2: words 1 .. 7) or both (3; the default: every
 *                                  record output the pipeline has); word 0 is the box's area (leon_pipeline_gauge_regions).  Every word is
 *                                  below 2^53, so the numbers are exact; a record's fault is its status word, not a throw
 *   p.proposeRegions(window, frames, {maxBoxes, mvMin, acMin, intra, connectivity, minCells, sources}) -> {regions: Int32Array [n][K][8],
 *                                  count: Int32Array [n], info: Int32Array [n][K][2] (cells, first), status: Int32Array [n]}: frames =
 *                                  [frameIndex, ...]; per frame the boxes of the connected components (connectivity 8 or 4) of its hot
 *                                  macroblocks -- a vector of mvMin half-pels or more, intra where `intra`, an ac_mag of acMin or more --
 *                                  with minCells cells or more, in raster order of their first cell (leon_pipeline_propose_regions);
 *                                  regions[i][k] = [frameIndex, x, y, width, height, 0, 0, 0] for k < min(count[i], K = maxBoxes, default
 *                                  16), a region record for readRegions and gaugeRegions, and an empty box behind; count is not capped.
 *                                  sources (1 motion, 2 activity, 3): by default every record output the pipeline has, each with its
 *                                  threshold; a request's fault is its status word, not a throw
 *   p.propagateMaps(window, maps, hops, {stride, planes, elemBytes, fill}) -> {via: Uint8Array [n][mh][mw] (0 fill, 1 forward, 2 backward),
 *                                  status: Int32Array [n]}: dense maps (masks, heatmaps, features) propagated along the motion vectors
 *                                  (leon_pipeline_propagate_maps, opts.motion).  maps = a Buffer / Uint8Array over [slots][planes][mh][mw]
 *                                  elements of elemBytes (1, 2, 4) bytes, mw = ceil(frameWidth / stride), mh likewise, WRITTEN IN
 *                                  PLACE; hops = [[targetFrameIndex, dstSlot, fwdSlot, bwdSlot], ...]: each writes maps[dstSlot], the
 *                                  map of frame target, as a gather through that frame's motion record from the maps of the pictures
 *                                  it predicts from (-1: not supplied); cells with neither get fill.  A hop's fault is its status word
 *                                  (10: a slot outside the buffer, or the destination among the sources), not a throw.  The maps lie
 *                                  back to back, and the library takes slots a multiple of 4 bytes apart only: planes * mh * mw *
 *                                  elemBytes must be a multiple of 4 (a 61 x 45 uint8 mask of one plane is refused with a throw; give
 *                                  it a second plane, or 2-byte elements)
 *   p.accumulate(window, hops, {parts, slots}) -> {slots: Int16Array, via: Uint8Array [n][mbh][mbw] (0 restart, 1 forward, 2 backward),
 *                                  status: Int32Array [n], layout}: motion and residual accumulated along a chain of predictions
 *                                  (leon_pipeline_accumulate, opts.motion; opts.residual for parts 2 and 3).  An accumulator lies over
 *                                  the CODED picture: parts & 1 the planes AX, AY, AGE (where a sample came from in the picture the
 *                                  chain started at, and after how many hops), parts & 2 the planes RY, RCb, RCr (the sum of the
 *                                  residual along that path), int16, at layout.axOffset .. layout.rcrOffset bytes into a slot of
 *                                  layout.slotBytes, rows layout.lumaStride / chromaStride elements apart.  parts: by default every part
 *                                  the pipeline's outputs allow.  slots: an Int16Array over a whole number of accumulators, WRITTEN IN
 *                                  PLACE and handed back, or how many to make (all zero; by default one more than the largest slot the
 *                                  hops name).  hops = [[targetFrameIndex, dstSlot, fwdSlot, bwdSlot], ...] as propagateMaps takes them;
 *                                  a hop with both sources -1 writes a chain's start (all zero).  A hop's fault is its status word
 *   p.releaseWindow(window); p.stats(); p.destroy();
 * Open GOPs (closed_gop = 0) need no option: their leading B pictures predict from the GOP before; where that GOP is not decoded (start,
 * seek target, broken_link) they are not delivered and the GOP's frames start at its I picture's displayIndex (include/leon_pipeline.h).
 */
const path = require('path');
const EventEmitter = require('events');

// an option that is a name of `table` or already its integer (anything else goes on as it is, for the addon or the caller to refuse); absent: 0
function named(value, table, text) {
  if (value === undefined) return 0;
  if (typeof value === 'string') {
    if (!(value in table)) throw new TypeError(text);
    return table[value];
  }
  return value;
}
// v: n integers (n undefined: any number of them), or TypeError(text); an undefined v is `absent` where one is given
function ints(v, n, text, absent) {
  if (v === undefined && absent) return absent;
  if (!Array.isArray(v) || (n !== undefined && v.length !== n) || !v.every(Number.isInteger)) throw new TypeError(text);
  return v;
}
// a record list [[k integers], ...] as the Int32Array the addon takes, or TypeError(text)
function rows(value, k, text) {
  if (!Array.isArray(value) || !value.every((r) => Array.isArray(r) && r.length === k && r.every(Number.isInteger))) throw new TypeError(text);
  return Int32Array.from(value.flat());
}
const OUTPUTS = { rgba: 1, ycbcr: 2, both: 3, tensor: 16, 'rgba+tensor': 17, 'ycbcr+tensor': 18, all: 19 };
const FILTERS = { triangle: 0, bicubic: 3 };
const REGIONS = 'regions: [[frameIndex, x, y, width, height], ...]';

class LeonPipeline extends EventEmitter {
  constructor(stream, opts) {
    super();
    opts = opts || {};
    const addon = opts.backend || require(path.join(__dirname, '..', 'napi', 'leon_napi.node'));
    if (!Buffer.isBuffer(stream)) stream = Buffer.from(stream.buffer, stream.byteOffset, stream.byteLength);
    this.autoRelease = opts.autoRelease !== false;
    this.ended = false;
    let output = named(opts.output, OUTPUTS, "output: 'rgba', 'ycbcr', 'both', 'tensor', 'rgba+tensor', 'ycbcr+tensor' or 'all'");
    if (opts.motion) output = (output || OUTPUTS.rgba) | 32;          // LEON_PIPELINE_OUTPUT_MOTION beside whatever output resolves to
    if (opts.activity) output = (output || OUTPUTS.rgba) | 128;       // LEON_PIPELINE_OUTPUT_ACTIVITY likewise
    if (opts.residual) output = (output || OUTPUTS.rgba) | 512;       // LEON_PIPELINE_OUTPUT_RESIDUAL likewise
    this._accumulateParts = 1 | (opts.residual ? 2 : 0);          // what accumulate writes without opts.parts: every part the outputs allow
    this._gaugeSources = (opts.motion ? 1 : 0) | (opts.activity ? 2 : 0);          // what gaugeRegions reads without opts.sources: every record output there is
    const tensorDtype = named(opts.tensorDtype, { float16: 1, bfloat16: 2, float32: 3, uint8: 8 }, "tensorDtype: 'float16', 'bfloat16', 'float32' or 'uint8'");
    const tensorLayout = named(opts.tensorLayout, { chw: 0, hwc: 1 }, "tensorLayout: 'chw' or 'hwc'");
    const tensorFilter = named(opts.tensorFilter, FILTERS, "tensorFilter: 'triangle' or 'bicubic'");
    // tensorSize [h, w] (, tensorCrop [x, y, w, h] in frame pixels): the tensors resampled on the device to a model's input size
    const list = (v, n, text) => ints(v === null ? undefined : v, n, text, new Array(n).fill(0));          // (absent or null: zeros)
    const [tensorOutHeight, tensorOutWidth] = list(opts.tensorSize, 2, 'tensorSize: [height, width]');
    const [tensorCropX, tensorCropY, tensorCropWidth, tensorCropHeight] = list(opts.tensorCrop, 4, 'tensorCrop: [x, y, width, height]');
    const resize = { tensorOutHeight, tensorOutWidth, tensorCropX, tensorCropY, tensorCropWidth, tensorCropHeight, tensorFilter };
    // tensorCanvas [h, w], tensorOrigin [x, y], tensorPadValue [r, g, b]: the image in a padded canvas; tensorLetterbox [h, w] derives them
    const [tensorCanvasHeight, tensorCanvasWidth] = list(opts.tensorCanvas, 2, 'tensorCanvas: [height, width]');
    const [tensorOriginX, tensorOriginY] = list(opts.tensorOrigin, 2, 'tensorOrigin: [x, y]');
    const [tensorPadR, tensorPadG, tensorPadB] = list(opts.tensorPadValue, 3, 'tensorPadValue: [r, g, b]');
    const [tensorLetterboxHeight, tensorLetterboxWidth] = list(opts.tensorLetterbox, 2, 'tensorLetterbox: [height, width]');
    const tensorOriginSet = opts.tensorOrigin === undefined || opts.tensorOrigin === null ? 0 : 1;
    Object.assign(resize, { tensorCanvasHeight, tensorCanvasWidth, tensorOriginX, tensorOriginY, tensorOriginSet, tensorPadR, tensorPadG, tensorPadB,
      tensorLetterboxHeight, tensorLetterboxWidth });
    this._p = addon.createPipeline(stream, Object.assign({}, opts, { output, tensorDtype, tensorLayout }, resize), (w, frames, status) => this._deliver(w, frames, status));
  }

  _deliver(window, frames, status) {
    if (window < 0) {
      this.ended = true;
      if (status) this.emit('error', new Error('leon pipeline stopped with status ' + status));
      this.emit('ended');
      return;
    }
    if (status) {
      this.emit('error', new Error('leon pipeline: window ' + window + ' failed with status ' + status));
      this._p.releaseWindow(window);
      return;
    }
    frames.forEach((f, i) => { f.window = window; f.index = i; });
    if (this._seekFirst !== undefined && window >= this._seekFirst) {
      this._seekFirst = undefined;
      this.emit('seeked', frames[0]);
    }
    this.emit('frames', window, frames);
    for (const f of frames) this.emit('frame', f);
    if (this.autoRelease) this._p.releaseWindow(window);
  }

  // a stream that is still arriving (opts.validBytes at construction; the Buffer has the file's final size): the loader
  // writes the next chunk into the same Buffer and reports how far it is valid now -- features/bitreader.js:332 addBuffer
  feed(validBytes) { this._p.feed(validBytes); }
  // (the addon gives back what the notify thread had queued for the old position: no stale window reaches _deliver)
  seek(seconds, opts) {
    const first = this._p.seek(seconds, !!(opts && opts.exact));
    this.ended = false;
    this._seekFirst = first;
    return first;
  }
  readFrame(window, index) { return this._p.readFrame(window, index); }
  readPlanes(window, index) { return this._p.readPlanes(window, index); }
  readTensor(window, index) { return this._p.readTensor(window, index); }
  readMotion(window, index) { return this._p.readMotion(window, index); }
  readResidual(window, index) { return this._p.readResidual(window, index); }
  // the addon hands the cells over as they lie, 8 bytes a macroblock; the fields as typed arrays of their own
  readActivity(window, index) {
    const r = this._p.readActivity(window, index), mbs = r.mbWidth * r.mbHeight;
    const v = new DataView(r.cells.buffer, r.cells.byteOffset, 8 * mbs);
    const out = { acCount: new Uint16Array(mbs), acMag: new Uint16Array(mbs), dcMag: new Uint16Array(mbs), blocks: new Uint8Array(mbs),
      qscale: new Uint8Array(mbs), summary: r.summary, mbWidth: r.mbWidth, mbHeight: r.mbHeight };
    for (let k = 0; k < mbs; k++) {
      out.acCount[k] = v.getUint16(8 * k, true);
      out.acMag[k] = v.getUint16(8 * k + 2, true);
      out.dcMag[k] = v.getUint16(8 * k + 4, true);
      out.blocks[k] = v.getUint8(8 * k + 6);
      out.qscale[k] = v.getUint8(8 * k + 7);
    }
    return out;
  }
  // regions: [[frameIndex, x, y, width, height], ...] of a delivered window's full-resolution frames, resampled to opts.size [h, w]
  readRegions(window, regions, opts) {
    opts = opts || {};
    const filter = named(opts.filter, FILTERS, "filter: 'triangle' or 'bicubic'");
    const size = ints(opts.size, 2, 'size: [height, width]');
    const boxes = rows(regions, 5, REGIONS);
    if (opts.fit === undefined && opts.anchor === undefined && opts.padValue === undefined) return this._p.readRegions(window, boxes, size[0], size[1], filter);
    const fit = named(opts.fit, { stretch: 0, letterbox: 1 }, "fit: 'stretch' or 'letterbox'");
    const anchor = named(opts.anchor, { centre: 0, center: 0, top_left: 1 }, "anchor: 'centre' or 'top_left'");
    const pad = ints(opts.padValue, 3, 'padValue: [r, g, b]', [0, 0, 0]);
    if (!Number.isInteger(fit) || !Number.isInteger(anchor)) throw new TypeError('fit, anchor: a name or an integer');
    return this._p.readRegions(window, boxes, size[0], size[1], filter, fit, anchor, pad[0], pad[1], pad[2]);
  }
  // regions: [[frameIndex, [a00, a01, tx, a10, a11, ty]], ...], Q16 integers: rotated boxes and affine crops sampled into opts.size [h, w]
  readWarpRegions(window, regions, opts) {
    opts = opts || {};
    const size = ints(opts.size, 2, 'size: [height, width]');
    const text = 'regions: [[frameIndex, [a00, a01, tx, a10, a11, ty]], ...] (Q16 integers)';
    if (!Array.isArray(regions) || !regions.every((r) => Array.isArray(r) && r.length === 2 && Array.isArray(r[1]))) throw new TypeError(text);
    const words = rows(regions.map((r) => [r[0]].concat(r[1])), 7, text);          // (the addon's record: the index and the matrix, 7 words)
    const pad = ints(opts.padValue, 3, 'padValue: [r, g, b]', [0, 0, 0]);
    return this._p.readWarpRegions(window, words, size[0], size[1], pad[0], pad[1], pad[2]);
  }
  // records: [[frameIndex, x, y, width, height, targetFrameIndex], ...]: one hop each along the window's motion records
  carryRegions(window, records) {
    return this._p.carryRegions(window, rows(records, 6, 'records: [[frameIndex, x, y, width, height, targetFrameIndex], ...]'));
  }
  // regions: [[frameIndex, x, y, width, height], ...]: the motion and activity records of each box's frame summed under the box
  gaugeRegions(window, regions, opts = {}) {
    const boxes = rows(regions, 5, REGIONS);
    const sources = opts.sources === undefined ? this._gaugeSources : opts.sources;
    if (!Number.isInteger(sources)) throw new TypeError('sources: 1 (motion), 2 (activity) or 3');
    return this._p.gaugeRegions(window, boxes, sources);
  }
  // frames: [frameIndex, ...]: the boxes of what each frame's motion and activity records say moved or was coded anew
  proposeRegions(window, frames, opts = {}) {
    ints(frames, undefined, 'frames: [frameIndex, ...]');
    const sources = opts.sources === undefined ? this._gaugeSources : opts.sources;
    const words = ints([sources, opts.intra ? 1 : 0, (sources & 1) ? opts.mvMin : 0, (sources & 2) ? opts.acMin : 0, opts.connectivity === undefined ? 8 : opts.connectivity,
      opts.minCells === undefined ? 1 : opts.minCells, opts.maxBoxes === undefined ? 16 : opts.maxBoxes, 0], 8,
    'sources: 1 (motion), 2 (activity) or 3; mvMin with motion, acMin with activity; connectivity, minCells, maxBoxes: integers');
    return this._p.proposeRegions(window, Int32Array.from(frames), Int32Array.from(words));
  }
  // hops: [[targetFrameIndex, dstSlot, fwdSlot, bwdSlot], ...]: each a gather through the target's motion record; maps is written in place
  propagateMaps(window, maps, hops, opts = {}) {
    if (!(maps instanceof Uint8Array)) throw new TypeError('maps: a Buffer or Uint8Array over [slots][planes][mh][mw]');
    const words = rows(hops, 4, 'hops: [[targetFrameIndex, dstSlot, fwdSlot, bwdSlot], ...]');
    const { stride = 1, planes = 1, elemBytes = 1, fill = 0 } = opts;
    ints([stride, planes, elemBytes, fill], 4, 'opts: {stride, planes, elemBytes, fill} are integers');
    return this._p.propagateMaps(window, maps, words, stride, planes, elemBytes, fill >>> 0);
  }
  // hops as propagateMaps takes them; opts.slots: an Int16Array of accumulators (written in place) or how many to make, all zero
  accumulate(window, hops, opts = {}) {
    const words = rows(hops, 4, 'hops: [[targetFrameIndex, dstSlot, fwdSlot, bwdSlot], ...]');
    const { parts = this._accumulateParts } = opts;
    let { slots } = opts;
    if (slots === undefined) slots = hops.reduce((m, h) => Math.max(m, h[1], h[2], h[3]), 0) + 1;
    if (!(slots instanceof Int16Array)) ints([slots], 1, 'opts.slots: an Int16Array over whole accumulators, or their number');
    ints([parts], 1, 'opts.parts: 1 (motion), 2 (residual) or 3');
    return this._p.accumulate(window, words, parts, slots);
  }
  releaseWindow(window) { this._p.releaseWindow(window); }
  stats() { return this._p.stats(); }
  destroy() { if (this._p) { this._p.destroy(); this._p = null; } }
}

// letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight) -> [outWidth, outHeight, x, y]: leon_pipeline_letterbox (no device)
LeonPipeline.letterbox = (srcWidth, srcHeight, canvasWidth, canvasHeight, backend) =>
  (backend || require(path.join(__dirname, '..', 'napi', 'leon_napi.node'))).letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight);

module.exports = { LeonPipeline };
