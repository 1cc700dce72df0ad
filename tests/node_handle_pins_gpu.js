#!/usr/bin/env node
/*
 * node_handle_pins_gpu.js -- the two handles of napi/leon_napi.node on a device: what every method refuses, called on the raw addon
 * object (a pipeline's lp._p, a create() decoder), not through js/leon_pipeline.js.  A decoder handle of 32 x 32; pipeline A with
 * output 'rgba' only (the "no tensor output" throws and the library's "has no motion / activity / residual output" refusals); pipeline
 * B with every output, in whose first 'frames' handler each of the seventeen methods gets too few arguments, a wrong-typed window, a
 * typed array of the wrong kind, a length that is no multiple of the record's words, no record, 65536 records (the clamp: the library
 * refuses it with its "1 .. 65535"), a window never delivered and an index past the window -- and after destroy() every method again.
 * Every case is refused on the host before any launch, and records {class, message} of what was thrown, or what came back (typed
 * arrays as {kind, values}).  tests/test_node_binding_pins_gpu.py compares the one JSON object on stdout with
 * tests/golden/node_handle_pins_gpu.json.
 *
 *   node tests/node_handle_pins_gpu.js tests/golden/streams/tiny_ip_32x32.jsv      -> {name: {returned | thrown}, ...}
 */
'use strict';
const fs = require('fs');
const path = require('path');
const PKG = path.join(__dirname, '..', 'mpeg1video-decoder-webgl_amd');
const { LeonPipeline } = require(path.join(PKG, 'js', 'leon_pipeline.js'));
const backend = require(path.join(PKG, 'napi', 'leon_napi.node'));
const stream = fs.readFileSync(process.argv[2]);

function ser(v) {
  if (v === undefined) return '<undefined>';
  if (v === null || typeof v === 'boolean' || typeof v === 'string' || typeof v === 'number') return v;
  if (ArrayBuffer.isView(v)) return { kind: v.constructor.name, values: Array.from(v) };
  if (Array.isArray(v)) return v.map(ser);
  const o = {};
  for (const k of Object.keys(v)) o[k] = ser(v[k]);
  return o;
}
const out = {};
function pin(name, fn) {
  if (name in out) throw new Error('two cases named ' + name);
  try { out[name] = { returned: ser(fn()) }; } catch (e) { out[name] = { thrown: { class: e.constructor.name, message: e.message } }; }
}
const i32 = (n) => new Int32Array(n);

// valid arguments of every method for window w (records of frame 0; nothing here is called with all of them on a pipeline that would run them)
function valid(w) {
  return { releaseWindow: [w], readFrame: [w, 0], readPlanes: [w, 0], readTensor: [w, 0], readMotion: [w, 0], readActivity: [w, 0], readResidual: [w, 0],
    readRegions: [w, Int32Array.from([0, 0, 0, 16, 16]), 8, 8, 0], readWarpRegions: [w, Int32Array.from([0, 65536, 0, 0, 0, 65536, 0]), 8, 8, 0, 0, 0],
    carryRegions: [w, Int32Array.from([0, 0, 0, 16, 16, 1])], gaugeRegions: [w, Int32Array.from([0, 0, 0, 16, 16]), 3],
    proposeRegions: [w, Int32Array.from([0]), Int32Array.from([3, 0, 1, 1, 8, 1, 16, 0])], propagateMaps: [w, new Uint8Array(32 * 32), Int32Array.from([1, 0, -1, -1]), 1, 1, 1, 0],
    stats: [], destroy: [], feed: [stream.length], seek: [0, false] };
}
const METHODS = Object.keys(valid(0));
// which argument is the record list, and its words per record
const RECORDS = { readRegions: 5, readWarpRegions: 7, carryRegions: 6, gaugeRegions: 5, proposeRegions: 1, propagateMaps: 4 };
const LIST_AT = { readRegions: 1, readWarpRegions: 1, carryRegions: 1, gaugeRegions: 1, proposeRegions: 1, propagateMaps: 2 };
const INDEXED = ['readFrame', 'readPlanes', 'readTensor', 'readMotion', 'readActivity', 'readResidual'];
const withArg = (args, at, v) => args.map((a, i) => (i === at ? v : a));
// stats() without what counts or times the run
const STABLE = ['frameWidth', 'frameHeight', 'codedWidth', 'codedHeight', 'pictureRate', 'keyMapGops', 'shardGops', 'firstGop', 'duration', 'parserThreads', 'gopsPerWindow', 'output', 'chromaWidth',
  'chromaHeight', 'tensorDtype', 'tensorElementBytes', 'tensorFrameBytes', 'tensorFramePitch', 'tensorGopPitch', 'tensorWidth', 'tensorHeight', 'tensorImageX', 'tensorImageY', 'tensorImageWidth',
  'tensorImageHeight', 'tensorLayout'];
function stats(p) {
  const s = p.stats(), stable = {};
  for (const k of STABLE) stable[k] = s[k];
  return { keys: Object.keys(s), stable: ser(stable) };
}

// ---- the decoder handle ---------------------------------------------------------------------------------------------------------
function decoder() {
  const h = backend.create({ codedWidth: 32, codedHeight: 32 });
  const T = 'decoder: ';
  pin(T + 'methods', () => Object.keys(h));
  for (const m of ['releaseSlot', 'convertRGBA', 'readPlanes', 'submitPicture', 'submitSparse']) {
    pin(T + m + ' without arguments', () => h[m]());
    if (!m.startsWith('submit')) pin(T + m + ' of a string', () => h[m]('x'));
  }
  pin(T + 'setQuantMatrices of 63 bytes', () => h.setQuantMatrices(new Uint8Array(63)));
  pin(T + 'setQuantMatrices of 63 bytes second', () => h.setQuantMatrices(new Uint8Array(64), new Uint8Array(63)));
  pin(T + 'setQuantMatrices of an Int8Array', () => h.setQuantMatrices(new Int8Array(64)));
  pin(T + 'setQuantMatrices of a number', () => h.setQuantMatrices(5));
  pin(T + 'setQuantMatrices of null and undefined', () => h.setQuantMatrices(null, undefined));
  pin(T + 'submitPicture with a short coefY', () => h.submitPicture({ type: 1, outSlot: 0, coefY: new Int16Array(32 * 32 - 1) }));
  pin(T + 'submitPicture with a Uint16Array coefCb', () => h.submitPicture({ type: 1, outSlot: 0, coefY: new Int16Array(32 * 32), coefCb: new Uint16Array(16 * 16) }));
  pin(T + 'submitPicture with a string type', () => h.submitPicture({ type: 'I' }));
  pin(T + 'submitPicture with an array for qscale', () => h.submitPicture({ type: 1, qscale: [1, 2, 3, 4] }));
  pin(T + 'submitSparse with a short grpOff', () => h.submitSparse({ type: 1, outSlot: 0, nEntries: 0, grpOff: new Uint32Array(2) }));
  pin(T + 'submitSparse with fewer entries than nEntries', () => h.submitSparse({ type: 1, outSlot: 0, nEntries: 5, grpOff: new Uint32Array(64), entries: new Uint32Array(4) }));
  pin(T + 'submitSparse with nEntries -1', () => h.submitSparse({ type: 1, outSlot: 0, nEntries: -1 }));
  pin(T + 'thirteen slots', () => { const s = []; for (let k = 0; k < 13; k++) s.push(h.acquireSlot()); return s; });
  pin(T + 'a fourteenth acquireSlot', () => h.acquireSlot());
  pin(T + 'releaseSlot past the ring', () => h.releaseSlot(13));
  pin(T + 'releaseSlot, freeDecodedSlots, sync', () => [h.releaseSlot(3), h.acquireSlot(), h.freeDecodedSlots(), h.sync()]);
  pin(T + 'destroy', () => h.destroy());
  for (const m of Object.keys(h)) pin(T + m + ' after destroy', () => h[m](0));
}

// ---- a pipeline's refusals in its first 'frames' handler ------------------------------------------------------------------------
function refusals(T, p, w, n) {
  const ok = valid(w);
  pin(T + 'methods', () => Object.keys(p));
  pin(T + 'stats', () => stats(p));
  for (const m of METHODS) {
    if (m === 'stats' || m === 'destroy') continue;          // (they take no argument; destroy comes last)
    pin(T + m + ' without arguments', () => p[m]());
    if (ok[m].length > 1 && m !== 'seek') pin(T + m + ' with one argument fewer', () => p[m](...ok[m].slice(0, -1)));          // (seek(seconds) is a whole call)
    if (m !== 'seek' && m !== 'feed') {
      pin(T + m + ' with a string window', () => p[m](...withArg(ok[m], 0, 'x')));
      if (m !== 'releaseWindow') pin(T + m + ' of a window never delivered', () => p[m](...withArg(ok[m], 0, w + 1000)));
    }
  }
  for (const m of INDEXED) {
    pin(T + m + ' with a string index', () => p[m](w, 'x'));
    pin(T + m + ' of an index past the window', () => p[m](w, n));
    pin(T + m + ' of index -1', () => p[m](w, -1));
  }
  for (const m of Object.keys(RECORDS)) {
    const k = RECORDS[m], at = LIST_AT[m], list = (v) => p[m](...withArg(ok[m], at, v));
    pin(T + m + ' with a Float32Array', () => list(new Float32Array(k)));
    pin(T + m + ' with a Uint32Array', () => list(new Uint32Array(k)));
    pin(T + m + ' with a plain array', () => list(new Array(k).fill(0)));
    if (k > 1) pin(T + m + ' with a word too many', () => list(i32(k + 1)));
    if (k > 1) pin(T + m + ' with a word too few', () => list(i32(2 * k - 1)));
    pin(T + m + ' with no record', () => list(i32(0)));
    pin(T + m + ' with 65536 records', () => list(i32(65536 * k)));
    pin(T + m + ' with 65537 records', () => list(i32(65537 * k)));
    for (let a = at + 1; a < ok[m].length; a++) pin(T + m + ' with a string for argument ' + a, () => p[m](...withArg(ok[m], a, 'x')));
  }
  const rr = valid(w).readRegions;
  for (let extra = 1; extra <= 4; extra++) pin(T + 'readRegions with ' + (5 + extra) + ' arguments', () => p.readRegions(...rr.concat([1, 0, 114, 7, 250].slice(0, extra))));
  pin(T + 'readRegions with a string anchor', () => p.readRegions(...rr.concat([1, 'x', 0, 0, 0])));
  pin(T + 'readRegions of size 0 x 8', () => p.readRegions(...withArg(rr, 2, 0)));
  pin(T + 'readRegions of size 8 x 4097', () => p.readRegions(...withArg(rr, 3, 4097)));
  pin(T + 'readWarpRegions of size 4097 x 8', () => p.readWarpRegions(...withArg(ok.readWarpRegions, 2, 4097)));
  pin(T + 'proposeRegions with a config of 7 words', () => p.proposeRegions(w, i32(1), i32(7)));
  pin(T + 'proposeRegions with a config of 9 words', () => p.proposeRegions(w, i32(1), i32(9)));
  pin(T + 'proposeRegions with a Uint8Array config', () => p.proposeRegions(w, i32(1), new Uint8Array(8)));
  pin(T + 'proposeRegions with maxBoxes 1025', () => p.proposeRegions(w, i32(1), Int32Array.from([3, 0, 1, 1, 8, 1, 1025, 0])));
  const pm = ok.propagateMaps;
  pin(T + 'propagateMaps with an Int32Array for the maps', () => p.propagateMaps(...withArg(pm, 1, i32(256))));
  pin(T + 'propagateMaps with a Float32Array for the maps', () => p.propagateMaps(...withArg(pm, 1, new Float32Array(256))));
  pin(T + 'propagateMaps with a map that is no whole number of slots', () => p.propagateMaps(...withArg(pm, 1, new Uint8Array(32 * 32 + 4))));
  pin(T + 'propagateMaps with an empty map', () => p.propagateMaps(...withArg(pm, 1, new Uint8Array(0))));
  pin(T + 'propagateMaps with stride 0', () => p.propagateMaps(...withArg(pm, 3, 0)));
  pin(T + 'propagateMaps with elemBytes 3', () => p.propagateMaps(...withArg(pm, 5, 3)));
  pin(T + 'propagateMaps with fill -1', () => p.propagateMaps(...withArg(withArg(pm, 6, -1), 0, w + 1000)));
  pin(T + 'feed of -1', () => p.feed(-1));
  pin(T + 'feed of a string', () => p.feed('x'));
  pin(T + 'feed past the stream', () => p.feed(stream.length + 1));
  pin(T + 'seek of a string', () => p.seek('x'));
}

function destroyed(T, p, w) {
  const ok = valid(w);
  pin(T + 'destroy', () => p.destroy());
  for (const m of METHODS) pin(T + m + ' after destroy', () => p[m](...ok[m]));
  for (const m of ['feed', 'releaseWindow', 'seek']) pin(T + m + ' without arguments after destroy', () => p[m]());
}

function finish() {
  // one case a line
  process.stdout.write('{\n' + Object.keys(out).map((k) => JSON.stringify(k) + ': ' + JSON.stringify(out[k])).join(',\n') + '\n}\n');
}

// B: every output; the handler is left through destroy(), so no 'ended' comes and the script ends because nothing holds the loop
function pipelineB() {
  const lp = new LeonPipeline(stream, { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, autoRelease: false, output: 'all', motion: true, activity: true, residual: true });
  let first = true;
  lp.on('error', (e) => { throw e; });
  lp.on('frames', (w, frames) => {
    if (!first) return;
    first = false;
    refusals('B: ', lp._p, w, frames.length);
    destroyed('B: ', lp._p, w);
    finish();
  });
}

// A: RGBA only -- what needs a tensor or a record output is refused with valid arguments
function pipelineA() {
  const lp = new LeonPipeline(stream, { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, autoRelease: false });
  let first = true;
  lp.on('error', (e) => { throw e; });
  lp.on('frames', (w) => {
    if (!first) return;
    first = false;
    const p = lp._p, ok = valid(w);
    pin('A: stats', () => stats(p));
    for (const m of ['readPlanes', 'readTensor', 'readMotion', 'readActivity', 'readResidual', 'readRegions', 'readWarpRegions', 'carryRegions', 'gaugeRegions', 'proposeRegions', 'propagateMaps']) {
      pin('A: ' + m + ' with valid arguments', () => p[m](...ok[m]));
    }
    pin('A: readRegions with fit', () => p.readRegions(...ok.readRegions.concat([1, 0, 0, 0, 0])));
    pin('A: readTensor without arguments comes before the output', () => p.readTensor());
    pin('A: readRegions with a bad list comes before the output', () => p.readRegions(...withArg(ok.readRegions, 1, i32(4))));
    pin('A: readRegions with 6 arguments comes before the output', () => p.readRegions(...ok.readRegions.concat([1])));
    pin('A: readWarpRegions with a bad list comes before the output', () => p.readWarpRegions(...withArg(ok.readWarpRegions, 1, i32(6))));
    destroyed('A: ', p, w);
    pipelineB();
  });
}

decoder();
pipelineA();
