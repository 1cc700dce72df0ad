#!/usr/bin/env node
/*
 * node_wrapper_pins.js -- mpeg1video-decoder-webgl_amd/js/leon_pipeline.js over a recording stand-in for the addon (opts.backend): no
 * addon, no device.  Every case records what came back and what reached the backend (typed arrays as {kind, values}), or {class,
 * message} of what was thrown.  tests/test_node_binding_pins.py compares the one JSON object on stdout with
 * tests/golden/node_wrapper_pins.json, recorded once from the wrapper as it stood before its call shapes were folded into helpers.
 *
 *   node tests/node_wrapper_pins.js      -> {name: {returned | thrown, calls, ...}, ...}
 */
'use strict';
const path = require('path');
const { LeonPipeline } = require(path.join(__dirname, '..', 'mpeg1video-decoder-webgl_amd', 'js', 'leon_pipeline.js'));

function ser(v) {
  if (v === undefined) return '<undefined>';
  if (v === null || typeof v === 'boolean' || typeof v === 'string') return v;
  if (typeof v === 'number') return Number.isFinite(v) ? v : String(v);
  if (typeof v === 'function') return '<function>';
  if (v instanceof Error) return { class: v.constructor.name, message: v.message };
  if (ArrayBuffer.isView(v)) return { kind: v.constructor.name, values: Array.from(v) };
  if (Array.isArray(v)) return v.map(ser);
  const o = {};
  for (const k of Object.keys(v)) o[k] = k === 'backend' ? '<backend>' : ser(v[k]);
  return o;
}

const METHODS = ['releaseWindow', 'readFrame', 'readPlanes', 'readTensor', 'readMotion', 'readActivity', 'readResidual', 'readRegions', 'readWarpRegions',
  'carryRegions', 'gaugeRegions', 'proposeRegions', 'propagateMaps', 'stats', 'destroy', 'feed', 'seek'];

// the stand-in: createPipeline and every method of the handle record their marshalled arguments; `returns` says what a method gives back
function stub(calls, returns) {
  const backend = {
    createPipeline(stream, opts, cb) {
      calls.push({ call: 'createPipeline', stream: ser(stream), opts: ser(opts), cb: ser(cb) });
      backend.deliver = cb;
      const h = {};
      for (const m of METHODS) h[m] = (...args) => { calls.push({ call: m, args: ser(args) }); return returns && m in returns ? returns[m] : m + ' result'; };
      return h;
    },
    letterbox(...args) { calls.push({ call: 'letterbox', args: ser(args) }); return [1, 2, 3, 4]; }
  };
  return backend;
}

const out = {};
function pin(name, fn) {
  if (name in out) throw new Error('two cases named ' + name);
  const calls = [];
  const r = { calls };
  try { r.returned = ser(fn(calls)); } catch (e) { r.thrown = ser(e); }
  if (!name.startsWith('new:') && calls.length && calls[0].call === 'createPipeline') calls.shift();          // (the constructor's cases hold it)
  out[name] = r;
}
const STREAM = Buffer.from([0, 0, 1, 0xb3]);
const make = (calls, opts, returns) => new LeonPipeline(STREAM, Object.assign({ backend: stub(calls, returns) }, opts));
const state = (lp) => ({ gaugeSources: lp._gaugeSources, autoRelease: lp.autoRelease, ended: lp.ended });

// ---- the constructor ------------------------------------------------------------------------------------
const NAMES = { output: ['rgba', 'ycbcr', 'both', 'tensor', 'rgba+tensor', 'ycbcr+tensor', 'all'], tensorDtype: ['float16', 'bfloat16', 'float32', 'uint8'],
  tensorLayout: ['chw', 'hwc'], tensorFilter: ['triangle', 'bicubic'] };
pin('new: no options', (calls) => state(new LeonPipeline(new Uint8Array([9, 0, 0, 1, 0xb3, 9]).subarray(1, 5), { backend: stub(calls) })));
pin('new: options pass through', (calls) => state(make(calls, { parserThreads: 3, gopsPerWindow: 2, validBytes: 4, startSeconds: 1.5, tensorScale: [1, 2, 3], autoRelease: false })));
for (const opt of Object.keys(NAMES)) {
  for (const v of NAMES[opt].concat([5, 'bogus', true, null, [1], 2.5])) pin('new: ' + opt + ' ' + JSON.stringify(v), (calls) => state(make(calls, { [opt]: v })));
}
for (const rec of [['motion'], ['activity'], ['residual'], ['motion', 'activity'], ['motion', 'activity', 'residual']]) {
  for (const output of [undefined, 0, 64].concat(NAMES.output)) {
    pin('new: ' + rec.join('+') + ' beside output ' + JSON.stringify(output), (calls) => {
      const opts = { output };
      for (const k of rec) opts[k] = true;
      return state(make(calls, opts));
    });
  }
}
pin('new: motion 0, activity 1, residual ""', (calls) => state(make(calls, { motion: 0, activity: 1, residual: '' })));
const LISTS = { tensorSize: 2, tensorCrop: 4, tensorCanvas: 2, tensorOrigin: 2, tensorPadValue: 3, tensorLetterbox: 2 };
for (const opt of Object.keys(LISTS)) {
  const n = LISTS[opt], good = [11, 12, 13, 14].slice(0, n);
  const values = [good, null, undefined, good.slice(1), good.concat([15]), good.slice(1).concat([1.5]), good.slice(1).concat(['7']), 7, 'ab', new Int32Array(n), new Array(n).fill(0)];
  values.forEach((v, i) => pin('new: ' + opt + ' #' + i + ' ' + (v === undefined ? 'undefined' : JSON.stringify(ser(v))), (calls) => state(make(calls, { [opt]: v }))));
}
pin('new: every list at once', (calls) => state(make(calls, { output: 'tensor', tensorSize: [24, 40], tensorCrop: [5, 2, 80, 50], tensorCanvas: [48, 48], tensorOrigin: [0, 3],
  tensorPadValue: [114, 7, 250], tensorFilter: 'bicubic', tensorDtype: 'uint8', tensorLayout: 'hwc' })));
pin('new: tensorLetterbox with a crop and a pad value', (calls) => state(make(calls, { tensorLetterbox: [40, 40], tensorCrop: [0, 0, 32, 16], tensorPadValue: [1, 2, 3] })));

// ---- the methods that pass their arguments on ---------------------------------------------------------------
pin('pass through', (calls) => {
  const lp = make(calls, {}, { seek: 7, stats: { pictures: 1 }, readFrame: new Uint8Array([1, 2]) });
  const r = [lp.feed(12), lp.seek(1.5), lp.seek(2, { exact: true }), lp.seek(3, { exact: 0 }), lp.seek(4, {}), lp.readFrame(1, 2), lp.readPlanes(3, 4), lp.readTensor(5, 6), lp.readMotion(7, 8),
    lp.readResidual(9, 10), lp.releaseWindow(11), lp.stats(), lp._seekFirst, lp.destroy(), lp._p, lp.destroy()];
  return r;
});
pin('letterbox', (calls) => LeonPipeline.letterbox(96, 64, 40, 40, stub(calls)));
pin('readActivity splits the cells', (calls) => {
  const cells = new Uint8Array(24 + 8).subarray(8);          // (a view at an offset: the wrapper reads from byteOffset)
  for (let k = 0; k < 24; k++) cells[k] = 17 * k + 3;
  return make(calls, {}, { readActivity: { cells, summary: new Uint32Array([1, 2, 3, 4, 5, 6, 7, 8]), mbWidth: 3, mbHeight: 1 } }).readActivity(2, 1);
});

// ---- the record lists: a valid call, the empty list, a row one word short and one long, a non-integer word, a non-array ----------
function lists(method, k, call, row) {
  row = row || ((n) => [1, 2, 3, 4, 5, 6, 7, 8].slice(0, n));
  const cases = { valid: [row(k), row(k)], empty: [], short: [row(k), row(k - 1)], long: [row(k + 1)], 'non-integer': [row(k - 1).concat([0.5])], 'string word': [row(k - 1).concat(['1'])],
    'row not an array': [row(k), 5], 'not an array': 'x', 'a typed array': new Int32Array(k), undefined: undefined, null: null };
  for (const name of Object.keys(cases)) pin(method + ': records ' + name, (calls) => call(make(calls, { motion: true, activity: true }), cases[name]));
}
const SIZE = { size: [8, 16] };
lists('readRegions', 5, (lp, r) => lp.readRegions(3, r, SIZE));
lists('readWarpRegions', 2, (lp, r) => lp.readWarpRegions(3, r, SIZE), (n) => [4, [65536, 0, 1, 0, 65536, 2]].slice(0, n).concat(n > 2 ? [9] : []));
for (const [name, r] of [['matrix short', [[0, [1, 2, 3, 4, 5]]]], ['matrix long', [[0, [1, 2, 3, 4, 5, 6, 7]]]], ['matrix non-integer', [[0, [1, 2, 3, 4, 5, 6.5]]]], ['matrix not an array', [[0, 6]]],
  ['frame non-integer', [[0.5, [1, 2, 3, 4, 5, 6]]]]]) {
  pin('readWarpRegions: records ' + name, (calls) => make(calls).readWarpRegions(3, r, SIZE));
}
lists('carryRegions', 6, (lp, r) => lp.carryRegions(3, r));
lists('gaugeRegions', 5, (lp, r) => lp.gaugeRegions(3, r));
lists('propagateMaps', 4, (lp, r) => lp.propagateMaps(3, Buffer.alloc(8), r));
for (const [name, f] of [['valid', [0, 1, 2]], ['empty', []], ['non-integer', [0, 0.5]], ['string word', ['0']], ['a row', [[0]]], ['not an array', 'x'], ['a typed array', new Int32Array(2)], ['undefined', undefined]]) {
  pin('proposeRegions: frames ' + name, (calls) => make(calls, { motion: true, activity: true }).proposeRegions(3, f, { mvMin: 1, acMin: 2 }));
}

// ---- readRegions / readWarpRegions: size, filter, fit, anchor, padValue ------------------------------------------------------
const BOX = [[0, 1, 2, 30, 20]], WARP = [[0, [65536, 0, 0, 0, 65536, 0]]];
const rr = (name, opts) => pin('readRegions: ' + name, (calls) => make(calls).readRegions(4, BOX, opts));
rr('no options', undefined);
for (const [i, size] of [undefined, null, [8], [8, 16, 3], [8, 1.5], ['8', 16], 8, new Int32Array(2)].entries()) {
  rr('size #' + i, { size });
  pin('readWarpRegions: size #' + i, (calls) => make(calls).readWarpRegions(4, WARP, { size }));
}
pin('readWarpRegions: no options', (calls) => make(calls).readWarpRegions(4, WARP));
for (const filter of ['triangle', 'bicubic', 3, 'lanczos', 1.5, null, true]) rr('filter ' + JSON.stringify(filter), { size: [8, 16], filter });
rr('an unknown filter comes before a bad size', { filter: 'lanczos' });
rr('a bad size comes before bad regions', { size: [8] });
for (const fit of ['stretch', 'letterbox', 1, 7, 'cover', 1.5, null, true, [1]]) rr('fit ' + JSON.stringify(fit), { size: [8, 16], fit });
for (const anchor of ['centre', 'center', 'top_left', 1, 'bottom', 0.5, null, false]) rr('anchor ' + JSON.stringify(anchor), { size: [8, 16], anchor });
for (const [i, padValue] of [[1, 2, 3], [1, 2], [1, 2, 3, 4], [1, 2, 0.5], ['1', 2, 3], 5, null, new Uint8Array(3)].entries()) {
  rr('padValue #' + i, { size: [8, 16], padValue });
  pin('readWarpRegions: padValue #' + i, (calls) => make(calls).readWarpRegions(4, WARP, { size: [8, 16], padValue }));
}
rr('fit, anchor, padValue and filter', { size: [8, 16], filter: 'bicubic', fit: 'letterbox', anchor: 'top_left', padValue: [114, 7, 250] });
rr('an unknown fit comes before an unknown anchor', { size: [8, 16], fit: 'cover', anchor: 'bottom' });
rr('an unknown anchor comes before a bad padValue', { size: [8, 16], anchor: 'bottom', padValue: [1] });
rr('a bad padValue comes before a non-integer fit', { size: [8, 16], fit: 1.5, padValue: [1] });
rr('bad regions come before an unknown fit', { size: [8, 16], fit: 'cover' });
pin('readRegions: bad regions with fit', (calls) => make(calls).readRegions(4, [[1]], { size: [8, 16], fit: 'cover' }));

// ---- gaugeRegions / proposeRegions: sources and the eight words ----------------------------------------------------------------
const HAVE = { none: {}, motion: { motion: true }, activity: { activity: true }, both: { motion: true, activity: true } };
for (const have of Object.keys(HAVE)) {
  pin('gaugeRegions: sources absent, pipeline with ' + have, (calls) => make(calls, HAVE[have]).gaugeRegions(5, BOX));
  pin('gaugeRegions: opts {}, pipeline with ' + have, (calls) => make(calls, HAVE[have]).gaugeRegions(5, BOX, {}));
  pin('proposeRegions: default sources, pipeline with ' + have, (calls) => make(calls, HAVE[have]).proposeRegions(5, [0, 1], { mvMin: 2, acMin: 64 }));
  pin('proposeRegions: no thresholds, pipeline with ' + have, (calls) => make(calls, HAVE[have]).proposeRegions(5, [0, 1], {}));
  pin('proposeRegions: no options, pipeline with ' + have, (calls) => make(calls, HAVE[have]).proposeRegions(5, [0, 1]));
  pin('proposeRegions: mvMin only, pipeline with ' + have, (calls) => make(calls, HAVE[have]).proposeRegions(5, [0, 1], { mvMin: 2 }));
  pin('proposeRegions: acMin only, pipeline with ' + have, (calls) => make(calls, HAVE[have]).proposeRegions(5, [0, 1], { acMin: 64 }));
}
for (const sources of [1, 2, 3, 0, 7, '1', 1.5, null, true]) {
  pin('gaugeRegions: sources ' + JSON.stringify(sources), (calls) => make(calls, HAVE.both).gaugeRegions(5, BOX, { sources }));
  pin('proposeRegions: sources ' + JSON.stringify(sources), (calls) => make(calls, HAVE.both).proposeRegions(5, [0], { sources, mvMin: 2, acMin: 64 }));
}
const WORDS = { intra: [true, false, 1, 0, 'yes'], mvMin: [1, 0, 1.5, '2', null], acMin: [1, 0, 1.5, '2', null], connectivity: [4, 8, 6, 4.5, '8', null], minCells: [1, 5, 0, 2.5, null],
  maxBoxes: [1, 1024, 1025, 0.5, null, '16'] };
for (const word of Object.keys(WORDS)) {
  for (const v of WORDS[word]) pin('proposeRegions: ' + word + ' ' + JSON.stringify(v), (calls) => make(calls, HAVE.both).proposeRegions(5, [2], Object.assign({ mvMin: 3, acMin: 9 }, { [word]: v })));
}
pin('proposeRegions: every word', (calls) => make(calls, HAVE.both).proposeRegions(5, [2, 0], { sources: 3, intra: true, mvMin: 2, acMin: 200, connectivity: 4, minCells: 2, maxBoxes: 3 }));
pin('proposeRegions: sources 1 drops acMin, sources 2 drops mvMin', (calls) => {
  const lp = make(calls, HAVE.both);
  return [lp.proposeRegions(5, [2], { sources: 1, mvMin: 2, acMin: 'x' }), lp.proposeRegions(5, [2], { sources: 2, mvMin: 'x', acMin: 9 })];
});

// ---- propagateMaps: the maps and the four numbers ---------------------------------------------------------------------------------
const HOPS = [[1, 2, 0, -1]];
const maps = { Buffer: Buffer.from([1, 2, 3, 4]), Uint8Array: new Uint8Array([5, 6, 7, 8]), Float32Array: new Float32Array(2), Uint8ClampedArray: new Uint8ClampedArray(4), ArrayBuffer: new ArrayBuffer(4),
  array: [1, 2, 3, 4], undefined: undefined };
for (const kind of Object.keys(maps)) pin('propagateMaps: maps ' + kind, (calls) => make(calls).propagateMaps(6, maps[kind], HOPS));
for (const [i, opts] of [{ fill: -1 }, { fill: 0x3C00, stride: 4, planes: 2, elemBytes: 2 }, { fill: 4294967295 }, { fill: 4294967296 }, { fill: 0.5 }, { stride: '4' }, { planes: null }, { elemBytes: 1.5 },
  { stride: undefined }, {}].entries()) {
  pin('propagateMaps: opts #' + i + ' ' + JSON.stringify(opts), (calls) => make(calls).propagateMaps(6, maps.Buffer, HOPS, opts));
}
pin('propagateMaps: bad maps come before bad hops', (calls) => make(calls).propagateMaps(6, [1], [[1]]));
pin('propagateMaps: bad hops come before bad opts', (calls) => make(calls).propagateMaps(6, maps.Buffer, [[1]], { fill: 0.5 }));

// ---- _deliver: what the addon's callback turns into ------------------------------------------------------------------------------
function events(lp, log) {
  for (const ev of ['frames', 'frame', 'seeked', 'ended', 'error']) lp.on(ev, (...args) => log.push({ event: ev, args: ser(args), ended: lp.ended }));
}
const FRAMES = () => [{ gop: 0, displayIndex: 0, type: 1, ts: 0 }, { gop: 0, displayIndex: 1, type: 2, ts: 40 }];
function delivered(name, opts, drive) {
  pin('_deliver: ' + name, (calls) => {
    const backend = stub(calls, { seek: 7 }), lp = new LeonPipeline(STREAM, Object.assign({ backend }, opts)), log = [];
    events(lp, log);
    drive(backend.deliver, lp, log, calls);
    return { log, state: state(lp) };
  });
}
delivered("'ended' without a status", {}, (d) => d(-1, [], 0));
delivered("'ended' with a status", {}, (d) => d(-1, [], -5));
delivered("'ended' with undefined frames and status", {}, (d) => d(-1));
delivered('a window', {}, (d) => d(3, FRAMES(), 0));
delivered('a window of no frames', {}, (d) => d(3, [], 0));
delivered('a failed window is released', {}, (d) => d(3, FRAMES(), -4));
delivered('a failed window is released without autoRelease too', { autoRelease: false }, (d) => d(3, FRAMES(), -4));
delivered('autoRelease: false', { autoRelease: false }, (d) => d(3, FRAMES(), 0));
delivered('autoRelease: 0 is not false', { autoRelease: 0 }, (d) => d(3, FRAMES(), 0));
delivered('seeked comes with the first window at or past the seek', {}, (d, lp, log) => {
  d(5, FRAMES(), 0);
  d(-1, [], 0);
  log.push({ seek: lp.seek(2.5, { exact: true }), ended: lp.ended, seekFirst: lp._seekFirst });
  d(6, FRAMES(), 0);
  d(7, FRAMES(), 0);
  d(8, FRAMES(), 0);
  d(-1, [], 0);
});
delivered('a failed window does not answer a seek', {}, (d, lp, log) => {
  log.push({ seek: lp.seek(0) });
  d(7, FRAMES(), -4);
  d(9, FRAMES(), 0);
});

// one case a line
process.stdout.write('{\n' + Object.keys(out).map((k) => JSON.stringify(k) + ': ' + JSON.stringify(out[k])).join(',\n') + '\n}\n');
