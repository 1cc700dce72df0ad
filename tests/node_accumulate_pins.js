#!/usr/bin/env node
/*
 * node_accumulate_pins.js -- LeonPipeline.accumulate (mpeg1video-decoder-webgl_amd/js/leon_pipeline.js) over a recording stand-in for
 * the addon (opts.backend): no addon, no device.  In the manner of node_wrapper_pins.js, for the one method that came after it: every
 * case records what came back and what reached the backend (typed arrays as {kind, values}), or {class, message} of what was thrown.
 * tests/test_pipeline_accumulate_node_gpu.py compares the one JSON object on stdout with tests/golden/node_accumulate_pins.json.
 *
 *   node tests/node_accumulate_pins.js      -> {name: {returned | thrown, calls}, ...}
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

// the stand-in: the handle's accumulate records its marshalled arguments
function stub(calls) {
  return { createPipeline() { return { accumulate: (...args) => { calls.push({ call: 'accumulate', args: ser(args) }); return 'accumulate result'; } }; } };
}

const out = {};
function pin(name, fn) {
  if (name in out) throw new Error('two cases named ' + name);
  const calls = [];
  const r = { calls };
  try { r.returned = ser(fn(calls)); } catch (e) { r.thrown = ser(e); }
  out[name] = r;
}
const STREAM = Buffer.from([0, 0, 1, 0xb3]);
const make = (calls, opts) => new LeonPipeline(STREAM, Object.assign({ backend: stub(calls) }, opts));
const BOTH = { motion: true, residual: true };
const HOPS = [[1, 2, 0, -1], [4, 3, 2, -1]];

pin('valid', (calls) => make(calls, BOTH).accumulate(3, HOPS, { parts: 3, slots: new Int16Array(4) }));
// without options: every part the outputs allow, one slot more than the largest the hops name
const HAVE = { nothing: {}, motion: { motion: true }, residual: { residual: true }, 'motion+residual': BOTH, 'motion+activity': { motion: true, activity: true } };
for (const have of Object.keys(HAVE)) {
  pin('defaults: pipeline with ' + have, (calls) => make(calls, HAVE[have]).accumulate(3, [[1, 2, 4, -1]]));
  pin('opts {}: pipeline with ' + have, (calls) => make(calls, HAVE[have]).accumulate(3, [[1, 2, -1, 3]], {}));
}
pin('a chain\'s start alone', (calls) => make(calls, BOTH).accumulate(3, [[0, 0, -1, -1]]));
// the record list, as the wrapper's other methods take theirs
const row = (n) => [1, 2, 3, 4, 5, 6].slice(0, n);
const LISTS = { valid: [row(4), row(4)], empty: [], short: [row(4), row(3)], long: [row(5)], 'non-integer': [row(3).concat([0.5])], 'string word': [row(3).concat(['1'])],
  'row not an array': [row(4), 5], 'not an array': 'x', 'a typed array': new Int32Array(4), undefined: undefined, null: null };
for (const name of Object.keys(LISTS)) pin('hops: records ' + name, (calls) => make(calls, BOTH).accumulate(3, LISTS[name], { slots: 2 }));
// slots: an Int16Array as it is, an integer as it is, anything else a TypeError
const SLOTS = { Int16Array: new Int16Array([1, -2]), 'Int16Array view': new Int16Array(8).subarray(2, 6), number: 7, zero: 0, negative: -1, 'non-integer': 1.5, string: '2', null: null,
  Uint8Array: new Uint8Array(4), Buffer: Buffer.alloc(4), Int32Array: new Int32Array(2), array: [1, 2], object: {} };
for (const kind of Object.keys(SLOTS)) pin('slots: ' + kind, (calls) => make(calls, BOTH).accumulate(3, HOPS, { slots: SLOTS[kind] }));
for (const parts of [1, 2, 3, 0, 4, -1, 1.5, '3', null, true]) pin('parts: ' + JSON.stringify(parts), (calls) => make(calls, BOTH).accumulate(3, HOPS, { parts, slots: 1 }));
pin('bad hops come before bad slots', (calls) => make(calls, BOTH).accumulate(3, [[1]], { slots: 'x', parts: 1.5 }));
pin('bad slots come before bad parts', (calls) => make(calls, BOTH).accumulate(3, HOPS, { slots: 'x', parts: 1.5 }));
pin('the window goes on as it is', (calls) => make(calls, BOTH).accumulate('w', HOPS, { slots: 1 }));

// one case a line
process.stdout.write('{\n' + Object.keys(out).map((k) => JSON.stringify(k) + ': ' + JSON.stringify(out[k])).join(',\n') + '\n}\n');
