#!/usr/bin/env node
/*
 * node_addon_refusal_pins.js -- what napi/leon_napi.node refuses before it touches a device: letterbox, create and createPipeline with
 * too few and wrong-typed arguments, a wrong-typed option of every group, the tensorLetterbox rules and validBytes.  An option set the
 * addon accepts is pinned by what it reaches: the stream is Buffer.alloc(16), which the library refuses ("no sequence header") before
 * any device call -- nothing here gets as far as a pipeline.  Every case records {class, message} of what was thrown (or what came
 * back); tests/test_node_binding_pins.py compares the one JSON object on stdout with tests/golden/node_addon_refusal_pins.json.
 *
 * The script ends by itself or not at all: a refusal that leaves the threadsafe function unreleased keeps the event loop alive, and
 * that is the only check of that cleanup -- no process.exit() here.
 *
 *   node tests/node_addon_refusal_pins.js      -> {name: {returned | thrown}, ...}
 */
'use strict';
const path = require('path');
const addon = require(path.join(__dirname, '..', 'mpeg1video-decoder-webgl_amd', 'napi', 'leon_napi.node'));

const out = {};
function pin(name, fn) {
  if (name in out) throw new Error('two cases named ' + name);
  try {
    const r = fn();
    out[name] = { returned: r === undefined ? '<undefined>' : (r !== null && typeof r === 'object' && !Array.isArray(r)) ? '<object>' : r };
  } catch (e) { out[name] = { thrown: { class: e.constructor.name, message: e.message } }; }
}
const cb = () => {};
const stream = () => Buffer.alloc(16);
const pipe = (name, opts) => pin('createPipeline: ' + name, () => addon.createPipeline(stream(), opts, cb));

pin('abiVersion', () => addon.abiVersion());
pin('exports', () => Object.keys(addon).sort());

pin('letterbox: no arguments', () => addon.letterbox());
pin('letterbox: three arguments', () => addon.letterbox(96, 64, 40));
pin('letterbox: a string', () => addon.letterbox(96, '64', 40, 40));
pin('letterbox: an object last', () => addon.letterbox(96, 64, 40, {}));
pin('letterbox: valid', () => addon.letterbox(96, 64, 40, 40));
pin('letterbox: a fifth argument is ignored', () => addon.letterbox(96, 64, 40, 40, 'x'));
pin('letterbox: a double truncates', () => addon.letterbox(96.9, 64, 40, 40));
pin('letterbox: refused by the library', () => addon.letterbox(0, 1, 1, 1));

pin('create: no arguments', () => addon.create());
pin('create: a string field', () => addon.create({ codedWidth: '32', codedHeight: 32 }));
pin('create: an object field', () => addon.create({ codedWidth: 32, codedHeight: 32, nSlots: {} }));
pin('create: alpha as a string', () => addon.create({ codedWidth: 32, codedHeight: 32, alpha: 'yes' }));
pin('create: no size (refused by the library)', () => addon.create({}));
pin('create: a size that is no multiple of 16 (refused by the library)', () => addon.create({ codedWidth: 30, codedHeight: 32 }));

pin('createPipeline: no arguments', () => addon.createPipeline());
pin('createPipeline: two arguments', () => addon.createPipeline(stream(), {}));
pin('createPipeline: a Uint8Array stream', () => addon.createPipeline(new Uint8Array(16), {}, cb));
pin('createPipeline: a string stream', () => addon.createPipeline('stream', {}, cb));
pin('createPipeline: a callback that is no function', () => addon.createPipeline(stream(), {}, {}));
pin('createPipeline: callback and options swapped', () => addon.createPipeline(stream(), cb, {}));

pipe('no options reaches the library', {});
pipe('null and undefined options count as absent', { deviceId: null, parserThreads: undefined, tensorDtype: null, tensorOutWidth: undefined, tensorLayout: null, tensorCanvasWidth: null,
  tensorScale: null, tensorBias: undefined, startSeconds: null, validBytes: null });
// a string in one option of each group (the config group, tensorDtype, the resize group, tensorLayout, the canvas group)
const GROUPS = { config: ['deviceId', 'parserThreads', 'gopsPerWindow', 'windowsInFlight', 'maxGopPictures', 'loop', 'shardIndex', 'shardCount', 'gpuParser', 'displayFlavour', 'output'],
  dtype: ['tensorDtype'], resize: ['tensorOutWidth', 'tensorOutHeight', 'tensorCropX', 'tensorCropY', 'tensorCropWidth', 'tensorCropHeight', 'tensorFilter'], layout: ['tensorLayout'],
  canvas: ['tensorCanvasWidth', 'tensorCanvasHeight', 'tensorOriginX', 'tensorOriginY', 'tensorOriginSet', 'tensorPadR', 'tensorPadG', 'tensorPadB', 'tensorLetterboxWidth', 'tensorLetterboxHeight'] };
for (const g of Object.keys(GROUPS)) {
  for (const name of GROUPS[g]) pipe(g + ' group: ' + name + ' as a string', { [name]: 'x' });
  pipe(g + ' group: ' + GROUPS[g][0] + ' as an object', { [GROUPS[g][0]]: {} });
  pipe(g + ' group: ' + GROUPS[g][0] + ' as a double reaches the library', { [GROUPS[g][0]]: 1.5 });
}
pipe('a bad integer option comes before a bad tensorScale', { tensorDtype: 'x', tensorScale: 5 });
pipe('a bad tensorScale comes before a bad resize option', { tensorScale: 5, tensorOutWidth: 'x' });
pipe('startSeconds as a string is ignored', { startSeconds: 'x' });
pipe('startSeconds as a number reaches the library', { startSeconds: 2.5 });
for (const key of ['tensorScale', 'tensorBias']) {
  pipe(key + ' as a number', { [key]: 5 });
  pipe(key + ' as a string', { [key]: 'abc' });
  pipe(key + ' as a Float32Array', { [key]: new Float32Array(3) });
  pipe(key + ' of length 2', { [key]: [1, 2] });
  pipe(key + ' of length 4', { [key]: [1, 2, 3, 4] });
  pipe(key + ' with a string element', { [key]: [1, '2', 3] });
  pipe(key + ' with a null element', { [key]: [1, 2, null] });
  pipe(key + ' of three numbers reaches the library', { [key]: [1, 2.5, -3] });
}
// tensorLetterbox derives the size, the canvas and the origin: it stands alone
const LB = { tensorLetterboxWidth: 40, tensorLetterboxHeight: 40 };
for (const beside of ['tensorOutWidth', 'tensorOutHeight', 'tensorCanvasWidth', 'tensorCanvasHeight', 'tensorOriginSet']) pipe('tensorLetterbox beside ' + beside, Object.assign({ [beside]: 1 }, LB));
pipe('tensorLetterboxWidth alone beside tensorOutWidth', { tensorLetterboxWidth: 40, tensorOutWidth: 8 });
pipe('tensorLetterbox beside tensorOriginX without tensorOriginSet reaches the stream', Object.assign({ tensorOriginX: 3 }, LB));
pipe('tensorLetterbox without a crop asks the stream for its size', LB);
pipe('tensorLetterbox with a crop reaches the library', Object.assign({ tensorCropWidth: 32, tensorCropHeight: 16 }, LB));
pipe('tensorLetterbox with a crop of no width is refused by the letterbox rule', Object.assign({ tensorCropX: 4 }, LB));
pipe('tensorLetterboxHeight alone with a crop', { tensorLetterboxHeight: 40, tensorCropWidth: 32, tensorCropHeight: 16 });
pipe('a canvas without an origin is centred and reaches the library', { tensorCanvasWidth: 48, tensorCanvasHeight: 48, tensorOutWidth: 40, tensorOutHeight: 24 });
pipe('every tensor option reaches the library', { output: 16, tensorDtype: 8, tensorLayout: 1, tensorOutWidth: 40, tensorOutHeight: 24, tensorFilter: 3, tensorCanvasWidth: 48, tensorCanvasHeight: 48,
  tensorOriginX: 1, tensorOriginY: 2, tensorOriginSet: 1, tensorPadR: 114, tensorPadG: 7, tensorPadB: 250 });
// validBytes: an integer between 0 and the stream's length
for (const v of [-1, 1.5, 17, 'x', true, {}, NaN, Infinity, 4294967296]) pipe('validBytes ' + (typeof v === 'object' ? '{}' : String(v)), { validBytes: v });
for (const v of [0, 8, 16]) pipe('validBytes ' + v + ' reaches the library', { validBytes: v });
pipe('validBytes -1 beside a tensor option', { validBytes: -1, output: 16 });
pipe('a bad integer option comes before a bad validBytes', { validBytes: -1, tensorLayout: 'x' });
pipe('the tensorLetterbox rule comes before a bad validBytes', Object.assign({ validBytes: -1, tensorOutWidth: 8 }, LB));

// one case a line
process.stdout.write('{\n' + Object.keys(out).map((k) => JSON.stringify(k) + ': ' + JSON.stringify(out[k])).join(',\n') + '\n}\n');
