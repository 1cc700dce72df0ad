"""GPU, under Node: motion and residual accumulated along the motion vectors through the real addon -- LeonPipeline.accumulate(window,
hops, {parts, slots}) with opts.motion and opts.residual, equal byte for byte to the Python host road (Pipeline.accumulate) of the same
stream, whose results tests/test_pipeline_accumulate_gpu.py pins to accumulate_hop; slots the wrapper makes are all zero; a hop's fault
is a status word, a call's a throw.  CPU, under Node: the wrapper's new method over a recording stand-in for the addon
(tests/node_accumulate_pins.js against tests/golden/node_accumulate_pins.json), in the manner of tests/test_node_binding_pins.py."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT

NODE = pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")

JSDIR = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "js")
STREAM = os.path.join(ROOT, "tests", "golden", "streams", "ibbp_96x64.jsv")
PARTS = 3

_SCRIPT = r"""
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, motion: true, residual: true });
const slotBytes = %(slot_bytes)d;
const b64 = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('base64');
const got = {};
let threw = 0;
lp.on('frames', (window, frames) => {
  const n = frames.length, count = 2 + n, bytes = Buffer.alloc(count * slotBytes), hops = [];
  for (let i = 0; i < bytes.length; i++) bytes[i] = (i * 7 + (i >> 8) * 13 + window) & 255;
  const slots = new Int16Array(bytes.buffer, bytes.byteOffset, bytes.length / 2);
  for (let t = 0; t < n; t++) hops.push([t, 2 + t, 0, 1]);
  hops.push([n, 2, 0, 1], [0, 2, 2, 1]);
  const r = lp.accumulate(window, hops, { parts: %(parts)d, slots });
  // a chain's start, in slots the wrapper makes: all zero, one more than the largest slot named, every part the outputs allow
  const z = lp.accumulate(window, [[0, 1, -1, -1]]);
  got[window] = { n, same: r.slots === slots, slots: b64(r.slots), via: b64(r.via), status: Array.from(r.status), layout: r.layout,
    kinds: [r.slots.constructor.name, r.via.constructor.name, r.status.constructor.name],
    made: { length: z.slots.length, zero: z.slots.every((v) => v === 0), status: Array.from(z.status), parts: z.layout.parts, via: Array.from(z.via).every((v) => v === 0) } };
  for (const bad of [() => lp.accumulate(window + 1000, hops, { slots }), () => lp.accumulate(window, [], { slots }), () => lp.accumulate(window, [[0, 2, 0]], { slots }),
                     () => lp.accumulate(window, [[0, 2, 0, 0.5]], { slots }), () => lp.accumulate(window, hops, { slots: slots.subarray(0, slots.length - 2) }),
                     () => lp.accumulate(window, hops, { slots: [1, 2] }), () => lp.accumulate(window, hops, { slots, parts: 4 }), () => lp.accumulate(window, hops, { slots: 0 }),
                     () => lp.accumulate(window, hops, { slots: new Uint8Array(count * slotBytes) })]) {
    try { bad(); } catch (e) { threw++; }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, threw, enumerable: Object.keys(lp._p).includes('accumulate') })); lp.destroy(); });
"""


@NODE
@pytest.mark.gpu
def test_accumulate_through_the_addon():
    import leon_ctypes as L
    want, lay = {}, [None]

    def on_window(window, frames):
        pipe, n = frames[0]["_pipe"], len(frames)
        lay[0] = pipe.accumulate_layout(PARTS)
        i = np.arange((2 + n) * lay[0].slot_bytes, dtype=np.int64)
        slots = ((i * 7 + (i >> 8) * 13 + window) & 255).astype(np.uint8).reshape(2 + n, lay[0].slot_bytes)
        hops = [(t, 2 + t, 0, 1) for t in range(n)] + [(n, 2, 0, 1), (0, 2, 2, 1)]
        via, status = pipe.accumulate(window, slots, hops, PARTS)
        want[window] = (n, slots, via, status)
    pipe = L.Pipeline(open(STREAM, "rb").read(), on_window=on_window, motion=True, residual=True, gops_per_window=1, gpu_parser=True, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "parts": PARTS, "slot_bytes": lay[0].slot_bytes}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert sorted(int(w) for w in r["got"]) == sorted(want) and want
    moved = 0
    names = {"codedWidth": "coded_width", "codedHeight": "coded_height", "parts": "parts", "planes": "planes", "lumaStride": "luma_stride", "chromaStride": "chroma_stride",
             "axOffset": "ax_offset", "ayOffset": "ay_offset", "ageOffset": "age_offset", "ryOffset": "ry_offset", "rcbOffset": "rcb_offset", "rcrOffset": "rcr_offset",
             "slotBytes": "slot_bytes", "slotPitch": "slot_pitch"}
    for w, (n, slots, via, status) in want.items():
        g = r["got"][str(w)]
        assert g["n"] == n and g["same"] and g["kinds"] == ["Int16Array", "Uint8Array", "Int32Array"]
        assert g["status"] == status.tolist() and g["status"][-2:] == [L.REGION_FRAME, L.REGION_SLOT] and g["status"][:-2] == [0] * n
        assert base64.b64decode(g["slots"]) == slots.tobytes()
        assert base64.b64decode(g["via"]) == via.tobytes()
        assert g["layout"] == {k: getattr(lay[0], v) for k, v in names.items()}
        assert g["made"] == {"length": 2 * lay[0].slot_bytes // 2, "zero": True, "status": [0], "parts": 3, "via": True}
        moved += int((via[:n] != 0).sum())
    assert moved > 0
    assert r["threw"] == 9 * len(want)
    assert r["enumerable"] is False          # the handle's enumerable keys are what they were


@NODE
def test_wrapper_method_over_a_recording_backend():
    out = subprocess.run(["node", os.path.join(ROOT, "tests", "node_accumulate_pins.js")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads(out.stdout)
    with open(os.path.join(ROOT, "tests", "golden", "node_accumulate_pins.json")) as f:
        want = json.load(f)
    assert list(got) == list(want) and len(want) >= 30, (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    differ = [name for name in want if got[name] != want[name]]
    assert not differ, "\n".join("%s\n  got  %s\n  want %s" % (n, json.dumps(got[n])[:600], json.dumps(want[n])[:600]) for n in differ[:10])
    # what the fixture is to hold, by hand: the marshalled call, the defaults, the order of the refusals
    assert want["valid"]["calls"] == [{"call": "accumulate", "args": [3, {"kind": "Int32Array", "values": [1, 2, 0, -1, 4, 3, 2, -1]}, 3, {"kind": "Int16Array", "values": [0, 0, 0, 0]}]}]
    assert want["valid"]["returned"] == "accumulate result"
    assert want["defaults: pipeline with motion"]["calls"][0]["args"][2:] == [1, 5] and want["defaults: pipeline with motion+residual"]["calls"][0]["args"][2:] == [3, 5]
    assert want["hops: records short"]["thrown"]["class"] == "TypeError" and not want["hops: records short"]["calls"]
    assert want["hops: records empty"]["calls"][0]["args"][1] == {"kind": "Int32Array", "values": []}          # (the addon refuses a call of no hops)
    assert want["bad hops come before bad slots"]["thrown"]["message"].startswith("hops:")
    assert want["bad slots come before bad parts"]["thrown"]["message"].startswith("opts.slots:")
