"""GPU, under Node: dense maps propagated along the motion vectors through the real addon -- LeonPipeline.propagateMaps(window, maps,
hops, {stride, planes, elemBytes, fill}) with opts.motion, equal byte for byte to the Python host road (Pipeline.propagate_maps) of
the same stream, whose results tests/test_pipeline_propagate_gpu.py pins to propagate_map; a hop's fault is a status word, a call's
a throw."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

JSDIR = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "js")
STREAM = os.path.join(ROOT, "tests", "golden", "streams", "ibbp_96x64.jsv")
STRIDE, PLANES, ELEM, FILL = 2, 2, 2, 0xBEEF          # maps [slots][2][mh][mw] of 2-byte elements at stride 2: a multiple of 4 bytes whatever the frame

_SCRIPT = r"""
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, motion: true });
const opts = { stride: %(stride)d, planes: %(planes)d, elemBytes: %(elem)d, fill: %(fill)d };
const slotBytes = %(planes)d * %(mh)d * %(mw)d * %(elem)d;
const got = {};
let threw = 0;
lp.on('frames', (window, frames) => {
  const n = frames.length, slots = 2 + n, maps = Buffer.alloc(slots * slotBytes), hops = [];
  for (let i = 0; i < maps.length; i++) maps[i] = (i * 7 + (i >> 8) * 13 + window) & 255;
  for (let t = 0; t < n; t++) hops.push([t, 2 + t, 0, 1]);
  hops.push([n, 2, 0, 1], [0, 2, 2, 1]);
  const r = lp.propagateMaps(window, maps, hops, opts);
  got[window] = { n, maps: maps.toString('base64'), via: Buffer.from(r.via.buffer, r.via.byteOffset, r.via.length).toString('base64'), status: Array.from(r.status),
    kinds: [r.via.constructor.name, r.status.constructor.name] };
  for (const bad of [() => lp.propagateMaps(window + 1000, maps, hops, opts), () => lp.propagateMaps(window, maps, [], opts),
                     () => lp.propagateMaps(window, maps, [[0, 2, 0]], opts), () => lp.propagateMaps(window, maps, [[0, 2, 0, 0.5]], opts),
                     () => lp.propagateMaps(window, maps.subarray(0, maps.length - 2), hops, opts), () => lp.propagateMaps(window, [1, 2], hops, opts),
                     () => lp.propagateMaps(window, maps, hops, Object.assign({}, opts, { stride: 3 }))]) {
    try { bad(); } catch (e) { threw++; }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, threw })); lp.destroy(); });
"""


def test_propagate_maps_through_the_addon():
    import base64
    import leon_ctypes as L
    want, size = {}, [0, 0]

    def on_window(window, frames):
        n = len(frames)
        info = frames[0]["_pipe"].info
        mh, mw = -(-info.frame_height // STRIDE), -(-info.frame_width // STRIDE)
        size[:] = [mh, mw]
        slot_bytes = PLANES * mh * mw * ELEM
        i = np.arange((2 + n) * slot_bytes, dtype=np.int64)
        maps = ((i * 7 + (i >> 8) * 13 + window) & 255).astype(np.uint8).view(np.uint16).reshape(2 + n, PLANES, mh, mw)
        hops = [(t, 2 + t, 0, 1) for t in range(n)] + [(n, 2, 0, 1), (0, 2, 2, 1)]
        via, status = frames[0]["_pipe"].propagate_maps(window, maps, hops, STRIDE, fill=FILL)
        want[window] = (n, maps, via, status)
    pipe = L.Pipeline(open(STREAM, "rb").read(), on_window=on_window, motion=True, gops_per_window=1, gpu_parser=True, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "stride": STRIDE, "planes": PLANES, "elem": ELEM, "fill": FILL, "mh": size[0],
                                                   "mw": size[1]}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert sorted(int(w) for w in r["got"]) == sorted(want) and want
    moved = 0
    for w, (n, maps, via, status) in want.items():
        g = r["got"][str(w)]
        assert g["n"] == n and g["kinds"] == ["Uint8Array", "Int32Array"]
        assert g["status"] == status.tolist() and g["status"][-2:] == [L.REGION_FRAME, L.REGION_SLOT] and g["status"][:-2] == [0] * n
        assert base64.b64decode(g["maps"]) == maps.tobytes()
        assert base64.b64decode(g["via"]) == via.tobytes()
        moved += int((via[:n] != 0).sum())
    assert moved > 0
    assert r["threw"] == 7 * len(want)
