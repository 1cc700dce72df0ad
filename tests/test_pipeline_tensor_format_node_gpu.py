"""GPU, under Node: uint8 channels-last tensors through the real addon -- LeonPipeline.readTensor with tensorDtype 'uint8' and
tensorLayout 'hwc' returns a Uint8Array equal to the oracle's RGB bytes (resized with leon_ctypes.resize_rgb when tensorSize is
given); stats() reports the layout."""
import hashlib
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

_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const refused = [];
for (const bad of [{ tensorDtype: 'int8' }, { tensorLayout: 'nhwc' }, { tensorDtype: 'uint8', tensorBias: [0, 0, 1] }, { tensorLayout: 2 }]) {
  try { new LeonPipeline(fs.readFileSync(%(stream)r), Object.assign({ backend, output: 'tensor' }, bad)).destroy(); refused.push(false); } catch (e) { refused.push(String(e.message)); }
}
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), Object.assign({ backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, output: 'tensor',
  tensorDtype: 'uint8', tensorLayout: %(layout)r }, %(extra)s));
const got = [];
lp.on('frame', (f) => {
  const t = lp.readTensor(f.window, f.index);
  got.push({ gop: f.gop, di: f.displayIndex, sha: sha(t), n: t.length, kind: t.constructor.name });
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused, stats: lp.stats() })); lp.destroy(); });
"""


def _node(script):
    out = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("size", [None, (40, 56)], ids=["frame-size", "resized"])
def test_read_uint8_tensor_through_the_addon(size, layout):
    import leon_ctypes as L
    from test_pipeline_gpu import oracle_frames
    want = {}
    for k, v in oracle_frames(open(STREAM, "rb").read()).items():
        rgb = v[..., :3] if size is None else L.resize_rgb(v[..., :3], None, size)
        want[k] = hashlib.sha256(np.ascontiguousarray(rgb if layout == "hwc" else rgb.transpose(2, 0, 1)).tobytes()).hexdigest()
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "layout": layout, "extra": json.dumps({} if size is None else {"tensorSize": list(size)})})
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want)
    s = r["stats"]
    h, w = size or (s["frameHeight"], s["frameWidth"])
    assert (s["output"], s["tensorDtype"], s["tensorElementBytes"], s["tensorLayout"]) == (16, L.TENSOR_U8, 1, layout)
    assert (s["tensorHeight"], s["tensorWidth"], s["tensorFrameBytes"]) == (h, w, 3 * h * w)
    for f in r["got"]:
        assert f["kind"] == "Uint8Array" and f["n"] == 3 * h * w
        assert f["sha"] == want[(f["gop"], f["di"])], f
    # an unknown dtype names the four, an unknown layout the two; the library refuses uint8 with a bias and layout 2
    assert all(r["refused"]), r["refused"]
    assert all(n in r["refused"][0] for n in ("float16", "bfloat16", "float32", "uint8")) and "hwc" in r["refused"][1]
