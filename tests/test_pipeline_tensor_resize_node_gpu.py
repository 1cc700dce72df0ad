"""GPU, under Node: the resized tensor output through the real addon -- LeonPipeline with tensorSize / tensorCrop, readTensor equal
to the Python expectation (the table T looked up with leon_ctypes.resize_rgb of the oracle's RGBA); stats() reports the tensor's size."""
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
STREAM = os.path.join(ROOT, "tests", "golden", "streams", "leon_synth_352x240.jsv")

_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
let refused = false;
try { new LeonPipeline(fs.readFileSync(%(stream)r), { backend, output: 'rgba', tensorSize: [10, 10] }); } catch (e) { refused = true; }
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: %(gpu)s, output: 'tensor',
  tensorDtype: 'float16', tensorSize: %(size)s, tensorCrop: %(crop)s });
const got = [];
lp.on('frame', (f) => {
  const t = lp.readTensor(f.window, f.index);
  got.push({ gop: f.gop, di: f.displayIndex, sha: sha(t), n: t.length, kind: t.constructor.name });
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused, stats: lp.stats() })); lp.destroy(); });
"""


@pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
def test_read_resized_tensor_through_the_addon(gpu_parser):
    import leon_ctypes as L
    from test_pipeline_gpu import oracle_frames
    size, crop = (112, 160), (16, 8, 320, 224)
    T = L.tensor_table("float16").view(np.uint16)
    want = {}
    for k, v in oracle_frames(open(STREAM, "rb").read()).items():
        r = L.resize_rgb(v[..., :3], crop, size)
        want[k] = hashlib.sha256(np.stack([T[c][r[..., c]] for c in range(3)]).tobytes()).hexdigest()
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1" if gpu_parser else "-1", "size": json.dumps(list(size)),
                                                   "crop": json.dumps(list(crop))}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["refused"], "tensorSize without a tensor output must throw"
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want)
    s = r["stats"]
    assert (s["tensorHeight"], s["tensorWidth"], s["tensorFrameBytes"], s["frameWidth"], s["frameHeight"]) == (112, 160, 3 * 112 * 160 * 2, 352, 240)
    for f in r["got"]:
        assert f["kind"] == "Uint16Array" and f["n"] == 3 * 112 * 160
        assert f["sha"] == want[(f["gop"], f["di"])], f
