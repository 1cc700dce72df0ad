"""GPU, under Node: the padded canvas through the real addon -- LeonPipeline.readTensor with tensorLetterbox returns the canvas, equal
to the oracle's RGB bytes through leon_ctypes.resize_rgb pasted into an array of the pad value; stats() reports the canvas's size and
the image rectangle; tensorCanvas / tensorOrigin / tensorPadValue give the same tensors as tensorLetterbox."""
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
PAD = (114, 7, 250)

_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.byteLength)).digest('hex');
const data = fs.readFileSync(%(stream)r);
const refused = [];
for (const bad of [{ tensorCanvas: [40, 40] }, { tensorSize: [27, 40], tensorCanvas: [40, 40], tensorPadValue: [0, 256, 0] }, { tensorSize: [27, 40], tensorCanvas: [40, 39] },
                   { tensorSize: [27, 40], tensorLetterbox: [40, 40] }, { tensorLetterbox: [40] }]) {
  try { new LeonPipeline(data, Object.assign({ backend, output: 'tensor' }, bad)).destroy(); refused.push(false); } catch (e) { refused.push(String(e.message)); }
}
const lp = new LeonPipeline(data, Object.assign({ backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, output: 'tensor',
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
@pytest.mark.parametrize("how", ["letterbox", "canvas"])
def test_read_canvas_tensor_through_the_addon(how, layout):
    import leon_ctypes as L
    from test_pipeline_gpu import oracle_frames
    (oh, ow), (x, y), (ch, cw) = (27, 40), (0, 6), (40, 40)
    assert L.letterbox(96, 64, cw, ch) == (ow, oh, x, y)
    want = {}
    for k, v in oracle_frames(open(STREAM, "rb").read()).items():
        hwc = np.empty((ch, cw, 3), dtype=np.uint8)
        hwc[:] = np.asarray(PAD, dtype=np.uint8)
        hwc[y:y + oh, x:x + ow] = L.resize_rgb(v[..., :3], None, (oh, ow))
        want[k] = hashlib.sha256(np.ascontiguousarray(hwc if layout == "hwc" else hwc.transpose(2, 0, 1)).tobytes()).hexdigest()
    extra = {"tensorLetterbox": [ch, cw], "tensorPadValue": list(PAD)} if how == "letterbox" else \
            {"tensorSize": [oh, ow], "tensorCanvas": [ch, cw], "tensorPadValue": list(PAD)}          # (origin: centred)
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "layout": layout, "extra": json.dumps(extra)})
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want)
    s = r["stats"]
    assert (s["output"], s["tensorDtype"], s["tensorElementBytes"], s["tensorLayout"]) == (16, L.TENSOR_U8, 1, layout)
    assert (s["tensorHeight"], s["tensorWidth"], s["tensorFrameBytes"]) == (ch, cw, 3 * ch * cw)
    assert (s["tensorImageX"], s["tensorImageY"], s["tensorImageWidth"], s["tensorImageHeight"]) == (x, y, ow, oh)
    for f in r["got"]:
        assert f["kind"] == "Uint8Array" and f["n"] == 3 * ch * cw
        assert f["sha"] == want[(f["gop"], f["di"])], f
    # a canvas without tensorSize, a pad value of 256, an image that leaves the canvas: the library refuses, naming the field;
    # tensorLetterbox beside tensorSize and a tensorLetterbox of one number: the binding does
    assert all(r["refused"]), r["refused"]
    assert "out_width" in r["refused"][0] and "pad[1]" in r["refused"][1] and "width" in r["refused"][2] and "tensorLetterbox" in r["refused"][3]
