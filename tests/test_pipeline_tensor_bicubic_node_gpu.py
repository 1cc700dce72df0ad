"""GPU, under Node: the bicubic filter through the real addon -- LeonPipeline with tensorFilter: 'bicubic', readTensor equal to the
Python expectation (the table T looked up with leon_ctypes.resize_rgb(filter=3) of the oracle's RGBA), written to a file for the script."""
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
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const want = JSON.parse(fs.readFileSync(%(index)r)), blob = fs.readFileSync(%(blob)r);
const stream = fs.readFileSync(%(stream)r);
let refused = 0;
for (const bad of [{ output: 'tensor', tensorSize: [40, 40], tensorFilter: 'lanczos' }, { output: 'tensor', tensorSize: [40, 40], tensorFilter: 2 },
                   { output: 'rgba', tensorFilter: 'bicubic' }]) {
  try { new LeonPipeline(stream, Object.assign({ backend }, bad)); } catch (e) { refused++; }
}
const lp = new LeonPipeline(stream, { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, output: 'tensor', tensorDtype: 'float16',
  tensorSize: [40, 40], tensorFilter: 'bicubic' });
const got = [];
lp.on('frame', (f) => {
  const t = lp.readTensor(f.window, f.index), at = want[f.gop + ',' + f.displayIndex];
  const bytes = Buffer.from(t.buffer, t.byteOffset, t.byteLength);
  got.push({ gop: f.gop, di: f.displayIndex, n: t.length, kind: t.constructor.name,
             equal: at !== undefined && bytes.equals(blob.subarray(at, at + bytes.length)) });
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused, stats: lp.stats() })); lp.destroy(); });
"""


def test_read_bicubic_tensor_through_the_addon(tmp_path):
    import leon_ctypes as L
    from test_pipeline_gpu import oracle_frames
    size = (40, 40)
    T = L.tensor_table("float16").view(np.uint16)
    index, blob = {}, b""
    want = oracle_frames(open(STREAM, "rb").read())
    for (gop, di), v in want.items():
        r = L.resize_rgb(v[..., :3], None, size, filter=L.RESIZE_BICUBIC)
        index["%d,%d" % (gop, di)] = len(blob)
        blob += np.stack([T[c][r[..., c]] for c in range(3)]).tobytes()
    (tmp_path / "want.json").write_text(json.dumps(index))
    (tmp_path / "want.bin").write_bytes(blob)
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "index": str(tmp_path / "want.json"), "blob": str(tmp_path / "want.bin")}],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["refused"] == 3, "an unknown filter name, filter 2 and a filter without a tensor output must throw"
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want)
    assert (r["stats"]["tensorHeight"], r["stats"]["tensorWidth"]) == size
    for f in r["got"]:
        assert f["kind"] == "Uint16Array" and f["n"] == 3 * 40 * 40
        assert f["equal"], f
