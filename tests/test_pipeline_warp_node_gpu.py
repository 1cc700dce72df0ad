"""GPU, under Node: warp regions through the real addon -- LeonPipeline.readWarpRegions(window, regions, {size, padValue}) returns a
Buffer of n * region bytes equal to the oracle's RGB bytes of each region's frame through leon_ctypes.warp_rgb and the element table,
for the 96 x 64 stream's (8, 32) call of tests/warp_structure.py; what the library refuses throws."""
import hashlib
import json
import shutil

import numpy as np
import pytest

import warp_structure as W
from resample_structure import STREAMS
from test_pipeline_regions_node_gpu import JSDIR, _node

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const data = fs.readFileSync(%(stream)r);
const regions = %(regions)s, size = %(size)s, bytes = %(bytes)d, padValue = %(pad)s;
const lp = new LeonPipeline(data, { backend, parserThreads: 2, gopsPerWindow: 2, gpuParser: 1, output: 'tensor', tensorDtype: 'float16', tensorLayout: 'hwc' });
const got = [], refused = [];
lp.on('frames', (window, frames) => {
  const b = lp.readWarpRegions(window, regions, { size, padValue });
  const shas = [];
  for (let i = 0; i < regions.length; i++) shas.push(crypto.createHash('sha256').update(b.subarray(i * bytes, (i + 1) * bytes)).digest('hex'));
  got.push({ keys: frames.map((f) => [f.gop, f.displayIndex]), n: b.length, isBuffer: Buffer.isBuffer(b), shas });
  const ident = [65536, 0, 0, 0, 65536, 0];
  for (const bad of [() => lp.readWarpRegions(window + 1000, regions, { size }), () => lp.readWarpRegions(window, [[frames.length, ident]], { size }),
                     () => lp.readWarpRegions(window, [[0, ident], [0, [5 * 65536, 0, 0, 0, 65536, 0]]], { size }),
                     () => lp.readWarpRegions(window, regions, { size, padValue: [0, 0, 256] }), () => lp.readWarpRegions(window, [[0, [1, 2, 3]]], { size }),
                     () => lp.readWarpRegions(window, regions, { size: [8] })]) {
    try { bad(); refused.push(false); } catch (e) { refused.push(String(e.message)); }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused })); lp.destroy(); });
"""


def test_read_warp_regions_through_the_addon(tmp_path):
    import leon_ctypes as L
    from test_pipeline_gpu import ibbp_stream, oracle_frames
    from test_pipeline_tensor_format_gpu import bits
    name, size = "96x64", (8, 32)
    cw, ch, gops, seed, frame = STREAMS[name]
    data = ibbp_stream(cw, ch, gops, seed=seed, frame=frame)
    rgba = oracle_frames(data)
    path = tmp_path / "s.jsv"
    path.write_bytes(data)
    regs = W.regions(frame, size, 9)
    nbytes = 3 * size[0] * size[1] * 2
    r = _node(_SCRIPT % {"js": JSDIR, "stream": str(path), "regions": json.dumps([[f, list(m)] for f, m in regs]), "size": json.dumps(list(size)), "bytes": nbytes,
                         "pad": json.dumps(list(W.PAD))})
    assert len(r["got"]) == 1
    g = r["got"][0]
    assert g["isBuffer"] and g["n"] == len(regs) * nbytes
    keys = [tuple(k) for k in g["keys"]]
    T = bits(L.tensor_table("float16"))
    for i, (f, m) in enumerate(regs):
        rgb = L.warp_rgb(rgba[keys[f]][..., :3], m, size, W.PAD)
        want = np.ascontiguousarray(np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1))
        assert g["shas"][i] == hashlib.sha256(want.tobytes()).hexdigest(), "region %d (%s)" % (i, W.matrices(frame, size)[i][0])
    assert all(r["refused"]), r["refused"]
    assert "not out for delivery" in r["refused"][0] and "region 0: frame 9" in r["refused"][1] and "region 1" in r["refused"][2] and "more than 4" in r["refused"][2]
    assert "pad value 2 is 256" in r["refused"][3] and "regions" in r["refused"][4] and "size" in r["refused"][5]
