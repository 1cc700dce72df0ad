"""GPU, under Node: regions of delivered frames through the real addon -- LeonPipeline.readRegions(window, regions, {size, filter})
returns a Buffer of n * region bytes equal to the oracle's RGB bytes of each region's frame through leon_ctypes.resize_rgb and the
element table, for the 96 x 64 call of tests/regions_structure.py; what the library refuses throws."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from regions_structure import BICUBIC, CALLS, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

JSDIR = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "js")

_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const data = fs.readFileSync(%(stream)r);
const regions = %(regions)s, size = %(size)s, bytes = %(bytes)d;
const lp = new LeonPipeline(data, { backend, parserThreads: 2, gopsPerWindow: 2, gpuParser: 1, output: 'tensor', tensorDtype: %(dtype)r, tensorLayout: %(layout)r,
  tensorLetterbox: [40, 40] });
const got = [], refused = [];
lp.on('frames', (window, frames) => {
  const b = lp.readRegions(window, regions, { size, filter: %(filter)r });
  const shas = [];
  for (let i = 0; i < regions.length; i++) shas.push(crypto.createHash('sha256').update(b.subarray(i * bytes, (i + 1) * bytes)).digest('hex'));
  got.push({ keys: frames.map((f) => [f.gop, f.displayIndex]), n: b.length, isBuffer: Buffer.isBuffer(b), shas });
  for (const bad of [() => lp.readRegions(window + 1000, regions, { size }), () => lp.readRegions(window, [[frames.length, 0, 0, 8, 8]], { size }),
                     () => lp.readRegions(window, [[0, 0, 0, 96, 64]], { size: [3, 5] }), () => lp.readRegions(window, regions, { size, filter: 2 }),
                     () => lp.readRegions(window, [[0, 0, 0, 8]], { size }), () => lp.readRegions(window, regions, { size: [8] })]) {
    try { bad(); refused.push(false); } catch (e) { refused.push(String(e.message)); }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused })); lp.destroy(); });
"""


def _node(script):
    out = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("dtype,layout,filt", [("uint8", "hwc", TRIANGLE), ("float16", "chw", BICUBIC)])
def test_read_regions_through_the_addon(tmp_path, dtype, layout, filt):
    import leon_ctypes as L
    from test_pipeline_gpu import ibbp_stream, oracle_frames
    from test_pipeline_tensor_format_gpu import bits
    call = CALLS["96x64"]
    cw, ch, gops, seed, frame = STREAMS["96x64"]
    data = ibbp_stream(cw, ch, gops, seed=seed, frame=frame)
    rgba = oracle_frames(data)
    path = tmp_path / "s.jsv"
    path.write_bytes(data)
    regs = call.regions(9)
    e = 1 if dtype == "uint8" else 2
    nbytes = 3 * call.size[0] * call.size[1] * e
    r = _node(_SCRIPT % {"js": JSDIR, "stream": str(path), "regions": json.dumps([list(x) for x in regs]), "size": json.dumps(list(call.size)), "bytes": nbytes,
                         "dtype": dtype, "layout": layout, "filter": FILTER_NAMES[filt]})
    assert len(r["got"]) == 1
    g = r["got"][0]
    keys = [tuple(k) for k in g["keys"]]
    assert sorted(keys) == sorted(rgba) and g["isBuffer"] and g["n"] == len(regs) * nbytes
    T = bits(L.tensor_table(dtype))
    for i, reg in enumerate(regs):
        rgb = L.resize_rgb(rgba[keys[reg[0]]][..., :3], tuple(reg[1:]), call.size, filt)
        hwc = np.stack([T[c][rgb[..., c]] for c in range(3)], axis=-1)
        want = np.ascontiguousarray(hwc if layout == "hwc" else hwc.transpose(2, 0, 1))
        assert g["shas"][i] == hashlib.sha256(want.tobytes()).hexdigest(), "region %d %s" % (i, reg)
    # a window not out for delivery, a frame outside the window, a ratio above 16, another filter: the library refuses and names the region;
    # a box of four numbers, a size of one: the binding does
    assert all(r["refused"]), r["refused"]
    assert "not out for delivery" in r["refused"][0] and "region 0: frame 9" in r["refused"][1] and "reduces by more than 16" in r["refused"][2]
    assert "filter 2" in r["refused"][3] and "regions" in r["refused"][4] and "size" in r["refused"][5]
