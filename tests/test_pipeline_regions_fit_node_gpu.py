"""GPU, under Node: letterboxed regions through the real addon -- LeonPipeline.readRegions(window, regions, {size, filter, fit, anchor,
padValue}) returns the bytes of Pipeline.read_regions with the same keywords (which tests/test_pipeline_regions_fit_gpu.py pins to the
oracle) for the 96 x 64 call of tests/fitted_structure.py; without the keywords it is the stretched call; what the library refuses of
the fit throws."""
import hashlib
import json
import shutil

import numpy as np
import pytest

from fitted_structure import CALLS
from regions_structure import BICUBIC
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_regions_node_gpu import JSDIR, _node

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

PAD = (114, 7, 250)
_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const data = fs.readFileSync(%(stream)r);
const regions = %(regions)s, size = %(size)s, padValue = %(pad)s;
const lp = new LeonPipeline(data, { backend, parserThreads: 2, gopsPerWindow: 2, gpuParser: 1, output: 'tensor', tensorDtype: 'float16', tensorLayout: 'hwc' });
const sha = (b) => crypto.createHash('sha256').update(b).digest('hex');
const got = [], refused = [];
lp.on('frames', (window, frames) => {
  const calls = { centre: { fit: 'letterbox', padValue }, top_left: { fit: 'letterbox', anchor: 'top_left', padValue }, stretch: { fit: 'stretch' }, plain: {} };
  const out = { keys: frames.map((f) => [f.gop, f.displayIndex]) };
  for (const k of Object.keys(calls)) {
    const b = lp.readRegions(window, regions, Object.assign({ size, filter: %(filter)r }, calls[k]));
    out[k] = { n: b.length, sha: sha(b) };
  }
  got.push(out);
  for (const bad of [{ fit: 'letterbox', padValue: [0, 256, 0] }, { fit: 'letterbox', anchor: 2 }, { fit: 2 }, { anchor: 'top_left' }, { fit: 'fill' }, { fit: 'letterbox', padValue: [1, 2] }]) {
    try { lp.readRegions(window, regions, Object.assign({ size }, bad)); refused.push(false); } catch (e) { refused.push(String(e.message)); }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused })); lp.destroy(); });
"""


def test_read_regions_with_a_fit_through_the_addon(tmp_path):
    import leon_ctypes as L
    from test_pipeline_gpu import ibbp_stream
    from test_pipeline_regions_gpu import run
    name, filt = "96x64", BICUBIC
    call = CALLS[name]
    cw, ch, gops, seed, frame = STREAMS[name]
    data = ibbp_stream(cw, ch, gops, seed=seed, frame=frame)
    path = tmp_path / "s.jsv"
    path.write_bytes(data)
    regs = call.regions(9)
    r = _node(_SCRIPT % {"js": JSDIR, "stream": str(path), "regions": json.dumps([list(x) for x in regs]), "size": json.dumps(list(call.size)),
                         "pad": json.dumps(list(PAD)), "filter": FILTER_NAMES[filt]})
    assert len(r["got"]) == 1
    g = r["got"][0]
    want = {}

    def on_frames(p, window, keys, frames):
        assert [list(k) for k in keys] == g["keys"]
        want["centre"] = p.read_regions(window, regs, call.size, filt, fit="letterbox", pad_value=PAD)
        want["top_left"] = p.read_regions(window, regs, call.size, filt, fit="letterbox", anchor="top_left", pad_value=PAD)
        want["stretch"] = want["plain"] = p.read_regions(window, regs, call.size, filt)
    run(L, data, "float16", "hwc", on_frames).close()
    for k, v in want.items():
        b = np.ascontiguousarray(v).tobytes()
        assert g[k]["n"] == len(b) and g[k]["sha"] == hashlib.sha256(b).hexdigest(), k
    assert len({g[k]["sha"] for k in ("centre", "top_left", "plain")}) == 3
    assert all(r["refused"]), r["refused"]
    assert "pad value 1 is 256" in r["refused"][0] and "anchor 2" in r["refused"][1] and "mode 2" in r["refused"][2] and "LEON_REGIONS_FIT_STRETCH" in r["refused"][3]
    assert "fit" in r["refused"][4] and "padValue" in r["refused"][5]
