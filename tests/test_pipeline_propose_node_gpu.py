"""GPU, under Node: boxes proposed from the motion and activity records through the real addon -- LeonPipeline.proposeRegions(window,
frames, {...}) with opts.motion and opts.activity, equal word for word to the Python host road (Pipeline.propose_regions) of the same
stream, whose results tests/test_pipeline_propose_gpu.py pins to propose_boxes; a request's fault is a status word, a call's a throw."""
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
# (the addon's options, the Python keywords)
CALLS = [({"mvMin": 1, "acMin": 40}, dict(mv_min=1, ac_min=40)),
         ({"mvMin": 2, "acMin": 200, "connectivity": 4, "maxBoxes": 3, "minCells": 2}, dict(mv_min=2, ac_min=200, connectivity=4, max_boxes=3, min_cells=2)),
         ({"sources": 1, "mvMin": 1, "intra": True}, dict(sources=1, mv_min=1, intra=True)),
         ({"sources": 2, "acMin": 1, "maxBoxes": 1}, dict(sources=2, ac_min=1, max_boxes=1))]

_SCRIPT = r"""
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, motion: true, activity: true });
const calls = %(calls)s;
const got = {};
let threw = 0;
lp.on('frames', (window, frames) => {
  const n = frames.length, requests = [];
  for (let f = 0; f < n; f++) requests.push(f);
  requests.push(n, 0, -1);
  got[window] = { n, by: [] };
  for (const opts of calls) {
    const r = lp.proposeRegions(window, requests, opts);
    got[window].by.push({ regions: Array.from(r.regions), count: Array.from(r.count), info: Array.from(r.info), status: Array.from(r.status),
      kinds: [r.regions, r.count, r.info, r.status].map((a) => a.constructor.name) });
  }
  for (const bad of [() => lp.proposeRegions(window + 1000, requests, calls[0]), () => lp.proposeRegions(window, [], calls[0]), () => lp.proposeRegions(window, [0.5], calls[0]),
                     () => lp.proposeRegions(window, requests, {}), () => lp.proposeRegions(window, requests, { mvMin: 1 }),
                     () => lp.proposeRegions(window, requests, { sources: 0 }), () => lp.proposeRegions(window, requests, { mvMin: 1, acMin: 1, connectivity: 6 }),
                     () => lp.proposeRegions(window, requests, { mvMin: 1, acMin: 1, maxBoxes: 1025 }), () => lp.proposeRegions(window, requests, { sources: 2, acMin: 1, intra: true })]) {
    try { bad(); } catch (e) { threw++; }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, threw })); lp.destroy(); });
"""


def test_propose_regions_through_the_addon():
    import leon_ctypes as L
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "calls": json.dumps([c for c, _ in CALLS])}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    want = {}

    def on_window(window, frames):
        n = len(frames)
        want[window] = (n, [frames[0]["_pipe"].propose_regions(window, list(range(n)) + [n, 0, -1], fill=0, **kw) for _, kw in CALLS])
    pipe = L.Pipeline(open(STREAM, "rb").read(), on_window=on_window, motion=True, activity=True, gops_per_window=1, gpu_parser=True, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert sorted(int(w) for w in r["got"]) == sorted(want) and want
    boxes = 0
    for w, (n, by) in want.items():
        g = r["got"][str(w)]
        assert g["n"] == n
        for b, (regions, count, info, status) in zip(g["by"], by):
            assert b["kinds"] == ["Int32Array"] * 4
            assert status.tolist() == [0] * n + [L.REGION_FRAME, 0, L.REGION_FRAME] and np.array_equal(np.array(b["status"]), status)
            assert np.array_equal(np.array(b["count"]), count) and np.array_equal(np.array(b["regions"]).reshape(regions.shape), regions)
            assert np.array_equal(np.array(b["info"]).reshape(info.shape), info)
            boxes += int(count[:n].sum())
    assert boxes > 0 and r["threw"] == 9 * len(want)
