"""GPU, under Node: boxes gauged against the motion and activity records through the real addon -- LeonPipeline.gaugeRegions(window,
regions, {sources}) with opts.motion and opts.activity, equal word for word to the Python host road (Pipeline.gauge_regions) of the
same stream, whose results tests/test_pipeline_gauge_gpu.py pins to gauge_box; a record's fault is a status word, a call's a throw."""
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
BOXES = [(0, 0, 90, 60), (32, 16, 48, 32), (89, 59, 1, 1), (5, 7, 12, 10), (15, 15, 2, 2)]          # the stream's frame is 90 x 60 in a 96 x 64 grid

_SCRIPT = r"""
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, motion: true, activity: true });
const boxes = %(boxes)s;
const got = {};
let threw = 0;
lp.on('frames', (window, frames) => {
  const n = frames.length, regions = [];
  for (let f = 0; f < n; f++) for (const b of boxes) regions.push([f, b[0], b[1], b[2], b[3]]);
  regions.push([n, 0, 0, 8, 8], [0, 0, 0, 0, 8]);
  got[window] = { n, by: {} };
  for (const sources of [undefined, 1, 2, 3]) {
    const r = lp.gaugeRegions(window, regions, sources === undefined ? {} : { sources });
    got[window].by[String(sources)] = { stats: Array.from(r.stats), status: Array.from(r.status), kinds: [r.stats.constructor.name, r.status.constructor.name],
      safe: Array.from(r.stats).every(Number.isSafeInteger) };
  }
  for (const bad of [() => lp.gaugeRegions(window + 1000, regions), () => lp.gaugeRegions(window, []), () => lp.gaugeRegions(window, [[0, 0, 0, 8, 8, 0]]),
                     () => lp.gaugeRegions(window, [[0, 0, 0, 8, 0.5]]), () => lp.gaugeRegions(window, regions, { sources: 0 }),
                     () => lp.gaugeRegions(window, regions, { sources: 4 }), () => lp.gaugeRegions(window, regions, { sources: 'motion' })]) {
    try { bad(); } catch (e) { threw++; }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, threw })); lp.destroy(); });
"""


def test_gauge_regions_through_the_addon():
    import leon_ctypes as L
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "boxes": json.dumps(BOXES)}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    want = {}

    def on_window(window, frames):
        n = len(frames)
        regions = [(f, *b) for f in range(n) for b in BOXES] + [(n, 0, 0, 8, 8), (0, 0, 0, 0, 8)]
        want[window] = (n, {str(s): frames[0]["_pipe"].gauge_regions(window, regions, sources=s) for s in (1, 2, 3)})
    pipe = L.Pipeline(open(STREAM, "rb").read(), on_window=on_window, motion=True, activity=True, gops_per_window=1, gpu_parser=True, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert sorted(int(w) for w in r["got"]) == sorted(want) and want
    for w, (n, by) in want.items():
        g = r["got"][str(w)]
        assert g["n"] == n
        for s, (stats, status) in by.items():
            for key in ([s, "undefined"] if s == "3" else [s]):
                b = g["by"][key]
                assert b["kinds"] == ["Float64Array", "Int32Array"] and b["safe"]
                assert np.array_equal(np.array(b["status"]), status) and status[-2:].tolist() == [L.REGION_FRAME, L.REGION_BOX] and (status[:-2] == 0).all()
                assert np.array_equal(np.array(b["stats"], dtype=np.int64).reshape(-1, 16), stats)
            assert (stats[:-2, 1:] != 0).any() and (stats[-2:] == 0).all()
    assert r["threw"] == 7 * len(want)
