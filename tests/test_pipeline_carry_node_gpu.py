"""GPU, under Node: boxes carried along the motion vectors through the real addon -- LeonPipeline.carryRegions(window, records) with
opts.motion, equal word for word to the Python host road (Pipeline.carry_regions) of the same stream, whose results
tests/test_pipeline_carry_gpu.py pins to carry_box; a record's fault is a status word, a call's a throw."""
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
BOXES = [(0, 0, 96, 64), (32, 16, 48, 32), (95, 63, 1, 1), (5, 7, 12, 10)]

_SCRIPT = r"""
const path = require('path'), fs = require('fs');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: 1, motion: true });
const boxes = %(boxes)s;
const got = {};
let threw = 0;
lp.on('frames', (window, frames) => {
  const n = frames.length, records = [];
  for (let s = 0; s < n; s++) for (let t = 0; t < n; t++) for (const b of boxes) records.push([s, b[0], b[1], b[2], b[3], t]);
  records.push([n, 0, 0, 8, 8, 0], [0, 0, 0, 0, 8, 0]);
  const r = lp.carryRegions(window, records);
  got[window] = { n, out: Array.from(r.out), votes: Array.from(r.votes), status: Array.from(r.status),
    kinds: [r.out.constructor.name, r.votes.constructor.name, r.status.constructor.name] };
  for (const bad of [() => lp.carryRegions(window + 1000, records), () => lp.carryRegions(window, []), () => lp.carryRegions(window, [[0, 0, 0, 8, 8]]),
                     () => lp.carryRegions(window, [[0, 0, 0, 8, 8, 0.5]])]) {
    try { bad(); } catch (e) { threw++; }
  }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, threw })); lp.destroy(); });
"""


def test_carry_regions_through_the_addon():
    import leon_ctypes as L
    out = subprocess.run(["node", "-e", _SCRIPT % {"js": JSDIR, "stream": STREAM, "boxes": json.dumps(BOXES)}], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    want = {}

    def on_window(window, frames):
        n = len(frames)
        records = [(s, *b, t) for s in range(n) for t in range(n) for b in BOXES] + [(n, 0, 0, 8, 8, 0), (0, 0, 0, 0, 8, 0)]
        want[window] = (n,) + frames[0]["_pipe"].carry_regions(window, records)
    pipe = L.Pipeline(open(STREAM, "rb").read(), on_window=on_window, motion=True, gops_per_window=1, gpu_parser=True, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert sorted(int(w) for w in r["got"]) == sorted(want) and want
    for w, (n, out_, votes, status) in want.items():
        g = r["got"][str(w)]
        assert g["n"] == n and g["kinds"] == ["Int32Array"] * 3
        assert np.array_equal(np.array(g["status"]), status) and status[-2:].tolist() == [L.REGION_FRAME, L.REGION_BOX] and (status == 0).any()
        assert np.array_equal(np.array(g["out"]).reshape(-1, 8), out_) and np.array_equal(np.array(g["votes"]).reshape(-1, 4), votes)
        assert (votes[:, 2:] != 0).any()
    assert r["threw"] == 4 * len(want)
