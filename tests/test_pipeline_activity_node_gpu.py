"""GPU, under Node: the frames' activity records through the real addon -- LeonPipeline.readActivity with opts.activity, equal to
leon_ctypes.activity_from_lists of the host front end's lists (tests/test_pipeline_activity_gpu.py expected_activity); readActivity
on a pipeline without the option throws."""
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
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: %(gpu)s, activity: %(activity)s });
const got = [];
let refused = null;
lp.on('frame', (f) => {
  if (!%(activity)s) {
    if (refused === null) { try { lp.readActivity(f.window, f.index); refused = false; } catch (e) { refused = true; } }
    return;
  }
  const a = lp.readActivity(f.window, f.index);
  got.push({ gop: f.gop, di: f.displayIndex, acCount: Array.from(a.acCount), acMag: Array.from(a.acMag), dcMag: Array.from(a.dcMag),
    blocks: Array.from(a.blocks), qscale: Array.from(a.qscale), summary: Array.from(a.summary),
    kinds: [a.acCount.constructor.name, a.blocks.constructor.name, a.summary.constructor.name], grid: [a.mbWidth, a.mbHeight] });
  if (refused === null) { try { lp.readActivity(f.window, 1000); refused = false; } catch (e) { refused = true; } }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused, stats: lp.stats() })); lp.destroy(); });
"""


def _node(script):
    out = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
def test_read_activity_through_the_addon(gpu_parser):
    from test_pipeline_activity_gpu import expected_activity
    want, (mbw, mbh), _ = expected_activity(open(STREAM, "rb").read())
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1" if gpu_parser else "-1", "activity": "true"})
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want)
    assert r["refused"] is True, "readActivity of a frame the window does not have must throw"
    assert r["stats"]["output"] == 1 | 128
    for f in r["got"]:
        cells, summary = want[(f["gop"], f["di"])]
        assert f["kinds"] == ["Uint16Array", "Uint8Array", "Uint32Array"] and f["grid"] == [mbw, mbh]
        for js, field in (("acCount", "ac_count"), ("acMag", "ac_mag"), ("dcMag", "dc_mag"), ("blocks", "blocks"), ("qscale", "qscale")):
            assert f[js] == cells[field].reshape(-1).tolist(), (f["gop"], f["di"], field)
        assert f["summary"] == summary.tolist()


def test_read_activity_without_the_option_throws():
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1", "activity": "false"})
    assert r["refused"] is True and r["stats"]["output"] == 1
