"""GPU, under Node: the frames' residual records through the real addon -- LeonPipeline.readResidual with opts.residual, equal to what the
Python binding reads of the same stream (tests/test_pipeline_residual_gpu.py run_residual) and to the oracle's residual; readResidual
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
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, gpuParser: %(gpu)s, residual: %(residual)s });
const got = [];
let refused = null;
lp.on('frame', (f) => {
  if (!%(residual)s) {
    if (refused === null) { try { lp.readResidual(f.window, f.index); refused = false; } catch (e) { refused = true; } }
    return;
  }
  const r = lp.readResidual(f.window, f.index);
  got.push({ gop: f.gop, di: f.displayIndex, y: Array.from(r.y), cb: Array.from(r.cb), cr: Array.from(r.cr),
    kinds: [r.y.constructor.name, r.cb.constructor.name, r.cr.constructor.name], size: [r.codedWidth, r.codedHeight] });
  if (refused === null) { try { lp.readResidual(f.window, 1000); refused = false; } catch (e) { refused = true; } }
});
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => { console.log(JSON.stringify({ got, refused, stats: lp.stats() })); lp.destroy(); });
"""


def _node(script):
    out = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
def test_read_residual_through_the_addon(gpu_parser):
    import leon_ctypes as L
    from test_pipeline_residual_gpu import expected_residual, run_residual
    data = open(STREAM, "rb").read()
    want, (cw, ch) = expected_residual(data)
    python, _ = run_residual(L, data, gops_per_window=1, gpu_parser=None if gpu_parser else False)
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1" if gpu_parser else "-1", "residual": "true"})
    assert sorted((f["gop"], f["di"]) for f in r["got"]) == sorted(want) == sorted(python)
    assert r["refused"] is True, "readResidual of a frame the window does not have must throw"
    assert r["stats"]["output"] == 1 | 512
    for f in r["got"]:
        key = (f["gop"], f["di"])
        assert f["kinds"] == ["Int16Array"] * 3 and f["size"] == [cw, ch]
        for name, py, w in zip(("y", "cb", "cr"), python[key], want[key]):
            assert f[name] == py.reshape(-1).tolist(), (key, name)
            assert np.array_equal(py, w), (key, name)


def test_read_residual_without_the_option_throws():
    r = _node(_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1", "residual": "false"})
    assert r["refused"] is True and r["stats"]["output"] == 1
