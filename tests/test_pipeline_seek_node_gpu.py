"""GPU, under Node: LeonPipeline.seek through the real addon gives the oracle's frames (stale windows and the old
position's 'ended' never reach JavaScript), and LeonPlayer over the pipeline seeks the pipeline it has instead of
destroying it and creating another -- with accurateSeek from the frame on screen at the new time."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]

JSDIR = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "js")
STREAM = os.path.join(ROOT, "tests", "golden", "streams", "leon_synth_352x240.jsv")      # 2 GOPs of 12, 25 pictures/s

_PIPE_SCRIPT = r"""
const path = require('path'), fs = require('fs'), crypto = require('crypto');
const { LeonPipeline } = require(path.join(%(js)r, 'leon_pipeline.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const lp = new LeonPipeline(fs.readFileSync(%(stream)r), { backend, parserThreads: 2, gopsPerWindow: 1, windowsInFlight: 2, gpuParser: %(gpu)s });
const runs = [[]], seeked = [], firsts = [];
let ended = 0;
lp.on('frame', (f) => {      // by window id: the rest of a window delivered before a seek still belongs to its run
  runs[firsts.filter((x) => f.window >= x).length].push({ gop: f.gop, di: f.displayIndex, ts: f.ts, w: f.window,
                               sha: crypto.createHash('sha256').update(lp.readFrame(f.window, f.index)).digest('hex') });
  if (runs.length === 1 && runs[0].length === 3) { runs.push([]); firsts.push(lp.seek(0.6)); }      // while windows are in flight
});
lp.on('seeked', (f) => seeked.push({ gop: f.gop, di: f.displayIndex }));
lp.on('error', (e) => { console.error(String(e)); process.exit(3); });
lp.on('ended', () => {
  ended++;
  if (runs.length === 2) { runs.push([]); firsts.push(lp.seek(0.7, { exact: true })); return; }
  console.log(JSON.stringify({ runs, seeked, firsts, ended }));
  lp.destroy();
});
"""

_PLAYER_SCRIPT = r"""
const path = require('path'), crypto = require('crypto');
const { LeonPlayer } = require(path.join(%(js)r, 'leon_player.js'));
const backend = require(path.join(%(js)r, '..', 'napi', 'leon_napi.node'));
const ev = [], shown = [];
const p = new LeonPlayer({ backend, pipeline: true, realtime: false, parserThreads: 2, gpuParser: %(gpu)s, accurateSeek: %(accurate)s,
  render: (rgba, f) => shown.push({ gop: f.gop, di: f.displayIndex, ts: f.ts, sha: crypto.createHash('sha256').update(rgba).digest('hex') }) });
for (const e of ['loadedmetadata', 'seeking', 'seeked', 'ended', 'error']) p.on(e, () => ev.push(e));
let pipe0 = null, destroyed = 0, cut = -1, same = null;
p.on('loadedmetadata', () => {
  pipe0 = p._pipe;
  const d = pipe0.destroy.bind(pipe0);
  pipe0.destroy = () => { destroyed++; d(); };
});
p.on('ended', () => {
  if (cut < 0) { cut = shown.length; p.currentTime = %(seek)s; same = p._pipe === pipe0; p.play(); return; }
  console.log(JSON.stringify({ ev, shown, cut, same, after: p._pipe === pipe0, destroyed }));
  p.destroy();
});
p.src = %(stream)r;
p.play();
"""


def _node(script):
    out = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def want():
    from test_pipeline_gpu import oracle_frames
    return {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in oracle_frames(open(STREAM, "rb").read()).items()}


@pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
def test_leon_pipeline_seek_through_the_addon(want, gpu_parser):
    r = _node(_PIPE_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "1" if gpu_parser else "-1"})
    run0, run1, run2 = r["runs"]
    assert r["ended"] == 2, "the first position was seeked away from: only the two later runs end"
    first1, first2 = r["firsts"]
    assert all(f["w"] < first1 for f in run0) and all(f["w"] >= first1 for f in run1) and all(f["w"] >= first2 for f in run2)
    assert [(f["gop"], f["di"]) for f in run1] == [(1, d) for d in range(12)]          # 0.6 s: the second GOP's key entry
    # EXACT at 0.7 s: the frame on screen is the one with the largest ts <= 700 ms
    assert run2[0]["ts"] <= 700.0 < run2[1]["ts"] and [(f["gop"], f["di"]) for f in run2] == [(1, d) for d in range(run2[0]["di"], 12)]
    assert r["seeked"] == [{"gop": 1, "di": 0}, {"gop": 1, "di": run2[0]["di"]}]
    for f in run0 + run1 + run2:
        assert f["sha"] == want[(f["gop"], f["di"])], f


@pytest.mark.parametrize("gpu_parser,accurate", [(False, False), (True, False), (True, True)], ids=["host-parser", "gpu-parser", "accurate"])
def test_player_seeks_the_pipeline_it_has(want, gpu_parser, accurate):
    r = _node(_PLAYER_SCRIPT % {"js": JSDIR, "stream": STREAM, "gpu": "true" if gpu_parser else "false",
                                "accurate": "true" if accurate else "false", "seek": "0.7"})
    assert r["same"] and r["after"] and r["destroyed"] == 0, "currentTime= replaced the native pipeline"
    assert "error" not in r["ev"] and r["ev"].count("ended") == 2
    assert r["ev"].index("seeking") < r["ev"].index("seeked") < len(r["ev"]) - 1
    first, second = r["shown"][:r["cut"]], r["shown"][r["cut"]:]
    assert [(s["gop"], s["di"]) for s in first] == [(g, d) for g in range(2) for d in range(12)]
    if accurate:
        assert second[0]["ts"] <= 700.0 < second[1]["ts"] and second[0]["gop"] == 1
        assert [(s["gop"], s["di"]) for s in second] == [(1, d) for d in range(second[0]["di"], 12)]
    else:
        assert [(s["gop"], s["di"]) for s in second] == [(1, d) for d in range(12)]
    for s in r["shown"]:
        assert s["sha"] == want[(s["gop"], s["di"])], s
