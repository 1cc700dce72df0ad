"""GPU: the motion family at more than one trip of k_motion's loop, through the pipeline.  A stream of 656 x 400 is 41 x 25 = 1025
macroblocks: the loop's second trip, one lane of it holding one macroblock (mbs % 4 == 1), and rows of 41 -- the smallest grid that
takes the second trip (the other motion, carry and propagate tests decode 330 macroblocks at most).  One closed GOP of six pictures,
written once per module; per parser one run that, inside the window's callback, reads every record, carries boxes between every pair
of frames and propagates maps onto every frame.  The oracles are the ones of the tests beside this: motion_from_maps on the host
parser's maps, carry_box, propagate_map."""
import functools

import numpy as np
import pytest

import carry_cases as K
import propagate_cases as M
from test_pipeline_carry_gpu import refs_by_lookup
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import assert_motion, expected_motion
from test_pipeline_propagate_gpu import assert_window as assert_propagate_window
from test_pipeline_propagate_gpu import propagate_window

pytestmark = pytest.mark.gpu

FW, FH, MBW, MBH = 656, 400, 41, 25
FILL = -55
# the whole frame; macroblock columns 33 .. 40 and rows 20 .. 24 (the last one is macroblock 1024, the second trip's); a box inside
# one macroblock; one across the rows' ends
BOXES = [(0, 0, FW, FH), (33 * 16, 20 * 16, 8 * 16, 5 * 16), (5, 7, 12, 10), (600, 100, 56, 200)]
# (stride, element bytes, planes)
PROPAGATE_SHAPES = [(16, 4, 2), (1, 1, 1)]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@functools.lru_cache(maxsize=None)
def case():
    """(stream bytes, expected records by (gop, display index)): built once per process and left unchanged"""
    data = ibbp_stream(FW, FH, [6], 45)
    want, grid = expected_motion(data)
    assert grid == (MBW, MBH) and len(want) == 6
    return data, want


@functools.lru_cache(maxsize=None)
def delivered(gpu_parser):
    """one run of the pipeline: the window's records, its carried boxes and its propagated maps, as the library gave them"""
    import leon_ctypes as L
    data, _ = case()
    out = {}

    def on_window(window, frames):
        pipe = frames[0]["_pipe"]
        frames = list(frames)
        n = len(frames)
        out["layout"] = pipe.motion_layout
        out["motion"] = {(f["gop"], f["display_index"]): pipe.read_motion(window, f["_i"]) + (f["motion"]["fwd_gop"], f["motion"]["fwd_display"], f["motion"]["bwd_display"])
                         for f in frames}
        out["records"] = [pipe.read_motion(window, i)[:2] for i in range(n)]
        fwd, bwd = pipe.carry_refs(window)
        out["refs"] = (fwd.tolist(), bwd.tolist())
        out["lookup"] = refs_by_lookup(frames)
        out["regions"] = [(s, x, y, w, h, t) for s in range(n) for t in range(n) for (x, y, w, h) in BOXES]
        out["carry"] = pipe.carry_regions(window, out["regions"], fill=FILL)
        out["propagate"] = propagate_window(L, pipe, window, frames, roads=("host",), shapes=PROPAGATE_SHAPES)
    pipe = L.Pipeline(data, on_window=on_window, motion=True, gops_per_window=1, gpu_parser=gpu_parser, parser_threads=2)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return out


PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])


@PARSERS
def test_records_equal_the_definition(L, gpu_parser):
    _, want = case()
    assert any((v[1] == 1).any() for v in want.values()) and any((v[1] == 2).any() for v in want.values()) and any((v[1] == 3).any() for v in want.values())
    # the premise: the second trip's macroblock, 1024, is one whose record is not all zero in some picture
    assert any(v[0].reshape(-1, 4)[1024].any() for v in want.values())
    got = delivered(gpu_parser)
    assert (got["layout"].mb_width, got["layout"].mb_height, got["layout"].mbs) == (MBW, MBH, 1025)
    assert_motion(got["motion"], want, "656 x 400")


@PARSERS
def test_carry_regions_equal_carry_box(L, gpu_parser):
    got = delivered(gpu_parser)
    assert got["refs"] == got["lookup"]
    fwd, bwd = got["refs"]
    want = K.expected(L, FW, FH, got["records"], got["regions"], FILL, fwd, bwd, len(got["records"]))
    K.assert_equal(got["carry"], want, got["regions"], "656 x 400")
    status, votes = want[2], want[1]
    assert (status == 0).any() and (votes[status == 0][:, 2:] != 0).any(), "no box of the window moved"
    far = [i for i, r in enumerate(got["regions"]) if r[1:5] == BOXES[1] and status[i] == 0 and r[0] != r[5]]
    assert far and (votes[far][:, 0] > 0).any()          # the box over macroblock 1024 is carried by records that vote


@PARSERS
def test_propagate_maps_equal_propagate_map(L, gpu_parser):
    got = delivered(gpu_parser)
    r = got["propagate"]
    assert [run["shape"] for run in r["runs"]] == PROPAGATE_SHAPES
    assert_propagate_window(L, r, "656 x 400")
    assert {0, 1, 2} <= set(np.unique(r["runs"][1]["want"][1]).tolist())
