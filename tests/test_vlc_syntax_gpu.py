"""GPU: the streams of tools/syntax_streams.py (the whole slice-layer syntax, see tests/test_vlc_syntax.py) through the
pipeline with the GPU slice-layer parser (csrc/leon_vlc_gpu.h) and with the host parser.  The expected frames come from
the oracle run on the tensors that were handed to the WRITER (helpers.oracle_frames_from_tensors) -- no parser of this
repository is in the loop, so a mistake the host parser and its GPU port share does not cancel out.  Planes and RGBA are
both compared: the colour conversion must not be what hides a chroma sample that is off by one."""
import threading

import numpy as np
import pytest

from helpers import oracle_frames_from_tensors

import syntax_streams as X
from test_vlc_syntax import NAMES, case

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])
_want = {}


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def want_of(name):
    """the tensor oracle's frames of a case, computed once and left unchanged"""
    if name not in _want:
        cw, ch = X.CASES[name]["size"]
        _want[name] = oracle_frames_from_tensors(case(name)[0], cw, ch)
    return _want[name]


def run_all_outputs(L, data, **kw):
    planes, rgba, lock = {}, {}, threading.Lock()

    def on_window(window, frames):
        with lock:
            for f in frames:
                k = (f["gop"], f["display_index"])
                planes[k] = f["_pipe"].read_planes(f)
                rgba[k] = L.read_frame(f)
    pipe = L.Pipeline(data, on_window=on_window, output="all", **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return planes, rgba


def assert_frames_are_the_tensor_oracles(planes, rgba, want, what, loops=1):
    assert set(planes) == set(rgba) == {(g + l, d) for (g, d) in want for l in range(loops)}, what
    for (g, d), w in sorted(want.items()):
        for l in range(loops):                                  # one GOP per stream: a loop continues the GOP numbering
            k = (g + l, d)
            assert len(planes[k]) == len(w["planes"]), (what, k)
            for pname, have, exp in zip(("Y", "Cb", "Cr", "A"), planes[k], w["planes"]):
                assert have.shape == exp.shape, (what, k, pname, have.shape, exp.shape)
                bad = np.argwhere(have != exp)
                assert bad.size == 0, "%s frame %s: plane %s differs from the oracle on the written tensors in %d samples, first (row, col) %s: %d, want %d" % (
                    what, k, pname, len(bad), bad[0].tolist(), have[tuple(bad[0])], exp[tuple(bad[0])])
            assert np.array_equal(rgba[k], w["rgba"]), "%s frame %s: RGBA differs although the planes agree" % (what, k)


@PARSERS
@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_pipeline_decodes_what_was_written(L, name, window, gpu_parser):
    pics, data, _ = case(name)
    extra = {}
    if name == "f3_f5_stuffed" and window == 2:
        extra["loop"] = 2
    if name == "per_picture" and window == 1:
        extra["windows_in_flight"] = 1
    planes, rgba = run_all_outputs(L, data, parser_threads=2, gops_per_window=window, gpu_parser=gpu_parser, **extra)
    assert_frames_are_the_tensor_oracles(planes, rgba, want_of(name), "%s, %s" % (name, "GPU parser" if gpu_parser else "host parser"),
                                         loops=extra.get("loop", 1))


def test_long_ring_walk_equals_the_host_parsed_pipeline(L):
    """208x112 in one slice per picture, dense: the longest walk through the GPU parser's bit window refills at a small
    size.  Above it is held against the tensor oracle; here also frame by frame against the pipeline on the host parser."""
    data = case("dense_one_slice_208x112")[1]
    a = run_all_outputs(L, data, parser_threads=2, gops_per_window=1, gpu_parser=True)
    b = run_all_outputs(L, data, parser_threads=2, gops_per_window=1, gpu_parser=False)
    assert set(a[0]) == set(b[0]) and len(a[0]) == 6
    for k in a[0]:
        assert all(np.array_equal(x, y) for x, y in zip(a[0][k], b[0][k])) and np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("name", ["lastmb_ip", "per_picture"])
def test_last_macroblock_inside_the_byte_of_its_predecessor_gpu_parser_reads_like_the_host(L, name):
    """the reference's byte-granular end-of-slice test (tests/test_vlc_syntax.py): written without the
    writer's guard, the stream loses those macroblocks (P: lastmb_ip, B: per_picture) in both parsers alike -- same
    frames from both, and not the frames of the tensors that were written"""
    pics, data, _ = X.build_case(X.CASES.get(name) or X.QUIRK_CASES[name], keep_last_mb=False)
    want = oracle_frames_from_tensors(pics, 96, 64)
    a = run_all_outputs(L, data, parser_threads=1, gops_per_window=1, gpu_parser=True)
    b = run_all_outputs(L, data, parser_threads=1, gops_per_window=1, gpu_parser=False)
    assert set(a[0]) == set(b[0]) == set(want)
    for k in a[0]:
        assert all(np.array_equal(x, y) for x, y in zip(a[0][k], b[0][k])) and np.array_equal(a[1][k], b[1][k]), k
    assert any(not np.array_equal(a[1][k], want[k]["rgba"]) for k in want)
