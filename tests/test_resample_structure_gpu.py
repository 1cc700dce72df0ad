"""GPU: the twelve resize kernels (k_resample<element bytes, layout, filter>: one device function, resample_body) at the
geometries of tests/resample_structure.py -- every tile, chunk and store-line edge that tests/test_resample_structure.py shows them to
reach, on three small streams whose two unequal GOPs share a window.  Expected = T[c][resize_rgb(ORACLE RGB, crop, size, filter)], the
expectation of the existing tensor tests; compared as bit patterns, every frame of every window, no tolerance."""
import pytest

import resample_structure as R
from resample_structure import BICUBIC, CASES, TRIANGLE
from test_pipeline_gpu import ibbp_stream, oracle_frames
from test_pipeline_tensor_bicubic_gpu import expected as expected_bicubic
from test_pipeline_tensor_format_gpu import assert_tensors, expected as expected_triangle, run_format

pytestmark = pytest.mark.gpu

# a staging-side or arithmetic case: a kernel with per-lane element stores and one with the packed store
STAGING_FORMATS = [("float16", "chw"), ("uint8", "hwc")]
# a store-side case: the four packed kernels (uint8 CHW, HWC of 1-, 2- and 4-byte elements) and the three element types of float CHW
STORE_FORMATS = [("uint8", "chw"), ("uint8", "hwc"), ("float16", "hwc"), ("float32", "hwc"), ("float16", "chw"), ("bfloat16", "chw"), ("float32", "chw")]
RUNS = [(c, f, d, l) for c in CASES for f in c.filters for d, l in (STORE_FORMATS if c.kind == "store" else STAGING_FORMATS)]
# one staging case and one store case through the host parser as well, and with a window per GOP
BOTH_WAYS = [(R.BY_NAME["ratio16-two-tiles"], "uint8", "hwc"), (R.BY_NAME["store-width-33"], "uint8", "chw")]


def run_id(run):
    return "-".join([run[0].name] + [R.FILTER_NAMES.get(v, v) for v in run[1:]])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def streams():
    """name -> (stream bytes, {(gop, display index): the oracle's RGBA}): written and decoded once per module"""
    made = {}

    def get(name):
        if name not in made:
            cw, ch, gops, seed, (fw, fh) = R.STREAMS[name]
            data = ibbp_stream(cw, ch, gops, seed=seed, frame=(fw, fh))
            rgba = oracle_frames(data)
            assert [sum(1 for g, _ in rgba if g == k) for k in range(len(gops))] == gops and len(set(gops)) == len(gops)          # unequal GOPs
            assert all(v.shape == (fh, fw, 4) for v in rgba.values())
            if fh & 1:
                assert all((v[fh - 1] == 255).all() for v in rgba.values())          # the fill row
            made[name] = (data, rgba)
        return made[name]
    return get


def check(L, streams, case, filt, dtype, layout, **kw):
    data, rgba = streams(case.stream)
    want = (expected_bicubic if filt == BICUBIC else expected_triangle)(L, rgba, dtype, layout, case.size, case.crop)
    kw.setdefault("gops_per_window", 2)
    kw.setdefault("gpu_parser", True)
    got = run_format(L, data, dtype, layout, parser_threads=2, tensor_size=case.size, tensor_crop=case.crop, tensor_filter=filt, **kw)[0]
    assert_tensors(got, want, "%s %s %s %s %s" % (case.name, R.FILTER_NAMES[filt], dtype, layout, kw))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_case(L, streams, run):
    case, filt, dtype, layout = run
    assert case.fact(case, filt), case.why
    check(L, streams, case, filt, dtype, layout)


@pytest.mark.parametrize("filt", [TRIANGLE, BICUBIC], ids=["triangle", "bicubic"])
@pytest.mark.parametrize("run", BOTH_WAYS, ids=run_id)
def test_host_parser(L, streams, run, filt):
    case, dtype, layout = run
    check(L, streams, case, filt, dtype, layout, gpu_parser=False)


@pytest.mark.parametrize("filt", [TRIANGLE, BICUBIC], ids=["triangle", "bicubic"])
@pytest.mark.parametrize("run", BOTH_WAYS, ids=run_id)
def test_a_window_per_gop(L, streams, run, filt):
    """two windows of unequal length, the first delivered and the last: every frame of both"""
    case, dtype, layout = run
    check(L, streams, case, filt, dtype, layout, gops_per_window=1)
