"""GPU: k_box_tables and k_fields through leon_pipeline_field_tensors_kernel (include/leon_pipeline.h) on hand-made items, against
leon_ctypes.field_tensor, the header's text in numpy, on the cases of tests/fields_cases.py (the ones tests/test_fields_cases.py pins on
the CPU): the whole output buffer compared for equality -- every tensor, and what the kernel is to leave alone still holding the
sentinel: a refused record's tensor, the pitch gap behind every tensor, a status array that is NULL.  The shapes are the smallest at
which the walk can go wrong: one macroblock, a frame smaller than its coded picture, out sizes around the 32 x 8 tile and the 16-byte
store, ratios of 16 and above."""
import numpy as np
import pytest

import fields_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def cases(L):
    return F.cases(L)


def check(L, cases, *prefixes):
    got = [c for c in cases if c["what"].startswith(prefixes)]
    assert got, prefixes
    for c in got:
        want_out, want_status = F.expected(L, c)
        items = c["items"].copy()
        out, status = L.field_tensors_kernel(c["fw"], c["fh"], c["cw"], c["ch"], items, c["records"], c["size"], c["channels"], source=c["source"], dtype=c["dtype"],
                                             pitch=c.get("pitch"), status=c.get("status", True), fill=F.FILL, status_fill=F.STATUS_FILL, scratch_limit=c.get("scratch_limit", 0))
        assert np.array_equal(items, c["items"]), c["what"]
        assert status.tolist() == (want_status.tolist() if c.get("status", True) else [F.STATUS_FILL] * len(want_status)), c["what"]
        assert out.shape == want_out.shape and np.array_equal(out, want_out), (c["what"], np.argwhere(out != want_out)[:4].tolist())
    return got


@pytest.mark.parametrize("shape", F.SHAPES)
def test_every_shape_box_and_refusal(L, cases, shape):
    assert len(check(L, cases, "window, %dx%d " % shape[:2])) == 9


def test_tile_and_store_edges(L, cases):
    assert len(check(L, cases, "tile,")) == 2 * len(F.TILE_SIZES)


def test_ratio_of_16_and_one_above(L, cases):
    assert len(check(L, cases, "ratio,")) == 2


def test_small_boxes_enlarged(L, cases):
    assert len(check(L, cases, "enlarged,")) == 3


def test_channel_counts_shifts_and_an_odd_frame(L, cases):
    assert len(check(L, cases, "channels,", "odd frame")) == 4


def test_extremes_and_rounding_ties(L, cases):
    assert len(check(L, cases, "extremes,", "ties,")) == 6


def test_record_sources_layouts(L, cases):
    assert len(check(L, cases, "motion record,", "residual record,")) == 4


def test_bytes_left_alone_and_chunks(L, cases):
    assert len(check(L, cases, "alone,")) == 6


def test_no_case_is_left_out(cases):
    prefixes = ("window,", "tile,", "ratio,", "enlarged,", "channels,", "odd frame", "extremes,", "ties,", "motion record,", "residual record,", "alone,")
    assert all(c["what"].startswith(prefixes) for c in cases)
