"""CPU: the definition of leon_pipeline_field_tensors on the CPU (leon_pipeline_field_tensor_record: csrc/leon_fields.h's plain loop over
samples behind the regions' own judgement and the pixel road's table builder) against leon_ctypes.field_tensor, the header's text in
numpy integers and np.float32 on the pure-Python resize_weights, on the cases of tests/fields_cases.py -- the ones
tests/test_fields_kernel_gpu.py runs through the kernel.  Every tensor byte and every status word compared for equality; a refused
record's tensor still holds the sentinel; the items are left as they were.  No GPU."""
import numpy as np
import pytest

import fields_cases as F


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def cases(L):
    return F.cases(L)


def run(L, c):
    """the records of a case one by one through the CPU definition -> (out [n, pitch] uint8, status [n]) as the kernel's call gives them"""
    items = c["items"].copy()
    out = np.full((len(c["records"]), F.pitch_of(c)), F.FILL, dtype=np.uint8)
    status = np.zeros(len(c["records"]), dtype=np.int32)
    for i, r in enumerate(c["records"]):
        status[i], t = L.field_tensor_record(c["fw"], c["fh"], c["cw"], c["ch"], items, r, c["size"], c["channels"], source=c["source"], dtype=c["dtype"], fill=F.FILL)
        out[i, :F.region_bytes(c)] = t.view(np.uint8).reshape(-1)
    assert np.array_equal(items, c["items"]), c["what"]
    return out, status


def check(L, cases, *prefixes):
    got = [c for c in cases if c["what"].startswith(prefixes)]
    assert got, prefixes
    for c in got:
        want_out, want_status = F.expected(L, c)
        out, status = run(L, c)
        assert status.tolist() == want_status.tolist(), c["what"]
        assert np.array_equal(out, want_out), (c["what"], np.argwhere(out != want_out)[:4].tolist())
    return got


@pytest.mark.parametrize("shape", F.SHAPES)
def test_every_shape_box_and_refusal(L, cases, shape):
    got = check(L, cases, "window, %dx%d " % shape[:2])
    assert len(got) == 9
    seen = set()
    for c in got:
        seen |= set(F.expected(L, c)[1].tolist())
    assert {0, L.REGION_RESERVED, L.REGION_FRAME, L.REGION_BOX} <= seen


def test_tile_and_store_edges(L, cases):
    assert len(check(L, cases, "tile,")) == 2 * len(F.TILE_SIZES)


def test_ratio_of_16_and_one_above(L, cases):
    got = check(L, cases, "ratio,")
    assert F.expected(L, got[0])[1].tolist() == [0, L.REGION_RATIO_X, 0, L.REGION_RATIO_Y, L.REGION_RATIO_X] and F.expected(L, got[1])[1].tolist() == [0]


def test_small_boxes_enlarged(L, cases):
    assert len(check(L, cases, "enlarged,")) == 3


def test_channel_counts_shifts_and_an_odd_frame(L, cases):
    assert len(check(L, cases, "channels,", "odd frame")) == 4


def test_extremes_and_rounding_ties(L, cases):
    got = check(L, cases, "extremes,", "ties,")
    assert len(got) == 6
    # the ties are ties: the constants times the scales lie halfway between two elements of the type
    c = [c for c in got if c["what"] == "ties, float16"][0]
    t = L.field_batch(F.expected(L, c)[0], len(c["channels"]), c["size"], "float16")
    assert t[0, 0, 0, 0] == 2048 and t[1, 0, 0, 0] == 2052 and t[0, 1, 0, 0] == 1024 and t[1, 1, 0, 0] == 1026 and t[6, 0, 0, 0] == -2048
    c = [c for c in got if c["what"] == "ties, bfloat16"][0]
    t = L.field_batch(F.expected(L, c)[0], len(c["channels"]), c["size"], "bfloat16")
    assert t[2, 0, 0, 0] == 0x4380 and t[3, 0, 0, 0] == 0x4382 and t[7, 0, 0, 0] == 0xC380          # 256, 260, -256


def test_record_sources_layouts(L, cases):
    assert len(check(L, cases, "motion record,", "residual record,")) == 4


def test_bytes_left_alone(L, cases):
    got = check(L, cases, "alone,")
    assert len(got) == 6
    for c in got:
        out, _ = F.expected(L, c)
        assert (out[:, F.region_bytes(c):] == F.FILL).all()


def test_no_case_is_left_out(cases):
    prefixes = ("window,", "tile,", "ratio,", "enlarged,", "channels,", "odd frame", "extremes,", "ties,", "motion record,", "residual record,", "alone,")
    assert all(c["what"].startswith(prefixes) for c in cases)
