"""GPU: k_accumulate through leon_pipeline_accumulate_kernel (include/leon_pipeline.h) on hand-written motion and residual records,
against leon_ctypes.accumulate_hop, the header's text in numpy integers, on the cases of tests/accumulate_cases.py (the ones
tests/test_accumulate_cases.py pins on the CPU): every slot compared exactly -- destinations, sources and slots the call does not
name --, via and status exactly, and what the kernel is to leave alone -- a refused hop's slot and via, the bytes between the slots of
a pitched buffer, records behind the call's count, via and status that are NULL -- still holding the sentinel.  The shapes are the
smallest at which the walk can go wrong: 16 x 16 (one macroblock, a chroma row of 8 elements in a stride of 64), 64 x 48 (the luma
stride is the width: no pad behind the last plane of the motion part) and 128 x 32 (the chroma stride is the width: none behind RCr)."""
import numpy as np
import pytest

import accumulate_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def cases(L):
    return A.cases(L)


def run(L, c):
    buf = c["buf"].copy()
    via, status = L.accumulate_kernel(c["cw"], c["ch"], c.get("n_frames", len(c["motion"])), c["motion"], c["residual"], c["hops"], c["parts"], buf, via=c.get("via", True),
                                      status=c.get("status", True), via_fill=A.VIA_FILL, status_fill=A.STATUS_FILL, n=c.get("n"))
    return buf, via, status


def pick(cases, *prefixes):
    got = [c for c in cases if c["what"].startswith(prefixes)]
    assert got, prefixes
    return got


@pytest.mark.parametrize("cw,ch", A.SHAPES)
@pytest.mark.parametrize("parts", A.PARTS)
def test_every_shape_and_part(L, cases, cw, ch, parts):
    """seeded vectors that leave at every edge, small ones, the int16 extremes, an I picture; forward, backward, both and neither"""
    for c in pick(cases, "window, %dx%d parts %d" % (cw, ch, parts)):
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


@pytest.mark.parametrize("cw,ch", A.SHAPES)
def test_sources_in_the_last_slot(L, cases, cw, ch):
    """vectors into the bottom-right corner of the last slot of a buffer of exactly n_slots * slot_pitch: the funnel's spare dword"""
    got = pick(cases, "last slot, %dx%d" % (cw, ch))
    assert len(got) == 3
    for c in got:
        assert c["buf"].shape[1] == L.accumulate_layout(cw, ch, c["parts"]).slot_bytes and all(2 * 5 in h[2:4] for h in c["hops"])
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


@pytest.mark.parametrize("gap", [4, 256])
def test_a_pitch_larger_than_the_accumulator(L, cases, gap):
    got = pick(cases, "gap %d," % gap)
    assert len(got) == 9
    for c in got:
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


def test_ties_info_and_saturation(L, cases):
    got = pick(cases, "ties,", "info,", "saturation")
    assert len(got) == 3 + 3 + 6
    for c in got:
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


def test_hop_counts_with_refused_hops_between_valid_ones(L, cases):
    got = pick(cases, "one hop", "one refused hop", "2 hops", "4 hops", "10 hops")
    assert len(got) == 5
    for c in got:
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


def test_without_the_optional_outputs(L, cases):
    got = pick(cases, "via ")
    assert len(got) == 3
    for c in got:
        A.assert_equal(L, c, run(L, c), A.expected(L, c))


def test_a_window_of_no_frames_and_only_the_targets_records(L, cases):
    got = pick(cases, "a window of no frames", "only the target's records")
    assert len(got) == 4
    for c in got:
        want = A.expected(L, c)
        A.assert_equal(L, c, run(L, c), want)
        if c["what"].startswith("only"):
            assert want[2].tolist() == [0] and not np.array_equal(want[0][3], c["buf"][3])


def test_no_case_is_left_out(cases):
    """the tests above run every case of the list between them"""
    prefixes = ("window,", "last slot,", "gap 4,", "gap 256,", "ties,", "info,", "saturation", "one hop", "one refused hop", "2 hops", "4 hops", "10 hops", "via ",
                "a window of no frames", "only the target's records")
    assert all(c["what"].startswith(prefixes) for c in cases)
