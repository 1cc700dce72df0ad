"""GPU: k_suppress and k_match through leon_pipeline_suppress_kernel and leon_pipeline_match_kernel (include/leon_pipeline.h) on every
case of tests/overlap_cases.py, against leon_ctypes.suppress_boxes and match_boxes, the header's text as a sorted walk in Python
integers: every output compared exactly, with what the kernels are to leave alone -- the words of a refused row, everything behind
set n - 1, an optional output that went down as NULL -- still holding the sentinel.  The cases are the ones at which the kernels can
go wrong: the pairs of the header at one below, at and one above their threshold (the largest products among them), the chain whose
third row is kept, score ties and the ends of int32, K = 1, 2, 63, 64, 65, 255, 256, 257 and 1024 (a workgroup has 256 threads, the
sort pads to a power of two), sets with every kind of refused row and one without an accepted row, duplicated boxes on both sides of
a match, 256 identical boxes (a pair a round), both measures."""
import numpy as np
import pytest

import overlap_cases as O

pytestmark = pytest.mark.gpu

FILL = O.FILL


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.mark.parametrize("index", range(len(O.suppress_cases())), ids=[c.name for c in O.suppress_cases()])
def test_suppress_kernel_against_the_definition(L, index):
    c = O.suppress_cases()[index]
    got = L.suppress_kernel(c.fw, c.fh, c.n_frames, c.rows, fill=FILL, **c.kw())
    O.assert_equal(got, O.expected_suppress(L, index), O.SUPPRESS_NAMES, c.name)


@pytest.mark.parametrize("index", range(len(O.match_cases())), ids=[c.name for c in O.match_cases()])
def test_match_kernel_against_the_definition(L, index):
    c = O.match_cases()[index]
    got = L.match_kernel(c.fw, c.fh, c.n_frames, c.a, c.b, fill=FILL, **c.kw())
    O.assert_equal(got, O.expected_match(L, index), O.MATCH_NAMES, c.name)


def case(cases, name):
    return next(i for i, c in enumerate(cases) if c.name == name)


@pytest.mark.parametrize("name", ["chain", "n 5 with refused rows", "K 257"])
def test_suppress_optional_outputs_null_one_at_a_time_and_what_lies_behind_the_last_set(L, name):
    index = case(O.suppress_cases(), name)
    c, want = O.suppress_cases()[index], O.expected_suppress(L, index)
    for off, slot in (("with_out", 0), ("with_order", 1), ("with_status", 4)):
        w = [x.copy() for x in want]
        w[slot][:] = FILL
        O.assert_equal(L.suppress_kernel(c.fw, c.fh, c.n_frames, c.rows, fill=FILL, **{off: False}, **c.kw()), w, O.SUPPRESS_NAMES, "%s, %s off" % (name, off))
    n = c.rows.shape[0]
    rows = np.concatenate([c.rows, c.rows[:1], c.rows[:1]])          # two more sets behind set n - 1, which the call does not name
    scores = None if c.scores is None else np.concatenate([c.scores, np.zeros(2 * c.rows.shape[1] * c.stride, dtype=np.int32)])
    got = L.suppress_kernel(c.fw, c.fh, c.n_frames, rows, scores, score_stride=c.stride, threshold_q16=c.threshold, measure=c.measure, fill=FILL, n=n)
    O.assert_equal([g[:n] for g in got], want, O.SUPPRESS_NAMES, "%s, n %d of %d" % (name, n, n + 2))
    assert all((g[n:] == FILL).all() for g in got), "%s: something was written behind set %d" % (name, n - 1)


@pytest.mark.parametrize("name", ["second best and unmatched", "n 5 with refused rows", "sparse 257 x 257"])
def test_match_optional_outputs_null_one_at_a_time_and_what_lies_behind_the_last_set(L, name):
    index = case(O.match_cases(), name)
    c, want = O.match_cases()[index], O.expected_match(L, index)
    for off, slot in (("with_status_a", 4), ("with_status_b", 5)):
        w = [x.copy() for x in want]
        w[slot][:] = FILL
        O.assert_equal(L.match_kernel(c.fw, c.fh, c.n_frames, c.a, c.b, fill=FILL, **{off: False}, **c.kw()), w, O.MATCH_NAMES, "%s, %s off" % (name, off))
    n = c.a.shape[0]
    got = L.match_kernel(c.fw, c.fh, c.n_frames, np.concatenate([c.a, c.a[:1], c.a[:1]]), np.concatenate([c.b, c.b[:1], c.b[:1]]), fill=FILL, n=n, **c.kw())
    O.assert_equal([g[:n] for g in got], want, O.MATCH_NAMES, "%s, n %d of %d" % (name, n, n + 2))
    assert all((g[n:] == FILL).all() for g in got), "%s: something was written behind pair %d" % (name, n - 1)


def test_both_measures_on_one_set(L):
    """the nested boxes that propose's components give: IOMIN clears the inner ones, IOU at the same threshold keeps them"""
    rows = np.array([O.row(0, 0, 64, 64), O.row(16, 16, 8, 8), O.row(40, 40, 8, 8), O.row(8, 8, 48, 48)], dtype=np.int32)
    scores = [64 * 64, 64, 64, 48 * 48]
    for measure, by in ((O.IOMIN, [-1, 0, 0, 0]), (O.IOU, [-1, -1, -1, 0])):
        got = L.suppress_kernel(64, 64, 1, rows, scores, threshold_q16=32768, measure=measure, fill=FILL)
        assert got[2][0].tolist() == by and L.suppress_boxes(64, 64, 1, rows.tolist(), scores, 32768, measure)[2] == by
