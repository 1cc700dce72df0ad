"""CPU: the cases of the suppress and match tests (tests/overlap_cases.py) hold what they claim, and the definitions in Python integers
(leon_ctypes.suppress_boxes, match_boxes) give the results written out by hand for the hand-made cases: the three pairs of the
header's text at one below, at and one above their threshold, the chain whose third row is kept because its only suppressor was
itself suppressed, score ties, duplicated boxes on both sides of a match, a row that falls to its second best partner."""
import numpy as np
import pytest

import overlap_cases as O


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    return leon_ctypes


def test_the_pairs_reach_exactly_the_thresholds_they_state():
    O.check_pairs()


def test_the_definitions_on_the_three_pairs_of_the_header(L):
    a, b = O.row(0, 0, 3, 1), O.row(1, 0, 3, 1)
    assert L.suppress_boxes(64, 64, 1, [a, b], [1, 0], 32768)[2] == [-1, 0] and L.suppress_boxes(64, 64, 1, [a, b], [1, 0], 32769)[2] == [-1, -1]
    assert L.match_boxes(64, 64, 1, [a], [b], 32768)[:4] == ([0], [0], [32768], 1) and L.match_boxes(64, 64, 1, [a], [b], 32769)[:4] == ([-1], [-1], [0], 0)
    a, b = O.row(0, 0, 4, 4), O.row(4, 0, 4, 4)
    assert L.suppress_boxes(64, 64, 1, [a, b], None, 1)[2:4] == ([-1, -1], 2) and L.match_boxes(64, 64, 1, [a], [b], 1)[3] == 0
    a, b = O.row(16, 16, 8, 8), O.row(0, 0, 64, 64)
    assert L.suppress_boxes(64, 64, 1, [a, b], None, 65536, L.OVERLAP_IOMIN)[2] == [-1, 0] and L.suppress_boxes(64, 64, 1, [a, b], None, 65536, L.OVERLAP_IOU)[2] == [-1, -1]
    assert L.match_boxes(64, 64, 1, [a], [b], 65536, L.OVERLAP_IOMIN)[2] == [65536] and L.match_boxes(64, 64, 1, [a], [b], 1024, L.OVERLAP_IOU)[2] == [1024]


def test_the_chain_keeps_its_third_row(L):
    rows = [O.row(0, 0, 10, 10), O.row(4, 0, 10, 10), O.row(8, 0, 10, 10)]
    out, order, by, count, status = L.suppress_boxes(64, 64, 1, rows, [3, 2, 1], int(0.4 * 65536))
    assert by == [-1, 0, -1] and count == 2 and order == [0, 2, -1] and status == [0, 0, 0]
    assert out == [rows[0], rows[2], [0] * 8]
    # rows 1 and 2 DO reach the threshold with each other: a kernel that asks "does any better row overlap" suppresses row 2
    inter, den = O.terms(O.IOU, (4, 0, 10, 10), (8, 0, 10, 10))
    assert inter * 65536 >= int(0.4 * 65536) * den


def test_refused_rows_take_no_part(L):
    rows = [O.row(0, 0, 10, 10, r0=1), O.row(0, 0, 10, 10), O.row(0, 0, 10, 10, frame=4), O.row(1, 0, 10, 10), O.row(0, 0, 0, 0)]
    out, order, by, count, status = L.suppress_boxes(64, 64, 4, rows, [9, 1, 9, 0, 9])
    assert status == [1, 0, 2, 0, 3] and by == [None, -1, None, 1, None] and count == 1 and order == [1, -1, -1, -1, -1]
    ma, mb, ov, count, sa, sb = L.match_boxes(64, 64, 4, rows, rows)
    assert ma == [None, 1, None, 3, None] and mb == ma and ov == [None, 65536, None, 65536, None] and count == 2 and sa == sb == status


@pytest.mark.parametrize("index", range(len(O.suppress_cases())), ids=[c.name for c in O.suppress_cases()])
def test_every_suppress_case_holds_what_it_states(L, index):
    c = O.suppress_cases()[index]
    out, order, by, count, status = O.expected_suppress(L, index)
    n, k = c.rows.shape[:2]
    assert out.shape == (n, k, 8) and ((order >= 0).sum(axis=1) == count).all()
    if "refused rows" in c.name:
        assert set(status.reshape(-1).tolist()) == {0, 1, 2, 3}, "not every status word occurs"
        assert (by[status != 0] == O.FILL).all() and (n == 1 or count[1] == 0)
    for s in range(n):          # the kept rows come out in walk order: scores never rise, and every row behind count is zero
        kept = order[s][:count[s]]
        sc = c.set_scores(s)
        if sc is not None:
            assert all(sc[p] >= sc[q] for p, q in zip(kept[:-1], kept[1:]))
        assert (out[s][count[s]:] == 0).all() and np.array_equal(out[s][:count[s], :5], c.rows[s][kept][:, :5])


@pytest.mark.parametrize("index", range(len(O.match_cases())), ids=[c.name for c in O.match_cases()])
def test_every_match_case_holds_what_it_states(L, index):
    c = O.match_cases()[index]
    ma, mb, ov, count, sa, sb = O.expected_match(L, index)
    assert ma.shape == c.a.shape[:2] and mb.shape == c.b.shape[:2]
    if "refused rows" in c.name:
        assert set(sa.reshape(-1).tolist()) | set(sb.reshape(-1).tolist()) == {0, 1, 2, 3}
        assert (ma[sa != 0] == O.FILL).all() and (ov[sa != 0] == O.FILL).all() and (mb[sb != 0] == O.FILL).all()
    assert ((ov > 0) == (ma >= 0)).all() and (ov[ma >= 0] >= c.threshold).all()
