"""CPU: the case table of tests/propose_cases.py holds what it promises -- each named mask has the number of components it is built
for under connectivity 4 and 8, the records built from a mask are hot exactly there -- and the library's CPU definition of a request
(leon_pipeline_propose_record: leon_propose.h around a flood fill) equals leon_ctypes.propose_boxes, the header's text in Python
integers, bit for bit on every case: each source alone and both, the intra flag, K and min_cells around the counts.  No GPU."""
import numpy as np
import pytest

import propose_cases as P


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


FILL = -7
SMALL = ["1x1", "2x2", "6x4", "22x15", "61x45 in 4x3", "256x2", "2x256"]


def count_of(L, fw, fh, mask, connectivity):
    """the components of a mask by the oracle, through an activity record that is hot exactly there"""
    st, _, _, count = L.propose_boxes(fw, fh, 1, None, [P.cells_from(mask, 1)], 0, ac_min=P.AC_MIN, connectivity=connectivity, max_boxes=1)
    assert st == 0
    return count


@pytest.mark.parametrize("grid", SMALL + ["120x68"])
def test_masks_have_the_components_they_are_built_for(L, grid):
    fw, fh, mbw, mbh = P.GRIDS[grid]
    said = 0
    for name, build in P.MASKS.items():
        mask, n4, n8 = build(mbw, mbh)
        assert mask.shape == (mbh, mbw) and mask.dtype == bool
        for conn, n in ((4, n4), (8, n8)):
            if n is not None:
                said += 1
                inside = mask & P.hot_cells(L, fw, fh, None, P.cells_from(np.ones_like(mask), 0), ac_min=1)
                if (inside == mask).all():          # (a grid larger than its frame cuts cells off: the figure is the whole grid's)
                    assert count_of(L, fw, fh, mask, conn) == n, (grid, name, conn)
    assert said >= 16


def test_spiral_and_serpentine_are_one_cell_wide():
    for build in (P.spiral, P.serpentine):
        m = build(22, 15)[0]
        assert m.sum() > 100 and not (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).any()


def test_records_are_hot_exactly_on_their_mask(L):
    mask = P.random(0.5)(22, 15)[0]
    mv, info = P.motion_from(mask, 3)
    mag = np.abs(mv.astype(np.int64)).max(axis=2)
    assert ((mag >= P.MV_MIN) == mask).all() and (mag[mask] == P.MV_MIN).any() and (mag[mask] > P.MV_MIN).any() and (mag[~mask] == P.MV_MIN - 1).any()
    assert (P.motion_from(mask, 3, extreme=True)[0].astype(np.int64).min(axis=2)[mask] == -32768).all()
    c = P.cells_from(mask, 4)
    assert ((c["ac_mag"] >= P.AC_MIN) == mask).all() and (c["ac_mag"][mask] == P.AC_MIN).any() and (c["ac_mag"][~mask] == P.AC_MIN - 1).any()
    assert (P.cells_from(mask, 4, top=True)["ac_mag"][mask] == 65535).all()
    assert P.every_mask(3, 3).shape == (512, 3, 3) and P.every_mask(3, 3)[5].reshape(-1).tolist() == [True, False, True] + [False] * 6


def record_of(L, fw, fh, mbw, mbh, motion, activity, frame, what, **kw):
    st, regions, info, count = L.propose_record(fw, fh, mbw, mbh, len(motion or activity), motion, activity, frame, fill=FILL, **kw)
    want = P.expected(L, fw, fh, motion, activity, [frame], FILL, **kw)
    P.assert_equal((regions[None], info[None], np.array([count]), np.array([st])), want, what)
    return want


@pytest.mark.parametrize("grid", SMALL)
def test_propose_record_equals_propose_boxes_on_every_mask(L, grid):
    fw, fh, mbw, mbh = P.GRIDS[grid]
    for k, (name, build) in enumerate(P.MASKS.items()):
        mask = build(mbw, mbh)[0]
        other = P.random(0.2, seed=k)(mbw, mbh)[0]
        motion, activity = [P.motion_from(mask, k, intra=other)], [P.cells_from(other, k)]
        for conn in (4, 8):
            what = "%s, %s, connectivity %d" % (grid, name, conn)
            w = record_of(L, fw, fh, mbw, mbh, motion, None, 0, what + ", motion", mv_min=P.MV_MIN, connectivity=conn, max_boxes=8)
            count = int(w[2][0])
            record_of(L, fw, fh, mbw, mbh, None, activity, 0, what + ", activity", ac_min=P.AC_MIN, connectivity=conn, max_boxes=8)
            record_of(L, fw, fh, mbw, mbh, motion, activity, 0, what + ", both", mv_min=P.MV_MIN, ac_min=P.AC_MIN, connectivity=conn, max_boxes=8)
            record_of(L, fw, fh, mbw, mbh, motion, None, 0, what + ", intra", mv_min=P.MV_MIN, intra=True, connectivity=conn, max_boxes=8)
            for K in {1, max(1, count - 1), max(1, count), count + 1}:
                if K <= L.PROPOSE_MAX_BOXES:
                    record_of(L, fw, fh, mbw, mbh, motion, None, 0, what + ", K %d" % K, mv_min=P.MV_MIN, connectivity=conn, max_boxes=K)
            if count:
                largest = max(c for c, _ in L.propose_boxes(fw, fh, 1, motion, None, 0, mv_min=P.MV_MIN, connectivity=conn, max_boxes=1024)[2])
                for least in (2, largest, largest + 1):
                    if least <= L.PROPOSE_MAX_CELLS:
                        record_of(L, fw, fh, mbw, mbh, motion, None, 0, what + ", min_cells %d" % least, mv_min=P.MV_MIN, connectivity=conn, min_cells=least, max_boxes=8)


def test_the_whole_largest_grid_is_one_component_of_65536_cells(L):
    fw, fh, mbw, mbh = P.GRIDS["256x256"]
    mask = P.full(mbw, mbh)[0]
    activity = [P.cells_from(mask, 1, top=True)]
    st, regions, info, count = L.propose_record(fw, fh, mbw, mbh, 1, None, activity, 0, ac_min=65535, connectivity=4, max_boxes=2, min_cells=65536, fill=FILL)
    assert (st, count) == (0, 1) and regions.tolist() == [[0, 0, 0, 4096, 4096, 0, 0, 0], [0] * 8] and info.tolist() == [[65536, 0], [0, -1]]


def test_thresholds_at_one_below_and_one_above_a_value(L):
    """one hot cell whose value is v: hot at threshold v - 1 and v, cold at v + 1 -- a vector word of -32768 and an ac_mag of 65535 included"""
    fw, fh, mbw, mbh = P.GRIDS["6x4"]
    mask = np.zeros((mbh, mbw), dtype=bool)
    mask[2, 3] = True
    for v in (2, 77, 32768):
        mv = np.zeros((mbh, mbw, 4), dtype=np.int16)
        mv[2, 3, 1] = -v
        motion = [(mv, np.ones((mbh, mbw), dtype=np.uint8))]
        for t in (v - 1, v, v + 1):
            if 1 <= t <= 32768:
                w = record_of(L, fw, fh, mbw, mbh, motion, None, 0, "mv %d at %d" % (v, t), mv_min=t)
                assert int(w[2][0]) == (1 if t <= v else 0)
    for v in (2, 300, 65535):
        c = P.cells_from(mask, 0, ac_min=v, top=True)
        c["ac_mag"][mask] = v
        c["ac_mag"][~mask] = 0
        for t in (v - 1, v, v + 1):
            if 1 <= t <= 65535:
                w = record_of(L, fw, fh, mbw, mbh, None, [c], 0, "ac %d at %d" % (v, t), ac_min=t)
                assert int(w[2][0]) == (1 if t <= v else 0)


def test_cells_outside_the_frame_are_never_hot(L):
    """33 x 17 in a 4 x 3 grid: the last grid column and the last grid row lie wholly outside the frame, hot records or not"""
    mask = np.ones((3, 4), dtype=bool)
    motion, activity = [P.motion_from(mask, 1)], [P.cells_from(mask, 1)]
    w = record_of(L, 33, 17, 4, 3, motion, activity, 0, "33x17 in 4x3", mv_min=P.MV_MIN, ac_min=P.AC_MIN)
    assert w[0][0][0].tolist() == [0, 0, 0, 33, 17, 0, 0, 0] and w[1][0][0].tolist() == [6, 0] and int(w[2][0]) == 1
