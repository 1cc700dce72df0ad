"""GPU: k_propose through leon_pipeline_propose_kernel (include/leon_pipeline.h) on hand-made motion and activity records
(tests/propose_cases.py), against leon_ctypes.propose_boxes, the header's text as a breadth-first fill in Python integers: regions,
info, count and status compared exactly, the rows behind count holding the filler, and what the kernel is to leave alone -- the rows
of a refused request, everything behind request n - 1 -- still holding the sentinel.  The grids are 1 x 1, 2 x 2, 6 x 4, 22 x 15, a
61 x 45 and a 33 x 17 frame in a 4 x 3 grid, 256 x 2, 2 x 256, 120 x 68 under 1920 x 1080 and 256 x 256; the masks the ones at which
a label search can go wrong -- a one-cell-wide serpentine and a spiral through the whole grid (the longest path a label travels), a
comb whose teeth join in the last row (labels that merge late), a checkerboard (every cell alone under 4, one component under 8),
nested rings, a diagonal, the end of a row beside the start of the next, one component of 65536 cells -- and EVERY mask of the
3 x 3 and the 4 x 3 grid in one call each, both connectivities."""
import numpy as np
import pytest

import propose_cases as P

pytestmark = pytest.mark.gpu

FILL = -77


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def run(L, fw, fh, mbw, mbh, motion, activity, frames, what="", n=None, with_info=True, with_status=True, **kw):
    n_frames = len(motion if motion is not None else activity)
    got = L.propose_kernel(fw, fh, mbw, mbh, n_frames, motion, activity, frames, fill=FILL, n=n, with_info=with_info, with_status=with_status, **kw)
    count = len(frames) if n is None else n
    want = [w.copy() for w in P.expected(L, fw, fh, motion, activity, list(frames)[:count], FILL, **kw)]
    if not with_info:
        want[1][:] = FILL
    if not with_status:
        want[3][:] = FILL
    P.assert_equal([g[:count] for g in got], want, what)
    for name, g in zip(("regions", "info", "count", "status"), got):
        assert (g[count:] == FILL).all(), "%s: %s was written behind request %d" % (what, name, count - 1)
    return want


SMALL = ["1x1", "2x2", "6x4", "22x15", "61x45 in 4x3", "256x2", "2x256"]


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("grid", SMALL)
def test_every_mask_of_a_grid_from_each_source(L, grid, conn):
    """one window whose frame k holds mask k in its motion record and a seeded other mask in its activity record; every frame a request"""
    fw, fh, mbw, mbh = P.GRIDS[grid]
    masks = [build(mbw, mbh)[0] for build in P.MASKS.values()]
    others = [P.random(0.2, seed=k)(mbw, mbh)[0] for k in range(len(masks))]
    motion = [P.motion_from(m, k, intra=o) for k, (m, o) in enumerate(zip(masks, others))]
    activity = [P.cells_from(o, k) for k, o in enumerate(others)]
    frames = list(range(len(masks)))
    what = "%s, connectivity %d" % (grid, conn)
    w = run(L, fw, fh, mbw, mbh, motion, None, frames, what + ", motion", mv_min=P.MV_MIN, connectivity=conn, max_boxes=8)
    assert (w[2] > 8).any() or mbw * mbh < 32, "no request overflows K"
    run(L, fw, fh, mbw, mbh, None, activity, frames, what + ", activity", ac_min=P.AC_MIN, connectivity=conn, max_boxes=8)
    run(L, fw, fh, mbw, mbh, motion, activity, frames, what + ", both", mv_min=P.MV_MIN, ac_min=P.AC_MIN, connectivity=conn, max_boxes=8)
    run(L, fw, fh, mbw, mbh, motion, None, frames, what + ", intra", mv_min=P.MV_MIN, intra=True, connectivity=conn, max_boxes=8)
    run(L, fw, fh, mbw, mbh, motion, activity, frames, what + ", K 1024", mv_min=P.MV_MIN, ac_min=P.AC_MIN, connectivity=conn, max_boxes=1024)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", ["serpentine", "spiral", "comb", "rings", "checkerboard", "random 0.5", "random 0.6", "random 0.9"])
def test_masks_of_a_1080p_grid(L, name, conn):
    fw, fh, mbw, mbh = P.GRIDS["120x68"]
    mask = P.MASKS[name](mbw, mbh)[0]
    w = run(L, fw, fh, mbw, mbh, None, [P.cells_from(mask, 1)], [0], "120x68, %s, connectivity %d" % (name, conn), ac_min=P.AC_MIN, connectivity=conn, max_boxes=16)
    assert int(w[2][0]) >= 1


@pytest.mark.parametrize("name,conn", [("full", 4), ("checkerboard", 4), ("checkerboard", 8), ("serpentine", 4), ("spiral", 8), ("comb", 4), ("rings", 8), ("random 0.5", 4),
                                       ("random 0.6", 8), ("empty", 8)])
def test_masks_of_the_largest_grid(L, name, conn):
    """256 x 256: 16-bit labels at their end, the LDS at its largest with K = 1024, a component of 65536 cells, 32768 components"""
    fw, fh, mbw, mbh = P.GRIDS["256x256"]
    mask = P.MASKS[name](mbw, mbh)[0]
    w = run(L, fw, fh, mbw, mbh, [P.motion_from(mask, 2, extreme=name == "full")], None, [0], "256x256, %s, connectivity %d" % (name, conn),
            mv_min=32768 if name == "full" else P.MV_MIN, connectivity=conn, max_boxes=1024)
    if name == "full":
        assert w[1][0][0].tolist() == [65536, 0] and int(w[2][0]) == 1
        run(L, fw, fh, mbw, mbh, [P.motion_from(mask, 2, extreme=True)], None, [0], "256x256, full, min_cells 65536", mv_min=32768, connectivity=conn, max_boxes=3,
            min_cells=65536)
    if name == "checkerboard" and conn == 4:
        assert int(w[2][0]) == 32768


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("mbw,mbh", [(3, 3), (4, 3)])
def test_every_mask_of_a_small_grid_in_one_call(L, mbw, mbh, conn):
    """512 (4096) requests on 512 (4096) frames, frame k's activity record hot on mask number k"""
    masks = P.every_mask(mbw, mbh)
    activity = [P.cells_from(m, k) for k, m in enumerate(masks)]
    frames = list(range(len(masks)))
    run(L, 16 * mbw, 16 * mbh, mbw, mbh, None, activity, frames, "every mask of %d x %d, connectivity %d" % (mbw, mbh, conn), ac_min=P.AC_MIN, connectivity=conn, max_boxes=6)


@pytest.mark.parametrize("conn", (4, 8))
def test_k_and_min_cells_around_the_counts(L, conn):
    fw, fh, mbw, mbh = P.GRIDS["22x15"]
    mask = P.random(0.5)(mbw, mbh)[0]
    motion = [P.motion_from(mask, 5)]
    st, _, info, count = L.propose_boxes(fw, fh, 1, motion, None, 0, mv_min=P.MV_MIN, connectivity=conn, max_boxes=1024)
    largest = max(c for c, _ in info)
    assert count >= 3 and largest >= 3
    for K in (1, count - 1, count, count + 1):
        w = run(L, fw, fh, mbw, mbh, motion, None, [0], "K %d of %d" % (K, count), mv_min=P.MV_MIN, connectivity=conn, max_boxes=K)
        assert int(w[2][0]) == count
        if K > count:          # the rows behind count: the filler
            assert w[0][0][count:].tolist() == [[0, 0, 0, 0, 0, 0, 0, 0]] * (K - count) and w[1][0][count:].tolist() == [[0, -1]] * (K - count)
    for least, some in ((1, True), (2, True), (largest, True), (largest + 1, False)):
        w = run(L, fw, fh, mbw, mbh, motion, None, [0], "min_cells %d" % least, mv_min=P.MV_MIN, connectivity=conn, min_cells=least, max_boxes=count + 1)
        assert (int(w[2][0]) > 0) == some


def test_thresholds_at_one_below_and_one_above_a_value(L):
    fw, fh, mbw, mbh = P.GRIDS["6x4"]
    mask = np.zeros((mbh, mbw), dtype=bool)
    mask[2, 3] = True
    for v in (2, 77, 32768):
        mv = np.zeros((mbh, mbw, 4), dtype=np.int16)
        mv[2, 3, 2] = -v
        for t in (v - 1, v, v + 1):
            if 1 <= t <= 32768:
                w = run(L, fw, fh, mbw, mbh, [(mv, np.ones((mbh, mbw), dtype=np.uint8))], None, [0], "mv %d at %d" % (v, t), mv_min=t)
                assert int(w[2][0]) == (1 if t <= v else 0)
    for v in (2, 300, 65535):
        c = P.cells_from(mask, 0, ac_min=v, top=True)
        c["ac_mag"][mask] = v
        c["ac_mag"][~mask] = 0
        for t in (v - 1, v, v + 1):
            if 1 <= t <= 65535:
                w = run(L, fw, fh, mbw, mbh, None, [c], [0], "ac %d at %d" % (v, t), ac_min=t)
                assert int(w[2][0]) == (1 if t <= v else 0)


def test_cells_outside_the_frame_are_ignored(L):
    """33 x 17 in a 4 x 3 grid: a grid column and a grid row wholly outside the frame, both with hot records"""
    mask = np.ones((3, 4), dtype=bool)
    w = run(L, 33, 17, 4, 3, [P.motion_from(mask, 1)], [P.cells_from(mask, 1)], [0], "33x17 in 4x3", mv_min=P.MV_MIN, ac_min=P.AC_MIN, intra=True)
    assert w[0][0][0].tolist() == [0, 0, 0, 33, 17, 0, 0, 0] and w[1][0][0].tolist() == [6, 0] and int(w[2][0]) == 1


@pytest.mark.parametrize("n", (1, 3, 4, 5, 9))
def test_request_counts_refused_requests_and_null_outputs(L, n):
    fw, fh, mbw, mbh = P.GRIDS["6x4"]
    masks = [P.random(0.4, seed=s)(mbw, mbh)[0] for s in range(3)]
    motion, activity = [P.motion_from(m, s) for s, m in enumerate(masks)], [P.cells_from(m, s + 5) for s, m in enumerate(masks)]
    frames = [1, 3, 0, -1, 1, 2, 2 ** 31 - 1, 2, -2 ** 31][:n]          # refused requests between valid ones, a frame named twice
    kw = dict(mv_min=P.MV_MIN, ac_min=P.AC_MIN, max_boxes=4)
    w = run(L, fw, fh, mbw, mbh, motion, activity, frames, "n %d" % n, **kw)
    assert [int(s) for s in w[3]] == [0 if 0 <= f < 3 else L.REGION_FRAME for f in frames]
    for q, f in enumerate(frames):
        if not 0 <= f < 3:
            assert (w[0][q] == FILL).all() and (w[1][q] == FILL).all() and w[2][q] == FILL
    run(L, fw, fh, mbw, mbh, motion, activity, frames, "n %d, no info" % n, with_info=False, **kw)
    run(L, fw, fh, mbw, mbh, motion, activity, frames, "n %d, no status" % n, with_status=False, **kw)
    # what lies behind request n - 1 keeps the sentinel
    run(L, fw, fh, mbw, mbh, motion, activity, frames + [0, 1], "n %d of %d" % (n, n + 2), n=n, **kw)
