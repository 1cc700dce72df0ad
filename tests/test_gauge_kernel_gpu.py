"""GPU: k_gauge through leon_pipeline_gauge_kernel (include/leon_pipeline.h) on hand-written motion and activity records
(tests/gauge_cases.py), against leon_ctypes.gauge_box, the header's text in Python integers, for sources 1, 2 and 3: statistics and
status compared exactly, and what the kernel is to leave alone still holding the sentinel.  The grids are 1 x 1, 2 x 2, 6 x 4 and
22 x 15 macroblocks, a 61 x 45 frame in a 4 x 3 grid, 256 x 2 (4096 wide) and one 256 x 256 grid with every value at its extreme; the
boxes the ones at which the wave's walk over the covered macroblocks can go wrong -- one pixel at each corner, exactly one
macroblock, four macroblocks straddled by one pixel each, the whole frame, covers of 63, 64, 65 and 129 macroblocks around the
64-lane stride; the record counts the ones at which the four-records-a-workgroup grid can: 1, 3, 4, 5, 9, and refused records of each
status between valid ones."""
import numpy as np
import pytest

import gauge_cases as G

pytestmark = pytest.mark.gpu

FILL = -77


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def run(L, fw, fh, mbw, mbh, motion, activity, regions, sources, n=None, what="", want=None):
    got = L.gauge_kernel(fw, fh, mbw, mbh, G.N_FRAMES, motion, activity, regions, sources=sources, fill=FILL, n=n)
    count = len(regions) if n is None else n
    want = G.expected(L, fw, fh, motion, activity, regions[:count], sources, FILL) if want is None else want
    G.assert_equal([g[:count] for g in got], want, regions, "%s, sources %d" % (what, sources))
    for name, g in zip(("stats", "status"), got):
        assert (g[count:] == FILL).all(), "%s: %s was written behind record %d" % (what, name, count - 1)
    return got, want


def covered(box):
    x, y, w, h = box
    return ((x + w - 1) // 16 - x // 16 + 1), ((y + h - 1) // 16 - y // 16 + 1)


def common_boxes(fw, fh):
    """one pixel at each corner, exactly one macroblock, the whole frame, and -- where the frame has them -- four macroblocks
    straddled by one pixel each"""
    boxes = [(0, 0, 1, 1), (fw - 1, 0, 1, 1), (0, fh - 1, 1, 1), (fw - 1, fh - 1, 1, 1), (0, 0, min(16, fw), min(16, fh)), (0, 0, fw, fh)]
    if fw > 16 and fh > 16:
        boxes.append((15, 15, 2, 2))
        assert covered(boxes[-1]) == (2, 2)
    return boxes


# (frame, grid, the boxes beyond common_boxes with the macroblocks each is to cover)
GRIDS = {
    "1x1": (16, 16, 1, 1, []),
    "2x2": (32, 32, 2, 2, [((1, 1, 30, 30), 4)]),
    "6x4": (96, 64, 6, 4, [((16, 16, 16, 16), 1), ((31, 15, 34, 18), 12)]),
    "22x15": (352, 240, 22, 15, [((3, 5, 140, 106), 63), ((0, 0, 128, 128), 64), ((15, 15, 98, 98), 64), ((8, 8, 200, 72), 65), ((144, 160, 208, 80), 65), ((47, 31, 280, 120), 171)]),
    "61x45 in 4x3": (61, 45, 4, 3, [((60, 0, 1, 45), 3), ((0, 44, 61, 1), 4), ((45, 30, 16, 15), 4), ((47, 31, 10, 10), 4)]),
    "256x2": (4096, 32, 256, 2, [((16, 0, 1008, 16), 63), ((5, 3, 1019, 13), 64), ((3072, 16, 1024, 16), 64), ((1, 17, 1030, 9), 65), ((2000, 0, 2049, 16), 129),
                                 ((31, 15, 1026, 2), 132)]),
}


@pytest.mark.parametrize("sources", G.SOURCES)
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_boxes_of_a_grid(L, name, sources):
    fw, fh, mbw, mbh, extra = GRIDS[name]
    for box, mbs in extra:
        c = covered(box)
        assert c[0] * c[1] == mbs, (box, c)
    motion, activity = G.window(mbw, mbh, 31 + mbw)
    regions = G.on_every_frame(common_boxes(fw, fh) + [b for b, _ in extra])
    (stats, status), want = run(L, fw, fh, mbw, mbh, motion, activity, regions, sources, what=name)
    assert (status == 0).all() and stats[:, 0].tolist() == [w * h for (_, _, _, w, h) in regions]
    G.assert_not_vacuous(want[0], want[1], sources, name)


@pytest.mark.parametrize("sources", G.SOURCES)
def test_words_near_2_to_the_40(L, sources):
    """4096 x 4096, the whole frame, every cell at 65535 and every vector -32768: 2^24 * 65535 in words 2, 3, 4, 2^39 in words 12 .. 15"""
    motion, activity = G.extreme(256, 256)
    regions = [(1, 0, 0, 4096, 4096), (3, 0, 0, 4096, 4096), (1, 1, 1, 4094, 4094)]
    (stats, status), want = run(L, 4096, 4096, 256, 256, [None, motion[1], None], [None, activity[1], None], regions, sources, what="2^40")
    assert status.tolist() == [0, L.REGION_FRAME, 0]
    s = want[0][0].tolist()
    assert s[0] == 2 ** 24
    if sources & 2:
        assert s[1] == 2 ** 24 and s[2] == s[3] == s[4] == 2 ** 24 * 65535 and s[5:8] == [2 ** 24 * 31, 2 ** 24 * 6, 65535]
    if sources & 1:
        assert s[8:12] == [2 ** 24, 2 ** 24, 0, 2 ** 24] and s[12:] == [2 ** 39] * 4


@pytest.mark.parametrize("sources", G.SOURCES)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_record_counts(L, n, sources):
    fw, fh, mbw, mbh = 224, 160, 14, 10
    motion, activity = G.window(mbw, mbh, 35)
    rng = np.random.default_rng(n)
    regions = []
    for i in range(n + 3):
        x, y = int(rng.integers(0, fw)), int(rng.integers(0, fh))
        regions.append((i % 3, x, y, int(rng.integers(1, fw - x + 1)), int(rng.integers(1, fh - y + 1))))
    (stats, status), want = run(L, fw, fh, mbw, mbh, motion, activity, regions, sources, n=n, what="n = %d" % n)
    assert (status[:n] == 0).all()
    assert (want[0][:, 1:] != 0).any()


@pytest.mark.parametrize("sources", G.SOURCES)
def test_refused_records_between_valid_ones(L, sources):
    fw, fh, mbw, mbh = 224, 160, 14, 10
    motion, activity = G.window(mbw, mbh, 37)
    good = G.on_every_frame([(10, 10, 50, 40), (100, 80, 124, 80), (0, 0, 224, 160)])
    bad = [(0, 1, 1, 8, 8, 1, 0, 0), (0, 1, 1, 8, 8, 0, 1, 0), (0, 1, 1, 8, 8, 0, 0, 1), (3, 1, 1, 8, 8), (-1, 1, 1, 8, 8), (0, 220, 1, 8, 8), (0, 1, 1, 0, 8), (0, 1, 158, 8, 8),
           (9, 1, 1, 0, 8, 0, 4, 0)]
    regions = []
    for i, g in enumerate(good):
        regions.append(g + (0, 0, 0))
        regions.append(bad[i] + (0,) * (8 - len(bad[i])))
    n = len(regions)
    (stats, status), want = run(L, fw, fh, mbw, mbh, motion, activity, regions + [good[0] + (0, 0, 0)] * 3, sources, n=n, what="refused between valid")
    R, F, B = L.REGION_RESERVED, L.REGION_FRAME, L.REGION_BOX
    assert status[:n].tolist() == [0, R, 0, R, 0, R, 0, F, 0, F, 0, B, 0, B, 0, B, 0, R]
    assert (stats[1:n:2] == FILL).all() and (stats[0:n:2, 0] > 0).all()
    G.assert_not_vacuous(want[0], want[1], sources, "refused between valid")


@pytest.mark.parametrize("sources", G.SOURCES)
def test_a_window_of_no_frames(L, sources):
    """n_frames = 0 is a call the header admits: every record names a frame that is not there, and nothing of the window is read"""
    motion, activity = G.window(6, 4, 41)
    stats, status = L.gauge_kernel(96, 64, 6, 4, 0, motion, activity, [(0, 1, 1, 8, 8), (1, 1, 1, 8, 8)], sources=sources, fill=FILL)
    assert status.tolist() == [L.REGION_FRAME] * 2 and (stats == FILL).all()


@pytest.mark.parametrize("sources", G.SOURCES)
def test_only_the_records_that_are_read_are_there(L, sources):
    """one macroblock, and a window whose other frames have no record: each ring has one slot, which is not the frame's index"""
    motion, activity = G.window(1, 1, 43)
    (stats, status), want = run(L, 16, 16, 1, 1, [None, motion[1], None], [None, activity[1], None], [(1, 0, 0, 16, 16), (1, 3, 4, 5, 6)], sources, what="one record")
    assert (status == 0).all() and stats[:, 0].tolist() == [256, 30]


@pytest.mark.parametrize("sources", G.SOURCES)
def test_without_a_status(L, sources):
    """status may be NULL, through the library itself: the statistics are those of the call with it"""
    fw, fh, mbw, mbh = 224, 160, 14, 10
    motion, activity = G.window(mbw, mbh, 45)
    regions = G.on_every_frame(common_boxes(fw, fh)) + [(3, 1, 1, 8, 8)]
    want, want_status = L.gauge_kernel(fw, fh, mbw, mbh, G.N_FRAMES, motion, activity, regions, sources=sources, fill=FILL)
    assert (want_status[:-1] == 0).all() and want_status[-1] == L.REGION_FRAME
    mp, ap, keep = L._gauge_records(motion, activity, mbw, mbh, G.N_FRAMES)
    r, stats, cfg = L._records_array(regions), np.full_like(want, FILL), L.PipelineGaugeConfig(sources)
    rc = L.load().leon_pipeline_gauge_kernel(0, fw, fh, mbw, mbh, G.N_FRAMES, mp, ap, L.C.byref(cfg), r.ctypes.data, len(r), stats.ctypes.data, None)
    assert rc == L.OK, L.load().leon_last_error()
    assert np.array_equal(stats, want)


def test_call_refusals(L):
    fw, fh, mbw, mbh = 224, 160, 14, 10
    motion, activity = G.window(mbw, mbh, 39)
    ok = [(1, 1, 1, 8, 8)]
    for kw in (dict(n=0), dict(n=65536), dict(sources=0), dict(sources=4)):
        with pytest.raises(L.LeonError):
            L.gauge_kernel(fw, fh, mbw, mbh, 3, motion, activity, ok, **kw)
    cfg = L.PipelineGaugeConfig(3)
    cfg.reserved[6] = 1
    with pytest.raises(L.LeonError):
        L.gauge_kernel(fw, fh, mbw, mbh, 3, motion, activity, ok, cfg=cfg)
    with pytest.raises(L.LeonError):          # a frame larger than the grid
        L.gauge_kernel(fw + 1, fh, mbw, mbh, 3, motion, activity, ok)
    # a valid record that names a frame without the record it needs; a refused record needs none
    for m, a, sources in (([motion[0], None, motion[2]], activity, 1), (motion, [activity[0], None, activity[2]], 2), (motion, [activity[0], None, activity[2]], 3)):
        with pytest.raises(L.LeonError) as e:
            L.gauge_kernel(fw, fh, mbw, mbh, 3, m, a, ok, sources=sources)
        assert "no" in str(e.value) and "record" in str(e.value)
    stats, status = L.gauge_kernel(fw, fh, mbw, mbh, 3, [motion[0], None, None], [activity[0], None, None], [(0, 1, 1, 8, 8, 0, 0, 0), (1, 1, 1, 0, 8, 0, 0, 0), (2, 1, 1, 8, 8, 0, 0, 3)], fill=FILL)
    assert status.tolist() == [0, L.REGION_BOX, L.REGION_RESERVED] and stats[0, 0] == 64 and (stats[1:] == FILL).all()
