"""CPU: boxes gauged against a frame's motion and activity records (include/leon_pipeline.h, leon_pipeline_gauge_regions) -- the
structs' sizes, the library's CPU evaluation of one record (leon_pipeline_gauge_record: the text k_gauge compiles too) against
leon_ctypes.gauge_box, the header's text in Python integers, on the records of tests/gauge_cases.py for each set of sources; word 0
= w * h; the whole-picture identity against the summaries motion_record and activity_record compute; every status word and their
order; refused records leave their words alone.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gauge_cases as G
from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


FILL = -7
FW, FH, MBW, MBH = 61, 45, 4, 3          # a frame smaller than its coded grid


def test_struct_sizes_and_symbols(L, tmp_path):
    assert C.sizeof(L.PipelineGaugeConfig) == 32 and L.PipelineGaugeConfig.reserved.offset == 4
    call = L.PipelineGaugeRegionsCall
    assert C.sizeof(call) == 64
    assert [getattr(call, f).offset for f in ("regions", "n", "reserved0", "device_stats", "device_status", "stream", "reserved")] == [0, 8, 12, 16, 24, 32, 40]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %zu %d %d\\n", sizeof(leon_pipeline_gauge_config), '
                   'sizeof(leon_pipeline_gauge_regions_call), sizeof(leon_pipeline_region), LEON_GAUGE_MOTION, LEON_GAUGE_ACTIVITY);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["32", "64", "32", "1", "2"]
    assert (L.GAUGE_MOTION, L.GAUGE_ACTIVITY, L.GAUGE_WORDS) == (1, 2, 16)
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for sym in ("leon_pipeline_gauge_record", "leon_pipeline_gauge_regions_device", "leon_pipeline_gauge_regions", "leon_pipeline_gauge_kernel"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym


def test_the_cases_hold_what_they_promise(L):
    motion, activity = G.window(MBW, MBH, 3)
    a = activity[0]
    assert (a["blocks"] == 0).any() and (a["qscale"][a["blocks"] == 0] == 0).all() and (a["ac_mag"] == 65535).any() and (a["ac_count"] == 65535).any()
    assert all((activity[2][k] == 65535).all() for k in ("ac_count", "ac_mag", "dc_mag"))
    mv, info = G.extreme(MBW, MBH)[0][0]
    assert (mv == -32768).all() and (info == 3).all()


def record_of(L, motion, activity, rec, sources, fw=FW, fh=FH, mbw=MBW, mbh=MBH):
    """(status, stats) of the library, asserted equal to gauge_box's, with FILL where nothing is written"""
    st, stats = L.gauge_record(fw, fh, mbw, mbh, G.N_FRAMES, motion, activity, rec, sources=sources, fill=FILL)
    want = G.expected(L, fw, fh, motion, activity, [rec], sources, FILL)
    G.assert_equal((stats[None], np.array([st])), want, [rec], "gauge_record, sources %d" % sources)
    return st, stats.tolist()


BOXES = [(0, 0, 61, 45), (0, 0, 1, 1), (60, 44, 1, 1), (60, 0, 1, 1), (0, 44, 1, 1), (16, 16, 16, 16), (15, 15, 2, 2), (15, 15, 18, 18), (1, 1, 16, 16), (47, 31, 10, 10),
         (33, 17, 9, 13), (0, 0, 48, 32)]


@pytest.mark.parametrize("sources", G.SOURCES)
def test_gauge_record_equals_gauge_box(L, sources):
    motion, activity = G.window(MBW, MBH, 3)
    rng = np.random.default_rng(sources)
    boxes = list(BOXES)
    for _ in range(30):
        x, y = int(rng.integers(0, FW)), int(rng.integers(0, FH))
        boxes.append((x, y, int(rng.integers(1, FW - x + 1)), int(rng.integers(1, FH - y + 1))))
    regions = G.on_every_frame(boxes)
    got = [record_of(L, motion, activity, r, sources) for r in regions]
    stats, status = np.array([s for _, s in got]), np.array([st for st, _ in got])
    assert (status == 0).all()
    G.assert_not_vacuous(stats, status, sources, "sources %d" % sources)
    # word 0 is the box's area, and a source that was not asked for reads 0
    assert stats[:, 0].tolist() == [w * h for (_, _, _, w, h) in regions]
    if not sources & L.GAUGE_ACTIVITY:
        assert (stats[:, 1:8] == 0).all()
    if not sources & L.GAUGE_MOTION:
        assert (stats[:, 8:16] == 0).all()


def test_the_largest_words(L):
    """4096 x 4096, every cell at 65535 and every vector -32768: 2^24 * 65535 and 2^24 * 32768, below 2^41"""
    motion, activity = G.extreme(256, 256)
    st, s = L.gauge_record(4096, 4096, 256, 256, 3, [None, motion[1], None], [None, activity[1], None], (1, 0, 0, 4096, 4096), sources=3, fill=FILL)
    area = 4096 * 4096
    assert st == 0 and s.tolist() == [area, area, area * 65535, area * 65535, area * 65535, area * 31, area * 6, 65535, area, area, 0, area] + [area * 32768] * 4
    assert max(s.tolist()) < 2 ** 41


@pytest.mark.parametrize("mbw,mbh", [(1, 1), (6, 4), (22, 15)])
def test_the_whole_picture_gives_256_times_the_summaries(L, mbw, mbh):
    """a frame of its coded size: the whole-frame box against the summaries the library's own record calls compute from maps and lists"""
    rng = np.random.default_rng(mbw)
    mbs = mbw * mbh
    repadd = rng.choice(np.array([0, 1, 200], dtype=np.uint8), size=mbs)
    mb_dir = rng.integers(0, 4, size=mbs).astype(np.uint8)
    mv_fwd, mv_bwd = rng.integers(-2048, 2049, size=2 * mbs).astype(np.int16), rng.integers(-2048, 2049, size=2 * mbs).astype(np.int16)
    mv, info, msum = L.motion_record(3, mbw, mbh, repadd=repadd, mb_dir=mb_dir, mv_fwd=mv_fwd, mv_bwd=mv_bwd)
    gy, gc, n_y, n_c = L.activity_groups(mbw, mbh)
    counts = rng.integers(0, 5, size=n_y + 2 * n_c)
    grp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    e = rng.integers(0, 2 ** 26, size=int(grp_off[-1])).astype(np.uint32)
    entries = (e & ~np.uint32(0xffff)) | (rng.integers(-300, 301, size=e.size).astype(np.int16).view(np.uint16).astype(np.uint32))
    cells, asum = L.activity_record(mbw, mbh, grp_off, entries, rng.integers(1, 32, size=mbs).astype(np.uint8))
    assert asum[0] > 0 and msum[:4].any()
    st, s = L.gauge_record(16 * mbw, 16 * mbh, mbw, mbh, 1, [(mv, info)], [cells], (0, 0, 0, 16 * mbw, 16 * mbh), sources=3)
    assert st == 0 and s[0] == 256 * mbs
    assert s[1:7].tolist() == [256 * int(asum[k]) for k in (0, 1, 2, 3, 5, 6)] and s[7] == int(asum[4])
    assert s[8:16].tolist() == [256 * int(v) for v in msum]


def test_status_words_in_their_order(L):
    motion, activity = G.window(MBW, MBH, 3)
    cases = [((0, 1, 1, 8, 8, 1, 0, 0), L.REGION_RESERVED), ((0, 1, 1, 8, 8, 0, -1, 0), L.REGION_RESERVED), ((0, 1, 1, 8, 8, 0, 0, 2 ** 31 - 1), L.REGION_RESERVED),
             ((9, 1, 1, 0, 8, 0, 5, 0), L.REGION_RESERVED),                    # the reserved word in front of the frame and the box
             ((3, 1, 1, 0, 8), L.REGION_FRAME), ((-1, 1, 1, 8, 8), L.REGION_FRAME), ((2 ** 31 - 1, 1, 1, 8, 8), L.REGION_FRAME),          # the frame in front of the box
             ((0, 1, 1, 0, 8), L.REGION_BOX), ((0, 1, 1, 8, 0), L.REGION_BOX), ((0, -1, 1, 8, 8), L.REGION_BOX), ((0, 1, -1, 8, 8), L.REGION_BOX),
             ((0, 54, 1, 8, 8), L.REGION_BOX), ((0, 1, 38, 8, 8), L.REGION_BOX), ((0, 0, 0, 62, 45), L.REGION_BOX), ((0, 0, 0, 61, 46), L.REGION_BOX),
             ((0, 2 ** 31 - 1, 1, 2 ** 31 - 1, 8), L.REGION_BOX), ((0, 62, 0, 1, 1), L.REGION_BOX), ((0, 1, 1, -2 ** 31, 8), L.REGION_BOX),
             ((0, 53, 37, 8, 8), L.REGION_OK), ((2, 0, 0, 61, 45), L.REGION_OK)]
    for sources in G.SOURCES:
        for rec, want in cases:
            st, stats = record_of(L, motion, activity, rec + (0,) * (8 - len(rec)), sources)
            assert st == want, (rec, st, want)
            if st:
                assert stats == [FILL] * 16, "a refused record was written: %s" % (rec,)


def test_record_pointers_and_refusals(L):
    motion, activity = G.window(MBW, MBH, 3)
    rec = (1, 1, 1, 8, 8)
    # NULL is allowed for the other frames, and for the array the sources do not ask for ...
    assert L.gauge_record(FW, FH, MBW, MBH, 3, [None, motion[1], None], [None, activity[1], None], rec, sources=3)[0] == 0
    assert L.gauge_record(FW, FH, MBW, MBH, 3, [None, motion[1], None], None, rec, sources=1)[0] == 0
    assert L.gauge_record(FW, FH, MBW, MBH, 3, None, [None, activity[1], None], rec, sources=2)[0] == 0
    # ... a refused record needs none at all ...
    assert L.gauge_record(FW, FH, MBW, MBH, 3, [None] * 3, [None] * 3, (0, 1, 1, 0, 8), sources=3)[0] == L.REGION_BOX
    # ... and the frame's own is needed
    for m, a, sources, word in (([None] * 3, activity, 3, "motion"), (motion, [None] * 3, 3, "activity"), (None, activity, 1, "null"), (motion, None, 2, "null")):
        with pytest.raises(L.LeonError) as e:
            L.gauge_record(FW, FH, MBW, MBH, 3, m, a, rec, sources=sources)
        assert e.value.code == L.ERR_INVALID and word in str(e.value)
    for sources in (0, 4, -1, 7):
        with pytest.raises(L.LeonError) as e:
            L.gauge_record(FW, FH, MBW, MBH, 3, motion, activity, rec, sources=sources)
        assert "sources" in str(e.value)
    for k in range(7):
        cfg = L.PipelineGaugeConfig(3)
        cfg.reserved[k] = 1
        with pytest.raises(L.LeonError) as e:
            L.gauge_record(FW, FH, MBW, MBH, 3, motion, activity, rec, cfg=cfg)
        assert "reserved" in str(e.value)
    for fw, fh, mbw, mbh in ((65, 45, 4, 3), (61, 49, 4, 3), (0, 45, 4, 3), (61, 45, 0, 3), (61, 45, 4, 257)):
        with pytest.raises(L.LeonError):
            L.gauge_record(fw, fh, mbw, mbh, 3, motion, activity, rec)
    assert L.load().leon_pipeline_gauge_record(FW, FH, MBW, MBH, 3, None, None, None, None, None) == L.ERR_INVALID
