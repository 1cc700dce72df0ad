"""GPU: k_carry through leon_pipeline_carry_device (include/leon_pipeline.h) on hand-written motion records (tests/carry_cases.py),
against leon_ctypes.carry_box, the header's text in Python integers: out, votes and status compared exactly, and what the kernel is to
leave alone still holding the sentinel.  The boxes are the ones at which the wave's walk over the covered macroblocks can go wrong --
one macroblock, box edges on macroblock borders, a last pixel that is the first of a macroblock, exactly one trip of 64 lanes, a
second trip with one live lane, a rectangle whose row length divides no trip, the whole frame, the edges of a frame smaller than its
grid -- the record counts the ones at which the four-waves-a-workgroup grid can: 1, 4, 5 (a second workgroup with three idle waves),
259, and refused records between valid ones."""
import numpy as np
import pytest

import carry_cases as K

pytestmark = pytest.mark.gpu

FILL = -77


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def run(L, fw, fh, mbw, mbh, records, regions, n=None, what=""):
    got = L.carry_device(fw, fh, mbw, mbh, K.N_FRAMES, K.FWD, K.BWD, records, regions, fill=FILL, n=n)
    count = len(regions) if n is None else n
    want = K.expected(L, fw, fh, records, regions[:count], FILL)
    K.assert_equal([g[:count] for g in got], want, regions, what)
    for name, g in zip(("out", "votes", "status"), got):
        assert (g[count:] == FILL).all(), "%s: %s was written behind record %d" % (what, name, count - 1)
    return got


FW, FH, MBW, MBH = 224, 160, 14, 10
BOXES = {
    "1x1": [(0, 0, 1, 1), (223, 159, 1, 1), (16, 32, 1, 1), (15, 31, 1, 1)],
    "inside one macroblock": [(33, 17, 9, 13), (17, 17, 15, 15), (32, 16, 16, 16)],
    "edges on macroblock borders": [(16, 32, 48, 16), (0, 0, 32, 32), (160, 128, 32, 32), (64, 16, 16, 96)],
    "last pixel the first of a macroblock": [(5, 7, 12, 10), (16, 16, 17, 17), (30, 3, 35, 62)],
    "64 macroblocks": [(0, 0, 128, 128), (3, 5, 120, 122), (15, 15, 98, 98)],
    "65 macroblocks": [(0, 0, 208, 80), (8, 8, 200, 72)],
    "8 x 9 macroblocks": [(16, 0, 128, 144), (20, 9, 120, 130)],
    "the whole frame": [(0, 0, 224, 160)],
}


def covered(box):
    x, y, w, h = box
    return ((x + w - 1) // 16 - x // 16 + 1), ((y + h - 1) // 16 - y // 16 + 1)


# what a name promises of its boxes
IS = {
    "1x1": lambda b: b[2:] == (1, 1),
    "inside one macroblock": lambda b: covered(b) == (1, 1),
    "edges on macroblock borders": lambda b: all(v % 16 == 0 for v in b),
    "last pixel the first of a macroblock": lambda b: (b[0] + b[2] - 1) % 16 == 0 and (b[1] + b[3] - 1) % 16 == 0,
    "64 macroblocks": lambda b: covered(b) == (8, 8),
    "65 macroblocks": lambda b: covered(b) == (13, 5),
    "8 x 9 macroblocks": lambda b: covered(b) == (8, 9),
    "the whole frame": lambda b: b == (0, 0, FW, FH),
}


@pytest.mark.parametrize("name", sorted(BOXES))
def test_boxes(L, name):
    assert all(IS[name](b) for b in BOXES[name])
    records = K.window(MBW, MBH, 31)
    regions = K.pairs(BOXES[name])
    out, votes, status = run(L, FW, FH, MBW, MBH, records, regions, what=name)
    assert (status == 0).all()
    assert (votes[:, 0] > 0).any() and (votes[:, 2:] != 0).any()


def test_frame_smaller_than_its_grid(L):
    """61 x 45 in 64 x 48: boxes on the right and bottom edges, and the clamp against the FRAME's edges"""
    records = K.window(4, 3, 33)
    records[1] = K.uniform(4, 3, (-60, -50, 0, 0), 1)
    boxes = [(60, 0, 1, 45), (0, 44, 61, 1), (45, 30, 16, 15), (60, 44, 1, 1), (0, 0, 61, 45), (47, 31, 10, 10)]
    out, votes, status = run(L, 61, 45, 4, 3, records, K.pairs(boxes), what="61 x 45")
    assert (status == 0).all()
    at = K.pairs(boxes).index((0, 47, 31, 10, 10, 1))
    assert out[at].tolist() == [1, 51, 35, 10, 10, 0, 0, 0] and votes[at].tolist() == [100, 0, 30, 25]          # (47 + 30, 31 + 25) clamped to (61 - 10, 45 - 10)


@pytest.mark.parametrize("n", [1, 4, 5, 259])
def test_record_counts(L, n):
    records = K.window(MBW, MBH, 35)
    rng = np.random.default_rng(n)
    regions = []
    for i in range(n + 3):
        x, y = int(rng.integers(0, FW)), int(rng.integers(0, FH))
        s, t = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 1))[i % 5]
        regions.append((s, x, y, int(rng.integers(1, FW - x + 1)), int(rng.integers(1, FH - y + 1)), t))
    out, votes, status = run(L, FW, FH, MBW, MBH, records, regions, n=n, what="n = %d" % n)
    assert (status[:n] == 0).all()


def test_refused_records_between_valid_ones(L):
    records = K.window(MBW, MBH, 37)
    good = K.pairs([(10, 10, 50, 40), (100, 80, 124, 80)])
    bad = [(0, 1, 1, 8, 8, 1, 1, 0), (3, 1, 1, 8, 8, 1), (0, 1, 1, 8, 8, -1), (0, 220, 1, 8, 8, 1), (0, 1, 1, 0, 8, 1), (1, 1, 1, 8, 8, 2), (2, 1, 1, 8, 8, 1),
           (9, 1, 1, 0, 8, 1, 0, 4)]
    regions = []
    for i, g in enumerate(good):
        regions.append(g + (0, 0))
        regions.append(bad[i] + (0,) * (8 - len(bad[i])))
    n = len(regions)
    out, votes, status = run(L, FW, FH, MBW, MBH, records, regions + [good[0] + (0, 0)] * 3, n=n, what="refused between valid")
    assert status[:n].tolist() == [0, L.REGION_RESERVED, 0, L.REGION_FRAME, 0, L.REGION_FRAME, 0, L.REGION_BOX, 0, L.REGION_BOX, 0, L.REGION_NO_REFERENCE,
                                   0, L.REGION_NO_REFERENCE, 0, L.REGION_RESERVED]
    assert (out[1:n:2] == FILL).all() and (votes[1:n:2] == FILL).all() and (out[0:n:2, 0] != FILL).all()


@pytest.mark.parametrize("v,minus,plus", [(1, 0, 1), (-1, 1, 0), (3, -1, 2), (-3, 2, -1), (-2, 1, -1), (2, -1, 1)])
def test_ties_on_the_device(L, v, minus, plus):
    records = [None, K.uniform(MBW, MBH, (v, -v, 0, 0), 1), K.uniform(MBW, MBH, (v, v, -v, -v), 1 | 2)]
    regions = [(0, 40, 30, 70, 70, 1), (1, 40, 30, 70, 70, 0), (0, 40, 30, 7, 3, 1), (1, 40, 30, 7, 3, 0), (0, 40, 30, 70, 70, 2)]
    out, votes, status = run(L, FW, FH, MBW, MBH, records, regions, what="ties")
    assert votes[:, 2:].tolist() == [[minus, plus], [plus, minus], [minus, plus], [plus, minus], [0, 0]] and (status == 0).all()


def test_sums_near_2_to_the_40(L):
    """4096 x 4096, the whole frame, every vector -32768 and every macroblock bidirectional under D = 3: |SH| = |SV| = 2^40, A = 2^25"""
    records = [None, None, K.uniform(256, 256, (-32768,) * 4, 3)]
    regions = [(0, 0, 0, 4096, 4096, 2), (2, 0, 0, 4096, 4096, 0), (0, 1, 1, 4094, 4094, 2)]
    out, votes, status = run(L, 4096, 4096, 256, 256, records, regions, what="2^40")
    assert votes[0].tolist() == [2 ** 25, 0, 16384, 16384] and votes[1].tolist() == [2 ** 25, 0, -16384, -16384] and (status == 0).all()
    assert out[0].tolist() == [2, 0, 0, 4096, 4096, 0, 0, 0] and out[2].tolist() == [2, 2, 2, 4094, 4094, 0, 0, 0]


def test_a_window_of_no_frames(L):
    """n_frames = 0 is a call the header admits: every record names a frame that is not there, and nothing of the window is read"""
    out, votes, status = L.carry_device(FW, FH, MBW, MBH, 0, K.FWD, K.BWD, K.window(MBW, MBH, 41), [(0, 1, 1, 8, 8, 1), (1, 1, 1, 8, 8, 0)], fill=FILL)
    assert status.tolist() == [L.REGION_FRAME] * 2 and (out == FILL).all() and (votes == FILL).all()


def test_only_the_record_that_votes_is_there(L):
    """one macroblock, and a window whose other frames have no record: the ring has one slot, which is not the frame's index"""
    records = [None, K.uniform(1, 1, (6, -4, 0, 0), 1), None]
    out, votes, status = run(L, 16, 16, 1, 1, records, [(0, 2, 3, 9, 8, 1), (1, 2, 3, 9, 8, 0), (0, 0, 0, 16, 16, 1)], what="one record")
    assert (status == 0).all() and (votes[:, 2:] != 0).all()


@pytest.mark.parametrize("votes,status", [(False, True), (True, False), (False, False)])
def test_without_the_optional_outputs(L, votes, status):
    """votes and status may be NULL, through the library itself: what is asked for is what the call with everything gives"""
    records, regions = K.window(MBW, MBH, 43), K.pairs(BOXES["8 x 9 macroblocks"]) + [(3, 1, 1, 8, 8, 1)]
    want = L.carry_device(FW, FH, MBW, MBH, K.N_FRAMES, K.FWD, K.BWD, records, regions, fill=FILL)
    assert (want[2][:-1] == 0).all() and want[2][-1] == L.REGION_FRAME
    ptrs, keep = L._carry_records(records, MBW, MBH)
    f, b, r = np.array(K.FWD, dtype=np.int32), np.array(K.BWD, dtype=np.int32), L._records_array(regions)
    got = [np.full_like(w, FILL) for w in want]
    rc = L.load().leon_pipeline_carry_device(0, FW, FH, MBW, MBH, K.N_FRAMES, f.ctypes.data, b.ctypes.data, ptrs, r.ctypes.data, len(r), got[0].ctypes.data,
                                             got[1].ctypes.data if votes else None, got[2].ctypes.data if status else None)
    assert rc == L.OK, L.load().leon_last_error()
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]) if votes else (got[1] == FILL).all()
    assert np.array_equal(got[2], want[2]) if status else (got[2] == FILL).all()


def test_call_refusals(L):
    records = K.window(MBW, MBH, 39)
    for kw in (dict(n=0), dict(n=65536)):
        with pytest.raises(L.LeonError):
            L.carry_device(FW, FH, MBW, MBH, 3, K.FWD, K.BWD, records, [(0, 1, 1, 8, 8, 1)], **kw)
    with pytest.raises(L.LeonError):          # a frame larger than the grid
        L.carry_device(FW + 1, FH, MBW, MBH, 3, K.FWD, K.BWD, records, [(0, 1, 1, 8, 8, 1)])
    with pytest.raises(L.LeonError):          # a reference outside the window
        L.carry_device(FW, FH, MBW, MBH, 3, [-1, 3, 0], K.BWD, records, [(0, 1, 1, 8, 8, 1)])
    with pytest.raises(L.LeonError):          # the record that votes is missing
        L.carry_device(FW, FH, MBW, MBH, 3, K.FWD, K.BWD, [records[0], None, records[2]], [(0, 1, 1, 8, 8, 1)])
