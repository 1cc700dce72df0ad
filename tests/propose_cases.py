"""Hand-made masks and records for the tests of leon_pipeline_propose_regions (tests/test_propose_cases.py on the CPU,
tests/test_propose_kernel_gpu.py on the device).  The oracle of both is leon_ctypes.propose_boxes: the header's text as a
breadth-first fill in Python integers.  A mask is a bool array [mbh, mbw] of the cells that are to be hot; MASKS builds the named
ones for a grid together with the number of components each is built to have under connectivity 4 and 8 (None where the grid is too
small for the figure to be said in a line).  motion_from / cells_from turn a mask into a seeded motion entry / activity record that
is hot exactly there at a given threshold: the hot cells stand AT the threshold or above it, the cold ones below."""
import numpy as np

MV_MIN, AC_MIN = 5, 300          # the thresholds of the records built here, unless a test asks for others
GRIDS = {                        # name: (frame width, frame height, mbw, mbh)
    "1x1": (16, 16, 1, 1),
    "2x2": (32, 32, 2, 2),
    "6x4": (96, 64, 6, 4),
    "22x15": (352, 240, 22, 15),
    "61x45 in 4x3": (61, 45, 4, 3),
    "256x2": (4096, 32, 256, 2),
    "2x256": (32, 4096, 2, 256),
    "120x68": (1920, 1080, 120, 68),
    "256x256": (4096, 4096, 256, 256),
}


def empty(mbw, mbh):
    return np.zeros((mbh, mbw), dtype=bool), 0, 0


def full(mbw, mbh):
    return np.ones((mbh, mbw), dtype=bool), 1, 1


def corners(mbw, mbh):
    m = np.zeros((mbh, mbw), dtype=bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    n = 4 if mbw >= 3 and mbh >= 3 else None
    return m, n, n


def checkerboard(mbw, mbh):
    j, i = np.mgrid[0:mbh, 0:mbw]
    m = (i + j) % 2 == 0
    alone = (mbw * mbh + 1) // 2
    return m, alone, 1 if min(mbw, mbh) >= 2 else alone


def serpentine(mbw, mbh):
    """every other row whole, joined by one cell at alternating ends: a path one cell wide through the whole grid"""
    m = np.zeros((mbh, mbw), dtype=bool)
    m[0::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m, 1, 1


def spiral(mbw, mbh):
    """a walker that keeps a cold cell between its arms: from the top left corner inwards, one cell wide"""
    m = np.zeros((mbh, mbw), dtype=bool)
    i, j, d = 0, 0, 0
    steps = [(1, 0), (0, 1), (-1, 0), (0, -1)]

    def free(a, b):
        return not (0 <= a < mbw and 0 <= b < mbh) or not m[b, a]

    m[0, 0] = True
    while True:
        for turn in (0, 1):
            di, dj = steps[(d + turn) % 4]
            a, b = i + di, j + dj
            if 0 <= a < mbw and 0 <= b < mbh and not m[b, a] and free(a + di, b + dj):
                i, j, d = a, b, (d + turn) % 4
                m[j, i] = True
                break
        else:
            return m, 1, 1


def comb(mbw, mbh):
    """teeth in every other column that join only in the last row"""
    m = np.zeros((mbh, mbw), dtype=bool)
    m[:, 0::2] = True
    m[-1] = True
    return m, 1, 1


def rings(mbw, mbh):
    """nested rings a cold cell apart: boxes that lie inside each other, components that do not touch"""
    j, i = np.mgrid[0:mbh, 0:mbw]
    d = np.minimum(np.minimum(i, mbw - 1 - i), np.minimum(j, mbh - 1 - j))
    n = ((min(mbw, mbh) - 1) // 2) // 2 + 1
    return d % 2 == 0, n, n


def diagonal(mbw, mbh):
    m = np.zeros((mbh, mbw), dtype=bool)
    k = np.arange(min(mbw, mbh))
    m[k, k] = True
    return m, len(k), 1


def row_end(mbw, mbh):
    """the last cell of the first row and the first of the second: neighbours in raster order, not in the grid"""
    m = np.zeros((mbh, mbw), dtype=bool)
    m[0, -1] = True
    if mbh > 1:
        m[1, 0] = True
    n = 2 if mbw >= 3 and mbh >= 2 else None
    return m, n, n


def random(density, seed=7):
    def build(mbw, mbh):
        return np.random.default_rng(seed + mbw * 1000 + mbh).random((mbh, mbw)) < density, None, None
    return build


MASKS = {"empty": empty, "full": full, "corners": corners, "checkerboard": checkerboard, "serpentine": serpentine, "spiral": spiral, "comb": comb, "rings": rings,
         "diagonal": diagonal, "row end": row_end, "random 0.1": random(0.1), "random 0.5": random(0.5), "random 0.6": random(0.6), "random 0.9": random(0.9)}


def every_mask(mbw, mbh):
    """all 2^(mbw * mbh) masks of a small grid, [n, mbh, mbw]: bit k of the mask's number is raster cell k"""
    n = mbw * mbh
    return ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(bool).reshape(-1, mbh, mbw)


def motion_from(mask, seed, mv_min=MV_MIN, intra=None, extreme=False):
    """(mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8): a hot cell has one word of magnitude mv_min exactly (every fourth cell: a
    larger one; extreme: -32768) in a seeded place and sign, every other word of every cell lies below mv_min; info is seeded from
    1 .. 3, and 4 where `intra` (a mask) says so"""
    rng = np.random.default_rng(seed)
    mbh, mbw = mask.shape
    mv = rng.integers(-(mv_min - 1), mv_min, size=(mbh, mbw, 4)).astype(np.int64)
    at = rng.integers(0, 4, size=(mbh, mbw))
    big = np.where(rng.integers(0, 4, size=(mbh, mbw)) == 0, np.minimum(mv_min + rng.integers(0, 4000, size=(mbh, mbw)), 32767), mv_min)
    big = np.where(rng.integers(0, 2, size=(mbh, mbw)) == 0, -big, np.minimum(big, 32767))
    if extreme:
        big[:] = -32768
    jj, ii = np.nonzero(mask)
    mv[jj, ii, at[jj, ii]] = big[jj, ii]
    info = rng.integers(1, 4, size=(mbh, mbw)).astype(np.uint8)
    if intra is not None:
        info[intra] = 4
    return mv.astype(np.int16), info


def cells_from(mask, seed, ac_min=AC_MIN, top=False):
    """cells [mbh, mbw] of ACTIVITY_CELL: ac_mag is ac_min exactly at every other hot cell and above it at the rest (top: 65535), below
    ac_min at the cold ones; the other fields are seeded and say nothing"""
    import leon_ctypes as L
    rng = np.random.default_rng(seed)
    mbh, mbw = mask.shape
    c = np.zeros((mbh, mbw), dtype=L.ACTIVITY_CELL)
    for name in ("ac_count", "dc_mag"):
        c[name] = rng.integers(0, 65536, size=(mbh, mbw))
    c["blocks"] = rng.integers(0, 64, size=(mbh, mbw))
    c["qscale"] = rng.integers(0, 32, size=(mbh, mbw))
    hot = np.where(rng.integers(0, 2, size=(mbh, mbw)) == 0, ac_min, rng.integers(ac_min, 65536, size=(mbh, mbw)))
    if top:
        hot[:] = 65535
    c["ac_mag"] = np.where(mask, hot, rng.integers(0, ac_min, size=(mbh, mbw)))
    return c


def hot_cells(L, fw, fh, motion, cells, mv_min=None, ac_min=None, intra=False):
    """the hot mask straight from the arrays, for the tests that count cells: the header's three terms and the frame's edge"""
    hot = None
    if mv_min is not None:
        mv, info = motion
        hot = np.abs(np.asarray(mv).astype(np.int64)).max(axis=2) >= mv_min
        if intra:
            hot = hot | ((np.asarray(info) & 4) != 0)
    if ac_min is not None:
        a = np.asarray(cells)["ac_mag"].astype(np.int64) >= ac_min
        hot = a if hot is None else hot | a
    mbh, mbw = hot.shape
    return hot & (16 * np.arange(mbw)[None, :] < fw) & (16 * np.arange(mbh)[:, None] < fh)


def expected(L, fw, fh, motion, activity, frames, fill, **kw):
    """(regions [n, K, 8], info [n, K, 2], count [n], status [n]) by propose_boxes, `fill` where a refused request leaves its words"""
    n, K = len(frames), kw.get("max_boxes", 16)
    n_frames = max(len(motion) if motion is not None else 0, len(activity) if activity is not None else 0)
    regions, info = np.full((n, K, 8), fill, dtype=np.int64), np.full((n, K, 2), fill, dtype=np.int64)
    count, status = np.full(n, fill, dtype=np.int64), np.zeros(n, dtype=np.int64)
    memo = {}
    for q, f in enumerate(frames):
        if f not in memo:
            memo[f] = L.propose_boxes(fw, fh, n_frames, motion, activity, f, **kw)
        st, r, i, c = memo[f]
        status[q] = st
        if st == 0:
            regions[q], info[q], count[q] = r, i, c
    return regions, info, count, status


def assert_equal(got, want, what=""):
    for name, g, w in zip(("regions", "info", "count", "status"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(v) for v in np.argwhere(g != w)[0])
            raise AssertionError("%s: %s differs in %d requests, first at %s: %s, expected %s" % (
                what, name, len({int(b[0]) for b in np.argwhere(g != w)}), at, g[at[:-1]].tolist() if len(at) > 1 else g[at], w[at[:-1]].tolist() if len(at) > 1 else w[at]))
