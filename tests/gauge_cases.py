"""Hand-written records and boxes for the tests of leon_pipeline_gauge_regions (tests/test_pipeline_gauge_abi.py on the CPU,
tests/test_gauge_kernel_gpu.py on the device).  The oracle of both is leon_ctypes.gauge_box: the header's text in Python integers.
Every window here has three frames.  Their motion records are carry_cases.window's (an I, a P and a B picture's); their activity
cells are seeded: frame 0 mixes cells that code nothing (blocks == 0, and qscale 0 there), cells at 65535 and ordinary ones, frame 1
is ordinary with a sprinkling of both extremes, frame 2 has EVERY cell at 65535 with all six blocks coded.  extreme() is the window
whose vectors are all -32768 on top of that."""
import numpy as np

import carry_cases as K

N_FRAMES = 3
SOURCES = (1, 2, 3)


def saturated(mbw, mbh):
    """every cell at 65535, all six blocks coded, qscale 31"""
    import leon_ctypes as L
    c = np.zeros((mbh, mbw), dtype=L.ACTIVITY_CELL)
    c["ac_count"], c["ac_mag"], c["dc_mag"], c["blocks"], c["qscale"] = 65535, 65535, 65535, 63, 31
    return c


def cells(mbw, mbh, seed, empty=0.3, full=0.2):
    """a seeded record as k_activity writes them: a share `empty` of the cells code nothing (all 0), a share `full` stand at 65535"""
    import leon_ctypes as L
    rng = np.random.default_rng(seed)
    c = np.zeros((mbh, mbw), dtype=L.ACTIVITY_CELL)
    kind = rng.random((mbh, mbw))
    for name in ("ac_count", "ac_mag", "dc_mag"):
        c[name] = rng.integers(0, 65536, size=(mbh, mbw))
        c[name][kind >= 1.0 - full] = 65535
    c["blocks"] = rng.integers(1, 64, size=(mbh, mbw))
    c["qscale"] = rng.integers(1, 32, size=(mbh, mbw))
    for name in c.dtype.names:
        c[name][kind < empty] = 0
    return c


def window(mbw, mbh, seed):
    """(motion, activity) of the three frames"""
    return K.window(mbw, mbh, seed), [cells(mbw, mbh, seed + 10), cells(mbw, mbh, seed + 11, empty=0.1, full=0.1), saturated(mbw, mbh)]


def extreme(mbw, mbh):
    """every vector word -32768 on every bidirectional macroblock, every cell at 65535: the largest words a grid can give"""
    return [K.uniform(mbw, mbh, (-32768,) * 4, 3)] * N_FRAMES, [saturated(mbw, mbh)] * N_FRAMES


def on_every_frame(boxes, n_frames=N_FRAMES):
    """every box on every frame of the window: (frame, x, y, w, h)"""
    return [(f, x, y, w, h) for (x, y, w, h) in boxes for f in range(n_frames)]


def expected(L, fw, fh, motion, activity, regions, sources, fill, n_frames=N_FRAMES):
    """(stats [n, 16], status [n]) by gauge_box as Python-integer arrays, `fill` where a refused record leaves its words alone"""
    n = len(regions)
    stats, status = np.full((n, 16), fill, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i, r in enumerate(regions):
        st, s = L.gauge_box(fw, fh, n_frames, motion, activity, list(r) + [0] * (8 - len(r)), sources)
        status[i] = st
        if st == 0:
            stats[i] = s
    return stats, status


def assert_equal(got, want, regions, what=""):
    for name, g, w in zip(("stats", "status"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            i = int(np.argwhere(g != w)[0][0])
            raise AssertionError("%s: %s differs in %d records, first at %d (%s): %s, expected %s" % (
                what, name, len({int(b[0]) for b in np.argwhere(g != w)}), i, list(regions[i]), g[i].tolist(), w[i].tolist()))


def assert_not_vacuous(stats, status, sources, what=""):
    """the expected statistics of the accepted records say something beyond word 0, in every word group the sources ask for"""
    ok = np.asarray(stats)[np.asarray(status) == 0]
    assert len(ok), what
    if sources & 2:
        assert (ok[:, 1:8] != 0).any(axis=0).all(), (what, "an activity word is 0 in every record")
    if sources & 1:
        assert (ok[:, 8:16] != 0).any(), (what, "every motion word is 0")
    assert (ok[:, 0] > 0).all(), what
