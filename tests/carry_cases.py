"""Hand-written motion records and carry records for the tests of leon_pipeline_carry_regions (tests/test_pipeline_carry_abi.py on
the CPU, tests/test_carry_kernel_gpu.py on the device).  The oracle of both is leon_ctypes.carry_box: the header's text in Python
integers.  Every window here has three frames: frame 0 an I picture (no record votes for it), frame 1 a P picture that predicts from
frame 0 (fwd[1] = 0), frame 2 a closed GOP's leading B picture that names frame 0 for both directions (fwd[2] = bwd[2] = 0: D = 3).
Frame 1 to frame 2, and back, has no prediction between them."""
import numpy as np

FWD, BWD = [-1, 0, 0], [-1, -1, 0]
N_FRAMES = 3


def uniform(mbw, mbh, vec, info):
    """(mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8): the same vector quadruple and info byte in every macroblock"""
    mv = np.empty((mbh, mbw, 4), dtype=np.int16)
    mv[:, :] = np.asarray(vec, dtype=np.int16)
    return mv, np.full((mbh, mbw), info, dtype=np.uint8)


def varied(mbw, mbh, seed, limit=64):
    """a seeded record as k_motion writes them: info one of 1, 2, 3, 4, the vectors of a direction a macroblock does not use 0"""
    rng = np.random.default_rng(seed)
    info = rng.choice(np.array([1, 2, 3, 4], dtype=np.uint8), size=(mbh, mbw))
    mv = rng.integers(-limit, limit + 1, size=(mbh, mbw, 4)).astype(np.int16)
    mv[..., 0:2][(info & 1) == 0] = 0
    mv[..., 2:4][(info & 2) == 0] = 0
    return mv, info


def window(mbw, mbh, seed):
    """records of the three frames: the I picture's (all intra), a P picture's (forward or intra), a B picture's"""
    p_mv, p_info = varied(mbw, mbh, seed)
    p_info = np.where(p_info == 4, 4, 1).astype(np.uint8)
    p_mv[..., 2:4] = 0
    p_mv[..., 0:2][p_info == 4] = 0
    return [uniform(mbw, mbh, (0, 0, 0, 0), 4), (p_mv, p_info), varied(mbw, mbh, seed + 1)]


def pairs(boxes):
    """every box along every joined pair of the window, both senses: (frame, x, y, w, h, target)"""
    return [(s, x, y, w, h, t) for (x, y, w, h) in boxes for s, t in ((0, 1), (1, 0), (0, 2), (2, 0))]


def expected(L, fw, fh, records, regions, fill, fwd=FWD, bwd=BWD, n_frames=N_FRAMES):
    """(out [n, 8], votes [n, 4], status [n]) int32 by carry_box, `fill` where a refused record leaves its words alone"""
    n = len(regions)
    out, votes, status = np.full((n, 8), fill, dtype=np.int64), np.full((n, 4), fill, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i, r in enumerate(regions):
        rec = list(r) + [0] * (8 - len(r))
        st, o, v = L.carry_box(fw, fh, n_frames, fwd, bwd, records, rec)
        status[i] = st
        if st == 0:
            out[i], votes[i] = o, v
    return out, votes, status


def assert_equal(got, want, regions, what=""):
    for name, g, w in zip(("out", "votes", "status"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            i = int(np.argwhere(g != w)[0][0])
            raise AssertionError("%s: %s differs in %d records, first at %d (%s): %s, expected %s" % (
                what, name, len({int(b[0]) for b in np.argwhere(g != w)}), i, list(regions[i]), g[i].tolist(), w[i].tolist()))
