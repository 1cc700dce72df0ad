"""Maps, shapes and the expected records for the tests of k_motion on maps of the test's own choosing (tests/test_motion_cases.py on the
CPU, tests/test_motion_kernel_gpu.py through leon_pipeline_motion_kernel on the device).  The oracle is leon_ctypes.motion_from_maps:
the header's text in numpy, independent of the C code.

k_motion (csrc/leon_kernels.h) walks a picture with 256 lanes, four consecutive macroblocks per lane and trip: a trip covers 1024
macroblocks, a wave 256.  SHAPES are (mbw, mbh) chosen by mbs = mbw * mbh; both factors are at most 256, so a count without such a
factoring is replaced by the nearest one that has it, with the same mbs % 4 and on the same side of the boundary it stands at."""
import numpy as np

from record_cases import SENTINEL, permutation  # noqa: F401  (K.SENTINEL, K.permutation in the tests)

LANES, PER_LANE = 256, 4
TRIP = LANES * PER_LANE          # macroblocks per trip of the loop

SHAPES = [
    (1, 1), (2, 1), (3, 1), (4, 1), (5, 1),      # 1 .. 5: lanes 0 and 1 of one wave
    (17, 15),                                    # 255: the first wave's last lane, three of its four
    (16, 16),                                    # 256: the first wave full
    (29, 9),                                     # 261 for 257 (prime): the second wave's first lane full, its second lane holds one
    (33, 31),                                    # 1023: the end of one trip, the last lane holds three
    (32, 32),                                    # 1024: one full trip
    (41, 25),                                    # 1025: a second trip with one lane that holds one macroblock
    (24, 43),                                    # 1032 for 1028 (4 x 257): a second trip of full lanes only (two of them)
    (121, 17),                                   # 2057 for 2049 (3 x 683; 2053 is prime): a third trip, its last lane holds one
    (120, 68),                                   # 8160: the 1080p grid, eight trips
    (256, 256),                                  # 65536: 64 full trips, the largest picture
]
SMALL = [s for s in SHAPES if s[0] * s[1] <= 2057]          # the shapes that run with both padding bytes

REPADD = (0, 1, 127, 128, 255)
EDGES = (0, 1, -1, 2047, -2047, 2048, -2048)


def trips(mbs):
    return -(-mbs // TRIP)


def last_trip_lanes(mbs):
    """lanes that hold a macroblock in the loop's last trip"""
    return -(-(mbs - TRIP * (trips(mbs) - 1)) // PER_LANE)


def ceil4(v):
    return (v + 3) // 4 * 4


def _vectors(rng, mbs, with_min):
    """int16 [mbs, 2]: spread over the whole range, two in five at an edge value (-32768 only where asked)"""
    v = rng.integers(-32767, 32768, size=(mbs, 2)).astype(np.int16)
    edges = np.array(EDGES + ((-32768,) if with_min else ()), dtype=np.int16)
    at = rng.random((mbs, 2)) < 0.4
    v[at] = rng.choice(edges, size=int(at.sum()))
    return v


def maps(mbw, mbh, type, seed, with_min=False):
    """(repadd, mb_dir, mv_fwd, mv_bwd) of a picture of `type`, None where the type has no such map: repadd from REPADD, mb_dir any
    byte, vectors from _vectors; a vector map is never zero at a macroblock that does not use it (intra, or its direction bit clear)"""
    mbs = mbw * mbh
    if type == 1:
        return None, None, None, None
    rng = np.random.default_rng([seed, mbw, mbh, type])
    repadd = rng.choice(np.array(REPADD, dtype=np.uint8), size=mbs)
    mb_dir = rng.integers(0, 256, size=mbs).astype(np.uint8) if type == 3 else None
    d = np.where(repadd >= 128, 0, 1 if type == 2 else mb_dir & 3)
    fwd = _vectors(rng, mbs, with_min)
    fwd[((d & 1) == 0) & ~fwd.any(axis=1)] = (1234, -4321)
    if type == 2:
        return repadd, None, fwd.reshape(-1), None
    bwd = _vectors(rng, mbs, with_min)
    bwd[((d & 2) == 0) & ~bwd.any(axis=1)] = (-1234, 4321)
    return repadd, mb_dir, fwd.reshape(-1), bwd.reshape(-1)


def bound_maps(mbw, mbh, word=-2048):
    """a B picture's maps with both directions everywhere and every vector word `word`: at 256 x 256 and -2048 the sums reach 2^27"""
    mbs = mbw * mbh
    return np.zeros(mbs, np.uint8), np.full(mbs, 3, np.uint8), np.full(2 * mbs, word, np.int16), np.full(2 * mbs, word, np.int16)


def expected(L, mbw, mbh, type, m):
    """(mv [mbh, mbw, 4] int16, info [mbh, mbw] uint8, summary [8] uint32) of a picture of `type` with the maps m, by motion_from_maps.
    A P picture's record does not depend on the maps it does not have, so m may hold them (a B picture's maps run as type P)."""
    repadd, mb_dir, fwd, bwd = m
    if type == 1:
        return L.motion_from_maps(1, mbw, mbh)
    if type == 2:
        return L.motion_from_maps(2, mbw, mbh, repadd=repadd, mv_fwd=fwd)
    return L.motion_from_maps(3, mbw, mbh, repadd=repadd, mb_dir=mb_dir, mv_fwd=fwd, mv_bwd=bwd)


def picture(type, m):
    """a picture as leon_ctypes.motion_kernel takes it"""
    return (type,) + tuple(m)


def without_tail_group(ring, lay):
    """a copy of the ring [ring_frames, record_pitch] with the unspecified bytes the kernel may write zeroed in every record: the
    vectors and info bytes of macroblocks mbs .. ceil4(mbs) - 1, which it makes from the maps' padding"""
    out = ring.copy()
    mbs, io = int(lay.mbs), int(lay.info_offset)
    out[:, 8 * mbs:8 * ceil4(mbs)] = 0
    out[:, io + mbs:io + ceil4(mbs)] = 0
    return out


def assert_ring(ring, lay, frames, want, what="", sentinel=SENTINEL):
    """ring: uint8 [ring_frames, record_pitch] as it came back; frames: [(picture, ring index)]; want[picture] = (mv, info, summary).
    Every named record's three specified parts equal its picture's, exactly; its bytes behind the groups of four that hold the last
    macroblock (8 * ceil4(mbs) .. info_offset, info_offset + ceil4(mbs) .. summary_offset, record_bytes .. pitch) and every record
    that no frame names still hold the sentinel.  Vectorised over the frames of a picture."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1, 2)
    mbs, io, so, rb = int(lay.mbs), int(lay.info_offset), int(lay.summary_offset), int(lay.record_bytes)
    assert ring.shape[1] == lay.record_pitch
    named = np.zeros(len(ring), dtype=bool)
    named[frames[:, 1]] = True
    assert named.sum() == len(frames)
    rest = ring[~named]
    assert (rest == sentinel).all(), "%s: records no frame names were written: ring indices %s" % (what, np.flatnonzero(~named)[(rest != sentinel).any(axis=1)][:8].tolist())
    for p in np.unique(frames[:, 0]):
        idx = frames[frames[:, 0] == p, 1]
        rec = ring[idx]
        mv, info, summary = want[int(p)]
        for name, got, exp in (("summary", rec[:, so:so + 32], summary.view(np.uint8)), ("info", rec[:, io:io + mbs], info.reshape(-1)),
                               ("mv", rec[:, :8 * mbs], mv.reshape(-1).view(np.uint8))):
            bad = (got != exp[None, :]).any(axis=1)
            if bad.any():
                r = int(idx[bad][0])
                g = ring[r]
                if name == "summary":
                    detail = "%s, expected %s" % (g[so:so + 32].view(np.uint32).tolist(), summary.tolist())
                elif name == "info":
                    at = np.flatnonzero(g[io:io + mbs] != info.reshape(-1))
                    detail = "at macroblocks %s: %s, expected %s" % (at[:6].tolist(), g[io + at[:6]].tolist(), info.reshape(-1)[at[:6]].tolist())
                else:
                    at = np.flatnonzero((g[:8 * mbs].view(np.int16).reshape(-1, 4) != mv.reshape(-1, 4)).any(axis=1))
                    detail = "at macroblocks %s" % at[:6].tolist()
                raise AssertionError("%s: picture %d at ring index %d (%d records differ): %s %s" % (what, p, r, int(bad.sum()), name, detail))
        for name, a, b in (("behind the vectors", 8 * ceil4(mbs), io), ("behind info", io + ceil4(mbs), so), ("behind the summary", rb, ring.shape[1])):
            assert (rec[:, a:b] == sentinel).all(), "%s: picture %d: bytes %s (%d .. %d) were written" % (what, p, name, a, b)
