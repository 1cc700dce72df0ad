"""GPU: k_motion through leon_pipeline_motion_kernel (include/leon_pipeline.h) on maps of the test's own choosing
(tests/motion_cases.py), against leon_ctypes.motion_from_maps, the header's text in numpy.  Every case runs the kernel once on a ring
that holds 0xA5 in every byte, has more records than frames and is named by a permutation that is not the identity, and compares the
three specified parts of every written record exactly, every record no frame names, and inside a written record the bytes behind the
groups of four that hold its last macroblock (motion_cases.assert_ring).

What the cases pin, none of which a stream through the pipeline reaches: the strided loop from its second trip on (1025, 1032, 2057,
8160 and 65536 macroblocks), every mbs % 4 and every mbs below 4, the guard that keeps a map's padding out of the summary (padding
bytes of 0xFF: intra macroblocks; of 0x00: forward macroblocks of a P picture), the tail stores, the summary at its bound of 2^27
through the shuffles, LDS and lane 0's adds, -32768, repadd 127 against 128, bits of mb_dir above the low two, garbage in unused
directions, and the launch cut into chunks of 65535 frames."""
import functools

import numpy as np
import pytest

import motion_cases as K
import record_cases
from record_cases import L  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in K.SHAPES]


@functools.lru_cache(maxsize=None)
def shape_case(mbw, mbh):
    """(pictures I, P, B for motion_kernel, their expected records): built once per process and left unchanged"""
    import leon_ctypes as L_
    ms = [K.maps(mbw, mbh, t, 11) for t in (1, 2, 3)]
    return [K.picture(t, m) for t, m in zip((1, 2, 3), ms)], [K.expected(L_, mbw, mbh, t, m) for t, m in zip((1, 2, 3), ms)]


def run(L, *case, **kw):
    return record_cases.run(L.motion_kernel, L.motion_layout, K.assert_ring, *case, **kw)


@pytest.mark.parametrize("mbw,mbh", K.SHAPES, ids=IDS)
def test_every_shape_and_type(L, mbw, mbh):
    """I, P and B pictures of one grid in one call, the B picture twice; the maps' padding is 0xFF, so a macroblock counted behind
    mbs - 1 is one intra macroblock too many.  The smaller shapes run again with padding 0x00 (a P picture's padding then reads as
    forward macroblocks): the two rings are equal, but for the unspecified bytes of the last group of four behind macroblock mbs - 1,
    which are made from the padding."""
    pictures, want = shape_case(mbw, mbh)
    ring = run(L, mbw, mbh, pictures, want, [2, 0, 1, 2])
    if (mbw, mbh) in K.SMALL:
        again = run(L, mbw, mbh, pictures, want, [2, 0, 1, 2], pad_byte=0x00)
        assert np.array_equal(K.without_tail_group(ring, L.motion_layout(mbw, mbh)), K.without_tail_group(again, L.motion_layout(mbw, mbh)))


def test_summary_at_its_bound(L):
    """256 x 256, both directions everywhere, every vector word -2048: 2^27 in each of the four sums, through 64 trips, the shuffles,
    the four waves' LDS words and lane 0's adds; the same maps as a P picture have no backward part"""
    import leon_ctypes as L_
    m = K.bound_maps(256, 256)
    want = [K.expected(L_, 256, 256, 3, m), K.expected(L_, 256, 256, 2, m)]
    assert want[0][2].tolist() == [65536, 65536, 0, 65536] + [1 << 27] * 4 and want[1][2].tolist() == [65536, 0, 0, 65536, 1 << 27, 1 << 27, 0, 0]
    ring = run(L, 256, 256, [K.picture(3, m), K.picture(2, m)], want, [0, 1], what="the bound")
    lay = L.motion_layout(256, 256)
    frames = K.permutation(2, 4, 5)
    s = [ring[r, lay.summary_offset:lay.summary_offset + 32].view(np.uint32).tolist() for r in frames]
    assert s[0][4:8] == [1 << 27] * 4 and [s[0][0], s[0][1], s[0][3]] == [65536] * 3 and s[0][2] == 0
    assert s[1][6:8] == [0, 0] and s[1][4:6] == [1 << 27] * 2


def test_minus_32768_counts_as_32768(L):
    """17 x 15 = 255 macroblocks: seeded maps with -32768 among the vectors, and a B picture that holds nothing else"""
    import leon_ctypes as L_
    mbw, mbh = 17, 15
    ms = [(2, K.maps(mbw, mbh, 2, 21, with_min=True)), (3, K.maps(mbw, mbh, 3, 21, with_min=True)), (3, K.bound_maps(mbw, mbh, word=-32768))]
    want = [K.expected(L_, mbw, mbh, t, m) for t, m in ms]
    assert all((w[0] == -32768).any() for w in want)
    assert want[2][2].tolist() == [255, 255, 0, 255] + [255 * 32768] * 4
    run(L, mbw, mbh, [K.picture(t, m) for t, m in ms], want, [0, 1, 2], what="-32768")


def test_i_picture_without_maps_beside_p_and_b(L):
    """13 x 7 = 91 macroblocks, seven frames of three pictures: the I picture has four null maps (and, a second one, four maps of
    garbage that must not show)"""
    import leon_ctypes as L_
    mbw, mbh = 13, 7
    ms = [K.maps(mbw, mbh, t, 31) for t in (1, 2, 3)]
    pictures = [K.picture(1, ms[0]), K.picture(2, ms[1]), K.picture(3, ms[2]), K.picture(1, ms[2])]
    want = [K.expected(L_, mbw, mbh, t, m) for t, m in zip((1, 2, 3), ms)]
    want.append(want[0])
    assert pictures[0][1:] == (None, None, None, None) and want[0][2].tolist() == [0, 0, 91, 0, 0, 0, 0, 0]
    run(L, mbw, mbh, pictures, want, [0, 2, 1, 0, 3, 2, 0, 1], extra=3, what="I without maps")


def test_launch_chunks(L):
    """65535 + 2 frames of one macroblock: the launch is cut behind frame 65534, and the second launch's descriptors start at 65535.
    Five pictures with different records, adjacent frames never the same picture, frame i at ring index i from 16 on (the first 16
    shuffled, three unnamed records at the end): a second chunk that read the first chunk's descriptors would leave ring index 65535
    unwritten"""
    import leon_ctypes as L_
    z, v = np.zeros(1, np.uint8), lambda a, b: np.array([a, b], np.int16)
    ms = [(1, (None, None, None, None)), (2, (z, None, v(-2048, 7), None)), (2, (z, None, v(0, 0), None)),
          (3, (z, z + 3, v(100, -100), v(-3, 2047))), (3, (z, z + 2, v(9, 9), v(-32768, 1)))]
    want = [K.expected(L_, 1, 1, t, m) for t, m in ms]
    assert len({w[0].tobytes() + w[1].tobytes() + w[2].tobytes() for w in want}) == 5
    n = 65535 + 2
    ring_index = np.arange(n, dtype=np.int32)
    ring_index[:16] = np.random.default_rng(6).permutation(16)
    assert not np.array_equal(ring_index[:16], np.arange(16))
    frames = np.stack([np.arange(n, dtype=np.int32) % 5, ring_index], axis=1)
    ring = L.motion_kernel(1, 1, [K.picture(t, m) for t, m in ms], frames, ring_frames=n + 3, pad_byte=0xFF, fill=K.SENTINEL)
    lay = L.motion_layout(1, 1)
    for r in (65534, 65535, 65536, n - 1):          # the chunk's border first, by name
        mv, info, summary = want[r % 5]
        got = ring[r]
        assert got[lay.summary_offset:lay.summary_offset + 32].view(np.uint32).tolist() == summary.tolist(), "ring index %d is not picture %d's record" % (r, r % 5)
        assert got[:8].view(np.int16).tolist() == mv.reshape(-1).tolist() and got[lay.info_offset] == info.reshape(-1)[0], "ring index %d is not picture %d's record" % (r, r % 5)
    K.assert_ring(ring, lay, frames, want, "65537 frames")          # then the whole ring, one comparison per picture


def test_refusals_leave_the_ring_alone(L):
    mbw, mbh = 3, 2
    lay = L.motion_layout(mbw, mbh)
    m = K.maps(mbw, mbh, 3, 41)
    repadd, mb_dir, fwd, bwd = m
    good = [K.picture(1, (None,) * 4), K.picture(2, m), K.picture(3, m)]
    frames = [(0, 2), (1, 0), (2, 3)]
    ring = np.full((4, lay.record_pitch), K.SENTINEL, dtype=np.uint8)

    def refused(pictures=good, frames=frames, mbw=mbw, mbh=mbh, **kw):
        with pytest.raises(L.LeonError) as e:
            L.motion_kernel(mbw, mbh, pictures, frames, ring=ring, **kw)
        assert e.value.code == L.ERR_INVALID, e.value
        assert (ring == K.SENTINEL).all(), "a refused call wrote the ring"

    refused(pictures=None, n_pictures=3)
    refused(frames=None, n_frames=3)
    assert L.load().leon_pipeline_motion_kernel(0, mbw, mbh, (L.PipelineMotionPicture * 1)(L.PipelineMotionPicture(1)), 1, np.zeros(2, np.int32).ctypes.data, 1, 4, 0,
                                                 None) == L.ERR_INVALID
    for w, h in ((0, 2), (3, 0), (257, 2), (3, 257), (-1, 2)):
        refused(mbw=w, mbh=h)
    for t in (0, 4, -1):
        refused(pictures=[(t,) + tuple(m)] + good[1:])
    refused(pictures=[good[0], (2, None, None, fwd, None), good[2]])
    refused(pictures=[good[0], (2, repadd, None, None, None), good[2]])
    refused(pictures=[good[0], good[1], (3, repadd, None, fwd, bwd)])
    refused(pictures=[good[0], good[1], (3, repadd, mb_dir, fwd, None)])
    refused(frames=[(0, 2), (3, 0), (2, 3)])
    refused(frames=[(0, 2), (-1, 0), (2, 3)])
    refused(frames=[(0, 2), (1, 4), (2, 3)])
    refused(frames=[(0, 2), (1, -1), (2, 3)])
    refused(frames=[(0, 2), (1, 0), (2, 2)])
    refused(n_frames=0)
    refused(n_frames=-1)
    refused(frames=[(0, 0), (1, 1), (2, 2), (0, 3), (1, 3)])          # more frames than the ring has records
    refused(n_pictures=0)
    refused(ring_frames=0)
    refused(ring_frames=2)                                            # three frames in a ring of two
    refused(ring_frames=(1 << 20) + 1)
    refused(pad_byte=256)
    refused(pad_byte=-1)
    # ... and the same arguments are accepted
    out = L.motion_kernel(mbw, mbh, good, frames, ring=ring, pad_byte=0xFF)
    assert out is ring
    import leon_ctypes as L_
    K.assert_ring(ring, lay, frames, [K.expected(L_, mbw, mbh, t, m) for t in (1, 2, 3)], "accepted")
