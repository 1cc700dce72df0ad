"""GPU: k_activity and k_activity_summary through leon_pipeline_activity_kernel (include/leon_pipeline.h) on lists of the test's own
choosing (tests/activity_cases.py, the table the CPU test holds against the host's text), against leon_ctypes.activity_from_lists, the
header's text in numpy.  Every case runs the kernels once on a ring that holds 0xA5 in every byte, has more records than frames and is
named by a permutation that is not the identity -- so records land at ring indices that are not 0 -- and compares both specified parts
of every written record exactly, every record no frame names, and inside a written record every unspecified byte
(activity_cases.assert_ring).  The padding behind every list holds 0xFF, a level of -1 for whoever reads past a list; the smaller
cases run again with 0x00.  Every list's capacity is exactly grp_off[last]."""
import functools

import numpy as np
import pytest

import activity_cases as K
import record_cases
from record_cases import L  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NAMES = sorted(K.named())


@functools.lru_cache(maxsize=None)
def want(name):
    import leon_ctypes as L_
    return K.expected(L_, K.named()[name])


def run(L, *case, **kw):
    return record_cases.run(L.activity_kernel, L.activity_layout, K.assert_ring, *case, **kw)


@pytest.mark.parametrize("name", NAMES)
def test_every_case(L, name):
    """the case's picture twice and an empty picture of the same grid between, in one call; again with padding 0x00: the same ring"""
    mbw, mbh, lists = K.named()[name]
    import leon_ctypes as L_
    pictures, wants = [lists, K.empty(mbw, mbh)], [want(name), K.expected(L_, (mbw, mbh, K.empty(mbw, mbh)))]
    assert int(lists[0][-1]) == len(lists[1])          # the capacity handed over is exactly what the lists hold
    ring = run(L, mbw, mbh, pictures, wants, [0, 1, 0], what=name)
    again = run(L, mbw, mbh, pictures, wants, [0, 1, 0], pad_byte=0x00, what=name)
    assert np.array_equal(ring, again)


@pytest.mark.parametrize("mbw,mbh", [(120, 68), (256, 256)], ids=["1080p", "256x256"])
def test_large_grids(L, mbw, mbh):
    """the 1080p grid (15 tasks a row, 1020 tasks) and the largest picture (8192 tasks, 2048 workgroups a frame; every summary word
    through 256 trips of the second kernel)"""
    import leon_ctypes as L_
    lists = K.lists(mbw, mbh, 17)
    w = K.expected(L_, (mbw, mbh, lists))
    assert w[1][0] > 0.9 * mbw * mbh
    run(L, mbw, mbh, [lists], [w], [0, 0], extra=1)


def test_capacity_is_exactly_the_lists_end(L):
    """the clamp: a list whose capacity is exactly grp_off[last] gives the right record with 0xFF behind its last entry; the same list
    handed over with room to spare gives the same record"""
    import leon_ctypes as L_
    mbw, mbh, (grp_off, entries, qscale) = K.named()["13x3"]
    w = want("13x3")
    n = len(entries)
    assert int(grp_off[-1]) == n and n % 64 != 0
    roomy = np.concatenate([entries, np.full(100, 0x00010001, np.uint32)])          # entries behind the lists' end: never read
    assert np.array_equal(K.expected(L_, (mbw, mbh, (grp_off, roomy, qscale)))[0], w[0])
    run(L, mbw, mbh, [(grp_off, entries, qscale, n), (grp_off, roomy, qscale, n + 100)], [w, w], [0, 1], what="capacity")


def test_launch_chunks(L):
    """65535 + 2 frames of one macroblock: both kernels' launches are cut behind frame 65534, and the second launches' descriptors
    start at 65535.  Five pictures with different records, adjacent frames never the same picture, frame i at ring index i from 16 on
    (the first 16 shuffled, three unnamed records at the end)"""
    import leon_ctypes as L_
    lists = [K.empty(1, 1), K.one_macroblock(1, 7), K.one_macroblock(2, -3, dc_level=100), K.one_macroblock(0, 1, dc_level=-32768), K.one_macroblock(63, 255)]
    wants = [K.expected(L_, (1, 1, x)) for x in lists]
    assert len({w[0].tobytes() + w[1].tobytes() for w in wants}) == 5
    n = 65535 + 2
    ring_index = np.arange(n, dtype=np.int32)
    ring_index[:16] = np.random.default_rng(6).permutation(16)
    assert not np.array_equal(ring_index[:16], np.arange(16))
    frames = np.stack([np.arange(n, dtype=np.int32) % 5, ring_index], axis=1)
    ring = L.activity_kernel(1, 1, lists, frames, ring_frames=n + 3, pad_byte=0xFF, fill=K.SENTINEL)
    lay = L.activity_layout(1, 1)
    for r in (65534, 65535, 65536, n - 1):          # the chunk's border first, by name
        K.assert_record(ring[r], lay, wants[r % 5], "ring index %d is not picture %d's record" % (r, r % 5))
    K.assert_ring(ring, lay, frames, wants, "65537 frames")          # then the whole ring, one comparison per picture


def test_refusals_leave_the_ring_alone(L):
    mbw, mbh, (grp_off, entries, qscale) = K.named()["5x2"]
    lay = L.activity_layout(mbw, mbh)
    good = [(grp_off, entries, qscale), K.empty(mbw, mbh)]
    frames = [(0, 2), (1, 0), (0, 3)]
    ring = np.full((4, lay.record_pitch), K.SENTINEL, dtype=np.uint8)
    n_groups = len(grp_off) - 1

    def refused(pictures=good, frames=frames, mbw=mbw, mbh=mbh, **kw):
        with pytest.raises(L.LeonError) as e:
            L.activity_kernel(mbw, mbh, pictures, frames, ring=ring, **kw)
        assert e.value.code == L.ERR_INVALID, e.value
        assert (ring == K.SENTINEL).all(), "a refused call wrote the ring"

    refused(pictures=None, n_pictures=2)
    refused(frames=None, n_frames=3)
    assert L.load().leon_pipeline_activity_kernel(0, mbw, mbh, (L.PipelineActivityPicture * 1)(), 1, np.zeros(2, np.int32).ctypes.data, 1, 4, 0, None) == L.ERR_INVALID
    for w, h in ((0, 2), (5, 0), (257, 2), (5, 257), (-1, 2)):
        refused(mbw=w, mbh=h)
    for g in (0, n_groups // 2, n_groups - 1):          # grp_off not monotonic
        bad = grp_off.copy()
        bad[g] = bad[g + 1] + 1
        refused(pictures=[(bad, entries, qscale), good[1]])
    refused(pictures=[(grp_off, entries, qscale, len(entries) - 1), good[1]])          # grp_off[last] above the capacity
    refused(pictures=[(None, entries, qscale), good[1]])
    refused(pictures=[(grp_off, entries, None), good[1]])
    refused(pictures=[(grp_off, None, qscale, len(entries)), good[1]])
    refused(frames=[(0, 2), (2, 0), (0, 3)])
    refused(frames=[(0, 2), (-1, 0), (0, 3)])
    refused(frames=[(0, 2), (1, 4), (0, 3)])
    refused(frames=[(0, 2), (1, -1), (0, 3)])
    refused(frames=[(0, 2), (1, 0), (0, 2)])
    refused(n_frames=0)
    refused(frames=[(0, 0), (1, 1), (0, 2), (0, 3), (1, 3)])          # more frames than the ring has records
    refused(n_pictures=0)
    refused(ring_frames=0)
    refused(ring_frames=2)
    refused(ring_frames=(1 << 20) + 1)
    refused(pad_byte=256)
    refused(pad_byte=-1)
    # ... and the same arguments are accepted
    out = L.activity_kernel(mbw, mbh, good, frames, ring=ring, pad_byte=0xFF)
    assert out is ring
    import leon_ctypes as L_
    K.assert_ring(ring, lay, frames, [K.expected(L_, (mbw, mbh, x)) for x in good], "accepted")
