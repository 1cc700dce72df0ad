"""GPU: k_residual through leon_pipeline_residual_kernel (include/leon_pipeline.h) on pictures of the test's own choosing
(tests/residual_cases.py, whose premises tests/test_residual_cases.py checks on the CPU), against the oracle: lo_pass1_plane followed by
lo_pass2_residual_plane on each case's dense planes.  Bit-exact, no tolerance.  Every case runs the kernel once on a ring that holds
0xA5 in every byte, has more records than frames and is named by a permutation that is not the identity -- so records land at ring
indices that are not 0 -- and compares every specified element of every written record, the bytes behind record_bytes, and every record
no frame names (residual_cases.assert_ring; the pad columns are unspecified and not looked at).  The padding behind every list and map
holds 0xFF, a level of -1 for whoever reads past a list; every case runs again with 0x00.  Every list's capacity is exactly
grp_off[last]."""
import numpy as np
import pytest

import residual_cases as K
from record_cases import L  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NAMES = sorted(K.named())


def run(L, cw, ch, cases, wants, frame_pictures, extra=2, pad_byte=0xFF, what=""):
    n = len(frame_pictures)
    frames = np.stack([np.asarray(frame_pictures, dtype=np.int32), K.permutation(n, n + extra, 5)], axis=1)
    assert frames[:, 1].max() > 0
    ring = L.residual_kernel(cw, ch, [K.picture(c) for c in cases], frames, ring_frames=n + extra, pad_byte=pad_byte, fill=K.SENTINEL)
    K.assert_ring(L, ring, L.residual_layout(cw, ch), frames, wants, "%s, padding 0x%02X" % (what, pad_byte))
    return ring


@pytest.mark.parametrize("name", NAMES)
def test_every_case(L, name):
    """the case's picture twice and an empty picture of the same size between, in one call; again with padding 0x00: the same ring"""
    case = K.named()[name]
    cw, ch = case["cw"], case["ch"]
    nothing = K.empty(cw, ch)
    wants = [K.expected(name), K.expected_of(nothing)]
    assert int(case["grp_off"][-1]) == len(case["entries"])          # the capacity handed over is exactly what the lists hold
    ring = run(L, cw, ch, [case, nothing], wants, [0, 1, 0], what=name)
    again = run(L, cw, ch, [case, nothing], wants, [0, 1, 0], pad_byte=0x00, what=name)
    assert np.array_equal(ring, again)


@pytest.mark.parametrize("n", [1, 3, 5])
def test_frames_share_pictures(L, n):
    """1, 3 and 5 frames of two pictures with different matrices, maps and lists"""
    a, b = K.named()["144x32_c8"], K.named()["dense_2047_144x32"]
    assert a["qm"].tobytes() != b["qm"].tobytes()
    run(L, 144, 32, [a, b], [K.expected("144x32_c8"), K.expected("dense_2047_144x32")], [0, 1, 0, 1, 1][:n], extra=3, what="%d frames" % n)


def test_1080p_grid(L):
    """the 1080p grid (30 luma and 15 chroma groups a row, 3060 tasks): every group length, every column"""
    case = K.make(1920, 1088, 8, 17, True)
    run(L, 1920, 1088, [case], [K.expected_of(case)], [0, 0], extra=1, what="1080p")


def test_capacity_is_exactly_the_lists_end(L):
    """the clamp: a list whose capacity is exactly grp_off[last] gives the right record with 0xFF behind its last entry; the same list
    handed over with room to spare gives the same record"""
    case = K.named()["48x32_c8"]
    n = len(case["entries"])
    assert int(case["grp_off"][-1]) == n
    roomy = dict(case, entries=np.concatenate([case["entries"], np.full(100, 0x00010001, np.uint32)]))          # entries behind the lists' end: never read
    w = K.expected("48x32_c8")
    frames = np.array([(0, 2), (1, 0)], np.int32)
    ring = L.residual_kernel(48, 32, [K.picture(case, n), K.picture(roomy, n + 100)], frames, ring_frames=3, pad_byte=0xFF, fill=K.SENTINEL)
    K.assert_ring(L, ring, L.residual_layout(48, 32), frames, [w, w], "capacity")


def test_launch_chunks(L):
    """65535 + 2 frames of 16x16: the launches are cut behind frame 65534, and the second launch's descriptors start at 65535.  Five
    pictures with different records, adjacent frames never the same picture, frame i at ring index i from 16 on (the first 16 shuffled,
    three unnamed records at the end)"""
    cases = [K.empty(16, 16)] + [K.one_block(v) for v in (64, -64, 200, -1000)]
    wants = [K.expected_of(c) for c in cases]
    assert len({w[0].tobytes() for w in wants}) == 5
    n = 65535 + 2
    ring_index = np.arange(n, dtype=np.int32)
    ring_index[:16] = np.random.default_rng(6).permutation(16)
    assert not np.array_equal(ring_index[:16], np.arange(16))
    frames = np.stack([np.arange(n, dtype=np.int32) % 5, ring_index], axis=1)
    ring = L.residual_kernel(16, 16, [K.picture(c) for c in cases], frames, ring_frames=n + 3, pad_byte=0xFF, fill=K.SENTINEL)
    lay = L.residual_layout(16, 16)
    for r in (65534, 65535, 65536, n - 1):          # the chunk's border first, by name
        K.assert_record(L, ring[r], lay, wants[r % 5], "ring index %d is not picture %d's record" % (r, r % 5))
    K.assert_ring(L, ring, lay, frames, wants, "65537 frames")          # then the whole ring, one comparison per picture


def test_refusals_leave_the_ring_alone(L):
    case = K.named()["48x32_c4"]
    cw, ch = 48, 32
    lay = L.residual_layout(cw, ch)
    grp_off, entries, qscale, intra, qm, pm = K.picture(case)
    good = [K.picture(case), K.picture(K.empty(cw, ch))]
    frames = [(0, 2), (1, 0), (0, 3)]
    ring = np.full((4, lay.record_pitch), K.SENTINEL, dtype=np.uint8)
    n_groups = len(grp_off) - 1

    def refused(pictures=good, frames=frames, cw=cw, ch=ch, **kw):
        with pytest.raises(L.LeonError) as e:
            L.residual_kernel(cw, ch, pictures, frames, ring=ring, **kw)
        assert e.value.code == L.ERR_INVALID, e.value
        assert (ring == K.SENTINEL).all(), "a refused call wrote the ring"

    refused(pictures=None, n_pictures=2)
    refused(frames=None, n_frames=3)
    assert L.load().leon_pipeline_residual_kernel(0, cw, ch, (L.PipelineResidualPicture * 1)(), 1, np.zeros(2, np.int32).ctypes.data, 1, 4, 0, None) == L.ERR_INVALID
    for w, h in ((0, 32), (48, 0), (4112, 32), (48, 4112), (-16, 32), (40, 32), (48, 24)):
        refused(cw=w, ch=h)
    for g in (0, n_groups // 2, n_groups - 1):          # grp_off not monotonic
        bad = grp_off.copy()
        bad[g] = bad[g + 1] + 1
        refused(pictures=[(bad, entries, qscale, intra, qm, pm), good[1]])
    refused(pictures=[(grp_off, entries, qscale, intra, qm, pm, len(entries) - 1), good[1]])          # grp_off[last] above the capacity
    refused(pictures=[(grp_off, entries, qscale, intra, qm, pm, (1 << 29) + 1), good[1]])
    for k in (0, 2, 3, 4, 5):          # a null grp_off, qscale, intra, matrices, premultiplier
        refused(pictures=[tuple(None if i == k else a for i, a in enumerate(good[0])), good[1]])
    refused(pictures=[(grp_off, None, qscale, intra, qm, pm, len(entries)), good[1]])
    refused(frames=[(0, 2), (2, 0), (0, 3)])
    refused(frames=[(0, 2), (-1, 0), (0, 3)])
    refused(frames=[(0, 2), (1, 4), (0, 3)])
    refused(frames=[(0, 2), (1, 0), (0, 2)])
    refused(n_frames=0)
    refused(n_pictures=0)
    refused(ring_frames=0)
    refused(ring_frames=2)
    refused(pad_byte=256)
    refused(pad_byte=-1)
    # ... and the same arguments are accepted
    out = L.residual_kernel(cw, ch, good, frames, ring=ring, pad_byte=0xFF)
    assert out is ring
    K.assert_ring(L, ring, lay, frames, [K.expected("48x32_c4"), K.expected_of(K.empty(cw, ch))], "accepted")
