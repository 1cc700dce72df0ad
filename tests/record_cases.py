"""What the tests of k_motion and k_activity on supplied pictures share (motion_cases.py, activity_cases.py, test_*_kernel_gpu.py): the
byte a ring holds before a launch, the ring indices a call names, the library fixture and the run both GPU tests make of a case."""
import numpy as np
import pytest

SENTINEL = 0xA5                  # what a ring holds before the launch


def permutation(n_frames, ring_frames, seed):
    """ring indices of n_frames frames in a ring of ring_frames > n_frames records: distinct, and not the identity"""
    assert ring_frames > n_frames
    ring = np.random.default_rng([seed, n_frames, ring_frames]).permutation(ring_frames)[:n_frames]
    if np.array_equal(ring, np.arange(n_frames)):
        ring = ring[::-1].copy() if n_frames > 1 else np.array([ring_frames - 1])
    return ring.astype(np.int32)


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def run(kernel, layout, assert_ring, mbw, mbh, pictures, want, frame_pictures, extra=2, pad_byte=0xFF, what=""):
    """kernel (motion_kernel, activity_kernel) once on a ring of SENTINEL, frame i at the ring index a permutation gives it; the case module's assert_ring"""
    n = len(frame_pictures)
    frames = np.stack([np.asarray(frame_pictures, dtype=np.int32), permutation(n, n + extra, 5)], axis=1)
    assert frames[:, 1].max() > 0
    ring = kernel(mbw, mbh, pictures, frames, ring_frames=n + extra, pad_byte=pad_byte, fill=SENTINEL)
    assert_ring(ring, layout(mbw, mbh), frames, want, "%s, padding 0x%02X" % (what or "%d x %d" % (mbw, mbh), pad_byte))
    return ring
