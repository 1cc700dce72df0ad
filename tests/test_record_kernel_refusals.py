"""CPU: what leon_pipeline_motion_kernel, leon_pipeline_activity_kernel and leon_pipeline_residual_kernel refuse before any device call, by
code AND text.  The GPU tests of the kernels (test_motion_kernel_gpu.py, test_activity_kernel_gpu.py, test_residual_kernel_gpu.py) compare
codes only; a caller sees the message, and the calls state most of theirs through shared checks under their own prefix.  The expected
strings are literals, recorded from the library as it stood before the calls shared one harness (residual: before that harness staged
through the piece stager).  Every call is on a 5 x 2 grid (residual: a coded size of 16 times that) with a ring of four records that
holds 0xA5 beforehand and afterwards."""
import numpy as np
import pytest

import activity_cases as A
import motion_cases as M
import residual_cases as R

MBW, MBH, RING, FILL = 5, 2, 4, 0xA5
BIG = (1 << 20) + 1

# ---- arguments the calls refuse alike: {name: keyword arguments of leon_ctypes.*_kernel that replace the good ones} ----------------
COMMON = {
    "null_pictures": dict(pictures=None, n_pictures=2),
    "null_frames": dict(frames=None, n_frames=3),
    "null_ring": dict(null_ring=True),
    "grid_0x2": dict(mbw=0, mbh=2),
    "grid_257x2": dict(mbw=257, mbh=2),
    "grid_5x257": dict(mbw=5, mbh=257),
    "n_pictures_0": dict(n_pictures=0),
    "n_pictures_big": dict(n_pictures=BIG),
    "ring_frames_0": dict(ring_frames=0),
    "ring_frames_2": dict(ring_frames=2),
    "ring_frames_big": dict(ring_frames=BIG),
    "n_frames_0": dict(n_frames=0),
    "n_frames_above_ring": dict(frames=[(0, 0), (1, 1), (0, 2), (0, 3), (1, 3)]),
    "pad_byte_minus_1": dict(pad_byte=-1),
    "pad_byte_256": dict(pad_byte=256),
    "frame_picture_minus_1": dict(frames=[(0, 2), (-1, 0), (0, 3)]),
    "frame_picture_n": dict(frames=[(0, 2), (None, 0), (0, 3)]),          # None: the number of pictures
    "frame_ring_minus_1": dict(frames=[(0, 2), (1, -1), (0, 3)]),
    "frame_ring_4": dict(frames=[(0, 2), (1, 4), (0, 3)]),
    "frame_ring_twice": dict(frames=[(0, 2), (1, 0), (0, 2)]),
}

MOTION = {
    "null_pictures": "null argument",
    "null_frames": "null argument",
    "null_ring": "null argument",
    "grid_0x2": "motion kernel: 0 x 2 macroblocks (1 .. 256 each)",
    "grid_257x2": "motion kernel: 257 x 2 macroblocks (1 .. 256 each)",
    "grid_5x257": "motion kernel: 5 x 257 macroblocks (1 .. 256 each)",
    "n_pictures_0": "motion kernel: 0 pictures (1 .. 1048576)",
    "n_pictures_big": "motion kernel: 1048577 pictures (1 .. 1048576)",
    "ring_frames_0": "motion kernel: a ring of 0 records (1 .. 1048576)",
    "ring_frames_2": "motion kernel: 3 frames (1 .. the ring's 2 records)",
    "ring_frames_big": "motion kernel: a ring of 1048577 records (1 .. 1048576)",
    "n_frames_0": "motion kernel: 0 frames (1 .. the ring's 4 records)",
    "n_frames_above_ring": "motion kernel: 5 frames (1 .. the ring's 4 records)",
    "pad_byte_minus_1": "motion kernel: pad_byte -1 (0 .. 255)",
    "pad_byte_256": "motion kernel: pad_byte 256 (0 .. 255)",
    "frame_picture_minus_1": "motion kernel: frame 1 names picture -1 of 3",
    "frame_picture_n": "motion kernel: frame 1 names picture 3 of 3",
    "frame_ring_minus_1": "motion kernel: frame 1 names record -1 of a ring of 4",
    "frame_ring_4": "motion kernel: frame 1 names record 4 of a ring of 4",
    "frame_ring_twice": "motion kernel: frame 2 names record 2, which an earlier frame names",
    "type_0": "motion kernel: picture 0 has type 0",
    "p_without_mv_fwd": "motion kernel: picture 1 (type 2) lacks a map",
    "b_without_mb_dir": "motion kernel: picture 2 (type 3) lacks a map",
    "reserved_word": "motion kernel: a reserved word of picture 1 is not 0",
}

ACTIVITY = {
    "null_pictures": "null argument",
    "null_frames": "null argument",
    "null_ring": "null argument",
    "grid_0x2": "activity kernel: 0 x 2 macroblocks (1 .. 256 each)",
    "grid_257x2": "activity kernel: 257 x 2 macroblocks (1 .. 256 each)",
    "grid_5x257": "activity kernel: 5 x 257 macroblocks (1 .. 256 each)",
    "n_pictures_0": "activity kernel: 0 pictures (1 .. 1048576)",
    "n_pictures_big": "activity kernel: 1048577 pictures (1 .. 1048576)",
    "ring_frames_0": "activity kernel: a ring of 0 records (1 .. 1048576)",
    "ring_frames_2": "activity kernel: 3 frames (1 .. the ring's 2 records)",
    "ring_frames_big": "activity kernel: a ring of 1048577 records (1 .. 1048576)",
    "n_frames_0": "activity kernel: 0 frames (1 .. the ring's 4 records)",
    "n_frames_above_ring": "activity kernel: 5 frames (1 .. the ring's 4 records)",
    "pad_byte_minus_1": "activity kernel: pad_byte -1 (0 .. 255)",
    "pad_byte_256": "activity kernel: pad_byte 256 (0 .. 255)",
    "frame_picture_minus_1": "activity kernel: frame 1 names picture -1 of 2",
    "frame_picture_n": "activity kernel: frame 1 names picture 2 of 2",
    "frame_ring_minus_1": "activity kernel: frame 1 names record -1 of a ring of 4",
    "frame_ring_4": "activity kernel: frame 1 names record 4 of a ring of 4",
    "frame_ring_twice": "activity kernel: frame 2 names record 2, which an earlier frame names",
    "grp_off_decreases": "activity kernel: grp_off decreases at group 3 (255 after 256)",
    "grp_off_above_n_entries": "activity kernel: grp_off ends at 1668, the list has 1667 entries",
    "n_entries_above_2_to_the_30": "activity kernel: picture 0 has 1073741825 entries (at most 2^30)",
    "null_qscale": "activity kernel: null argument",
}


RESIDUAL = {
    "null_pictures": "null argument",
    "null_frames": "null argument",
    "null_ring": "null argument",
    "grid_0x2": "residual kernel: a coded size of 0 x 32 (multiples of 16)",
    "grid_257x2": "residual kernel: 257 x 2 macroblocks (1 .. 256 each)",
    "grid_5x257": "residual kernel: 5 x 257 macroblocks (1 .. 256 each)",
    "n_pictures_0": "residual kernel: 0 pictures (1 .. 1048576)",
    "n_pictures_big": "residual kernel: 1048577 pictures (1 .. 1048576)",
    "ring_frames_0": "residual kernel: a ring of 0 records (1 .. 1048576)",
    "ring_frames_2": "residual kernel: 3 frames (1 .. the ring's 2 records)",
    "ring_frames_big": "residual kernel: a ring of 1048577 records (1 .. 1048576)",
    "n_frames_0": "residual kernel: 0 frames (1 .. the ring's 4 records)",
    "n_frames_above_ring": "residual kernel: 5 frames (1 .. the ring's 4 records)",
    "pad_byte_minus_1": "residual kernel: pad_byte -1 (0 .. 255)",
    "pad_byte_256": "residual kernel: pad_byte 256 (0 .. 255)",
    "frame_picture_minus_1": "residual kernel: frame 1 names picture -1 of 2",
    "frame_picture_n": "residual kernel: frame 1 names picture 2 of 2",
    "frame_ring_minus_1": "residual kernel: frame 1 names record -1 of a ring of 4",
    "frame_ring_4": "residual kernel: frame 1 names record 4 of a ring of 4",
    "frame_ring_twice": "residual kernel: frame 2 names record 2, which an earlier frame names",
    "grp_off_decreases": "residual kernel: grp_off decreases at group 3 (769 after 770)",
    "grp_off_above_n_entries": "residual kernel: grp_off ends at 1797, the list has 1796 entries",
    "n_entries_above_2_to_the_29": "residual kernel: picture 0 has 536870913 entries (at most 2^29)",
    "null_qscale": "residual kernel: null argument",
    "null_intra": "residual kernel: picture 1 lacks its intra map, matrices or premultiplier",
    "null_matrices": "residual kernel: picture 0 lacks its intra map, matrices or premultiplier",
    "null_premultiplier": "residual kernel: picture 0 lacks its intra map, matrices or premultiplier",
    "reserved_word": "residual kernel: a reserved word of picture 1 is not 0",
}


def motion_good():
    m = M.maps(MBW, MBH, 3, 41)
    return [M.picture(1, (None,) * 4), M.picture(2, m), M.picture(3, m)], m


def activity_good():
    return [A.named()["5x2"][2], A.empty(MBW, MBH)]


def residual_good():
    return [R.picture(R.make(16 * MBW, 16 * MBH, 8, 1, False)), R.picture(R.empty(16 * MBW, 16 * MBH))]


def motion_only():
    good, (repadd, mb_dir, fwd, bwd) = motion_good()
    return {
        "type_0": dict(pictures=[(0, repadd, mb_dir, fwd, bwd)] + good[1:]),
        "p_without_mv_fwd": dict(pictures=[good[0], (2, repadd, None, None, None), good[2]]),
        "b_without_mb_dir": dict(pictures=[good[0], good[1], (3, repadd, None, fwd, bwd)]),
        "reserved_word": dict(reserved=(1, 7)),          # picture 1's reserved0 = 7
    }


def activity_only():
    good = activity_good()
    grp_off, entries, qscale = good[0]
    down = grp_off.copy()
    down[3] = down[4] + 1
    return {
        "grp_off_decreases": dict(pictures=[(down, entries, qscale), good[1]]),
        "grp_off_above_n_entries": dict(pictures=[(grp_off, entries, qscale, len(entries) - 1), good[1]]),
        "n_entries_above_2_to_the_30": dict(pictures=[(grp_off, entries, qscale, (1 << 30) + 1), good[1]]),
        "null_qscale": dict(pictures=[(grp_off, entries, None), good[1]]),
    }


def residual_only():
    good = residual_good()
    grp_off, entries, qscale, intra, qm, pm = good[0]
    down = grp_off.copy()
    down[3] = down[4] + 1
    return {
        "grp_off_decreases": dict(pictures=[(down,) + good[0][1:], good[1]]),
        "grp_off_above_n_entries": dict(pictures=[good[0] + (len(entries) - 1,), good[1]]),
        "n_entries_above_2_to_the_29": dict(pictures=[good[0] + ((1 << 29) + 1,), good[1]]),
        "null_qscale": dict(pictures=[(grp_off, entries, None, intra, qm, pm), good[1]]),
        "null_intra": dict(pictures=[good[0], good[1][:3] + (None,) + good[1][4:]]),
        "null_matrices": dict(pictures=[good[0][:4] + (None, pm), good[1]]),
        "null_premultiplier": dict(pictures=[good[0][:5] + (None,), good[1]]),
        "reserved_word": dict(reserved=(1, 7)),          # picture 1's reserved0 = 7
    }


GOOD = {"motion": lambda: motion_good()[0], "activity": activity_good, "residual": residual_good}
ONLY = {"motion": motion_only, "activity": activity_only, "residual": residual_only}
TEXTS = {"motion": MOTION, "activity": ACTIVITY, "residual": RESIDUAL}


def call(L, kind, null_ring=False, reserved=None, **kw):
    """one refused call -> (code, message, the ring afterwards)"""
    good = GOOD[kind]()
    kernel, layout = {"motion": (L.motion_kernel, L.motion_layout), "activity": (L.activity_kernel, L.activity_layout),
                      "residual": (lambda mbw, mbh, *a, **k: L.residual_kernel(16 * mbw, 16 * mbh, *a, **k), lambda mbw, mbh: L.residual_layout(16 * mbw, 16 * mbh))}[kind]
    ring = np.full((RING, int(layout(MBW, MBH).record_pitch)), FILL, dtype=np.uint8)
    kw.setdefault("pictures", good)
    kw.setdefault("frames", [(0, 2), (1, 0), (0, 3)])
    if kw["frames"] is not None:
        kw["frames"] = [(len(good) if p is None else p, r) for p, r in kw["frames"]]
    kw.setdefault("mbw", MBW)
    kw.setdefault("mbh", MBH)
    if null_ring or reserved:          # what the wrappers have no argument for: the library itself, on structures of the test's own
        lib, fr = L.load(), np.ascontiguousarray(kw["frames"], dtype=np.int32)
        if kind == "motion":
            keep = [[None if a is None else np.ascontiguousarray(a) for a in p[1:]] for p in good]
            pics = (L.PipelineMotionPicture * len(good))(*[L.PipelineMotionPicture(p[0], 0, *[None if a is None else a.ctypes.data for a in k]) for p, k in zip(good, keep)])
            fn = lib.leon_pipeline_motion_kernel
        else:
            struct, fn, parts = ((L.PipelineActivityPicture, lib.leon_pipeline_activity_kernel, 3) if kind == "activity" else
                                 (L.PipelineResidualPicture, lib.leon_pipeline_residual_kernel, 6))
            keep = [[np.ascontiguousarray(a) for a in p[:parts]] for p in good]
            pics = (struct * len(good))(*[struct(*[a.ctypes.data if a.size else None for a in k], k[1].size, 0) for k in keep])
        if reserved:
            pics[reserved[0]].reserved0 = reserved[1]
        size = (16 * MBW, 16 * MBH) if kind == "residual" else (MBW, MBH)
        rc = fn(0, *size, pics, len(good), fr.ctypes.data, len(fr), RING, 0, None if null_ring else ring.ctypes.data)
        return rc, lib.leon_last_error().decode(), ring
    with pytest.raises(L.LeonError) as e:
        kernel(kw.pop("mbw"), kw.pop("mbh"), kw.pop("pictures"), kw.pop("frames"), ring=ring, **kw)
    prefix = "leon error %d: " % e.value.code          # (LeonError's own text in front of the library's)
    assert str(e.value).startswith(prefix)
    return e.value.code, str(e.value)[len(prefix):], ring


def all_cases(kind):
    return {**COMMON, **ONLY[kind]()}


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.mark.parametrize("kind,name", [(k, n) for k, table in TEXTS.items() for n in table])
def test_refusal(L, kind, name):
    code, message, ring = call(L, kind, **all_cases(kind)[name])
    assert code == L.ERR_INVALID
    assert message == TEXTS[kind][name]
    assert (ring == FILL).all(), "a refused call wrote the ring"


def test_every_case_has_its_text():
    assert all(set(TEXTS[kind]) == set(all_cases(kind)) for kind in TEXTS)
