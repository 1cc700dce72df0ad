"""CPU: the structure of k_letterbox as tests/canvas_structure.py states it -- for every case the GPU test runs, and for all four
packed kernels and float CHW, every byte of a frame's tensor has exactly one writer: the image tiles store exactly the image's bytes,
the pad workgroups exactly the others, nothing lands outside the tensor, every pad element carries its address's channel, and a
16-byte line wholly inside a pad run leaves as one b128 store.  Each case's reason for being there is a predicate, checked here."""
import numpy as np
import pytest

import canvas_structure as S
from canvas_structure import CASES, KERNELS

KERNEL = pytest.mark.parametrize("eb,layout", KERNELS, ids=["%d-%s" % k for k in KERNELS])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_case_is_what_it_is_here_for(case):
    assert case.holds(), case.why
    (oh, ow), (x, y), (ch, cw) = case.size, case.origin, case.canvas
    assert x >= 0 and y >= 0 and x + ow <= cw and y + oh <= ch
    assert case.box[2] <= 16 * ow and case.box[3] <= 16 * oh


def test_the_table_of_the_issue():
    want = {"letterbox": ((27, 40), (0, 6), (40, 40)), "pillarbox": ((40, 20), (10, 0), (40, 40)), "all-start-classes": ((17, 33), (2, 1), (19, 37)),
            "one-line": ((4, 3), (5, 2), (9, 12)), "one-element-pad": ((8, 32), (1, 1), (10, 34)), "small-image-big-canvas": ((8, 8), (190, 55), (64, 200)),
            "canvas-equals-image": ((4, 38), (0, 0), (4, 38))}
    for name, v in want.items():
        c = S.BY_NAME[name]
        assert (c.size, c.origin, c.canvas) == v
    c = S.BY_NAME["unfused-road"]
    assert c.canvas == (32, 48) and c.stream == "100x57"
    assert {n for n, c in S.BY_NAME.items() if S.BICUBIC in c.filters} >= {"all-start-classes", "one-line", "canvas-equals-image"}


@KERNEL
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_byte_has_one_writer(case, eb, layout):
    f = case.facts(eb, layout)
    assert f["in_bounds"], "a store leaves the tensor"
    w = f["writers"]
    assert len(w) == 3 * case.canvas[0] * case.canvas[1] * eb
    bad = np.flatnonzero(w != 1)
    assert not len(bad), "byte %d has %d writers (%d bytes are not written once)" % (bad[0], w[bad[0]], len(bad))
    assert f["sides_ok"], "an image store on a pad byte, or a pad store on an image byte"
    assert f["channel_ok"], "a pad element with another channel's value"


@KERNEL
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_lines_and_runs(case, eb, layout):
    f = case.facts(eb, layout)
    runs, kinds = f["runs"], f["kinds"]
    # the runs are the complement of the image, from the definition
    mask = S.image_mask(case.size, case.origin, case.canvas, eb, layout)
    assert sum(b - a for a, b in runs) == int((~mask).sum()) and all(not mask[a:b].any() for a, b in runs)
    assert all(mask[a - 1] for a, _ in runs if a > 0) and all(mask[b] for _, b in runs if b < len(mask))
    inside = np.zeros(len(kinds), dtype=bool)          # the whole lines wholly inside a run
    for a, b in runs:
        inside[(a + 15) // 16:b // 16] = True
    for i, k in enumerate(kinds):
        whole_image = bool(mask[16 * i:16 * i + 16].all()) and 16 * i + 16 <= len(mask)
        if inside[i]:
            assert k == {"pad b128"}, (i, k)
        elif whole_image:
            assert k <= {"image b128", "image elem"} and k, (i, k)
        else:
            assert "pad b128" not in k and "image b128" not in k and k, (i, k)
    # the launch: image tile rows, then whole rows of workgroups for the pad -- none when the image fills the canvas
    gx, gy, extra = f["grid"]
    assert (extra == 0) == (case.size == case.canvas) and gy + extra <= 65535 and extra * gx >= f["pad_groups"]


def test_the_largest_canvas_fits_the_grid():
    """4096 x 4096 fp32 around a one-tile image: the pad's workgroup rows stay inside gridDim.y"""
    rows, groups = S.pad_groups((1, 1), (4096, 4096), 4, 1)
    assert rows == groups == 3 * 4096 * 4096 * 4 // 16 // S.PAD_LINES_PER_GROUP and rows + 1 <= 65535
