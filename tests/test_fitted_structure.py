"""CPU: the structure of k_fitted, from tests/fitted_structure.py -- the kernel's own grid and store expressions.  For every region of
the calls the fit's tests share, both anchors and all six element-size / layout kernels: every byte of the region's tensor is stored
exactly once, pad stores cover pad bytes only and image stores image bytes only, idle tiles are exactly the canvas's tiles the image
has none of, and nothing is stored outside the tensor.  Then the facts each box is listed for, the rectangles the issue computed, and
that the pure-Python letterbox integers are the library's (leon_pipeline_region_fit_rect, leon_pipeline_letterbox)."""
import numpy as np
import pytest

import fitted_structure as F
from fitted_structure import ANCHORS, CALLS, CENTRE, KERNELS, TOP_LEFT

CASES = [(name, i) for name in sorted(CALLS) for i in range(len(CALLS[name].listed))]


@pytest.mark.parametrize("name,i", CASES, ids=lambda v: str(v))
def test_every_byte_once_by_the_right_kind_of_store(name, i):
    call = CALLS[name]
    box = call.listed[i][0]
    for anchor in ANCHORS:
        for eb, layout in KERNELS:
            f = F.region_facts(box[2:], call.size, anchor, eb, layout)
            what = (name, box, anchor, eb, layout)
            assert f["in_bounds"], what
            assert ((f["image_writers"] + f["pad_writers"]) == 1).all(), what
            assert (f["image_writers"][~f["mask"]] == 0).all() and (f["pad_writers"][f["mask"]] == 0).all(), what
            gx, gy, pad_rows = f["grid"]
            assert len(f["idle"]) == gx * gy - f["tiles"][0] * f["tiles"][1], what
            assert pad_rows >= 1 and pad_rows * gx * 1024 * 16 >= f["bytes"], what


def test_the_listed_rectangles_and_facts():
    seen = set()
    for name, call in CALLS.items():
        ch, cw = call.size
        gx, gy, _ = F.grid(call.size, 1)
        for box, (w, h, x, y), facts in call.listed:
            assert F.rect(box, call.size) == (x, y, w, h), (name, box)
            assert F.rect(box, call.size, TOP_LEFT) == (0, 0, w, h)
            f = F.region_facts(box[2:], call.size, CENTRE, 1, "hwc")
            assert (F.FILLS in facts) == ((w, h) == (cw, ch)) == bool(f["mask"].all()), (name, box)
            assert (F.FEWER_COLUMNS in facts) == (f["tiles"][0] < gx), (name, box)
            assert (F.FEWER_ROWS in facts) == (f["tiles"][1] < gy), (name, box)
            assert (F.ONE_COLUMN in facts) == (w == 1), (name, box)
            assert (F.RATIO_16 in facts) == (box[2] == 16 * w or box[3] == 16 * h), (name, box)
            seen.update(facts)
    assert seen == {F.FILLS, F.FEWER_COLUMNS, F.FEWER_ROWS, F.ONE_COLUMN, F.RATIO_16}
    assert F.grid(CALLS["96x64"].size, 1)[:2] == (2, 3) and CALLS["96x64"].size[1] & 1


def test_a_fill_has_no_pad_store_and_one_column_one_store_per_row():
    for eb, layout in KERNELS:
        f = F.region_facts((74, 38), (19, 37), CENTRE, eb, layout)
        assert f["pad_writers"].sum() == 0 and f["image_writers"].sum() == f["bytes"]
        f = F.region_facts((3, 60), (19, 37), CENTRE, eb, layout)
        assert f["image_writers"].sum() == 3 * 19 * eb


def test_the_restatement_is_the_librarys():
    import leon_ctypes as L
    rng = np.random.default_rng(37)
    sizes = [(b[2], b[3], c.size) for c in CALLS.values() for b in c.boxes]
    sizes += [(int(w), int(h), (int(ch), int(cw))) for w, h, cw, ch in rng.integers(1, 4097, (300, 4))]
    sizes += [(1, 4096, (1, 4096)), (4096, 1, (4096, 1)), (4096, 1, (1, 4096)), (1, 1, (4096, 4096)), (4095, 4096, (4096, 4095))]
    for w, h, (ch, cw) in sizes:
        ow, oh, x, y = L.letterbox(w, h, cw, ch)
        assert F.letterbox(w, h, cw, ch) == (ow, oh, x, y)
        assert L.region_fit_rect(w, h, (ch, cw)) == F.rect((0, 0, w, h), (ch, cw)) == (x, y, ow, oh)
        assert L.region_fit_rect(w, h, (ch, cw), anchor="top_left") == F.rect((0, 0, w, h), (ch, cw), TOP_LEFT) == (0, 0, ow, oh)
        assert 1 <= ow <= cw and 1 <= oh <= ch and x + ow <= cw and y + oh <= ch
        assert L.region_fit_rect(w, h, (ch, cw), fit=None) == (0, 0, cw, ch)
