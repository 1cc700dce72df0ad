"""CPU: what the calls of tests/regions_structure.py hold, proved from resample_structure.tile_facts (the kernel's own expressions over
the tables of leon_ctypes.resize_weights): one launch of k_regions mixes regions of 2 taps and of 32 (bicubic: 4 and 64), footprints of
one chunk and of seven, boxes on every frame edge, every start offset of the staged groups, the fill row tapped and not tapped.  Also
the placement of a call's output: region_bytes and the default pitch."""
import pytest

import regions_structure as S
from regions_structure import BICUBIC, CALLS, FILTERS, TRIANGLE
from resample_structure import STREAMS


def facts(call, filt):
    return [call.tiles(b, filt) for b in call.boxes]


def test_boxes_lie_inside_their_frames_and_the_streams_exist():
    for name, call in CALLS.items():
        assert name in STREAMS
        fw, fh = call.frame
        for x, y, w, h in call.boxes + ([call.refused] if call.refused else []):
            assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= fw and y + h <= fh
        oh, ow = call.size
        assert all(w <= 16 * ow and h <= 16 * oh for _, _, w, h in call.boxes)


@pytest.mark.parametrize("filt", FILTERS)
def test_608x57_mixes_ratio_16_identity_and_enlargement(filt):
    call = CALLS["608x57"]
    assert call.frame == (608, 57) and call.size == (13, 37)
    t = facts(call, filt)
    widest, least = (32, 2) if filt == TRIANGLE else (64, 4)
    # ratio 16 across: the filter's widest rows, the footprint split into 6 or 7 chunks
    for k in (0, 4):
        assert call.boxes[k][2] == 16 * call.size[1]
        assert max(x["taps_x"][1] for x in t[k]) == widest and max(x["n_chunks"] for x in t[k]) in (6, 7)
    # identity: every row of both tables has the filter's least taps
    assert call.boxes[1][2:] == (call.size[1], call.size[0])
    assert all(x["taps_x"] == (least, least) and x["taps_y"] == (least, least) and x["n_chunks"] == 1 for x in t[1])
    # an enlargement of about 2
    assert 2 * call.boxes[2][2] in (call.size[1] - 1, call.size[1] + 1) and all(x["taps_x"][1] == least for x in t[2])
    # so one call holds regions whose table rows are `least` and `widest` entries long
    assert {max(x["taps_x"][1] for x in r) for r in t} >= {least, widest}
    # boxes on the left, right, top and bottom frame edges
    fw, fh = call.frame
    assert any(b[0] == 0 for b in call.boxes) and any(b[0] + b[2] == fw for b in call.boxes)
    assert any(b[1] == 0 for b in call.boxes) and any(b[1] + b[3] == fh for b in call.boxes)
    # the fill row (the last row of the odd height) is tapped by the first and the fourth box, not by the second and the third
    tapped = [any(x["fill_weights"] for x in r) for r in t]
    assert fh & 1 and tapped[0] and tapped[3] and not tapped[1] and not tapped[2]
    # partial tiles on both axes: 37 = 32 + 5, 13 = 8 + 5
    assert all({x["nox"] for x in r} == {32, 5} and {x["noy"] for x in r} == {8, 5} for r in t)


def test_608x57_start_offsets():
    offs = {x["x_off"] for r in facts(CALLS["608x57"], TRIANGLE) for x in r}
    assert offs >= {0, 3, 4, 5}
    assert len({x["x_off"] for r in facts(CALLS["608x57"], BICUBIC) for x in r}) >= 4


def test_608x57_the_refused_box_reduces_by_more_than_16():
    call = CALLS["608x57"]
    x, y, w, h = call.refused
    assert w > 16 * call.size[1] and h <= 16 * call.size[0]
    import leon_ctypes as L
    with pytest.raises(ValueError, match="reduces by more than 16"):
        L.resize_weights(call.frame[0], x, w, call.size[1])


@pytest.mark.parametrize("filt", FILTERS)
def test_96x64_corners_single_tiles_and_one_pixel(filt):
    call = CALLS["96x64"]
    fw, fh = call.frame
    t = facts(call, filt)
    assert all(len(r) == 1 and r[0]["nox"] == 32 and r[0]["noy"] == 8 for r in t)          # a region is one whole tile
    corners = {(b[0] == 0, b[1] == 0) for b in call.boxes if (b[0] == 0 or b[0] + b[2] == fw) and (b[1] == 0 or b[1] + b[3] == fh) and b[2:] != (fw, fh)}
    assert corners == {(True, True), (True, False), (False, True), (False, False)}
    assert call.boxes[-1] == (fw - 1, fh - 1, 1, 1)          # one pixel enlarged to 32 x 8
    assert any(b[0] & 1 and b[1] & 1 for b in call.boxes)
    if filt == TRIANGLE:
        assert {r[0]["x_off"] for r in t} >= {0, 6, 7} and {r[0]["y_off"] for r in t} == {0, 1}


@pytest.mark.parametrize("filt", FILTERS)
def test_100x57_the_unfused_road(filt):
    call = CALLS["100x57"]
    fw, fh = call.frame
    assert fw % 8 and fh & 1
    t = facts(call, filt)
    assert all(len(r) == 2 for r in t)
    tapped = [any(x["fill_weights"] for x in r) for r in t]
    assert tapped[0] and tapped[1] and tapped[2] and not tapped[4]
    assert len({max(x["taps_x"][1] for x in r) for r in t}) >= 3          # regions of several row lengths in one call


def test_regions_cover_every_frame_out_of_order():
    for call in CALLS.values():
        regs = call.regions(9)
        frames = [r[0] for r in regs]
        assert len(regs) == 10 and set(frames) == set(range(9)) and frames != sorted(frames)
        assert frames.count(frames[0]) == 2          # two regions on one frame
        assert {r[1:] for r in regs} == set(call.boxes)


def test_region_bytes_and_the_default_pitch():
    assert S.placement((13, 37), 1) == (1443, 1536)          # a gap of 93 bytes behind every region
    assert S.placement((13, 37), 2) == (2886, 3072)
    assert S.placement((13, 37), 4) == (5772, 5888)
    assert S.placement((8, 32), 1) == (768, 768) and S.placement((16, 24), 2) == (2304, 2304)          # dense
    for eb in (1, 2, 4):
        n, pitch = S.placement((224, 224), eb)
        assert n == pitch == 150528 * eb          # 224 x 224 is dense in every element type
