"""CPU: the facts the shared warp calls (tests/warp_structure.py) exist for, proved from the kernel's expressions stated there -- a
tile whose footprint fits the stage and one that must be split, a piece wholly outside the frame, footprints cut by each of the four
frame edges, a footprint that takes the fill row of an odd height -- and what k_warp stands on whatever the record: every tap of every
sample of a piece lies inside the piece's staged box, every staged box fits the stage, and the smallest piece fits it for every
matrix the judgement lets through."""
import math

import numpy as np
import pytest

import warp_structure as W

CASES = [(name, size) for name in sorted(W.SIZES) for size in W.SIZES[name]]


def facts(name, size):
    wh = W.frame_wh(name)
    return {mname: W.tile_facts(wh, m, size) for mname, m in W.matrices(wh, size)}


def pieces(tiles):
    return [p for t in tiles for p in t["pieces"]]


def test_a_tile_that_fits_and_one_that_must_split():
    f = facts("100x57", (8, 32))
    assert [t["level"] for t in f["identity"]] == [0] and len(pieces(f["identity"])) == 1
    assert [t["level"] for t in f["rot45"]] == [0]
    split = f["rot45_scale4"]
    assert split[0]["g"] == 2 and not split[0]["whole_fits"] and split[0]["level"] == 1 and len(pieces(split)) == 2
    # the whole tile's footprint is indeed too large for the stage, not only its bound
    sx0, sx1, sy0, sy1 = W.footprint(dict(W.matrices(W.frame_wh("100x57"), (8, 32)))["rot45_scale4"], 2, 0, 0, 32, 8)
    assert (sx1 - sx0 + 1) * (sy1 - sy0) > W.STAGE_PX
    # three tiles on both axes, S = 1, 2 and 4 side by side in one call
    many = facts("608x57", (24, 70))
    assert len(many["identity"]) == 9 and {many[k][0]["g"] for k in ("identity", "scale2", "rot45_scale4")} == {0, 1, 2}


@pytest.mark.parametrize("name,size", CASES, ids=lambda v: str(v))
def test_outside_edges_and_the_fill_row(name, size):
    f = facts(name, size)
    fw, fh = W.frame_wh(name)
    assert all(p["outside"] for p in pieces(f["outside"]))
    assert not any(p["outside"] for p in pieces(f["identity"]))
    for edge in ("left", "right", "top", "bottom"):
        assert any(p["cut_" + edge] and not p["outside"] for p in pieces(f[edge])), edge
    if fh & 1:
        assert any(p["fill_row"] for p in pieces(f["bottom"])) and any(p["fill_row"] for p in pieces(f["fill_row"]))
    if fw & 7:          # a width that is no multiple of 8: a staged group of 8 columns holds frame and pad
        assert any(p["box"][0] < fw < p["box"][1] and (fw - p["box"][0]) & 7 for p in pieces(f["right"]))


@pytest.mark.parametrize("name,size", CASES, ids=lambda v: str(v))
def test_every_tap_lies_in_its_piece_box_and_every_box_fits(name, size):
    wh = W.frame_wh(name)
    for mname, m in W.matrices(wh, size):
        W.assert_record_facts(wh, mname, m, size)


def test_the_smallest_piece_fits_whatever_the_matrix():
    """|a| <= 2^(16 + g) + 1 for every entry the judgement lets through: the last level's bound fits the stage for all of them, and the
    first level that fits is found for columns of the largest norm at every angle"""
    for g in range(3):
        lim = (1 << (16 + g)) + 1
        worst = (lim, lim, 0, lim, lim, 0)          # beyond what any legal matrix has: each column's norm is at most lim
        pw, ph = W.piece_size(W.LEVELS - 1)
        assert (W.span_bound(lim, lim, g, pw, ph, 8) + 1) * W.span_bound(lim, lim, g, pw, ph, 2) <= W.STAGE_PX
        assert W.level_fits(worst, g, W.LEVELS - 1)
        for deg0 in range(0, 360, 5):
            for deg1 in range(0, 360, 15):
                m = (int(lim * math.cos(math.radians(deg0))), int(lim * math.cos(math.radians(deg1))), 12345,
                     int(lim * math.sin(math.radians(deg0))), int(lim * math.sin(math.radians(deg1))), -54321)
                assert W.supersample(m) is not None and W.supersample(m) <= g
                assert W.level_fits(m, g, W.level_of(m, g))
    assert W.piece_size(0) == (W.TILE_X, W.TILE_Y) and [W.piece_size(k) for k in range(W.LEVELS)] == [(32, 8), (16, 8), (16, 4), (8, 4), (8, 2)]


def test_the_regions_are_dealt_over_every_frame_out_of_order():
    regs = W.regions(W.frame_wh("96x64"), (8, 32), 9)
    frames = [r[0] for r in regs]
    assert set(frames) == set(range(9)) and frames != sorted(frames) and len(frames) > len(set(frames))
