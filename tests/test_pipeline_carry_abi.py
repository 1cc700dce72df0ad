"""CPU: boxes carried along the motion vectors (include/leon_pipeline.h, leon_pipeline_carry_regions) -- the structs' sizes, the
resolution of a window's references (leon_pipeline_carry_refs) on hand-written frame lists, the library's CPU evaluation of one hop
(leon_pipeline_carry_record) against leon_ctypes.carry_box, the header's text in Python integers, on hand-written records, and the
hop levels of carry_plan.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import carry_cases as K
from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def test_struct_sizes_and_symbols(L, tmp_path):
    assert C.sizeof(L.PipelineCarryRegion) == 32 and L.PipelineCarryRegion.target.offset == 20 and L.PipelineCarryRegion.reserved.offset == 24
    assert C.sizeof(L.PipelineCarryRegionsCall) == 64
    call = L.PipelineCarryRegionsCall
    assert [getattr(call, f).offset for f in ("regions", "n", "reserved0", "device_out", "device_votes", "device_status", "stream", "reserved")] == [0, 8, 12, 16, 24, 32, 40, 48]
    assert C.sizeof(L.PipelineRegion) == 32          # the output record
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %d\\n", sizeof(leon_pipeline_carry_region), '
                   'sizeof(leon_pipeline_carry_regions_call), LEON_REGION_NO_REFERENCE);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["32", "64", "9"]
    assert L.REGION_NO_REFERENCE == 9
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for sym in ("leon_pipeline_carry_refs", "leon_pipeline_carry_record", "leon_pipeline_get_carry_refs", "leon_pipeline_carry_regions_device",
                "leon_pipeline_carry_regions", "leon_pipeline_carry_device"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym


# a closed IBBP GOP of six pictures in display order: B0 B1 I2 B3 B4 P5 -- (display, fwd_display, bwd_display)
CLOSED6 = [(0, 2, 2), (1, 2, 2), (2, -1, -1), (3, 2, 5), (4, 2, 5), (5, 2, -1)]


def gop_frames(gop, pictures, fwd_gop=None):
    """frames and motion of one GOP: leading B pictures (display below the I picture's) name fwd_gop where it is given"""
    frames = [(gop, d) for d, _, _ in pictures]
    motion = [(fwd_gop[0] if fwd_gop is not None and d < 2 else gop, fwd_gop[1] if fwd_gop is not None and d < 2 else f, b) for d, f, b in pictures]
    return frames, motion


def test_carry_refs_closed_gops(L):
    f0, m0 = gop_frames(7, CLOSED6)
    f1, m1 = gop_frames(8, CLOSED6)
    fwd, bwd = L.carry_refs(f0 + f1, m0 + m1)
    assert fwd.tolist() == [2, 2, -1, 2, 2, 2] + [8, 8, -1, 8, 8, 8]
    assert bwd.tolist() == [2, 2, -1, 5, 5, -1] + [8, 8, -1, 11, 11, -1]
    fwd, bwd = L.carry_refs([], [])
    assert len(fwd) == 0 and len(bwd) == 0


def test_carry_refs_open_gop_predecessor_in_and_out_of_the_window(L):
    f0, m0 = gop_frames(3, CLOSED6)
    f1, m1 = gop_frames(4, CLOSED6, fwd_gop=(3, 5))          # open: the leading B pictures point into GOP 3's last anchor
    fwd, bwd = L.carry_refs(f0 + f1, m0 + m1)                # both GOPs in the window
    assert fwd.tolist() == [2, 2, -1, 2, 2, 2] + [5, 5, -1, 8, 8, 8]
    assert bwd.tolist() == [2, 2, -1, 5, 5, -1] + [8, 8, -1, 11, 11, -1]
    fwd, bwd = L.carry_refs(f1, m1)                          # the predecessor in an earlier window
    assert fwd.tolist() == [-1, -1, -1, 2, 2, 2] and bwd.tolist() == [2, 2, -1, 5, 5, -1]
    # the same display index in another GOP is no match
    fwd, bwd = L.carry_refs(f1 + gop_frames(9, CLOSED6)[0], m1 + gop_frames(9, CLOSED6)[1])
    assert fwd.tolist()[:3] == [-1, -1, -1]


def test_carry_refs_trimmed_anchor(L):
    """an EXACT seek onto display position 4: I2 was reconstructed and not delivered, so nothing of the window is that picture"""
    frames, motion = gop_frames(3, CLOSED6[4:])
    fwd, bwd = L.carry_refs(frames, motion)
    assert fwd.tolist() == [-1, -1] and bwd.tolist() == [1, -1]
    # dicts, as a callback gets them
    fwd2, bwd2 = L.carry_refs([{"gop": g, "display_index": d} for g, d in frames], [{"fwd_gop": g, "fwd_display": f, "bwd_display": b} for g, f, b in motion])
    assert fwd2.tolist() == fwd.tolist() and bwd2.tolist() == bwd.tolist()


FW, FH, MBW, MBH = 61, 45, 4, 3          # a frame smaller than its coded grid


def record_of(L, records, rec, fill=-7, fw=FW, fh=FH, mbw=MBW, mbh=MBH):
    """(status, out, votes) of the library, asserted equal to carry_box's, with `fill` where nothing is written"""
    st, out, votes = L.carry_record(fw, fh, mbw, mbh, K.N_FRAMES, K.FWD, K.BWD, records, rec, fill=fill)
    want = K.expected(L, fw, fh, records, [rec], fill)
    K.assert_equal((out[None], votes[None], np.array([st])), want, [rec], "carry_record")
    return st, out.tolist(), votes.tolist()


@pytest.mark.parametrize("dx,dy", [(3, 2), (-5, 1), (0, -4), (7, -7)])
def test_uniform_field_moves_the_box_exactly(L, dx, dy):
    records = [None, K.uniform(MBW, MBH, (2 * dx, 2 * dy, 0, 0), 1), None]
    box = (20, 15, 18, 13)
    st, out, votes = record_of(L, records, (0, *box, 1))          # from the reference to the P picture: sense -1
    assert st == 0 and out == [1, 20 - dx, 15 - dy, 18, 13, 0, 0, 0] and votes == [18 * 13, 0, -dx, -dy]
    st, out, votes = record_of(L, records, (1, *box, 0))          # from the P picture to its reference: sense +1
    assert st == 0 and out == [0, 20 + dx, 15 + dy, 18, 13, 0, 0, 0] and votes == [18 * 13, 0, dx, dy]


@pytest.mark.parametrize("v,minus,plus", [(1, 0, 1), (-1, 1, 0), (3, -1, 2), (-3, 2, -1), (2, -1, 1), (-2, 1, -1), (5, -2, 3), (-5, 3, -2)])
def test_ties_round_up_with_floor_division(L, v, minus, plus):
    """a uniform half-pel field of v: sense -1 gives floor(-v/2 + 1/2), sense +1 floor(v/2 + 1/2) -- .5 goes up on both sides of zero"""
    records = [None, K.uniform(MBW, MBH, (v, -v, 0, 0), 1), None]
    st, out, votes = record_of(L, records, (0, 20, 15, 9, 9, 1))
    assert st == 0 and votes[2:] == [minus, plus] and minus == (-v + 1) // 2
    st, out, votes = record_of(L, records, (1, 20, 15, 9, 9, 0))
    assert st == 0 and votes[2:] == [plus, minus] and plus == (v + 1) // 2


def test_all_intra_leaves_the_box(L):
    records = [None, K.uniform(MBW, MBH, (0, 0, 0, 0), 4), None]
    st, out, votes = record_of(L, records, (0, 3, 5, 40, 33, 1))
    assert st == 0 and out == [1, 3, 5, 40, 33, 0, 0, 0] and votes == [0, 40 * 33, 0, 0]


def test_same_frame_returns_the_box(L):
    st, out, votes = record_of(L, [None, None, None], (2, 3, 5, 40, 33, 2))
    assert st == 0 and out == [2, 3, 5, 40, 33, 0, 0, 0] and votes == [0, 0, 0, 0]


def test_both_directions_vote_twice(L):
    """D = 3: a bidirectional macroblock adds its weight for each direction"""
    records = [None, None, K.uniform(MBW, MBH, (8, 0, 16, 4), 3)]
    st, out, votes = record_of(L, records, (0, 20, 15, 10, 10, 2))
    assert st == 0 and votes == [200, 0, -6, -1] and out[1:3] == [14, 14]          # -(8 + 16) / 4 = -6, -(0 + 4) / 4 = -1
    st, out, votes = record_of(L, records, (2, 20, 15, 10, 10, 0))
    assert st == 0 and votes == [200, 0, 6, 1]
    mixed = K.varied(MBW, MBH, 5)
    assert {1, 2, 3, 4} <= set(mixed[1].reshape(-1).tolist())
    for rec in K.pairs([(0, 0, 61, 45), (17, 3, 30, 40), (16, 16, 16, 16)]):
        record_of(L, [None, K.window(MBW, MBH, 9)[1], mixed], rec)


@pytest.mark.parametrize("vec,box,want", [((200, 0), (5, 10, 20, 20), (0, 10)), ((-200, 0), (30, 10, 20, 20), (41, 10)),
                                          ((0, 200), (5, 10, 20, 20), (5, 0)), ((0, -200), (5, 10, 20, 20), (5, 25))])
def test_clamp_at_each_frame_edge(L, vec, box, want):
    records = [None, K.uniform(MBW, MBH, vec + (0, 0), 1), None]
    st, out, votes = record_of(L, records, (0, *box, 1))
    assert st == 0 and tuple(out[1:3]) == want and votes[2:] == [-vec[0] // 2, -vec[1] // 2]          # the votes are before the clamp


def test_status_words_in_their_order(L):
    records = K.window(MBW, MBH, 3)
    cases = [((0, 1, 1, 8, 8, 1, 1, 0), L.REGION_RESERVED), ((0, 1, 1, 8, 8, 1, 0, -1), L.REGION_RESERVED),
             ((9, 1, 1, 0, 8, 1, 0, 5), L.REGION_RESERVED),                    # the reserved word in front of the frame and the box
             ((3, 1, 1, 0, 8, 1), L.REGION_FRAME), ((-1, 1, 1, 8, 8, 1), L.REGION_FRAME),
             ((0, 1, 1, 8, 8, 3), L.REGION_FRAME), ((0, 1, 1, 8, 8, -1), L.REGION_FRAME),          # the target too
             ((1, 1, 1, 0, 8, 2), L.REGION_BOX),                                # an empty box in front of the missing reference
             ((0, 1, 1, 8, 0, 1), L.REGION_BOX), ((0, -1, 1, 8, 8, 1), L.REGION_BOX), ((0, 1, -1, 8, 8, 1), L.REGION_BOX),
             ((0, 54, 1, 8, 8, 1), L.REGION_BOX), ((0, 1, 38, 8, 8, 1), L.REGION_BOX), ((0, 0, 0, 62, 45, 1), L.REGION_BOX),
             ((0, 2 ** 31 - 1, 1, 2 ** 31 - 1, 8, 1), L.REGION_BOX),
             ((1, 1, 1, 8, 8, 2), L.REGION_NO_REFERENCE), ((2, 1, 1, 8, 8, 1), L.REGION_NO_REFERENCE),
             ((0, 53, 37, 8, 8, 1), L.REGION_OK), ((0, 0, 0, 61, 45, 2), L.REGION_OK)]
    for rec, want in cases:
        st, out, votes = record_of(L, records, rec + (0,) * (8 - len(rec)))
        assert st == want, (rec, st, want)
        if st:
            assert out == [-7] * 8 and votes == [-7] * 4, "a refused record was written: %s" % (rec,)


def test_record_pointers_and_refusals(L):
    records = K.window(MBW, MBH, 3)
    # a NULL record is allowed for frames that are not M ...
    st, _, _ = record_of(L, [None, records[1], None], (0, 1, 1, 8, 8, 1))
    assert st == 0
    # ... and refused where M's is needed
    with pytest.raises(L.LeonError) as e:
        L.carry_record(FW, FH, MBW, MBH, 3, K.FWD, K.BWD, [records[0], None, None], (0, 1, 1, 8, 8, 1))
    assert e.value.code == L.ERR_INVALID and "no record" in str(e.value)
    for fw, fh, mbw, mbh in ((65, 45, 4, 3), (61, 49, 4, 3), (0, 45, 4, 3), (61, 45, 0, 3), (61, 45, 4, 257)):
        with pytest.raises(L.LeonError):
            L.carry_record(fw, fh, mbw, mbh, 3, K.FWD, K.BWD, records, (0, 1, 1, 8, 8, 1))
    lib = L.load()
    assert lib.leon_pipeline_carry_record(FW, FH, MBW, MBH, 3, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.leon_pipeline_carry_refs(None, None, 3, None, None) == L.ERR_INVALID


def test_carry_record_equals_carry_box_on_seeded_records(L):
    """boxes of every alignment against a varied window, every joined pair and both senses"""
    fw, fh, mbw, mbh = 96, 64, 6, 4
    records = K.window(mbw, mbh, 21)
    rng = np.random.default_rng(4)
    boxes = [(0, 0, 96, 64), (0, 0, 1, 1), (95, 63, 1, 1), (16, 16, 32, 16), (15, 15, 18, 18), (1, 1, 16, 16)]
    for _ in range(40):
        x, y = int(rng.integers(0, 96)), int(rng.integers(0, 64))
        boxes.append((x, y, int(rng.integers(1, 96 - x + 1)), int(rng.integers(1, 64 - y + 1))))
    moved = 0
    for rec in K.pairs(boxes):
        st, out, votes = record_of(L, records, rec, fw=fw, fh=fh, mbw=mbw, mbh=mbh)
        assert st == 0
        moved += votes[2] != 0 or votes[3] != 0
    assert moved > 40


def ibbp_window(n):
    """(refs, frames, index of a display position) of synth.gop_ibbp(n) delivered whole, in display order"""
    import synth as S
    gop = S.gop_ibbp(n)
    order = sorted(d for _, d, _, _ in gop)
    at = {d: i for i, d in enumerate(order)}
    frames, fwd, bwd = [None] * n, [-1] * n, [-1] * n
    for t, d, f, b in gop:
        frames[at[d]] = {"gop": 4, "display_index": d, "type": t}
        if t == S.PIC_B and f is None:
            f = b          # a closed GOP's leading B picture names its I picture for both
        fwd[at[d]] = -1 if f is None else at[f]
        bwd[at[d]] = -1 if b is None else at[b]
    return (fwd, bwd), frames, at


@pytest.mark.parametrize("n", [6, 9, 12])
@pytest.mark.parametrize("start", ["I", "last P"])
def test_carry_plan_reaches_every_frame_once(L, n, start):
    import synth as S
    refs, frames, at = ibbp_window(n)
    src = at[2] if start == "I" else at[max(f["display_index"] for f in frames if f["type"] == S.PIC_P)]
    # frames of another GOP in the window play no part
    other = [{"gop": 5, "display_index": 2, "type": S.PIC_I}]
    levels, unreachable = L.carry_plan((refs[0] + [-1], refs[1] + [-1]), frames + other, src)
    assert unreachable == []
    carried, fwd, bwd = {src}, refs[0], refs[1]
    for hops in levels:
        assert hops
        for a, b in hops:
            assert a in carried, "level source %d was not carried earlier" % a
            assert fwd[b] == a or bwd[b] == a or fwd[a] == b or bwd[a] == b, "no prediction joins %d and %d" % (a, b)
        targets = [b for _, b in hops]
        assert len(set(targets)) == len(targets) and not set(targets) & carried, "a frame is reached twice"
        carried |= set(targets)
    assert carried == set(range(n))
    # B pictures go from the nearer of their references
    for hops in levels:
        for a, b in hops:
            if frames[b]["type"] == S.PIC_B:
                near = min({fwd[b], bwd[b]}, key=lambda r: (abs(frames[r]["display_index"] - frames[b]["display_index"]), r != fwd[b]))
                assert a == near, (a, b, near)


def test_carry_plan_lists_what_it_cannot_reach(L):
    """the trimmed GOP: B4 and P5 delivered, their I picture not -- from P5, B4 is reached through its backward reference; with the
    P picture's forward reference gone nothing else is; from a GOP whose leading B pictures point into an earlier window they are still
    reached through their backward reference"""
    levels, unreachable = L.carry_plan(([-1, -1], [1, -1]), [(3, 4, 3), (3, 5, 2)], 1)
    assert levels == [[(1, 0)]] and unreachable == []
    levels, unreachable = L.carry_plan(([-1, -1, -1], [2, -1, -1]), [(3, 4, 3), (3, 8, 2), (3, 5, 2)], 1)
    assert levels == [] and unreachable == [0, 2]
    refs, frames, at = ibbp_window(6)
    fwd = [-1 if frames[i]["display_index"] < 2 else v for i, v in enumerate(refs[0])]
    levels, unreachable = L.carry_plan((fwd, refs[1]), frames, at[2])
    assert unreachable == [] and {(at[2], at[0]), (at[2], at[1])} <= set(levels[-1])
