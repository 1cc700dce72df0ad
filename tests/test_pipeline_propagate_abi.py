"""CPU: dense maps propagated along the motion vectors (include/leon_pipeline.h, leon_pipeline_propagate_maps) -- the structs' sizes,
the layout call, the library's CPU evaluation of one hop (leon_pipeline_propagate_record: the text k_propagate compiles too) against
leon_ctypes.propagate_map, the header's text in numpy integers, on hand-written records, and the levels of propagate_plan.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import carry_cases as K
import propagate_cases as M
from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def test_struct_sizes_and_symbols(L, tmp_path):
    assert C.sizeof(L.PipelinePropagateHop) == 32 and L.PipelinePropagateHop.reserved.offset == 16
    assert C.sizeof(L.PipelinePropagateConfig) == 40
    assert [getattr(L.PipelinePropagateConfig, f).offset for f in ("stride", "planes", "elem_bytes", "n_slots", "fill", "reserved0", "slot_pitch_bytes", "maps_bytes")] == \
        [0, 4, 8, 12, 16, 20, 24, 32]
    assert C.sizeof(L.PipelinePropagateLayout) == 32
    call = L.PipelinePropagateMapsCall
    assert C.sizeof(call) == 64
    assert [getattr(call, f).offset for f in ("hops", "n", "reserved0", "maps", "device_via", "device_status", "stream", "reserved")] == [0, 8, 12, 16, 24, 32, 40, 48]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n", sizeof(leon_pipeline_propagate_hop), '
                   'sizeof(leon_pipeline_propagate_config), sizeof(struct leon_pipeline_propagate_layout), sizeof(leon_pipeline_propagate_maps_call), '
                   'LEON_REGION_SLOT);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["32", "40", "32", "64", "10"]
    assert L.REGION_SLOT == 10
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for sym in ("leon_pipeline_propagate_layout", "leon_pipeline_propagate_record", "leon_pipeline_propagate_maps_device", "leon_pipeline_propagate_maps",
                "leon_pipeline_propagate_kernel"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym


@pytest.mark.parametrize("fw,fh", [(64, 48), (61, 45), (16, 16), (4096, 4096)])
def test_layout(L, fw, fh):
    for s in M.STRIDES:
        for e in M.ELEMS:
            for planes in (1, 3, 4, 5, 4096):
                lay = L.propagate_layout(fw, fh, s, planes, e)
                mh, mw = M.cells(fw, fh, s)
                assert (lay.mw, lay.mh, lay.plane_bytes, lay.slot_bytes) == (mw, mh, mh * mw * e, planes * mh * mw * e)
                assert lay.fast_path == int((mw * e) % 4 == 0 and ((16 // s) * e) % 4 == 0)
                assert 1 <= lay.planes_per_group <= planes
                assert not lay.fast_path or lay.slot_bytes % 4 == 0
    for bad in ((0, 48, 1, 1, 1), (64, 4097, 1, 1, 1), (64, 48, 3, 1, 1), (64, 48, 32, 1, 1), (64, 48, 0, 1, 1), (64, 48, 1, 0, 1), (64, 48, 1, 4097, 1), (64, 48, 1, 1, 3),
                (64, 48, 1, 1, 8)):
        with pytest.raises(L.LeonError):
            L.propagate_layout(*bad)


def both(L, fw, fh, mbw, mbh, records, hops, s, maps, fill=0, what=""):
    """every hop through propagate_record (each on the result of the one before, as the oracle does) against propagate_map"""
    want = M.expected(L, fw, fh, len(records), records, hops, s, maps, fill)
    got_maps, buf = M.pitched(maps)          # (a pitch is a multiple of 4: the map's bytes rounded up)
    via, status = [], []
    for h in hops:
        st, v = L.propagate_record(fw, fh, mbw, mbh, len(records), records, h, s, got_maps, fill, via_fill=M.VIA_FILL)
        status.append(st)
        via.append(v)
    M.assert_equal((got_maps, np.array(via), np.array(status)), want, what)
    assert (buf[:, maps[0].nbytes:] == 0xA5).all(), what
    return want


@pytest.mark.parametrize("s", M.STRIDES)
def test_every_tie_of_both_signs(L, s):
    """uniform fields with every vector component in -4s .. 4s: every rounding case of floor((v + s) / (2 s)), ties of both signs among
    them, forward with (v, -v) and backward with (-v, v)"""
    fw, fh, mbw, mbh = 64, 48, 4, 3
    rng = np.random.default_rng(s)
    maps = M.rand_maps(rng, 3, 2, fw, fh, s, 2)
    for v in range(-4 * s, 4 * s + 1):
        records = [None, K.uniform(mbw, mbh, (v, -v, -v, v), 3)]
        want = both(L, fw, fh, mbw, mbh, records, [(1, 2, 0, -1), (1, 2, -1, 1)], s, maps, what="s %d, v %d" % (s, v))
        # the rounding itself, by hand, on the last hop (backward, (-v, v)): cells moved = floor((component + s) / (2 s))
        dx, dy = (-v + s) // (2 * s), (v + s) // (2 * s)
        mh, mw = M.cells(fw, fh, s)
        cy, cx = mh // 2, mw // 2
        if 0 <= cx + dx < mw and 0 <= cy + dy < mh:
            assert want[0][2, 0, cy, cx] == maps[1, 0, cy + dy, cx + dx]


@pytest.mark.parametrize("e", M.ELEMS)
def test_info_against_the_supplied_slots(L, e):
    """info 0, 1, 2, 3, 4 against forward only, backward only, both, neither, and one slot used for both"""
    fw, fh, mbw, mbh, s = 64, 48, 4, 3, 2
    rng = np.random.default_rng(10 + e)
    maps = M.rand_maps(rng, 4, 3, fw, fh, s, e)
    info = np.array([[0, 1, 2, 3], [4, 3, 2, 1], [1, 4, 0, 2]], dtype=np.uint8)
    mv = np.empty((mbh, mbw, 4), dtype=np.int16)
    mv[:, :] = (12, -8, -20, 4)
    records = [(mv, info)]
    hops = [(0, 3, 0, -1), (0, 3, -1, 1), (0, 3, 0, 1), (0, 3, -1, -1), (0, 3, 2, 2)]
    want = both(L, fw, fh, mbw, mbh, records, hops, s, maps, fill=0xC3B2A190, what="e %d" % e)
    via = want[1]
    assert sorted(np.unique(via[0]).tolist()) == [0, 1] and sorted(np.unique(via[1]).tolist()) == [0, 2] and sorted(np.unique(via[2]).tolist()) == [0, 1, 2]
    assert (via[3] == 0).all() and sorted(np.unique(via[4]).tolist()) == [0, 1, 2]
    # a bidirectional macroblock takes the forward map; all fill where nothing is supplied, the low e bytes of the word
    assert (via[2][0:8, 24:32] == 1).all() and (want[0][3] == (0xC3B2A190 & ((1 << (8 * e)) - 1))).sum() > 0
    fill_only = both(L, fw, fh, mbw, mbh, records, [(0, 3, -1, -1)], s, maps, fill=0xC3B2A190)[0][3]
    assert (fill_only == (0xC3B2A190 & ((1 << (8 * e)) - 1))).all()


@pytest.mark.parametrize("s", M.STRIDES)
@pytest.mark.parametrize("e", M.ELEMS)
@pytest.mark.parametrize("fw,fh,mbw,mbh", [(64, 48, 4, 3), (61, 45, 4, 3)])
def test_edges_extremes_and_seeded_records(L, fw, fh, mbw, mbh, s, e):
    """the clamp at each edge, vectors of +-2048 and of -32768 / 32767, and seeded records as k_motion writes them; 61 x 45 is a frame
    smaller than its 64 x 48 grid"""
    rng = np.random.default_rng(100 * s + e)
    maps = M.rand_maps(rng, 4, 2, fw, fh, s, e)
    what = "%d x %d, s %d, e %d" % (fw, fh, s, e)
    for vec in ((-6 * s, 0), (6 * s, 0), (0, -6 * s), (0, 6 * s), (6 * s, 6 * s), (-2048, 2048), (2048, -2048), (-32768, 32767), (32767, -32768), (2 * s * 5, 2 * s * 3)):
        records = [K.uniform(mbw, mbh, vec + vec[::-1], 3)]
        want = both(L, fw, fh, mbw, mbh, records, [(0, 3, 1, -1), (0, 2, -1, 0)], s, maps, what="%s, vector %s" % (what, vec))
        assert (want[1] != 0).all()
    for seed in (1, 2):
        records = [K.varied(mbw, mbh, seed, limit=40 * s), K.varied(mbw, mbh, seed + 7, limit=3)]
        want = both(L, fw, fh, mbw, mbh, records, [(0, 3, 1, 2), (1, 0, 3, -1), (1, 2, -1, 1)], s, maps, fill=0x11223344, what="%s, seed %d" % (what, seed))
        assert set(np.unique(want[1][0]).tolist()) == {0, 1, 2}


def test_an_i_picture_is_all_fill(L):
    maps = M.rand_maps(np.random.default_rng(5), 3, 2, 64, 48, 4, 2)
    want = both(L, 64, 48, 4, 3, [K.uniform(4, 3, (0, 0, 0, 0), 4)], [(0, 0, 1, 2)], 4, maps, fill=0xBEEF)
    assert (want[0][0] == 0xBEEF).all() and (want[1] == 0).all() and want[2].tolist() == [0]


def test_every_status_word_in_its_order(L):
    fw, fh, mbw, mbh, s = 64, 48, 4, 3, 4
    maps = M.rand_maps(np.random.default_rng(6), 3, 2, fw, fh, s, 1)
    records = [K.uniform(mbw, mbh, (8, 8, 0, 0), 1), None]
    cases = [((0, 0, 1, -1, 1, 0, 0, 0), L.REGION_RESERVED), ((0, 0, 1, -1, 0, 0, 0, 7), L.REGION_RESERVED), ((9, 9, 9, 9, 0, 1, 0, 0), L.REGION_RESERVED),
             ((2, 0, 1, -1), L.REGION_FRAME), ((-1, 0, 1, -1), L.REGION_FRAME), ((2, 7, 7, 7), L.REGION_FRAME),
             ((0, 3, 1, -1), L.REGION_SLOT), ((0, -1, 1, -1), L.REGION_SLOT), ((0, 0, 3, -1), L.REGION_SLOT), ((0, 0, -2, -1), L.REGION_SLOT), ((0, 0, 1, 3), L.REGION_SLOT),
             ((0, 0, 1, -2), L.REGION_SLOT), ((0, 1, 1, -1), L.REGION_SLOT), ((0, 1, -1, 1), L.REGION_SLOT), ((0, 2, 0, 2), L.REGION_SLOT),
             ((0, 0, 1, -1), 0), ((0, 0, -1, -1), 0), ((0, 2, 1, 1), 0)]
    for hop, st in cases:
        before = np.array(maps, copy=True)
        want = both(L, fw, fh, mbw, mbh, records, [hop], s, maps, what=str(hop))
        assert want[2].tolist() == [st], hop
        if st:          # a refused record: not one byte of the slot or of via
            assert np.array_equal(want[0], before) and (want[1] == M.VIA_FILL).all()
    # the call's own refusals are errors, not status words
    with pytest.raises(L.LeonError):
        L.propagate_record(fw, fh, mbw, mbh, 2, records, (0, 0, 1, -1), 3, np.array(maps, copy=True))
    for kw in (dict(planes=0), dict(planes=4097), dict(elem_bytes=3), dict(n_slots=0), dict(n_slots=65536), dict(reserved0=1),
               dict(slot_pitch_bytes=maps[0].nbytes - 4), dict(slot_pitch_bytes=maps[0].nbytes + 2), dict(maps_bytes=maps.nbytes - 1)):
        with pytest.raises(L.LeonError):
            L.propagate_record(fw, fh, mbw, mbh, 2, records, (0, 0, 1, -1), s, np.array(maps, copy=True), **kw)
    with pytest.raises(L.LeonError):          # the target's record is missing
        L.propagate_record(fw, fh, mbw, mbh, 2, records, (1, 0, 1, -1), s, np.array(maps, copy=True))
    with pytest.raises(L.LeonError):          # a frame larger than its grid
        L.propagate_record(65, fh, mbw, mbh, 2, records, (0, 0, 1, -1), 1, M.rand_maps(np.random.default_rng(1), 2, 1, 65, fh, 1, 1))


def test_a_pitch_larger_than_the_map(L):
    fw, fh, mbw, mbh, s = 61, 45, 4, 3, 2
    maps = M.rand_maps(np.random.default_rng(8), 3, 3, fw, fh, s, 2)
    view, buf = M.pitched(maps, 12)
    records = [K.varied(mbw, mbh, 4, limit=30)]
    want = M.expected(L, fw, fh, 1, records, [(0, 2, 0, 1)], s, maps)
    st, via = L.propagate_record(fw, fh, mbw, mbh, 1, records, (0, 2, 0, 1), s, view)
    M.assert_equal((np.ascontiguousarray(view), via[None], [st]), want, "pitched")
    assert (buf[:, maps[0].nbytes:] == 0xA5).all()


def test_float_elements_are_bytes(L):
    """fp16 heatmaps with NaN and infinity bit patterns come through bit for bit"""
    fw, fh, mbw, mbh, s = 64, 48, 4, 3, 4
    bits = M.rand_maps(np.random.default_rng(9), 2, 17, fw, fh, s, 2)
    bits[0, 0, 0, :4] = (0x7C00, 0xFC00, 0x7E01, 0xFFFF)
    maps = bits.view(np.float16)
    records = [K.uniform(mbw, mbh, (0, 0, 0, 0), 1)]
    st, via = L.propagate_record(fw, fh, mbw, mbh, 1, records, (0, 1, 0, -1), s, maps)
    assert st == 0 and np.array_equal(maps.view(np.uint16)[1], bits[0]) and (via == 1).all()


def ibbp(n):
    """one closed IBBP GOP of n pictures in display order (B B I B B P ...): (fwd, bwd, keys) with window index = display index"""
    fwd, bwd, keys = [], [], []
    for d in range(n):
        if d == 2:
            f, b, t = -1, -1, 1
        elif d % 3 == 2:
            f, b, t = d - 3, -1, 2
        elif d < 2:
            f, b, t = 2, 2, 3
        else:
            f, b, t = d // 3 * 3 - 1, d // 3 * 3 + 2, 3
        fwd.append(f), bwd.append(b), keys.append((5, d, t))
    return fwd, bwd, keys


def check_plan(levels, unreachable, fwd, bwd, group, src):
    """what propagate_plan promises, from the rule alone"""
    reach = {src}
    while True:
        more = {t for t in group if t not in reach and (fwd[t] in reach or bwd[t] in reach)}
        if not more:
            break
        reach |= more
    assert sorted(unreachable) == sorted(set(group) - reach)
    level = {src: 0}
    for n, hops in enumerate(levels, 1):
        assert hops
        for t, f, b in hops:
            assert t in reach and t not in level
            assert f == (fwd[t] if fwd[t] in reach else -1) and b == (bwd[t] if bwd[t] in reach else -1)
            refs = [r for r in (f, b) if r >= 0]
            assert refs and all(r in level and level[r] < n for r in refs) and max(level[r] for r in refs) == n - 1
        for t, _, _ in hops:
            level[t] = n
    assert set(level) == reach


@pytest.mark.parametrize("n", [6, 9, 12])
def test_plan_of_a_closed_gop(L, n):
    fwd, bwd, keys = ibbp(n)
    levels, unreachable = L.propagate_plan((fwd, bwd), keys, 2)
    check_plan(levels, unreachable, fwd, bwd, range(n), 2)
    assert unreachable == [] and len(levels) == n // 3
    assert levels[0] == [(0, 2, 2), (1, 2, 2), (5, 2, -1)]
    if n >= 9:          # a B picture waits for both anchors: B3 and B4 go with P8, one level behind P5
        assert levels[1] == [(3, 2, 5), (4, 2, 5), (8, 5, -1)]


def test_plan_from_a_p_picture(L):
    """a hop gathers through the target's record: nothing goes back from a P picture to the anchors before it"""
    fwd, bwd, keys = ibbp(9)
    levels, unreachable = L.propagate_plan((fwd, bwd), keys, 5)
    check_plan(levels, unreachable, fwd, bwd, range(9), 5)
    assert unreachable == [0, 1, 2] and levels == [[(3, -1, 5), (4, -1, 5), (8, 5, -1)], [(6, 5, 8), (7, 5, 8)]]
    levels, unreachable = L.propagate_plan((fwd, bwd), keys, 8)
    assert unreachable == [0, 1, 2, 3, 4, 5] and levels == [[(6, -1, 8), (7, -1, 8)]]


def test_plan_of_an_open_gop(L):
    """the leading B pictures point forward into the GOP before: not in the window, or in it and another GOP -- slot -1 both times"""
    fwd, bwd = [-1, -1, -1, 2, 2, 2], [2, 2, -1, 5, 5, -1]
    keys = [(4, d, t) for d, t in enumerate([3, 3, 1, 3, 3, 2])]
    levels, unreachable = L.propagate_plan((fwd, bwd), keys, 2)
    assert unreachable == [] and levels == [[(0, -1, 2), (1, -1, 2), (5, 2, -1)], [(3, 2, 5), (4, 2, 5)]]
    fwd2, bwd2 = [2, 2, -1, 2, 2, 2] + [5, 5, -1, 8, 8, 8], [2, 2, -1, 5, 5, -1] + [8, 8, -1, 11, 11, -1]
    keys2 = [(3, d, t) for d, t in enumerate([3, 3, 1, 3, 3, 2])] + keys
    levels, unreachable = L.propagate_plan((fwd2, bwd2), keys2, 8)
    check_plan(levels, unreachable, fwd2, bwd2, range(6, 12), 8)
    assert unreachable == [] and levels[0] == [(6, -1, 8), (7, -1, 8), (11, 8, -1)]
