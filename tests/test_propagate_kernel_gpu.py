"""GPU: k_propagate through leon_pipeline_propagate_kernel (include/leon_pipeline.h) on hand-written motion records, against
leon_ctypes.propagate_map, the header's text in numpy integers: the maps (every slot, the sources and the untouched ones too), via and
status compared exactly, and what the kernel is to leave alone -- a refused record's slot and via map, the bytes between the slots of a
pitched buffer, records behind the call's count -- still holding the sentinel.  The shapes are the ones at which the walk can go
wrong: a 16 x 16 frame (one macroblock, a map of one cell at stride 16), 64 x 48 (rows of whole dwords: the fast path where the
stride and element size allow it) and 61 x 45 in a 64 x 48 grid (odd rows: the cell path) for every stride and element size, plane
counts around the plane group, vectors that leave the map at each edge and the int16 extremes."""
import numpy as np
import pytest

import carry_cases as K
import propagate_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def run(L, fw, fh, records, hops, s, maps, fill=0, via=True, gap=0, n=None, what=""):
    mbw, mbh = (fw + 15) // 16, (fh + 15) // 16
    count = len(hops) if n is None else n
    want = M.expected(L, fw, fh, len(records), records, hops[:count], s, maps, fill)
    view, buf = M.pitched(maps, gap)
    got_via, status = L.propagate_kernel(fw, fh, mbw, mbh, len(records), records, hops, s, view, fill=fill, via=via, via_fill=M.VIA_FILL, status_fill=-77, n=n)
    M.assert_equal((view, got_via[:count] if via else None, status[:count]), want, what)
    assert (buf[:, maps[0].nbytes:] == 0xA5).all(), "%s: bytes between the slots were written" % what
    assert (status[count:] == -77).all() and (not via or (got_via[count:] == M.VIA_FILL).all()), "%s: written behind record %d" % (what, count - 1)
    return want


def window(mbw, mbh, s, seed):
    """six frames: two seeded records (vectors that leave the map; small ones), the int16 extremes, out at the bottom right / top
    left, out at the left / bottom, an I picture"""
    return [K.varied(mbw, mbh, seed, limit=40 * s), K.varied(mbw, mbh, seed + 1, limit=3), K.uniform(mbw, mbh, (-32768, 32767, 32767, -32768), 3),
            K.uniform(mbw, mbh, (6 * s, 6 * s, -6 * s, -6 * s), 3), K.uniform(mbw, mbh, (-6 * s, 0, 0, 6 * s), 3), K.uniform(mbw, mbh, (0, 0, 0, 0), 4)]


# sources in slots 0 .. 2 (2 is not the last slot: see test_sources_in_the_last_slot), destinations 3 .. 9
HOPS = [(0, 3, 0, 1), (1, 4, 1, 2), (2, 5, 0, -1), (2, 6, -1, 1), (3, 7, 2, 0), (4, 8, 1, 2), (5, 9, 0, 1)]


@pytest.mark.parametrize("e", M.ELEMS)
@pytest.mark.parametrize("s", M.STRIDES)
@pytest.mark.parametrize("fw,fh", [(64, 48), (61, 45)])
def test_every_stride_and_element_size(L, fw, fh, s, e):
    lay = L.propagate_layout(fw, fh, s, 2, e)
    assert lay.fast_path == int((lay.mw * e) % 4 == 0 and ((16 // s) * e) % 4 == 0)
    if (fw, fh) == (61, 45) and s == 1 and e < 4:
        assert not lay.fast_path          # rows of 61 or 122 bytes
    if (fw, fh) == (64, 48) and e == 4:
        assert lay.fast_path
    maps = M.rand_maps(np.random.default_rng(1000 * s + e), 10, 2, fw, fh, s, e)
    want = run(L, fw, fh, window(4, 3, s, 50 + s), HOPS, s, maps, fill=0xC3B2A190, what="%d x %d, s %d, e %d" % (fw, fh, s, e))
    assert (want[2] == 0).all() and set(np.unique(want[1][0]).tolist()) == {0, 1, 2} and (want[1][6] == 0).all()
    assert (want[0][9] == (0xC3B2A190 & ((1 << (8 * e)) - 1))).all()


def test_a_frame_of_one_macroblock(L):
    for s in M.STRIDES:
        for e in M.ELEMS:
            maps = M.rand_maps(np.random.default_rng(s + e), 4, 3, 16, 16, s, e)
            for vec in ((2 * s, -2 * s, 0, 0), (-32768, 32767, 0, 0), (1, 1, 0, 0)):
                run(L, 16, 16, [K.uniform(1, 1, vec, 1)], [(0, 3, 1, -1)], s, maps, what="16 x 16, s %d, e %d, %s" % (s, e, vec))


@pytest.mark.parametrize("planes", [1, 2, 3, 5, 7, 8, 9, 17, 33])
def test_plane_counts_around_the_plane_group(L, planes):
    """every plane of the destination, through whole groups and a partial last one, on both paths"""
    group = L.propagate_layout(64, 48, 2, 33, 2).planes_per_group
    assert group + 1 in (1, 2, 3, 5, 7, 8, 9, 17, 33) and L.propagate_layout(64, 48, 2, 2, 2).planes_per_group == 2
    for fw, fh, s, fast in ((64, 48, 2, 1), (61, 45, 1, 0)):
        assert L.propagate_layout(fw, fh, s, planes, 2).fast_path == fast
        maps = M.rand_maps(np.random.default_rng(planes), 10, planes, fw, fh, s, 2)
        run(L, fw, fh, window(4, 3, s, 60), HOPS[:3], s, maps, fill=0xFFFF1234, what="%d planes, %d x %d" % (planes, fw, fh))


@pytest.mark.parametrize("e", M.ELEMS)
def test_sources_in_the_last_slot(L, e):
    """vectors into the bottom-right corner of the last slot of a buffer: the funnel's second dword would lie behind the buffer"""
    for fw, fh, s in ((64, 48, 1), (64, 48, 4 // e if e < 4 else 4), (61, 45, 1)):
        maps = M.rand_maps(np.random.default_rng(e), 3, 2, fw, fh, s, e)
        for vec in ((32767, 32767), (2 * s * 61, 2 * s * 45), (2 * s * 3 + 1, 2 * s * 46)):
            run(L, fw, fh, [K.uniform(4, 3, vec + vec, 3)], [(0, 0, 2, -1), (0, 1, -1, 2)], s, maps, what="last slot, %d x %d, s %d, e %d, %s" % (fw, fh, s, e, vec))


@pytest.mark.parametrize("n", [1, 2, 5])
def test_record_counts_with_refused_records_between_valid_ones(L, n):
    fw, fh, s = 64, 48, 2
    records = window(4, 3, s, 70)
    bad = [(0, 3, 0, 1, 0, 0, 1, 0), (6, 4, 0, 1), (0, 10, 0, 1), (0, 4, 4, 1), (0, 5, 1, -2), (-1, 6, 0, 1), (0, 7, 0, 7)]
    codes = [L.REGION_RESERVED, L.REGION_FRAME, L.REGION_SLOT, L.REGION_SLOT, L.REGION_SLOT, L.REGION_FRAME, L.REGION_SLOT]
    hops, want_status = [], []
    for i in range(n):
        hops += [HOPS[i] + (0, 0, 0, 0), bad[i] + (0,) * (8 - len(bad[i]))]
        want_status += [0, codes[i]]
    count = len(hops)
    hops += [(1, 9, 0, 1, 0, 0, 0, 0)] * 2          # behind the call's count: not read
    maps = M.rand_maps(np.random.default_rng(n), 10, 3, fw, fh, s, 1)
    want = run(L, fw, fh, records, hops, s, maps, n=count, what="n = %d" % count)
    assert want[2].tolist() == want_status
    assert np.array_equal(want[0][9], maps[9]) and (want[1][1::2] == M.VIA_FILL).all()
    if n == 1:          # one record alone, and the refused one alone
        run(L, fw, fh, records, hops[:1], s, maps, what="n = 1")
        w = run(L, fw, fh, records, hops[1:2], s, maps, what="one refused record")
        assert np.array_equal(w[0], maps)


def test_without_a_via_map(L):
    for fw, fh, s, e in ((64, 48, 1, 1), (61, 45, 2, 2)):
        maps = M.rand_maps(np.random.default_rng(3), 10, 5, fw, fh, s, e)
        run(L, fw, fh, window(4, 3, s, 80), HOPS[:4], s, maps, via=False, what="via NULL, %d x %d" % (fw, fh))


@pytest.mark.parametrize("gap", [4, 256])
def test_a_pitch_larger_than_the_map(L, gap):
    for fw, fh, s, e in ((64, 48, 1, 1), (64, 48, 8, 4), (61, 45, 1, 1), (61, 45, 16, 2)):
        maps = M.rand_maps(np.random.default_rng(gap), 10, 3, fw, fh, s, e)
        run(L, fw, fh, window(4, 3, s, 90), HOPS, s, maps, gap=gap, what="gap %d, %d x %d, s %d, e %d" % (gap, fw, fh, s, e))


def test_a_window_of_no_frames(L):
    """n_frames = 0 is a call the header admits: every hop names a target that is not there, and nothing of the window is read"""
    fw, fh, s = 64, 48, 2
    maps = M.rand_maps(np.random.default_rng(5), 10, 2, fw, fh, s, 2)
    before = maps.copy()
    via, status = L.propagate_kernel(fw, fh, 4, 3, 0, window(4, 3, s, 96), HOPS[:2], s, maps, via_fill=M.VIA_FILL)
    assert status.tolist() == [L.REGION_FRAME] * 2 and (via == M.VIA_FILL).all() and np.array_equal(maps, before)


def test_only_the_record_that_is_read_is_there(L):
    """one macroblock, and a window whose other frames have no record: the ring has one slot, which is not the target's index"""
    for s, e in ((1, 1), (4, 2), (16, 4)):
        maps = M.rand_maps(np.random.default_rng(s), 4, 3, 16, 16, s, e)
        want = run(L, 16, 16, [None, K.uniform(1, 1, (2 * s, -2 * s, -4 * s, 2 * s), 3), None], [(1, 3, 0, 2)], s, maps, what="one record, s %d, e %d" % (s, e))
        assert want[2].tolist() == [0] and not np.array_equal(want[0][3], maps[3])


@pytest.mark.parametrize("via,status", [(False, True), (True, False), (False, False)])
def test_without_the_optional_outputs(L, via, status):
    """via and status may be NULL, through the library itself: what is asked for is what the call with everything gives"""
    fw, fh, s = 64, 48, 2
    records, hops = window(4, 3, s, 97), HOPS + [(6, 9, 0, 1)]
    maps = M.rand_maps(np.random.default_rng(6), 10, 3, fw, fh, s, 2)
    want_maps = maps.copy()
    want_via, want_status = L.propagate_kernel(fw, fh, 4, 3, len(records), records, hops, s, want_maps, via_fill=M.VIA_FILL, status_fill=-77)
    assert (want_status[:-1] == 0).all() and want_status[-1] == L.REGION_FRAME
    ptrs, keep = L._carry_records(records, 4, 3)
    h, cfg = L._records_array(hops), L._propagate_config(maps, s, 0)
    got_via, got_status = np.full_like(want_via, M.VIA_FILL), np.full_like(want_status, -77)
    rc = L.load().leon_pipeline_propagate_kernel(0, fw, fh, 4, 3, len(records), ptrs, L.C.byref(cfg), h.ctypes.data, len(h), maps.ctypes.data,
                                                 got_via.ctypes.data if via else None, got_status.ctypes.data if status else None)
    assert rc == L.OK, L.load().leon_last_error()
    assert np.array_equal(maps, want_maps)
    assert np.array_equal(got_via, want_via) if via else (got_via == M.VIA_FILL).all()
    assert np.array_equal(got_status, want_status) if status else (got_status == -77).all()


def test_call_refusals(L):
    fw, fh, s = 64, 48, 2
    records = window(4, 3, s, 95)
    maps = M.rand_maps(np.random.default_rng(4), 4, 2, fw, fh, s, 2)
    for kw in (dict(n=0), dict(n=65536), dict(planes=0), dict(elem_bytes=3), dict(n_slots=0), dict(n_slots=65536), dict(reserved0=1),
               dict(slot_pitch_bytes=maps[0].nbytes + 2), dict(slot_pitch_bytes=maps[0].nbytes - 4), dict(maps_bytes=maps.nbytes - 4)):
        before = np.array(maps, copy=True)
        with pytest.raises(L.LeonError):
            L.propagate_kernel(fw, fh, 4, 3, 6, records, [(0, 3, 0, 1)], s, maps, **kw)
        assert np.array_equal(maps, before)
    with pytest.raises(L.LeonError):          # a stride outside the definition
        L.propagate_kernel(fw, fh, 4, 3, 6, records, [(0, 3, 0, 1)], 3, maps)
    with pytest.raises(L.LeonError):          # a frame larger than the grid
        L.propagate_kernel(fw + 1, fh, 4, 3, 6, records, [(0, 3, 0, 1)], s, M.rand_maps(np.random.default_rng(4), 4, 2, fw + 1, fh, s, 2))
    with pytest.raises(L.LeonError):          # the record of a valid hop's target is missing
        L.propagate_kernel(fw, fh, 4, 3, 6, [None] + records[1:], [(0, 3, 0, 1)], s, maps)
    # ... while a refused hop needs none
    via, status = L.propagate_kernel(fw, fh, 4, 3, 6, [None] + records[1:], [(0, 3, 3, 1)], s, maps)
    assert status.tolist() == [L.REGION_SLOT]
