"""CPU: the premises of tests/motion_cases.py -- that its shapes reach the places of k_motion's walk they are named for, that its maps
hold the values streams do not carry, that the bound case sums to 2^27 -- and leon_pipeline_motion_record, the host's C text, against
motion_from_maps on every shape and type."""
import numpy as np
import pytest

import leon_ctypes as L
import motion_cases as K

MBS = [w * h for w, h in K.SHAPES]


def test_shapes_reach_what_they_exist_for():
    assert all(1 <= w <= 256 and 1 <= h <= 256 for w, h in K.SHAPES) and len(set(MBS)) == len(MBS)
    assert MBS[:5] == [1, 2, 3, 4, 5] and {255, 256, 1023, 1024, 1025, 8160, 65536} <= set(MBS) and (120, 68) in K.SHAPES
    assert {m % 4 for m in MBS} == {0, 1, 2, 3}
    assert {K.trips(m) for m in MBS} >= {1, 2, 3, 8, 64}
    assert any(K.trips(m) == 2 and K.last_trip_lanes(m) == 1 and m % 4 == 1 for m in MBS)          # one live lane that holds one macroblock
    assert any(K.trips(m) == 2 and K.last_trip_lanes(m) >= 1 and m % 4 == 0 for m in MBS)          # a second trip of full lanes
    assert any(K.trips(m) == 3 and m % 4 == 1 for m in MBS)
    assert any(m < 256 for m in MBS) and any(m < 4 for m in MBS)
    # around the first wave's end: its last lane partly and wholly filled, then the second wave's first lanes
    assert any(252 < m < 256 for m in MBS) and 256 in MBS and any(256 < m <= 264 and m % 4 == 1 for m in MBS)
    # the substitutes keep their residue and their side: 261 for 257, 1032 for 1028, 2057 for 2049
    for stands_for, has in ((257, 261), (1028, 1032), (2049, 2057)):
        assert has in MBS and has % 4 == stands_for % 4 and K.trips(has) == K.trips(stands_for) and (has > 256) == (stands_for > 256)
        assert not any(stands_for % a == 0 and stands_for // a <= 256 for a in range(1, 257))
        assert not any(m % 4 == stands_for % 4 and any(m % a == 0 and m // a <= 256 for a in range(1, 257)) for m in range(stands_for, has))
    assert all(w * h <= 2057 for w, h in K.SMALL) and {s[0] * s[1] % 4 for s in K.SMALL} == {0, 1, 2, 3}


def test_maps_hold_what_streams_do_not_carry():
    mbw, mbh = 120, 68
    for type in (2, 3):
        repadd, mb_dir, fwd, bwd = K.maps(mbw, mbh, type, 1, with_min=True)
        mv, info, summary = K.expected(L, mbw, mbh, type, (repadd, mb_dir, fwd, bwd))
        assert set(np.unique(repadd)) == set(K.REPADD)
        info = info.reshape(-1)
        assert (info[repadd == 127] != 4).all() and (info[repadd == 128] == 4).all() and (repadd == 127).any() and (repadd == 128).any()
        f = fwd.reshape(-1, 2)
        for e in K.EDGES + (-32768,):
            assert (f == e).any(), e
        assert (np.abs(f.astype(np.int64)) > 2048).mean() > 0.4 and f.min() == -32768 and f.max() > 30000
        d = np.where(repadd >= 128, 0, 1 if type == 2 else mb_dir & 3)
        assert f[(d & 1) == 0].any(axis=1).all() and ((d & 1) == 0).any()          # an unused direction holds a vector that is not zero ...
        assert not mv.reshape(-1, 4)[(d & 1) == 0, 0:2].any()                      # ... and the record shows none of it
        if type == 3:
            assert (mb_dir > 3).any() and {int(v) for v in np.unique(mb_dir & 3)} == {0, 1, 2, 3}
            assert {int(v) for v in np.unique(info)} == {0, 1, 2, 3, 4}
            b = bwd.reshape(-1, 2)
            assert b[(d & 2) == 0].any(axis=1).all() and ((d & 2) == 0).any() and not mv.reshape(-1, 4)[(d & 2) == 0, 2:4].any()
            assert b.min() == -32768
        else:
            assert mb_dir is None and bwd is None and {int(v) for v in np.unique(info)} == {1, 4}
        # -32768 counts as 32768 in the sums (motion_abs16)
        assert int(summary[4]) == int(np.abs(mv[..., 0].astype(np.int64)).sum()) and (mv[..., 0] == -32768).any()
    assert K.maps(mbw, mbh, 1, 1) == (None, None, None, None)
    without = K.maps(mbw, mbh, 3, 1)
    assert without[2].min() > -32768 and without[3].min() > -32768
    assert all(np.array_equal(a, b) for a, b in zip(K.maps(5, 1, 3, 9), K.maps(5, 1, 3, 9)))


def test_the_bound_case_sums_to_2_to_the_27():
    m = K.bound_maps(256, 256)
    mv, info, s = K.expected(L, 256, 256, 3, m)
    assert s.dtype == np.uint32 and s.tolist() == [65536, 65536, 0, 65536] + [1 << 27] * 4
    assert (info == 3).all() and (mv == -2048).all()
    mv, info, s = K.expected(L, 256, 256, 2, m)
    assert s.tolist() == [65536, 0, 0, 65536, 1 << 27, 1 << 27, 0, 0]


def test_permutation_is_not_the_identity():
    for n, r in ((1, 2), (3, 5), (6, 9), (65537, 65540)):
        p = K.permutation(n, r, 3)
        assert len(set(p.tolist())) == n and p.min() >= 0 and p.max() < r and not np.array_equal(p, np.arange(n))


@pytest.mark.parametrize("mbw,mbh", K.SHAPES, ids=["%dx%d" % s for s in K.SHAPES])
def test_host_text_equals_the_definition(mbw, mbh):
    lay = L.motion_layout(mbw, mbh)
    mbs = mbw * mbh
    for type in (1, 2, 3):
        m = K.maps(mbw, mbh, type, 7, with_min=True)
        want = K.expected(L, mbw, mbh, type, m)
        mv, info, summary, buf = L.motion_record(type, mbw, mbh, *m, fill=K.SENTINEL)
        for g, w in zip((mv, info, summary), want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (type, mbw, mbh)
        assert (buf[8 * mbs:lay.info_offset] == K.SENTINEL).all() and (buf[lay.info_offset + mbs:lay.summary_offset] == K.SENTINEL).all()
