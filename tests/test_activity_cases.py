"""CPU: leon_pipeline_activity_record, the host's C text of the ACTIVITY record (csrc/leon_activity.h), against
leon_ctypes.activity_from_lists, the header's text in numpy, byte for byte on the specified bytes, over the crafted lists of
tests/activity_cases.py; the premises of those lists; and an oracle that never walks a list: the dense planes leon_vlc_densify makes
of the fixture streams' lists, counted per macroblock."""
import os

import numpy as np
import pytest

import activity_cases as K
import leon_ctypes as L
from helpers import ROOT

STREAMS = os.path.join(ROOT, "tests", "golden", "streams")
NAMES = sorted(K.named())


def test_cases_reach_what_they_exist_for():
    assert {w for w, _ in K.SHAPES} == {1, 4, 5, 8, 9, 12, 13, 37} and {h for _, h in K.SHAPES} == {1, 2, 3}
    gy = {w: K.groups(w, 1)[0] for w in K.WIDTHS}
    gc = {w: K.groups(w, 1)[1] for w in K.WIDTHS}
    assert gy[1] == gy[4] == 1 and gy[5] == gy[8] == 2 and gc[8] == 1 and gc[9] == 2
    assert [w for w in K.WIDTHS if gy[w] % 2 == 1] == [1, 4, 9, 12]          # the last chroma group has no luma group 2c + 1
    assert gy[13] == 4 and gc[13] == 2 and gy[37] == 10 and gc[37] == 5
    seen_sizes, levels, outside = set(), set(), 0
    for name in NAMES:
        mbw, mbh, (grp_off, entries, qscale) = K.named()[name]
        gy_, gc_, n_y, n_c = K.groups(mbw, mbh)
        assert len(grp_off) >= n_y + 2 * n_c + 1 and (np.diff(grp_off.astype(np.int64)) >= 0).all() and grp_off[-1] == len(entries)
        assert len(qscale) == mbw * mbh and qscale.all()
        seen_sizes |= set(np.diff(grp_off.astype(np.int64)).tolist())
        levels |= set(np.unique((entries & 0xffff).astype(np.uint16).view(np.int16)).tolist())
        if name == "37x3":
            gid = np.repeat(np.arange(len(grp_off) - 1), np.diff(grp_off.astype(np.int64)))
            luma_last = (gid < n_y) & (gid % gy_ == gy_ - 1)
            outside = int((4 * (gy_ - 1) + ((entries[luma_last] >> 21) & 3) >= mbw).sum())
    assert set(K.GROUP_SIZES) <= seen_sizes and set(K.LEVELS) <= levels and outside > 0


def test_empty_and_saturated_by_name():
    cells, s = K.expected(L, K.named()["empty_13x3"])
    assert not cells.view(np.uint8).any() and not s.any()
    cells, s = K.expected(L, K.named()["saturated_378x255"])
    c = cells[0, 0]
    assert (int(c["ac_count"]), int(c["ac_mag"]), int(c["dc_mag"]), int(c["blocks"]), int(c["qscale"])) == (378, 65535, 1200, 63, 31)
    assert 378 * 255 == 96390 and s.tolist() == [1, 378, 65535, 1200, 65535, 31, 6, 0]
    cells, s = K.expected(L, K.named()["saturated_dc"])
    assert s.tolist() == [1, 0, 0, 65535, 0, 31, 6, 0]
    cells, s = K.expected(L, K.named()["past_2_to_the_32"])
    assert 132000 * 32768 > 1 << 32 and s.tolist() == [1, 65535, 65535, 0, 65535, 31, 6, 0]


@pytest.mark.parametrize("name", NAMES)
def test_host_text_equals_the_definition(name):
    case = K.named()[name]
    mbw, mbh, (grp_off, entries, qscale) = case
    want = K.expected(L, case)
    cells, summary, buf = L.activity_record(mbw, mbh, grp_off, entries, qscale, fill=K.SENTINEL)
    assert cells.dtype == L.ACTIVITY_CELL and summary.dtype == np.uint32
    K.assert_record(buf, L.activity_layout(mbw, mbh), want, name)
    # the record's rule on qscale: shown where something is coded, nowhere else
    assert ((cells["qscale"] != 0) == (cells["blocks"] != 0)).all()


def test_zero_levels_count_nothing():
    """the lists of the two front ends differ in entries with level 0: dropping them changes nothing"""
    mbw, mbh, (grp_off, entries, qscale) = K.named()["13x2"]
    keep = (entries & 0xffff) != 0
    assert not keep.all()
    gid = np.repeat(np.arange(len(grp_off) - 1), np.diff(grp_off.astype(np.int64)))
    off2 = np.zeros_like(grp_off)
    np.cumsum(np.bincount(gid[keep], minlength=len(grp_off) - 1), out=off2[1:])
    a, b = L.activity_record(mbw, mbh, grp_off, entries, qscale), L.activity_record(mbw, mbh, off2, entries[keep], qscale)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def dense_counts(p, mbw, mbh):
    """per macroblock, from the dense planes alone: (non-zero coefficients that are not DC, the sum of their magnitudes, the sum of the
    DC magnitudes, the block bits).  The coefficient (r, c) of block (R, q) of a plane stands at [8 R + r, 8 q + c]."""
    nz = np.zeros((mbh, mbw), np.int64)
    mag, dcm, blocks = nz.copy(), nz.copy(), nz.copy()
    for plane, per_mb, first in ((p["coef_y"], 2, 0), (p["coef_cb"], 1, 4), (p["coef_cr"], 1, 5)):
        a = np.abs(plane.astype(np.int64)).reshape(mbh * per_mb, 8, mbw * per_mb, 8).transpose(0, 2, 1, 3)      # [block row, block column, r, c]
        dc = a[:, :, 0, 0]
        ac_n = (a != 0).sum(axis=(2, 3)) - (dc != 0)
        ac_m = a.sum(axis=(2, 3)) - dc
        for by in range(per_mb):
            for bx in range(per_mb):
                sl = (slice(by, None, per_mb), slice(bx, None, per_mb))
                nz += ac_n[sl]
                mag += ac_m[sl]
                dcm += dc[sl]
                blocks |= ((ac_n[sl] + (dc[sl] != 0)) != 0).astype(np.int64) << (first + (2 * by + bx if per_mb == 2 else 0))
    return nz, mag, dcm, blocks


@pytest.mark.parametrize("name", ["ibbp_96x64", "leon_synth_352x240", "syntax_escape_ip_592x32", "yuva_ibbp_96x64", "custom_intra_ip_48x32"])
def test_fixture_streams_against_their_dense_planes(name):
    import leon_vlc_ctypes as V
    st = V.Stream(open(os.path.join(STREAMS, name + ".jsv"), "rb").read(), threads=1)
    mbw, mbh = st.info.coded_width // 16, st.info.coded_height // 16
    pictures = skipped = coded = 0
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        cells, summary = L.activity_record(mbw, mbh, p["grp_off"], p["entries"], p["qscale"])
        ref = L.activity_from_lists(mbw, mbh, p["grp_off"], p["entries"], p["qscale"])
        assert np.array_equal(cells, ref[0]) and np.array_equal(summary, ref[1])
        nz, mag, dcm, blocks = dense_counts(p, mbw, mbh)
        ok = (nz < 65535) & (mag < 65535) & (dcm < 65535)          # a saturated field says less than the planes
        skipped += int((~ok).sum())
        for field, plane in (("ac_count", nz), ("ac_mag", mag), ("dc_mag", dcm), ("blocks", blocks)):
            assert np.array_equal(cells[field][ok], plane[ok]), (name, pictures, field)
        assert np.array_equal(cells["qscale"], np.where(blocks != 0, p["qscale"].reshape(mbh, mbw), 0))
        pictures += 1
        coded += int((blocks != 0).sum())
    st.close()
    assert pictures >= 2 and coded > 0 and skipped == 0
