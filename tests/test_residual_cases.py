"""CPU: the premises of tests/residual_cases.py, the table tests/test_residual_kernel_gpu.py runs on the device -- that the hand-edited
lists still densify to the planes the oracle is given, that every group has the length chosen for it and the table holds every length,
level, column class, map value and edit it claims, and that the oracle's residual of every case lies inside int16 (the record's
saturation is a guard, not something a case reaches)."""
import numpy as np
import pytest

import residual_cases as K

NAMES = sorted(K.named())


def densify(case):
    """the lists back into planes as the definition reads them: level 0 writes nothing, a block at or behind the width is not shown"""
    cw, ch = case["cw"], case["ch"]
    planes = [np.zeros((ch, cw), np.int16), np.zeros((ch // 2, cw // 2), np.int16), np.zeros((ch // 2, cw // 2), np.int16)]
    for i, (plane, R, g, nb) in enumerate(K.plane_groups(cw, ch)):
        for e in case["entries"][case["grp_off"][i]:case["grp_off"][i + 1]]:
            level, off = np.int16(np.uint16(int(e) & 0xffff)), (int(e) >> 16) & 1022
            r, b, c = off >> 7, (off >> 4) & 7, (off >> 1) & 7
            if level != 0 and b < nb:
                assert planes[plane][8 * R + r, 64 * g + 8 * b + c] == 0, "two entries fill one cell"
                planes[plane][8 * R + r, 64 * g + 8 * b + c] = level
    return planes


@pytest.mark.parametrize("name", NAMES)
def test_lists_densify_to_the_planes_and_groups_have_their_lengths(name):
    case = K.named()[name]
    for got, want in zip(densify(case), case["coef"]):
        assert np.array_equal(got, want)
    assert np.array_equal(np.diff(case["grp_off"].astype(np.int64)), case["sizes"])
    assert int(case["grp_off"][-1]) == len(case["entries"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_residual_lies_inside_int16(name):
    res = K.oracle_residual(K.named()[name])
    lo, hi = min(int(p.min()) for p in res), max(int(p.max()) for p in res)
    assert -32768 < lo and hi < 32767, (lo, hi)
    for got, want in zip(K.expected(name), res):
        assert np.array_equal(got.astype(np.int32), want)


def test_table_holds_what_it_claims():
    cases = K.named()
    assert {(c["cw"], c["ch"]) for c in cases.values()} >= set(K.SIZES)
    lengths = set(np.concatenate([c["sizes"] for c in cases.values()]).tolist())
    assert lengths >= set(K.GROUP_SIZES), lengths
    levels = set(np.concatenate([c["entries"] & 0xffff for c in cases.values()]).tolist())
    assert levels >= {v & 0xffff for v in K.LEVELS} | {0}
    assert sum(c["n_zero"] for c in cases.values()) > 100 and sum(c["n_behind"] for c in cases.values()) > 100
    # live columns of a half: at most 2, at most 4, more (the row pass's three forms), each with a coefficient in its last column
    for columns in K.COLUMNS:
        c = cases["48x32_c%d" % columns]
        cols = np.flatnonzero(np.any(c["coef"][0].reshape(32, 6, 8) != 0, axis=(0, 1)))
        assert cols.max() == columns - 1
    # qscale 1 and 31, intra and non-intra, on macroblocks that code something; default and custom matrices
    for q in (1, 31):
        for ia in (0, 1):
            assert any(((c["qscale"] == q) & (c["intra"] == ia)).any() for c in cases.values() if len(c["entries"]))
    assert len({c["qm"].tobytes() for c in cases.values()}) > 2
    # an empty half beside a full one, in a luma task and in the chroma task
    c = cases["empty_half_128x16"]
    assert c["coef"][0][:8].all() and not c["coef"][0][8:].any() and c["coef"][1].all() and not c["coef"][2].any()
    # the record shows what the planes' clamp hides: negative values
    assert any(min(int(p.min()) for p in K.expected(n)) < 0 for n in NAMES)
    assert not any(p.any() for p in K.expected("empty_48x32"))
