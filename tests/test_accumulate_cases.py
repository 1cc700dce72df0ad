"""CPU: the library's CPU evaluation of one accumulate hop (leon_pipeline_accumulate_record: the text k_accumulate compiles too, walked
unit by unit) against leon_ctypes.accumulate_hop, the header's text in numpy integers, on the cases tests/test_accumulate_kernel_gpu.py
runs on the device (tests/accumulate_cases.py): the definition is pinned without a GPU.  Then the definition's own properties by hand:
both roundings at their ties, saturation, the invariant of the displacement, every status word in its order.  No GPU."""
import numpy as np
import pytest

import accumulate_cases as A
import carry_cases as K


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def cases(L):
    return {c["what"]: c for c in A.cases(L)}


def run_record(L, c):
    """the hops of a case through accumulate_record, each on the result of the one before (as the oracle does)"""
    buf, hops = c["buf"].copy(), c["hops"]
    n = len(hops) if c.get("n") is None else c["n"]
    via = np.full((len(hops), c["ch"] // 16, c["cw"] // 16), A.VIA_FILL, dtype=np.uint8)
    status = np.full(len(hops), A.STATUS_FILL, dtype=np.int64)
    for i, h in enumerate(hops[:n]):
        st, v = L.accumulate_record(c["cw"], c["ch"], c.get("n_frames", len(c["motion"])), c["motion"], c["residual"], h, c["parts"], buf, via_fill=A.VIA_FILL)
        if c.get("status", True):
            status[i] = st
        if c.get("via", True):
            via[i] = v
    return buf, via, status


def test_the_case_list_is_what_the_kernel_test_runs(L, cases):
    names = list(cases)
    assert len(names) == len(A.cases(L)) and len(names) >= 60          # (distinct names)
    for cw, ch in A.SHAPES:
        for parts in A.PARTS:
            for kind in ("window", "last slot", "gap 4", "gap 256"):
                assert "%s, %dx%d parts %d" % (kind, cw, ch, parts) in cases


def test_record_against_the_numpy_definition_on_every_case(L, cases):
    for c in cases.values():
        A.assert_equal(L, c, run_record(L, c), A.expected(L, c))


def test_the_cases_reach_what_they_are_for(L, cases):
    # the window: every via value, the I picture all restart and all zero
    c = cases["window, 64x48 parts 3"]
    want, via, status, _ = A.expected(L, c)
    assert status.tolist() == [0] * 7 and set(np.unique(via[0]).tolist()) == {0, 1, 2} and (via[6] == 0).all()
    acc = L.accumulate_views(want, L.accumulate_layout(64, 48, 3))
    assert all((acc[name][9] == 0).all() for name in acc)
    # saturation both ways, in every plane
    for sign, lim in ((1, 32767), (-1, -32768)):
        c = cases["saturation %+d, 64x48" % sign]
        acc = L.accumulate_views(A.expected(L, c)[0], L.accumulate_layout(64, 48, 3))
        for name in acc:
            if name == "AGE" and sign < 0:
                assert (acc[name][3] == -32766).all()          # -32767 + 1
            else:
                assert (acc[name][3, 8:-8, 8:-8] == lim).all() and (acc[name][4, 8:-8, 8:-8] == lim).all(), name
    # refused hops between valid ones: their slots as they were
    c = cases["10 hops, refused ones between"]
    want, via, status, _ = A.expected(L, c)
    assert status[:10].tolist() == [0, L.REGION_RESERVED, 0, L.REGION_FRAME, 0, L.REGION_SLOT, 0, L.REGION_SLOT, 0, L.REGION_SLOT]
    assert (status[10:] == A.STATUS_FILL).all() and (via[1:10:2] == A.VIA_FILL).all() and np.array_equal(want[8:], c["buf"][8:])
    assert A.expected(L, cases["a window of no frames"])[2].tolist() == [L.REGION_FRAME] * 2


@pytest.mark.parametrize("v", [1, -1, 2, -2, 3, -3, 4, -5, 7])
def test_both_roundings_by_hand(L, v):
    """luma (v + 1) >> 1, chroma (v + 2) >> 2, arithmetic shift: from zero sources AX, AY are the displacement itself"""
    cw, ch = 64, 48
    lay = L.accumulate_layout(cw, ch, 3)
    buf = np.zeros((2, lay.slot_bytes), dtype=np.uint8)
    acc = L.accumulate_views(buf, lay)
    acc["RY"][0] = np.arange(ch * cw, dtype=np.int16).reshape(ch, cw)
    acc["RCb"][0] = np.arange(ch * cw // 4, dtype=np.int16).reshape(ch // 2, cw // 2)
    zero = [tuple(np.zeros(s, dtype=np.int16) for s in ((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2)))]
    st, via = L.accumulate_record(cw, ch, 1, [K.uniform(4, 3, (v, -v, 0, 0), 1)], zero, (0, 1, 0, -1), 3, buf)
    assert st == 0 and (via == 1).all()
    dl, dc = (v + 1) >> 1, (v + 2) >> 2
    el, ec = (-v + 1) >> 1, (-v + 2) >> 2
    assert dl == int(np.floor((v + 1) / 2)) and dc == int(np.floor((v + 2) / 4))
    y, x = 24, 32
    assert acc["AX"][1, y, x] == dl and acc["AY"][1, y, x] == el and acc["AGE"][1, y, x] == 1
    assert acc["RY"][1, y, x] == acc["RY"][0, y + el, x + dl]
    assert acc["RCb"][1, y // 2, x // 2] == acc["RCb"][0, y // 2 + ec, x // 2 + dc]


def test_the_displacement_stays_inside_the_picture(L):
    """0 <= x + AX <= cw - 1 and 0 <= y + AY <= ch - 1 along a chain of hops with vectors that leave at every edge"""
    cw, ch = 128, 32
    lay = L.accumulate_layout(cw, ch, 1)
    buf = np.full((2, lay.slot_bytes), 0x5A, dtype=np.uint8)
    acc = L.accumulate_views(buf, lay)
    assert L.accumulate_record(cw, ch, 4, [K.uniform(8, 2, (0, 0, 0, 0), 4)] * 4, None, (0, 0, -1, -1), 1, buf)[0] == 0 and not buf[0].any()
    y, x = np.mgrid[0:ch, 0:cw]
    motion = [K.varied(8, 2, s, limit=90) for s in range(4)]
    for i in range(4):
        st, via = L.accumulate_record(cw, ch, 4, motion, None, (i, 1 - i % 2, i % 2, i % 2), 1, buf)
        d = 1 - i % 2
        assert st == 0
        assert ((x + acc["AX"][d] >= 0) & (x + acc["AX"][d] < cw) & (y + acc["AY"][d] >= 0) & (y + acc["AY"][d] < ch)).all()
        assert (acc["AGE"][d][np.repeat(np.repeat(via, 16, 0), 16, 1) == 0] == 0).all() and acc["AGE"][d].max() == i + 1


def test_every_status_word_in_its_order_and_the_call_refusals(L):
    cw, ch = 64, 48
    lay = L.accumulate_layout(cw, ch, 3)
    rng = np.random.default_rng(6)
    buf = A.slots(L, rng, cw, ch, 3, 3)
    motion, residual = [K.uniform(4, 3, (8, 8, 0, 0), 1), None], A.residuals(rng, cw, ch, 1) + [None]
    table = [((0, 0, 1, -1, 1, 0, 0, 0), L.REGION_RESERVED), ((9, 9, 9, 9, 0, 1, 0, 0), L.REGION_RESERVED), ((2, 0, 1, -1), L.REGION_FRAME), ((-1, 0, 1, -1), L.REGION_FRAME),
             ((2, 7, 7, 7), L.REGION_FRAME), ((0, 3, 1, -1), L.REGION_SLOT), ((0, -1, 1, -1), L.REGION_SLOT), ((0, 0, 3, -1), L.REGION_SLOT), ((0, 0, 1, -2), L.REGION_SLOT),
             ((0, 1, 1, -1), L.REGION_SLOT), ((0, 2, 0, 2), L.REGION_SLOT), ((0, 0, 1, -1), 0), ((0, 0, -1, -1), 0), ((0, 2, 1, 1), 0)]
    for hop, st in table:
        before = buf.copy()
        got, via = L.accumulate_record(cw, ch, 2, motion, residual, hop, 3, buf, via_fill=A.VIA_FILL)
        assert got == st, hop
        if st:
            assert np.array_equal(buf, before) and (via == A.VIA_FILL).all()
    for kw in (dict(n_slots=0), dict(n_slots=65536), dict(reserved=(0, 1)), dict(reserved=(1, 0)), dict(slot_pitch_bytes=lay.slot_bytes - 4), dict(slot_pitch_bytes=lay.slot_bytes + 2),
               dict(slots_bytes=buf.nbytes - 1)):
        with pytest.raises(L.LeonError):
            L.accumulate_record(cw, ch, 2, motion, residual, (0, 0, 1, -1), 3, buf.copy(), **kw)
    for parts in (0, 4, -1):
        with pytest.raises(L.LeonError):
            L.accumulate_record(cw, ch, 2, motion, residual, (0, 0, 1, -1), parts, buf.copy())
    with pytest.raises(L.LeonError):          # the target's records are missing
        L.accumulate_record(cw, ch, 2, motion, residual, (1, 0, 1, -1), 3, buf.copy())
    with pytest.raises(L.LeonError):          # ... or its residual record alone
        L.accumulate_record(cw, ch, 2, motion, [None, None], (0, 0, 1, -1), 3, buf.copy())
    with pytest.raises(L.LeonError):          # no residual records at all with the residual part
        L.accumulate_record(cw, ch, 2, motion, None, (0, 0, 1, -1), 3, buf.copy())
    with pytest.raises(L.LeonError):          # a coded size that is no multiple of 16
        L.accumulate_layout(60, ch, 1)
    assert L.accumulate_record(cw, ch, 2, motion, None, (0, 0, 1, -1), 1, A.slots(L, rng, cw, ch, 1, 3))[0] == 0          # the motion part needs none
