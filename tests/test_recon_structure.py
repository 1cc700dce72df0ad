"""CPU: the facts tests/test_recon_structure_gpu.py rests on.  Every case of tests/recon_structure.py shows the edge of recon_task /
column_pass / recon_luma_pair it is named for, the cases cover the whole list of edges between them, the short butterfly forms as
transcribed from csrc/leon_kernels.h equal the oracle's butterfly wherever the kernels choose them, col_final's fp32 sums stay below
2^24 on every case, and the cases themselves are pictures the oracle decodes and the sparse boundary lists as task_facts says."""
import numpy as np
import pytest

import recon_structure as R
from recon_structure import CASES, HEIGHT, ITEMS, PIC_B, PIC_I, PIC_P, tdiv256


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_shows_its_facts(case):
    for item, road, ptype, fact in case.facts:
        recs = R.facts_of(case.name, ptype, road)
        assert fact(recs), "%s (%s, type %d): %s" % (item, road, ptype, [R.brief(r) for r in recs])


def test_the_cases_cover_every_item():
    covered = [item for c in CASES for item, _, _, _ in c.facts]
    assert sorted(set(covered)) == sorted(set(ITEMS)), (set(ITEMS) - set(covered), set(covered) - set(ITEMS))
    assert len(set(ITEMS)) == len(ITEMS)
    assert {c.width for c in CASES} == set(R.WIDTHS)
    # under 20 macroblocks each, and every road's geometry exists at the widths: Rt 0 and 1
    assert all(c.width // 16 * (HEIGHT // 16) < 20 for c in CASES)


def test_pair_task_is_the_dense_p_and_b_display_front_only():
    for ptype in (PIC_I, PIC_P, PIC_B):
        for road in R.ROADS:
            f = R.road_flags(road)
            kinds = {r["kind"] for r in R.facts_of("pair-255-256", ptype, road)}
            assert ("pair" in kinds) == (road == "display-dense" and ptype != PIC_I), (road, ptype)
            assert ("alpha" in kinds) == f["alpha"]


# ---- the short forms, transcribed line by line from csrc/leon_kernels.h (div256(mad24k(a, k, c)) = trunc((a * k + c) / 256)) ----------

def lo2(X0, X1):
    x4 = tdiv256(X1 * 473 + 128) - X1
    x0 = x4 - tdiv256(X1 * 362 + 128)
    y7 = -x0 - tdiv256(X1 * 196 + 128)
    return np.stack([X1 + X0, x4 + X0, X0 - x0, X0 - y7, X0 + y7, x0 + X0, X0 - x4, X0 - X1], axis=-1)


def lo4(X0, X1, X2, X3):
    b7 = X1 + X3
    x4 = tdiv256(X1 * 473 + (X3 * 196 + 128)) - b7
    x0 = x4 - tdiv256((X1 - X3) * 362 + 128)
    x2 = tdiv256(X2 * 362 + 128) - X2
    y3, y4, y5, y6 = X0 + x2, X0 + X2, X0 - x2, X0 - X2
    y7 = -x0 - tdiv256(X3 * -473 + (X1 * 196 + 128))
    return np.stack([b7 + y4, x4 + y3, y5 - x0, y6 - y7, y6 + y7, x0 + y5, y3 - x4, y4 - b7], axis=-1)


def col_final(y4, b7, y3, x4, y5, x0, y6, y7):
    """(o0, o7) (o1, o6) (o5, o2) (o4, o3) = the four sums and differences, in fp32 like the kernel: exact below 2^24"""
    f = lambda v: np.asarray(v, np.int64).astype(np.float32)
    o = [f(y4) + f(b7), f(y3) + f(x4), f(y5) - f(x0), f(y6) - f(y7), f(y6) + f(y7), f(y5) + f(x0), f(y3) - f(x4), f(y4) - f(b7)]
    return np.stack(o, axis=-1).astype(np.int64)


def col_arm(X, n_live):
    X = [np.asarray(X[..., i], np.int64) for i in range(8)]
    if n_live <= 2:
        X0, X1 = X[0], X[1]
        x4 = tdiv256(X1 * 473 + 128) - X1
        x0 = x4 - tdiv256(X1 * 362 + 128)
        y7 = -x0 - tdiv256(X1 * 196 + 128)
        return col_final(X0, X1, X0, x4, X0, x0, X0, y7)
    if n_live <= 4:
        X0, X1, X2, X3 = X[:4]
        b7 = X1 + X3
        x4 = tdiv256(X1 * 473 + (X3 * 196 + 128)) - b7
        x0 = x4 - tdiv256((X1 - X3) * 362 + 128)
        x2 = tdiv256(X2 * 362 + 128) - X2
        y7 = -x0 - tdiv256(X3 * -473 + (X1 * 196 + 128))
        return col_final(X0 + X2, b7, X0 + x2, x4, X0 - x2, x0, X0 - X2, y7)
    b1, b3, b4 = X[4], X[2] + X[6], X[5] - X[3]
    tmp1, tmp2, b6 = X[1] + X[7], X[3] + X[5], X[1] - X[7]
    b7, m0 = tmp1 + tmp2, X[0]
    x4 = tdiv256(b6 * 473 + (b4 * -196 + 128)) - b7
    x0 = x4 - tdiv256((tmp1 - tmp2) * 362 + 128)
    x1 = m0 - b1
    x2 = tdiv256((X[2] - X[6]) * 362 + 128) - b3
    x3 = m0 + b1
    y7 = -x0 - tdiv256(b4 * 473 + (b6 * 196 + 128))
    return col_final(x3 + b3, b7, x1 + x2, x4, x1 - x2, x0, x3 - b3, y7)


# what the live entries can be.  Column pass: a DC of int16 * 256, an AC of [-2048, 2047] * premultiplier; row pass: trunc(2.5 w) of an
# int16 w, + 128 in entry 0.
DC = np.arange(-32768, 32768, dtype=np.int64) * 256
AC = np.unique(np.arange(-2048, 2048, dtype=np.int64)[:, None] * np.unique(R.PREMULTIPLIER)[None, :])
ROW = np.trunc(np.arange(-32768, 32768).astype(np.float32) * np.float32(2.5)).astype(np.int64)


def _inputs(n_live, first, rng, n=4000):
    """[.., 8] with entries n_live .. 7 zero: every value of each live entry on its own (beside seeded others), and seeded tuples"""
    pools = [first] + [AC if first is DC else ROW] * 7
    out = []
    for k in range(n_live):
        X = np.zeros((len(pools[k]), 8), np.int64)
        for j in range(n_live):
            X[:, j] = rng.choice(pools[j], len(X))
        X[:, k] = pools[k]
        out.append(X)
    X = np.zeros((n, 8), np.int64)
    for j in range(n_live):
        X[:, j] = rng.choice(np.concatenate([pools[j], pools[j][[0, -1]].repeat(200)]), n)
    return np.concatenate(out + [X])


def test_numpy_butterfly_is_the_oracles(O):
    rng = np.random.default_rng(8)
    X = _inputs(8, DC, rng, n=3000)[-3000:]
    X[0], X[1] = [DC[0]] + [AC[0]] * 7, [DC[-1]] + [AC[-1]] * 7
    mine = R.butterfly8(X)[0]
    for x, o in zip(X, mine):
        assert np.array_equal(O.butterfly8(x), o), x


@pytest.mark.parametrize("n_live", [1, 2, 3, 4, 5, 8])
def test_short_forms_equal_the_full_butterfly_when_the_higher_entries_are_zero(O, n_live):
    """'every dropped term is an exact zero': over every value an entry can take, the largest DC included"""
    rng = np.random.default_rng(n_live)
    for first, name in ((DC, "column pass"), (ROW + 128, "row pass")):
        X = _inputs(n_live, first, rng)
        full = R.butterfly8(X)[0]
        if name == "column pass":
            assert np.array_equal(col_arm(X, n_live), full), "butterfly8_col, n_live %d" % n_live
        elif n_live <= 2:
            assert np.array_equal(lo2(X[:, 0], X[:, 1]), full)
        elif n_live <= 4:
            assert np.array_equal(lo4(X[:, 0], X[:, 1], X[:, 2], X[:, 3]), full)
        for x, o in zip(X[-200:], full[-200:]):          # and the oracle itself on the seeded tuples
            assert np.array_equal(O.butterfly8(x), o)


def test_a_short_form_one_entry_too_short_differs():
    """the transcriptions can tell: entry 3 (5) live under the 2-input (4-input) form changes the result"""
    X = np.zeros((1, 8), np.int64)
    X[0, :3] = 1000, 44, 55
    assert not np.array_equal(col_arm(X, 2), R.butterfly8(X)[0]) and not np.array_equal(lo2(X[:, 0], X[:, 1]), R.butterfly8(X)[0])
    X[0, 4] = 32
    assert not np.array_equal(col_arm(X, 4), R.butterfly8(X)[0]) and not np.array_equal(lo4(*X[0, :4][:, None]), R.butterfly8(X)[0])


# ---- counters over all cases ----------------------------------------------------------------------------------------------------------

def _all_records(road, types=(PIC_I, PIC_P, PIC_B)):
    return [(c.name, t, r) for c in CASES for t in types for r in R.facts_of(c.name, t, road)]


def test_col_final_stays_below_2_to_24():
    """every input, sum and difference of col_final, over all cases (single-tile fronts with the A plane, and the pair fronts)"""
    recs = _all_records("yuva-plain-dense", (PIC_P,)) + _all_records("display-dense", (PIC_P,))
    largest = max(r["largest_col_final"] for _, _, r in recs)
    print("largest |value| through col_final: %d = 2^%.3f" % (largest, np.log2(largest)))
    assert 32767 * 256 < largest < 2 ** 24


def test_truncation_and_saturation_counters():
    for road in ("plain-dense", "display-dense", "yuva-display-sparse"):
        recs = _all_records(road)
        for ptype in (PIC_P, PIC_B):
            assert sum(r["trunc_differs"] for _, t, r in recs if t == ptype) > 0
        assert all(r["trunc_differs"] == 0 for _, t, r in recs if t == PIC_I)
        for c in CASES:
            sat = sum(r["saturating"] for n, _, r in recs if n == c.name)
            assert (sat > 0) == (c.name in R.SATURATING), (c.name, sat)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_sparsify_lists_what_task_facts_counts(case):
    import leon_vlc_ctypes as V
    cw = case.width
    t = case.picture(PIC_P)
    gY, gC, mbh = (cw // 8 + 7) // 8, (cw // 16 + 7) // 8, HEIGHT // 16
    grp_off, entries = V.sparsify(t["coef_y"], t["coef_cb"], t["coef_cr"], cw, HEIGHT, coef_a=t["coef_a"])
    counts = np.diff(grp_off.astype(np.int64))
    nY, nC = 2 * mbh * gY, mbh * gC
    assert len(counts) == 2 * nY + 2 * nC
    for r in R.facts_of(case.name, PIC_P, "yuva-plain-sparse"):
        if r["kind"] == "chroma":
            g0 = nY + r["Rt"] * gC + r["g"]
            got = [counts[g0], counts[g0 + nC]]
        else:
            g0 = 2 * r["Rt"] * gY + r["g"] + (nY + 2 * nC if r["kind"] == "alpha" else 0)
            got = [counts[g0], counts[g0 + gY]]
        assert got == r["entries"], R.brief(r)
        assert r["scatter_trips"] == [len(range(64, n, 64)) for n in got]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_oracle_decodes_every_case(O, case):
    n = case.width * HEIGHT
    for ptype in (PIC_I, PIC_P, PIC_B):
        out = R.expected(case.name, ptype, True)
        assert out.shape == (n * 5 // 2,) and np.array_equal(out[:n * 3 // 2], R.expected(case.name, ptype, False))
    # the forms differ: the prediction is in them
    assert not np.array_equal(R.expected(case.name, PIC_I, True), R.expected(case.name, PIC_P, True))
    assert not np.array_equal(R.expected(case.name, PIC_P, True), R.expected(case.name, PIC_B, True))


def test_the_model_of_the_column_pass_is_the_oracles_pass_1(O):
    """task_facts' own arithmetic (dequant, butterfly8, the hand-off) against lo_pass1_plane: the counters above rest on it"""
    for c in CASES:
        t = c.picture(PIC_P)
        cw = c.width
        want = O.pass1_plane(t["coef_y"], cw, HEIGHT, False, t["qscale"], t["intra"], cw // 16, R.QM, R.PREMULTIPLIER.astype(np.uint8))
        q, ia = t["qscale"].reshape(-1, cw // 16), t["intra"].reshape(-1, cw // 16)
        for Rb in range(HEIGHT // 8):
            for Q in range(cw // 8):
                X = t["coef_y"][8 * Rb:8 * Rb + 8, 8 * Q:8 * Q + 8].T.astype(np.int64)              # [c][i]
                o = R.butterfly8(R.dequant(X, [q[Rb // 2, Q // 2]] * 8, [ia[Rb // 2, Q // 2] != 0] * 8, np.arange(8)))[0]
                w = R.handoff_store(np.floor(o.astype(np.float32) * np.float32(0.4)).astype(np.int64))
                assert np.array_equal(w, want[8 * Rb:8 * Rb + 8, 8 * Q:8 * Q + 8]), (c.name, Rb, Q)


# ---- the streams of the cases a stream can carry (tests/test_recon_structure_gpu.py runs them through the pipeline) ----------------

def test_streams_carry_every_case_but_the_magnitudes():
    assert [c.name for c in CASES if not R.codable(c)] == list(R.SATURATING)


def test_streams_cover_every_item_but_those_of_the_abi_roads():
    """what the codable cases still show, asked of the pictures the streams carry: all but the levels no stream codes and yuva"""
    assert R.stream_items() == set(ITEMS) - set(R.ABI_ONLY) and set(R.ABI_ONLY) <= set(ITEMS)


@pytest.mark.parametrize("cw", R.WIDTHS)
def test_streams_are_whole_gops_and_parse_to_what_was_written(O, cw):
    from helpers import oracle_frames_from_tensors, stream_carried_masks
    from test_pipeline_gpu import oracle_frames
    import leon_vlc_ctypes as V
    data, pics, starts, names = R.stream(cw)
    # every GOP I B B P B B: display indices 0 .. 5 once each, none past the stream's longest GOP
    assert len(pics) == 6 * len(names) and starts == list(range(0, len(pics), 6))
    assert all(sorted(t["display"] for t in pics[s:s + 6]) == list(range(6)) and pics[s]["type"] == PIC_I for s in starts)
    st = V.Stream(data, threads=1)
    assert bytes(st.info.non_intra_qm) == R.QM_NON.tobytes() and bytes(st.info.intra_qm) == R.QM_INTRA.tobytes()
    for t in pics:
        p = st.next_picture(dense=True)
        assert p["type"] == t["type"] and p["temporal_reference"] == t["display"]
        for k, m in stream_carried_masks(t, cw, HEIGHT).items():
            assert np.array_equal(np.asarray(p[k]).reshape(-1)[m.reshape(-1)], np.asarray(t[k]).reshape(-1)[m.reshape(-1)]), (k, t["display"])
    assert st.next_picture(dense=True) is None
    want = oracle_frames_from_tensors(pics, cw, HEIGHT, gop_starts=starts, qm=R.QM)
    parsed = oracle_frames(data)
    assert set(want) == set(parsed) and all(np.array_equal(want[k]["rgba"], parsed[k]) for k in want)


def test_equivalent_forms_of_three_kernel_lines():
    """three one-line changes of csrc/leon_kernels.h that no test can tell apart, because the stored values are the same:
    mx >= 32768 against >: when the largest |s| of a lane is exactly 32768.0 every hand-off value is within +-32768, where the
    reference's store (handoff_store) is the int16 cast the kernel's store applies anyway; t = 128 against 0 in a half without
    coefficients: the byte is clamp((t + 256 p) >> 8) = p for both, every prediction p; clzll(colbits | 1) against clzll(colbits): the
    branch runs with colbits != 0 only"""
    w = np.arange(-32768, 32769, dtype=np.int64)
    assert np.array_equal(R.handoff_store(w), w.astype(np.int16).astype(np.int64))
    assert R.handoff_store(65536) != np.int64(65536).astype(np.int16) and R.handoff_store(-65537) != np.int64(-65537).astype(np.int16)
    p = np.arange(256)
    assert np.array_equal(np.clip((128 + 256 * p) >> 8, 0, 255), p) and np.array_equal(np.clip((0 + 256 * p) >> 8, 0, 255), p)
    for bits in [1 << k for k in range(64)] + [(1 << 64) - 1, 0x8000000000000001]:
        clz = 64 - bits.bit_length()
        assert 64 - (bits | 1).bit_length() == clz
