"""CPU: which branches of resample_body (csrc/leon_kernels.h) the geometries of tests/resample_structure.py reach -- every case shows
the fact it is there for, and together they show every item of the list below, so a case that drifts off its edge fails here, on any
machine.  The rounding ties and the clamps the arithmetic cases are about are counted on a seeded image.  The C table builder
(leon_pipeline_resize_weights) is held against the Python statement (leon_ctypes.resize_weights) entry for entry over every small axis
and a seeded sample of large ones, return code included, and resize_rgb against Pillow where Pillow imports, 0 differing bytes."""
import numpy as np
import pytest

import resample_structure as R
from resample_structure import BICUBIC, CASES, PACKED, TRIANGLE
from test_pipeline_tensor_bicubic_abi import c_weights
from test_pipeline_tensor_bicubic_gpu import unclamped_range

FILTERS = pytest.mark.parametrize("filt", [TRIANGLE, BICUBIC], ids=["triangle", "bicubic"])
TIE_CASES = ["two-times", "four-times"]
CLAMP_CASES = ["clamps-at-seam-and-fill-row"]


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    return leon_ctypes


def random_frame(case, seed=20240):
    """the oracle-independent image of a case's frame: random bytes of a fixed seed"""
    fw, fh = case.frame
    return np.random.default_rng(seed).integers(0, 256, (fh, fw, 3), dtype=np.uint8)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_every_case_exhibits_its_fact(case):
    assert case.kind in ("staging", "store") and case.stream in R.STREAMS and case.filters
    for f in case.filters:
        assert case.fact(case, f), "%s (%s) no longer shows: %s" % (case.name, R.FILTER_NAMES[f], case.why)


@pytest.mark.parametrize("name", sorted(R.STREAMS))
def test_streams_are_whole_gops(name):
    """the pipeline takes a temporal reference below the longest GOP of its stream only, and renders each into its own frame of the ring:
    the GOPs are unequal, so that in one window the frame_ids skip ring positions, and every display index lies inside the ring"""
    import synth as S
    gops = R.STREAMS[name][2]
    assert len(gops) == 2 and len(set(gops)) == 2
    written = [S.gop_ibbp(n) for n in gops]
    assert [len(g) for g in written] == gops
    for g in written:
        shown = sorted(d for _, d, _, _ in g)
        assert len(set(shown)) == len(shown) and shown[-1] < max(gops)


def tiles_of(pred, filt=None, kind=None):
    """the (case, filter, tile) for which pred(tile) holds"""
    return [(c.name, f, t) for c in CASES if kind in (None, c.kind) for f in c.filters if filt in (None, f) for t in c.tiles(f) if pred(t)]


def test_staging_facts_are_complete():
    facts = {
        "sw8 == 1": tiles_of(lambda t: t["sw8"] == 1),
        "sw8 == 65, triangle": tiles_of(lambda t: t["sw8"] == 65, TRIANGLE),
        "sw8 >= 67, bicubic": tiles_of(lambda t: t["sw8"] >= 67, BICUBIC),
        "sw8 does not divide 256, more than one pair a chunk": tiles_of(lambda t: 256 % t["sw8"] and t["col_step"] and t["last_rows"] > 2),
        "1 chunk": tiles_of(lambda t: t["n_chunks"] == 1),
        "2 chunks": tiles_of(lambda t: t["n_chunks"] == 2),
        ">= 3 chunks": tiles_of(lambda t: t["n_chunks"] >= 3),
        "last chunk of 1 row": tiles_of(lambda t: t["n_chunks"] >= 2 and t["last_rows"] == 1),
        "odd last chunk of >= 3 rows": tiles_of(lambda t: t["n_chunks"] >= 2 and t["last_rows"] >= 3 and t["last_rows"] & 1),
        "first_x - cx0 == 0": tiles_of(lambda t: t["x_off"] == 0),
        "first_x - cx0 == 7": tiles_of(lambda t: t["x_off"] == 7),
        "first_y - ry0 == 0": tiles_of(lambda t: t["y_off"] == 0),
        "first_y - ry0 == 1": tiles_of(lambda t: t["y_off"] == 1),
        "fill row tapped by a last chunk of several": tiles_of(lambda t: t["n_chunks"] >= 2 and t["fill_in_last_chunk"] and t["fill_weights"]),
        "fill row alone in the last chunk": tiles_of(lambda t: t["n_chunks"] >= 2 and t["fill_in_last_chunk"] and t["last_rows"] == 1),
        "fill row under a negative bicubic weight": tiles_of(lambda t: any(w < 0 for w in t["fill_weights"]), BICUBIC),
    }
    for filt in (TRIANGLE, BICUBIC):
        for n in (1, 31, 32):
            facts["nox == %d, filter %d" % (n, filt)] = tiles_of(lambda t: t["nox"] == n, filt)
        for n in (1, 7, 8):
            facts["noy == %d, filter %d" % (n, filt)] = tiles_of(lambda t: t["noy"] == n, filt)
    missing = sorted(k for k, v in facts.items() if not v)
    assert not missing, "no case shows: %s" % missing


def test_size_and_tap_facts_are_complete():
    def ratio(c):
        return (c.box[2] / c.size[1], c.box[3] / c.size[0])
    shown = {
        "1 x 1 at ratio 16 on both axes": [c for c in CASES if c.size == (1, 1) and ratio(c) == (16.0, 16.0)],
        "a 1 x 1 crop enlarged": [c for c in CASES if c.box[2:] == (1, 1) and c.size[0] > 1 and c.size[1] > 1],
        "exact 2x": [c for c in CASES if ratio(c) == (0.5, 0.5)],
        "exact 4x": [c for c in CASES if ratio(c) == (0.25, 0.25)],
        "scale 1": [c for c in CASES if ratio(c) == (1.0, 1.0)],
    }
    for filt in (TRIANGLE, BICUBIC):
        axes = [c.axes(filt) for c in CASES if filt in c.filters]
        for i, axis in enumerate("xy"):
            for side in ("lo", "hi"):
                shown["taps clipped by the frame, %s %s, filter %d" % (axis, side, filt)] = [a for a in axes if a[i]["clipped_" + side]]
                shown["taps leaving the crop, %s %s, filter %d" % (axis, side, filt)] = [a for a in axes if a[i]["leaves_" + side]]
        shown["an axis of the most taps, filter %d" % filt] = [a for a in axes if max(a[0]["max_taps"], a[1]["max_taps"]) >= (32 if filt == TRIANGLE else 64)]
    for name in TIE_CASES + CLAMP_CASES:
        assert name in R.BY_NAME
    assert all(set(c.filters) == {TRIANGLE, BICUBIC} for c in shown["exact 2x"] + shown["exact 4x"])
    missing = sorted(k for k, v in shown.items() if not v)
    assert not missing, "no case shows: %s" % missing


@pytest.mark.parametrize("eb,layout", PACKED, ids=["%d-%s" % p for p in PACKED])
def test_store_facts_are_complete(eb, layout):
    rows = [r for c in CASES if c.kind == "store" for r in c.store(eb, layout)]
    assert {r["start"] for r in rows} == set(range(0, 16, eb))                                    # every start class the element size has
    assert any(r["bytes"] < 16 and "b128" not in r["lines"] for r in rows)                        # a row shorter than a line
    assert any(r["bytes"] < 16 and r["start"] and r["start"] + r["bytes"] <= 16 for r in rows)    # ... behind another row in the same line
    assert any(r["bytes"] < 16 and r["start"] + r["bytes"] > 16 for r in rows) or eb == 4         # ... across two lines
    assert any(r["start"] == 0 and r["end"] == 0 and set(r["lines"]) == {"b128"} for r in rows)   # both ends aligned: b128 alone
    assert any(r["lines"][0] == "elem" and r["lines"][-1] == "elem" and "b128" in r["lines"] for r in rows)          # both ends ragged
    assert any(r["nox"] < 32 and r["noy"] == 8 for r in rows) and any(r["noy"] < 8 and r["nox"] == 32 for r in rows) and any(r["nox"] < 32 and r["noy"] < 8 for r in rows)
    # what the kernel's shapes rest on: a row's lines fit a power of two of lanes (4 for uint8 CHW, 32 for HWC)
    assert max(len(r["lines"]) for r in rows) <= (4 if layout == "chw" else 32)


def tie_counts(L, img, crop, size, filt):
    """(horizontal, vertical) sums with (sum + 2^21) & (2^22 - 1) == 0: the value lies exactly between two 8-bit results"""
    fh, fw = img.shape[:2]
    x, y, w, h = crop or (0, 0, fw, fh)
    fx, nx, wx = L.resize_weights(fw, x, w, size[1], filt)
    fy, ny, wy = L.resize_weights(fh, y, h, size[0], filt)

    def one_pass(src, first, count, weights):
        ties = 0
        out = np.empty((src.shape[0], len(first), 3), dtype=np.uint8)
        s64 = src.astype(np.int64)
        for o in range(len(first)):
            n = int(count[o])
            acc = np.tensordot(s64[:, first[o]:first[o] + n], weights[o, :n].astype(np.int64), axes=([1], [0])) + (1 << 21)
            ties += int(((acc & ((1 << 22) - 1)) == 0).sum())
            out[:, o] = np.clip(acc >> 22, 0, 255)
        return out, ties
    r0, r1 = int(fy.min()), int((fy + ny).max())
    hz, th = one_pass(img[r0:r1], fx, nx, wx)
    vt, tv = one_pass(hz.transpose(1, 0, 2), fy - r0, ny, wy)
    assert np.array_equal(vt.transpose(1, 0, 2), L.resize_rgb(img, crop, size, filt))          # the same two passes as the statement
    return th, tv


@FILTERS
@pytest.mark.parametrize("name", TIE_CASES)
def test_ties_are_real(L, name, filt):
    """at exact 2x and 4x the weights are multiples of 2^22 / 4, / 8, / 64 ...: sums land on the rounding tie, where 2^21 and 2^21 - 1 differ"""
    case = R.BY_NAME[name]
    th, tv = tie_counts(L, random_frame(case), case.crop, case.size, filt)
    assert th > 0 and tv > 0, (th, tv)


@pytest.mark.parametrize("name", CLAMP_CASES)
def test_clamps_are_real(L, name):
    case = R.BY_NAME[name]
    lo, hi = unclamped_range(L, random_frame(case), case.crop, case.size)
    assert lo < 0 and hi > 255, (lo, hi)


# ---- the C tables against the Python statement, swept ------------------------------------------------------------------------------------
def compare_axis(L, axis, filt):
    """leon_pipeline_resize_weights == resize_weights for one (in, crop_start, crop_size, out): 1 if both build tables, 0 if both refuse"""
    max_taps = L.RESIZE_MAX_TAPS_BICUBIC if filt == BICUBIC else L.RESIZE_MAX_TAPS
    try:
        pf, pn, pw = L.resize_weights(*axis, filter=filt)
    except ValueError:
        pf = None
    rc, first, count, w = c_weights(L, *axis, filt, max_taps)
    if pf is None:
        assert rc == L.ERR_INVALID, "%s filter %d: the statement refuses, the library returns %d" % (axis, filt, rc)
        return 0
    assert rc == L.OK, "%s filter %d: the library refuses (%s), the statement does not" % (axis, filt, L.load().leon_last_error())
    assert np.array_equal(first, pf) and np.array_equal(count, pn), "%s filter %d: first / count differ" % (axis, filt)
    assert np.array_equal(w[:, :pw.shape[1]], pw) and not w[:, pw.shape[1]:].any(), "%s filter %d: weights differ" % (axis, filt)
    assert all(not w[o, count[o]:].any() for o in range(0, len(count), max(1, len(count) // 16))), "%s filter %d: weights behind a count" % (axis, filt)
    return 1


@FILTERS
def test_c_tables_equal_the_statement_on_every_small_axis(L, filt):
    """all (in, out) with 1 <= in, out <= 48, the whole axis: 2304 geometries a filter, those of a ratio above 16 refused by both"""
    built = sum(compare_axis(L, (n, 0, n, out), filt) for n in range(1, 49) for out in range(1, 49))
    assert built == sum(1 for n in range(1, 49) for out in range(1, 49) if n <= 16 * out)


def sampled_axes(seed, n):
    """(in, crop_start, crop_size, out) with in, out <= 4096 and ratios up to 16 (and a few just beyond, which are refused): weighted
    towards ratios of exactly 16 and 1 / integer, and towards crops that touch either end of the axis.  Outputs are kept short of 600
    (the statement is a Python loop per output sample) but for a few of the full 4096."""
    rng = np.random.default_rng(seed)
    axes = []
    while len(axes) < n:
        kind = rng.integers(0, 6)
        out = int(rng.integers(1, 600)) if rng.integers(0, 20) else int(rng.integers(3500, 4097))
        if kind == 0:                                  # ratio exactly 16
            out = min(out, 256)
            crop = 16 * out
        elif kind == 1:                                # 1 / integer: exact enlargements
            k = int(rng.integers(1, 9))
            crop = max(1, out // k)
            out = crop * k
        elif kind == 2:                                # just around 16
            out = min(out, 255)
            crop = 16 * out + int(rng.integers(-2, 3))
        else:
            crop = int(rng.integers(1, min(4096, 16 * out) + 1))
        crop = max(1, min(crop, 4096))
        size = int(rng.integers(crop, min(4096, crop + 200) + 1))
        start = int((0, size - crop, rng.integers(0, size - crop + 1))[rng.integers(0, 3)])          # touching the start, the end, anywhere
        axes.append((size, start, crop, out))
    return axes


SAMPLED = 1200


@FILTERS
def test_c_tables_equal_the_statement_on_a_sample_of_large_axes(L, filt):
    axes = sampled_axes(4096 + filt, SAMPLED)
    assert any(c == 16 * o for _, _, c, o in axes) and any(c > 16 * o for _, _, c, o in axes) and any(o > c and o % c == 0 for _, _, c, o in axes)
    assert any(s == 0 and c < n for n, s, c, _ in axes) and any(s > 0 and s + c == n for n, s, c, _ in axes) and any(o > 3500 for _, _, _, o in axes)
    built = sum(compare_axis(L, a, filt) for a in axes)
    assert SAMPLED // 2 < built < SAMPLED


def test_refusals_agree(L):
    """empty and escaping crops, sizes outside 1 .. 4096, ratios beyond 16: refused by both, for both filters"""
    for filt in (TRIANGLE, BICUBIC):
        for axis in ((0, 0, 0, 1), (10, 0, 0, 4), (10, -1, 5, 4), (10, 6, 5, 4), (10, 10, 1, 4), (10, 11, 0, 4), (10, 0, 10, 0), (10, 0, 10, 4097), (4096, 0, 4096, 255),
                     (17, 0, 17, 1), (33, 1, 32, 1), (33, 17, 16, 1)):
            built = compare_axis(L, axis, filt)
            assert built == (1 if axis == (33, 17, 16, 1) else 0), axis


# ---- resize_rgb against Pillow ------------------------------------------------------------------------------------------------------------
def checkerboard(fw, fh):
    yy, xx = np.mgrid[0:fh, 0:fw]
    return np.repeat(((((yy + xx) & 1) * 255).astype(np.uint8))[..., None], 3, axis=2)


def assert_equals_pillow(L, img, crop, size, filt, what):
    from PIL import Image
    fh, fw = img.shape[:2]
    x, y, w, h = crop or (0, 0, fw, fh)
    oh, ow = size
    got = L.resize_rgb(img, crop, size, filter=filt)
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC if filt == BICUBIC else Image.BILINEAR, box=(x, y, x + w, y + h), reducing_gap=None))
    assert got.shape == ref.shape == (oh, ow, 3)
    assert int((got != ref).sum()) == 0, "%s: %d bytes differ from Pillow" % (what, int((got != ref).sum()))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_resize_rgb_equals_pillow_on_every_case(L, case):
    pytest.importorskip("PIL")
    fw, fh = case.frame
    for filt in case.filters:
        for kind, img in (("random", random_frame(case)), ("checkerboard", checkerboard(fw, fh))):
            assert_equals_pillow(L, img, case.crop, case.size, filt, "%s %s filter %d" % (case.name, kind, filt))


def small_geometries(seed, n):
    """(frame (w, h), crop, size (h, w)): frames up to 40 x 40, any crop inside, outputs up to 48 within a reduction of 16"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        fw, fh = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        w, h = int(rng.integers(1, fw + 1)), int(rng.integers(1, fh + 1))
        x, y = int(rng.integers(0, fw - w + 1)), int(rng.integers(0, fh - h + 1))
        ow, oh = int(rng.integers((w + 15) // 16, 49)), int(rng.integers((h + 15) // 16, 49))
        if rng.integers(0, 4) == 0:
            ow, oh = w * int(rng.integers(1, 5)), h * int(rng.integers(1, 5))          # scale 1 and exact enlargements
        out.append(((fw, fh), (x, y, w, h), (min(oh, 96), min(ow, 96))))
    return out


@FILTERS
def test_resize_rgb_equals_pillow_on_a_sample_of_small_geometries(L, filt):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(77 + filt)
    for i, ((fw, fh), crop, size) in enumerate(small_geometries(200, 200)):
        img = checkerboard(fw, fh) if i % 4 == 3 else rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
        assert_equals_pillow(L, img, crop, size, filt, "%dx%d %s -> %s filter %d" % (fw, fh, crop, size, filt))
