"""CPU: k_warp across the legal record set (tests/warp_structure.py: sweep), not only the 17 named matrices -- what every sweep record
holds (tests/warp_structure.py: assert_record_facts), what the sweep is there for (staged widths 1 .. 20 groups, 64 and more row pairs,
a second pass of stage (1)'s index walk at every width from 4 groups on,
pieces cut by two frame edges, the fill row under S = 4, records on the thresholds of warp_supersample), that it compares more than
pad with pad, the same facts over the boundary of the legal set -- with the finding that no legal record takes a level above 1 --
and a second, scalar statement of the definition of include/leon_pipeline.h against leon_ctypes.warp_rgb.  Nothing here touches a
device; tests/test_pipeline_warp_sweep_gpu.py runs the same records through the kernels."""
import ctypes as C

import numpy as np
import pytest

import leon_ctypes as L
import warp_structure as W

CASES = [(name, size) for name in sorted(W.SIZES) for size in W.SIZES[name]]


def pieces(tiles):
    return [p for t in tiles for p in t["pieces"]]


def is_cut(p):
    return not p["outside"] and (p["cut_left"] or p["cut_right"] or p["cut_top"] or p["cut_bottom"])


_facts = {}


def facts(name, size):
    """[(record name, m, tile_facts)] of one call's sweep, computed once"""
    if (name, size) not in _facts:
        wh = W.frame_wh(name)
        _facts[(name, size)] = [(n, m, W.tile_facts(wh, m, size)) for n, m in W.sweep(wh, size)]
    return _facts[(name, size)]


@pytest.mark.parametrize("name,size", CASES, ids=lambda v: str(v))
def test_every_sweep_record_is_legal_and_holds_the_per_record_facts(name, size):
    wh = W.frame_wh(name)
    sweep = W.sweep(wh, size)
    assert sweep == W.sweep(wh, size) and len({n for n, _ in sweep}) == len(sweep) and 90 <= len(sweep) <= 120
    assert sum(n.startswith("random") for n, _ in sweep) >= 48
    for n, m in sweep:
        assert W.record_status(0, m, 0, 9) == L.REGION_OK and L.warp_region_status(wh[0], wh[1], 9, (0, m), size) == L.REGION_OK, (n, m)
        W.assert_record_facts(wh, n, m, size)


def test_the_sweep_holds_what_it_is_here_for():
    """Between the streams: every staged width from 1 to 20 groups of 8 columns (21 as well, the most warp_span_bound allows); a piece
    of at least 64 row pairs at most 2 groups wide; a piece at least 17 groups wide of at most 4 pairs; a piece cut by two frame edges
    at once at S = 2 and at S = 4; a fill-row piece at S = 4; all four (g, level) that exist.  Stage (1)'s index walk: a lane stages one
    (row pair, group) slot a pass, 256 slots a pass, so only a piece with sw8 * n_pairs > 256 runs `pair += pair_step; col += col_step`
    and the wrap at `col >= sw8` -- the tallest piece (81 pairs, 2 groups) and the widest (21 groups, 2 pairs) are done in one pass.
    For every width from 4 to 21 groups some staged piece has more than 256 slots (below 4 groups none can: 81 pairs at most), and it
    is the piece of that width's named walk_* record.  That holds the widths where 256 is no multiple of sw8, col_step is not 0 and the
    wrap happens, and 4, 8 and 16, where it cannot.
    Only pieces that are staged count: one wholly outside stages nothing."""
    staged = [(t["g"], t["level"], p) for name, size in CASES for _, _, tiles in facts(name, size) for t in tiles for p in t["pieces"] if not p["outside"]]
    sw8 = {(p["box"][1] - p["box"][0]) // 8 for _, _, p in staged}
    assert set(range(1, 21)) <= sw8 and max(sw8) <= 21, sorted(sw8)
    shape = {((p["box"][1] - p["box"][0]) // 8, (p["box"][3] - p["box"][2]) // 2) for _, _, p in staged}
    assert any(w <= 2 and n >= 64 for w, n in shape) and any(w >= 17 and n <= 4 for w, n in shape)
    assert max(n for _, n in shape) <= 81
    for w in range(4, 22):
        assert any(ww == w and w * n > 256 for ww, n in shape), w
    # ... and through its own walk_* record, not by the seed's favour
    named_walks = {w for name, size in CASES for n, _, tiles in facts(name, size) for w in W.WALKS if n == "walk_%d" % w
                   for p in pieces(tiles) if not p["outside"] and p["box"][1] - p["box"][0] == 8 * w and w * (p["box"][3] - p["box"][2]) // 2 > 256}
    assert named_walks == set(range(4, 22))
    for g in (1, 2):
        assert any(gg == g and (p["cut_left"] or p["cut_right"]) and (p["cut_top"] or p["cut_bottom"]) for gg, _, p in staged), g
    assert any(g == 2 and p["fill_row"] for g, _, p in staged)
    assert {(g, level) for g, level, _ in staged} == {(0, 0), (1, 0), (2, 0), (2, 1)}


def test_threshold_records_take_the_stated_g():
    """host and device must pick the same S where a word decides it: column norm exactly lim_g is g, one word above it -- through the
    diagonal entry, through the off-diagonal entry, through a 45 degree pair -- is g + 1, and above lim_2 refused"""
    stated = W.thresholds()
    assert len(stated) == 15 and [g for _, _, g in stated] == [0, 1, 1, 0, 1, 1, 2, 2, 1, 2, 2, None, None, 2, None]
    for n, A, g in stated:
        m = (A[0], A[1], 0, A[2], A[3], 0)
        assert W.supersample(m) == g, n
        assert L.warp_region_status(96, 64, 9, (0, m), (8, 32)) == (L.REGION_OK if g is not None else L.REGION_SCALE), n
    for g, lim in enumerate(W.LIM):          # the 45 degree pair is the last word below and the first above
        c, _, d, _ = [A for n, A, _ in stated if n == "thr%d_45_at" % g][0]
        assert c * c + d * d <= lim * lim < c * c + (d + 1) * (d + 1) and abs(c - d) <= 1
    sweep = dict(W.sweep(W.frame_wh("96x64"), (8, 32)))
    for n, A, g in stated:
        assert (n in sweep) == (g is not None) and (g is None or W.supersample(sweep[n]) == g), n
    refused = W.sweep_refused(9)
    assert len(refused) == 10 and all(W.record_status(f, m, r, 9) == st for _, (f, m, r), st in refused)
    assert [st for _, _, st in refused] == [L.REGION_SCALE] * 2 + [L.REGION_OFFSET] * 2 + [L.REGION_SCALE] * 2 + [L.REGION_OFFSET] + [L.REGION_SCALE] * 2 + [L.REGION_OFFSET]
    assert all(L.warp_region_status(96, 64, 9, L.PipelineWarpRegion(f, (C.c_int32 * 6)(*m), r), (8, 32)) == st for _, (f, m, r), st in refused)


@pytest.mark.parametrize("name,size", CASES, ids=lambda v: str(v))
def test_a_call_compares_more_than_pad_with_pad(name, size):
    """at most a quarter of a call's records lie wholly outside the frame, at least half have a staged piece that a frame edge cuts"""
    f = facts(name, size)
    outside = sum(all(p["outside"] for p in pieces(tiles)) for _, _, tiles in f)
    cut = sum(any(is_cut(p) for p in pieces(tiles)) for _, _, tiles in f)
    assert 4 * outside <= len(f) and 2 * cut >= len(f), (outside, cut, len(f))
    by_name = {n: tiles for n, _, tiles in f}
    # what the named records say of themselves
    for n in ("tx+limit", "tx-limit", "ty+limit", "ty-limit", "tx-limit_lim2", "rank0_outside"):
        assert all(p["outside"] for p in pieces(by_name[n])), n
    assert not any(p["outside"] for p in pieces(by_name["rank0_inside"]))
    assert any(p["cut_right"] and p["cut_bottom"] for p in pieces(by_name["rank0_corner"]))


def test_the_regions_are_dealt_over_every_frame_out_of_order():
    regs = W.sweep_regions(W.frame_wh("96x64"), (8, 32), 9)
    frames = [r[0] for r in regs]
    assert set(frames) == set(range(9)) and frames != sorted(frames) and [m for _, m in regs] == [m for _, m in W.sweep(W.frame_wh("96x64"), (8, 32))]


# ---- the legal set as a whole --------------------------------------------------------------------------------------------------------
def span_bound_np(a, b, g, pw, ph, align):
    S2 = 2 << g
    d = np.abs(a) * (S2 * pw - 2) + np.abs(b) * (S2 * ph - 2)
    return ((d >> (g + 17)) + 3 + 2 * (align - 1)) & ~(align - 1)


def level_dwords_np(a00, a01, a10, a11, g, level):
    pw, ph = W.piece_size(level)
    return (span_bound_np(a00, a01, g, pw, ph, 8) + 1) * span_bound_np(a10, a11, g, pw, ph, 2)


STEP = 0.5          # degrees


def test_no_legal_record_takes_a_level_above_1():
    """kWarpLevels is 5, but levels 2 to 4 (pieces 16 x 4, 8 x 4, 8 x 2) are unreachable: k_warp's row loop `for py` takes one trip on
    every input.  Over the boundary of the legal set -- both column norms at lim_g, g = 0, 1, 2, both angles over the full turn in
    steps of 0.5 degrees, so every combination of signs -- level_of is at most 1, the bound of the level taken fits the stage, and the
    largest level-1 bound is (80 + 1) * 74 = 5994 dwords of the stage's 8192 (columns at 43.5 and 56 degrees), pinned by equality so that a change of the stage, of the
    piece sizes or of the thresholds shows up here.  The boundary bounds the interior: warp_span_bound is non-decreasing in |a| and
    |b|, and a column of smaller norm at the same angle has both entries no larger.  The angle grid is a sample of the boundary; the
    second half closes it: over each cell of 0.5 x 0.5 degrees every entry is replaced by the largest magnitude it takes anywhere in the
    cell, which dominates every legal matrix whose column angles lie in the cell, and level 1 still fits -- with the same maximum, so
    5994 is the legal set's, not only the grid's."""
    deg = np.arange(0.0, 360.0, STEP)
    worst = worst_cell = 0
    for g, lim in enumerate(W.LIM):
        cos, sin = np.trunc(lim * np.cos(np.radians(deg))).astype(np.int64), np.trunc(lim * np.sin(np.radians(deg))).astype(np.int64)
        assert (cos * cos + sin * sin <= lim * lim).all() and (cos * cos + sin * sin > (lim - 2) ** 2).all()          # the norm is lim_g's: g is g
        a00, a01, a10, a11 = cos[:, None], cos[None, :], sin[:, None], sin[None, :]
        fits0, fits1 = level_dwords_np(a00, a01, a10, a11, g, 0) <= W.STAGE_PX, level_dwords_np(a00, a01, a10, a11, g, 1) <= W.STAGE_PX
        assert (fits0 | fits1).all(), g                                    # level_of <= 1, and level_fits at that level
        assert fits0.all() == (g < 2)                                      # only S = 4 splits a tile at all
        worst = max(worst, int(level_dwords_np(a00, a01, a10, a11, g, 1)[~fits0].max(initial=0)))
        # the same through the scalar text, on a coarser grid, so that the vectorised copy above is the text's
        for i in range(0, len(deg), 45):
            for j in range(0, len(deg), 30):
                m = (int(cos[i]), int(cos[j]), 0, int(sin[i]), int(sin[j]), 0)
                level = W.level_of(m, g)
                assert W.supersample(m) == g and level == (0 if fits0[i, j] else 1) and W.level_fits(m, g, level)
        # every cell of the grid, entries at their largest magnitude inside it (the extremes of |cos|, |sin| over an interval lie at
        # its ends or at a multiple of 90 degrees, which is a grid point)
        hi_c = np.ceil(lim * np.maximum(np.abs(np.cos(np.radians(deg))), np.abs(np.cos(np.radians(deg + STEP))))).astype(np.int64)
        hi_s = np.ceil(lim * np.maximum(np.abs(np.sin(np.radians(deg))), np.abs(np.sin(np.radians(deg + STEP))))).astype(np.int64)
        assert g == 2 or (level_dwords_np(hi_c[:, None], hi_c[None, :], hi_s[:, None], hi_s[None, :], g, 0) <= W.STAGE_PX).all()          # S = 1, 2 never split
        worst_cell = max(worst_cell, int(level_dwords_np(hi_c[:, None], hi_c[None, :], hi_s[:, None], hi_s[None, :], g, 1).max()))
    assert worst <= worst_cell <= W.STAGE_PX
    assert worst == 5994 and worst_cell == 5994


def test_taps_and_relative_numerators_over_2000_legal_records():
    """seeded: g uniform, columns lim_g * r * (cos, sin) with independent angles and r in {1, U(0, 1)}, offsets uniform over the whole
    +-2^29, out size (24, 70): every tap in its staged box, every box within span_bound and the stage, both relative numerators below
    2^28 (the largest is about 2^26.4: |a| + |b| <= sqrt 2 * lim_2 words times 2S * 31 + 2S - 1 columns, plus the alignment's 8 pixels)"""
    rng = np.random.default_rng(2000)
    worst = 0
    for k in range(2000):
        g = int(rng.integers(0, 3))
        cols = [W.polar(W.LIM[g], 1.0 if rng.integers(0, 2) else float(rng.uniform()), float(rng.uniform(0.0, 360.0))) for _ in range(2)]
        tx, ty = (int(v) for v in rng.integers(-W.MAX_OFFSET, W.MAX_OFFSET + 1, 2))
        if k < 4:          # the four corners of the offsets' square
            tx, ty = W.MAX_OFFSET * (1 - 2 * (k & 1)), W.MAX_OFFSET * (1 - (k & 2))
        m = (cols[0][0], cols[1][0], tx, cols[0][1], cols[1][1], ty)
        assert W.record_status(0, m, 0, 1) == L.REGION_OK
        worst = max(worst, W.assert_record_facts((608, 57), "legal%d" % k, m, (24, 70)))
    assert 1 << 26 < worst < 1 << 27


# ---- the definition once more, scalar ------------------------------------------------------------------------------------------------
def warp_pixel(rgb, m, ox, oy, pad):
    """One output pixel from the text of include/leon_pipeline.h in plain Python integers: S x S samples, four taps each, the pad outside
    the frame, one rounding.  Independent of warp_rgb's padded border and clipped indices."""
    H, W_ = len(rgb), len(rgb[0])
    a00, a01, tx, a10, a11, ty = m
    s2 = max(a00 * a00 + a10 * a10, a01 * a01 + a11 * a11)
    g = 0 if s2 <= (2 ** 16 + 1) ** 2 else 1 if s2 <= (2 ** 17 + 1) ** 2 else 2
    assert s2 <= (2 ** 18 + 1) ** 2
    S = 1 << g

    def p(x, y, c):
        return rgb[y][x][c] if 0 <= x < W_ and 0 <= y < H else pad[c]
    acc = [0, 0, 0]
    for j in range(S):
        for i in range(S):
            NX = a00 * (2 * S * ox + 2 * i + 1) + a01 * (2 * S * oy + 2 * j + 1) + 2 * S * (tx - 32768)
            NY = a10 * (2 * S * ox + 2 * i + 1) + a11 * (2 * S * oy + 2 * j + 1) + 2 * S * (ty - 32768)
            qx, qy = ((NX >> (g + 1)) + 128) >> 8, ((NY >> (g + 1)) + 128) >> 8
            x0, fx, y0, fy = qx >> 8, qx & 255, qy >> 8, qy & 255
            for c in range(3):
                acc[c] += ((256 - fx) * (256 - fy) * p(x0, y0, c) + fx * (256 - fy) * p(x0 + 1, y0, c)
                           + (256 - fx) * fy * p(x0, y0 + 1, c) + fx * fy * p(x0 + 1, y0 + 1, c))
    assert max(acc) < 1 << 28
    return [(a + (1 << (15 + 2 * g))) >> (16 + 2 * g) for a in acc]


def test_the_scalar_definition_is_warp_rgb():
    """every sweep record of 100x57 (an odd height) at its three out sizes on a seeded random image: the four corner pixels and 32
    seeded pixels of warp_rgb equal the scalar statement"""
    name = "100x57"
    fw, fh = W.frame_wh(name)
    rng = np.random.default_rng(10057)
    image = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    rows = image.tolist()
    checked = 0
    for size in W.SIZES[name]:
        oh, ow = size
        for n, m in W.sweep((fw, fh), size):
            got = L.warp_rgb(image, m, size, W.PAD)
            assert got.shape == (oh, ow, 3) and got.dtype == np.uint8
            at = {(0, 0), (0, ow - 1), (oh - 1, 0), (oh - 1, ow - 1)} | {(int(y), int(x)) for y, x in zip(rng.integers(0, oh, 32), rng.integers(0, ow, 32))}
            for oy, ox in sorted(at):
                assert got[oy, ox].tolist() == warp_pixel(rows, m, ox, oy, W.PAD), (n, size, (ox, oy))
                checked += 1
    assert checked > 3 * 100 * 20
