"""The structure of k_warp (csrc/leon_kernels.h) and of the judgement it shares with the host (csrc/leon_warp.h), stated on the CPU:
how a record's supersampling follows from its matrix, into which pieces a 32 x 8 tile is cut, and which source footprint a piece
stages -- the bounding box of its four corner samples and their bilinear neighbours, aligned to 8 columns and even rows.  The
expressions are the kernel's, line for line; nothing here touches a device.

CALLS is the list tests/test_warp_structure.py (the facts), tests/test_pipeline_warp_gpu.py, tests/test_pipeline_warp_device_gpu.py
and tests/test_pipeline_warp_node_gpu.py (the kernels) share: per stream of resample_structure.STREAMS the out sizes and, for every
size, the named matrices.  sweep() is the wider list -- the legal record set beyond rotation x uniform scale -- that
tests/test_warp_sweep_structure.py and tests/test_pipeline_warp_sweep_gpu.py share.  A helper, not a test module."""
import math

import numpy as np

import leon_ctypes as L
from resample_structure import STREAMS

TILE_X, TILE_Y, BLOCK, STAGE_PX, LEVELS = 32, 8, 256, 8192, 5          # kResTileX, kResTileY, kRgbaBlock, kWarpStagePx, kWarpLevels
MAX_OFFSET = 1 << 29                                                   # kWarpMaxOffset


def supersample(m):
    """warp_supersample: g, or None above the last threshold"""
    s2 = max(m[0] * m[0] + m[3] * m[3], m[1] * m[1] + m[4] * m[4])
    return next((g for g in range(3) if s2 <= ((1 << (16 + g)) + 1) ** 2), None)


def record_status(frame, m, reserved, n_frames):
    """warp_record_status: the checks in their order"""
    if reserved:
        return L.REGION_RESERVED
    if frame < 0 or frame >= n_frames:
        return L.REGION_FRAME
    if supersample(m) is None:
        return L.REGION_SCALE
    if abs(m[2]) > MAX_OFFSET or abs(m[5]) > MAX_OFFSET:
        return L.REGION_OFFSET
    return L.REGION_OK


def numerator(a, b, t, g, ox, oy, i, j):
    S2 = 2 << g
    return a * (S2 * ox + 2 * i + 1) + b * (S2 * oy + 2 * j + 1) + S2 * (t - 32768)


def q(N, g):
    return ((N >> (g + 1)) + 128) >> 8


def piece_size(level):
    return (32 if level < 1 else 16 if level < 3 else 8), (8 if level < 2 else 4 if level < 4 else 2)


def span_bound(a, b, g, pw, ph, align):
    S2 = 2 << g
    d = abs(a) * (S2 * pw - 2) + abs(b) * (S2 * ph - 2)
    return ((d >> (g + 17)) + 3 + 2 * (align - 1)) & ~(align - 1)


def level_fits(m, g, level):
    pw, ph = piece_size(level)
    return (span_bound(m[0], m[1], g, pw, ph, 8) + 1) * span_bound(m[3], m[4], g, pw, ph, 2) <= STAGE_PX


def level_of(m, g):
    level = 0
    while level < LEVELS - 1 and not level_fits(m, g, level):
        level += 1
    return level


def footprint(m, g, x_first, y_first, qw, qh):
    """(sx0, sx1, sy0, sy1) of the piece of qw x qh output pixels at (x_first, y_first): what k_warp stages, [sx0, sx1) x [sy0, sy1)"""
    S = 1 << g
    x_last, y_last = x_first + qw - 1, y_first + qh - 1
    box = []
    for a, b, t in ((m[0], m[1], m[2]), (m[3], m[4], m[5])):
        n = [numerator(a, b, t, g, x_first, y_first, 0, 0), numerator(a, b, t, g, x_last, y_first, S - 1, 0),
             numerator(a, b, t, g, x_first, y_last, 0, S - 1), numerator(a, b, t, g, x_last, y_last, S - 1, S - 1)]
        box.append((q(min(n), g) >> 8, (q(max(n), g) >> 8) + 1))
    (x_lo, x_hi), (y_lo, y_hi) = box
    return x_lo & ~7, (x_hi + 8) & ~7, y_lo & ~1, (y_hi + 2) & ~1


def tile_facts(frame_wh, m, size_hw):
    """[{...}] per 32 x 8 tile in blockIdx order (y outer): the level, and per piece its footprint and what the frame makes of it"""
    fw, fh = frame_wh
    oh, ow = size_hw
    g = supersample(m)
    level = level_of(m, g)
    pw, ph = piece_size(level)
    tiles = []
    for oy0 in range(0, oh, TILE_Y):
        for ox0 in range(0, ow, TILE_X):
            nox, noy = min(TILE_X, ow - ox0), min(TILE_Y, oh - oy0)
            pieces = []
            for py in range(0, noy, ph):
                for px in range(0, nox, pw):
                    qw, qh = min(pw, nox - px), min(ph, noy - py)
                    sx0, sx1, sy0, sy1 = footprint(m, g, ox0 + px, oy0 + py, qw, qh)
                    pieces.append(dict(
                        at=(ox0 + px, oy0 + py), size=(qw, qh), box=(sx0, sx1, sy0, sy1), dwords=(sx1 - sx0 + 1) * (sy1 - sy0),
                        outside=sx1 <= 0 or sx0 >= fw or sy1 <= 0 or sy0 >= fh,
                        cut_left=sx0 < 0 < sx1, cut_right=sx0 < fw < sx1, cut_top=sy0 < 0 < sy1, cut_bottom=sy0 < fh < sy1,
                        fill_row=bool(fh & 1) and sy0 <= fh - 1 < sy1 and sx0 < fw and sx1 > 0))
            tiles.append(dict(at=(ox0, oy0), g=g, level=level, whole_fits=level_fits(m, g, 0), pieces=pieces))
    return tiles


# ---- the shared calls ---------------------------------------------------------------------------------------------------------------
# per stream: the out sizes (height, width).  (8, 32): one full tile; (13, 37): a tile and three part tiles, a row stride that is
# aligned to nothing; (1, 1); (24, 70): three tiles on both axes.
SIZES = {
    "96x64": [(8, 32), (1, 1)],
    "608x57": [(13, 37), (24, 70)],
    "100x57": [(8, 32), (13, 37), (24, 70)],
}
PAD = (114, 7, 250)


def matrices(frame_wh, size_hw):
    """[(name, m)] for one stream and out size: every matrix the issue lists, the boxes placed by the frame's and the out size"""
    fw, fh = frame_wh
    oh, ow = size_hw
    cx, cy = fw / 2.0, fh / 2.0
    box = L.warp_matrix_rotated_box
    return [
        ("identity", L.warp_matrix([1, 0, 3, 0, 1, 2])),
        ("rot90", box(cx, cy, ow, oh, 90, size_hw)),
        ("rot180", box(cx, cy, ow, oh, 180, size_hw)),
        ("rot270", box(cx, cy, ow, oh, 270, size_hw)),
        ("mirror", L.warp_matrix([-1, 0, cx + ow / 2.0, 0, 1, 1])),
        ("rot30", box(cx, cy, ow, oh, 30, size_hw)),
        ("rot45", box(cx, cy, ow, oh, 45, size_hw)),
        ("rot45_scale4", box(cx, cy, 4 * ow, 4 * oh, 45, size_hw)),
        ("scale2", L.warp_matrix([2, 0, 4, 0, 2, 6])),
        ("scale2.5", L.warp_matrix([2.5, 0, 1.25, 0, 2.5, 0.5])),
        ("scale0.25", box(cx, cy, ow / 4.0, oh / 4.0, 10, size_hw)),
        ("left", L.warp_matrix([1, 0, -ow / 2.0, 0, 1, 4])),
        ("right", L.warp_matrix([1, 0, fw - ow / 2.0, 0, 1, 4])),
        ("top", L.warp_matrix([1, 0, 5, 0, 1, -oh / 2.0])),
        ("bottom", L.warp_matrix([1, 0, 5, 0, 1, fh - oh / 2.0])),
        ("outside", L.warp_matrix([1, 0, fw + 40, 0, 1, 3])),
        ("fill_row", box(cx, fh - 1.0, ow, oh, 30, size_hw)),
    ]


def regions(frame_wh, size_hw, n_frames):
    """[(frame index, m)]: the matrices dealt over all frames out of their order (a stride of 4), several regions on one frame"""
    return [((4 * i + 1) % n_frames, m) for i, (_, m) in enumerate(matrices(frame_wh, size_hw))]


def frame_wh(name):
    return STREAMS[name][4]


def assert_record_facts(frame_wh, name, m, size_hw):
    """What k_warp stands on, asserted for every piece of every tile of one record at one out size: the staged box is aligned, fits
    the stage and lies within span_bound; every tap of every sub-sample lies in it; what a lane adds to the piece's first numerator,
    relative to the stage's origin, stays below 2^28 on both axes.  Returns the largest such relative numerator's magnitude."""
    g = supersample(m)
    S = 1 << g
    worst = 0
    for t in tile_facts(frame_wh, m, size_hw):
        pw, ph = piece_size(t["level"])
        for p in t["pieces"]:
            sx0, sx1, sy0, sy1 = p["box"]
            assert p["dwords"] <= STAGE_PX and (sx1 - sx0) % 8 == 0 and sx0 % 8 == 0 and sy0 % 2 == 0 and (sy1 - sy0) % 2 == 0, (name, p)
            assert sx1 - sx0 <= span_bound(m[0], m[1], g, pw, ph, 8) and sy1 - sy0 <= span_bound(m[3], m[4], g, pw, ph, 2), (name, p)
            ox = np.arange(p["at"][0], p["at"][0] + p["size"][0], dtype=np.int64)[None, :, None, None]
            oy = np.arange(p["at"][1], p["at"][1] + p["size"][1], dtype=np.int64)[:, None, None, None]
            i = np.arange(S, dtype=np.int64)[None, None, None, :]
            j = np.arange(S, dtype=np.int64)[None, None, :, None]
            nx, ny = numerator(m[0], m[1], m[2], g, ox, oy, i, j), numerator(m[3], m[4], m[5], g, ox, oy, i, j)
            x0, y0 = q(nx, g) >> 8, q(ny, g) >> 8
            assert sx0 <= x0.min() and x0.max() + 1 < sx1 and sy0 <= y0.min() and y0.max() + 1 < sy1, (name, p)
            # what a lane adds to the piece's first numerator stays far inside 32 bits
            rel = max(int(np.abs(nx - (sx0 << (17 + g))).max()), int(np.abs(ny - (sy0 << (17 + g))).max()))
            assert rel < 1 << 28, (name, p, rel)
            worst = max(worst, rel)
    return worst


# ---- the sweep: the legal record set beyond rotation x uniform scale -----------------------------------------------------------------
# What the judgement (leon_warp.h) lets through is any matrix whose two column norms are at most lim_g = 2^(16 + g) + 1 and any
# offset up to 2^29: shear, anisotropic scale, rank 1 and rank 0, records on the thresholds between two g, footprints 21 groups of 8
# columns wide or 81 row pairs high, footprints of more than 256 staging slots at every width.  sweep() names those families and adds seeded random records; tests/test_warp_sweep_structure.py
# proves on the CPU what they hold, tests/test_pipeline_warp_sweep_gpu.py runs them through the kernels.
LIM = [(1 << (16 + g)) + 1 for g in range(3)]
INT32_MIN = -(1 << 31)
SWEEP_SEED = 950
N_RANDOM = 48
# staged width in groups -> (r0, degrees of column 0, degrees of column 1) of the walk_* records: found by a search over whole degrees
# for footprints of that width with more than 256 slots; tests/test_warp_sweep_structure.py asserts that they are
WALKS = {4: (1, 80, 86), 5: (1, 90, 0), 6: (1, 56, 78), 7: (1, 40, 86), 8: (1, 32, 84), 9: (1, 24, 74), 10: (1, 18, 66), 11: (1, 18, 54),
         12: (1, 20, 40), 13: (0.8, 18, 82), 14: (0.8, 4, 88), 15: (0.9, 10, 90), 16: (0.9, 0, 84), 17: (1, 0, 86), 18: (1, 0, 70),
         19: (1, 0, 54), 20: (1, 0, 48), 21: (1, 4, 26)}


def polar(lim, r, deg):
    """(x, y) words of a column of norm r * lim at deg degrees, truncated towards zero: the norm never grows"""
    return int(lim * r * math.cos(math.radians(deg))), int(lim * r * math.sin(math.radians(deg)))


def placed(A, centre, size_hw):
    """the record of A = (a00, a01, a10, a11), integers in Q16, that maps the out size's middle to `centre` (frame pixels): t = centre
    - A (ow / 2, oh / 2), clipped to the legal offsets"""
    oh, ow = size_hw
    a00, a01, a10, a11 = A
    tx = int(math.floor(centre[0] * 65536 + 0.5)) - (a00 * ow + a01 * oh) // 2
    ty = int(math.floor(centre[1] * 65536 + 0.5)) - (a10 * ow + a11 * oh) // 2
    return (a00, a01, max(-MAX_OFFSET, min(MAX_OFFSET, tx)), a10, a11, max(-MAX_OFFSET, min(MAX_OFFSET, ty)))


def isqrt(n):
    r = int(math.sqrt(n))
    while r * r > n:
        r -= 1
    while (r + 1) * (r + 1) <= n:
        r += 1
    return r


def thresholds():
    """[(name, A, g)]: matrices on and one word above the thresholds of warp_supersample; g None: refused (LEON_REGION_SCALE).  Column
    norm exactly lim_g gives g; one word more in the diagonal or in the off-diagonal entry gives g + 1.  The 45 degree pair: column
    (c, d) with c = floor(lim / sqrt 2) and d the largest word with c^2 + d^2 <= lim^2, and (c, d + 1), the smallest above."""
    out = []
    for g, lim in enumerate(LIM):
        up = g + 1 if g < 2 else None
        c = isqrt(lim * lim // 2)
        d = isqrt(lim * lim - c * c)
        out += [("thr%d_at" % g, (lim, 0, 0, lim), g), ("thr%d_diag+1" % g, (lim + 1, 0, 0, lim), up), ("thr%d_off+1" % g, (lim, 0, 1, lim), up),
                ("thr%d_45_at" % g, (c, -d, d, c), g), ("thr%d_45+1" % g, (c, -(d + 1), d + 1, c), up)]
    return out


def sweep(frame_wh, size_hw):
    """[(name, m)] for one stream and out size, deterministic: the named families, placed by the frame's and the out size, and
    N_RANDOM seeded records.  Every record is legal (status 0)."""
    fw, fh = frame_wh
    oh, ow = size_hw
    cx, cy = fw / 2.0, fh / 2.0
    box = L.warp_matrix_rotated_box
    # where the named matrices put the out size's middle, in turn: the frame's centre and a point on each of its edges, so that the
    # smallest out size meets the frame's edges as well
    spots = [(cx, cy), (0.0, cy + 3.3), (cx + 4.7, float(fh)), (float(fw), cy - 2.6), (cx - 5.2, 0.0)]
    named = []
    for g, lim in enumerate(LIM):
        S = 1 << g
        # shear, both columns at their norm limit: x takes a share of v (horizontal), y takes a share of u (vertical)
        named.append(("shear_h_S%d" % S, (lim, polar(lim, 1, 60)[0], 0, polar(lim, 1, 60)[1])))
        named.append(("shear_v_S%d" % S, (polar(lim, 1, 30)[0], 0, polar(lim, 1, 30)[1], lim)))
    c30, s30 = polar(LIM[0], 1, 30)
    C30, S30 = polar(LIM[2], 1, 30)
    h30, k30 = polar(LIM[2], 0.5, 30)
    r30, r45 = polar(1 << 17, 1, 30), polar(1 << 17, 1, 45)
    named += [
        # anisotropic scale: S = 4 along an axis that is enlarged; the widest and the tallest level-0 footprints
        ("aniso_4_quarter", (4 << 16, 0, 0, 1 << 14)), ("aniso_quarter_4", (1 << 14, 0, 0, 4 << 16)),
        ("widest", (LIM[2], LIM[2], 0, 0)), ("tallest", (0, 0, LIM[2], LIM[2])),
        # rank 1: parallel columns at 30 degrees, equal at S = 1, opposite and unequal at S = 4
        ("rank1_S1", (c30, c30, s30, s30)), ("rank1_S4", (C30, -h30, S30, -k30)),
        # a reflection combined with a rotation (det < 0) at S = 2: 2 R(angle) diag(1, -1)
        ("reflect30_S2", (r30[0], r30[1], r30[1], -r30[0])), ("reflect45_S2", (r45[0], r45[1], r45[1], -r45[0])),
    ]
    named += [(n, A) for n, A, g in thresholds() if g is not None]
    out = [(n, placed(A, spots[k % len(spots)], size_hw)) for k, (n, A) in enumerate(named)]
    # stage (1)'s index walk: a lane stages one (row pair, group of 8 columns) slot a pass, so a piece of more than 256 slots sends
    # its lanes through `pair += pair_step; col += col_step` and the wrap at `col >= sw8`.  One record per staged width 4 .. 21 whose
    # pieces at a full tile have that width and more than 256 slots, placed in turn as above: columns r0 * lim_2 at t0 and lim_2 at t1
    for w, (r0, t0, t1) in sorted(WALKS.items()):
        c0, c1 = polar(LIM[2], r0, t0), polar(LIM[2], 1, t1)
        out.append(("walk_%d" % w, placed((c0[0], c1[0], c0[1], c1[1]), spots[w % len(spots)], size_hw)))
    out += [
        # rank 0: every pixel samples (tx, ty) -- a fractional position inside the frame, the frame's corner (half frame, half pad on
        # both axes), outside
        ("rank0_inside", (0, 0, int((cx + 0.3) * 65536), 0, 0, int((cy - 1.3) * 65536))),
        ("rank0_corner", (0, 0, fw << 16, 0, 0, fh << 16)),
        ("rank0_outside", (0, 0, (fw + 40) << 16, 0, 0, -(30 << 16))),
    ]
    # 45 degrees about each of the frame's corners at S = 2 and S = 4: pieces cut by two frame edges at once
    for S in (2, 4):
        for cname, (px, py) in (("tl", (0, 0)), ("tr", (fw, 0)), ("bl", (0, fh)), ("br", (fw, fh))):
            out.append(("corner_%s_S%d" % (cname, S), box(px, py, S * ow, S * oh, 45, size_hw)))
    # a box centred on the last row (the fill row of an odd height) at S = 4
    out.append(("fill_row_S4", box(cx, fh - 1.0, 4 * ow, 4 * oh, 10, size_hw)))
    one = 1 << 16
    out += [
        # the offset limits: 8192 pixels away, all pad
        ("tx+limit", (one, 0, MAX_OFFSET, 0, one, 2 * one)), ("tx-limit", (one, 0, -MAX_OFFSET, 0, one, 2 * one)),
        ("ty+limit", (one, 0, 3 * one, 0, one, MAX_OFFSET)), ("ty-limit", (one, 0, 3 * one, 0, one, -MAX_OFFSET)),
        # X = 4.00002 u - 8192 comes back to the frame at u = 2048: no out size of SIZES reaches that far, the region is all pad
        ("tx-limit_lim2", (LIM[2], 0, -MAX_OFFSET, 0, LIM[2], int(cy * 65536))),
        # exactly one source column inside the frame, the last one, at fraction 0.3 (output column 0); exactly one source row inside,
        # the first one, at fraction 0.7 (the last output row)
        ("one_column", (one, 0, (fw - 1) * one + 19661, 0, one, 3 * one)),
        ("one_row", (one, 0, 5 * one, 0, one, -(oh - 1) * one - 19661)),
    ]
    rng = np.random.default_rng([SWEEP_SEED, fw, fh, oh, ow])
    for k in range(N_RANDOM):
        g = int(rng.integers(0, 3))
        cols = []
        for _ in range(2):
            r = 1.0 if rng.integers(0, 2) else float(rng.uniform(0.0, 1.0))
            cols.append(polar(LIM[g], r, float(rng.uniform(0.0, 360.0))))
        where = int(rng.integers(0, 4))
        u, v = float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.0, 1.0))
        if where == 0:
            centre = (cx, cy)
        elif where == 1:          # a point on one of the four edges
            centre = [(0.0, v * fh), (float(fw), v * fh), (u * fw, 0.0), (u * fw, float(fh))][int(rng.integers(0, 4))]
        elif where == 2:
            centre = [(0.0, 0.0), (float(fw), 0.0), (0.0, float(fh)), (float(fw), float(fh))][int(rng.integers(0, 4))]
        else:                     # anywhere up to 20 pixels around the frame
            centre = (-20.0 + u * (fw + 40), -20.0 + v * (fh + 40))
        m = placed((cols[0][0], cols[1][0], cols[0][1], cols[1][1]), centre, size_hw)
        out.append(("random%02d_S%d" % (k, 1 << supersample(m)), m))          # (S of the record: two short columns fall below the drawn g)
    return out


def sweep_regions(frame_wh, size_hw, n_frames):
    """[(frame index, m)]: the sweep dealt over all frames out of their order, as regions() deals the matrices"""
    return [((4 * i + 1) % n_frames, m) for i, (_, m) in enumerate(sweep(frame_wh, size_hw))]


def sweep_refused(n_frames):
    """[(name, (frame, m, reserved), status word)]: the threshold records on the refused side.  INT32_MIN in a matrix word is a column
    norm of 2^31 (SCALE), in an offset word it has no negative (OFFSET): warp_record_status judges the scale first."""
    one = 1 << 16
    ident = (one, 0, 0, 0, one, 0)
    out = [
        ("thr2_diag+1", (0, (LIM[2] + 1, 0, 5 * one, 0, LIM[2], 4 * one), 0), L.REGION_SCALE),
        ("thr2_off+1", (1 % n_frames, (LIM[2], 0, 5 * one, 1, LIM[2], 4 * one), 0), L.REGION_SCALE),
        ("tx+limit+1", (2 % n_frames, (one, 0, MAX_OFFSET + 1, 0, one, 0), 0), L.REGION_OFFSET),
        ("ty-limit-1", (3 % n_frames, (one, 0, 0, 0, one, -MAX_OFFSET - 1), 0), L.REGION_OFFSET),
    ]
    for k in range(6):
        m = tuple(INT32_MIN if i == k else v for i, v in enumerate(ident))
        out.append(("int32_min_word%d" % k, ((4 + k) % n_frames, m, 0), L.REGION_OFFSET if k in (2, 5) else L.REGION_SCALE))
    return out


# what a bad record is refused for: (name, (frame, m, reserved), status word, the words of the host call's message)
def refused_records(n_frames):
    ident = L.warp_matrix([1, 0, 0, 0, 1, 0])
    return [
        ("scale5", (0, L.warp_matrix([5, 0, 0, 0, 1, 0]), 0), L.REGION_SCALE, "reduces by more than 4"),
        ("frame", (n_frames, ident, 0), L.REGION_FRAME, "frame %d is outside" % n_frames),
        ("reserved", (1, ident, 7), L.REGION_RESERVED, "reserved word is 7"),
        ("offset", (2, (65536, 0, (1 << 29) + 1, 0, 65536, 0), 0), L.REGION_OFFSET, "offset"),
    ]
