"""The structure of k_warp (csrc/leon_kernels.h) and of the judgement it shares with the host (csrc/leon_warp.h), stated on the CPU:
how a record's supersampling follows from its matrix, into which pieces a 32 x 8 tile is cut, and which source footprint a piece
stages -- the bounding box of its four corner samples and their bilinear neighbours, aligned to 8 columns and even rows.  The
expressions are the kernel's, line for line; nothing here touches a device.

CALLS is the list tests/test_warp_structure.py (the facts), tests/test_pipeline_warp_gpu.py, tests/test_pipeline_warp_device_gpu.py
and tests/test_pipeline_warp_node_gpu.py (the kernels) share: per stream of resample_structure.STREAMS the out sizes and, for every
size, the named matrices.  A helper, not a test module."""
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


# what a bad record is refused for: (name, (frame, m, reserved), status word, the words of the host call's message)
def refused_records(n_frames):
    ident = L.warp_matrix([1, 0, 0, 0, 1, 0])
    return [
        ("scale5", (0, L.warp_matrix([5, 0, 0, 0, 1, 0]), 0), L.REGION_SCALE, "reduces by more than 4"),
        ("frame", (n_frames, ident, 0), L.REGION_FRAME, "frame %d is outside" % n_frames),
        ("reserved", (1, ident, 7), L.REGION_RESERVED, "reserved word is 7"),
        ("offset", (2, (65536, 0, (1 << 29) + 1, 0, 65536, 0), 0), L.REGION_OFFSET, "offset"),
    ]
