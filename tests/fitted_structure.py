"""The structure of k_fitted (csrc/leon_kernels.h) and of its launch (resample_regions / resample_regions_device with a fit,
csrc/leon_pipeline_impl.h), stated on the CPU as canvas_structure.py states k_letterbox's: per region of a letterboxed call its image
rectangle -- the letterbox integers, restated here in pure Python -- the grid of the launch, which of its workgroups run, idle or pad
for that region, and every store of those that do.  The store expressions are the kernel's (canvas_structure.image_stores is
resample_body's with a canvas; pad_line is pad_body's); nothing here touches a device.

CALLS are the calls tests/test_fitted_structure.py (the facts, CPU), tests/test_pipeline_regions_fit_abi.py (the host's judgement) and
the GPU tests of the fit share: the three streams of resample_structure.STREAMS, one canvas each, the boxes with what each is there
for.  A helper, not a test module."""
import functools

import canvas_structure as CS
import regions_structure as RS
from resample_structure import BLOCK, TILE_X, TILE_Y

CENTRE, TOP_LEFT = "centre", "top_left"
ANCHORS = (CENTRE, TOP_LEFT)
KERNELS = CS.KERNELS          # (element bytes, layout) of the six kernels of a filter


def letterbox(sw, sh, cw, ch):
    """(ow, oh, x, y): the integers of leon_pipeline_letterbox (include/leon_pipeline.h), Python's unbounded integers"""
    if cw * sh <= ch * sw:
        ow, oh = cw, max(1, (2 * sh * cw + sw) // (2 * sw))
    else:
        oh, ow = ch, max(1, (2 * sw * ch + sh) // (2 * sh))
    return ow, oh, (cw - ow) // 2, (ch - oh) // 2


def rect(box, canvas_hw, anchor=CENTRE):
    """(X, Y, ow, oh) of a box (x, y, w, h) in a canvas (h, w): what leon_pipeline_region_fit_rect returns"""
    ow, oh, x, y = letterbox(box[2], box[3], canvas_hw[1], canvas_hw[0])
    return (0, 0, ow, oh) if anchor == TOP_LEFT else (x, y, ow, oh)


def grid(canvas_hw, element_bytes):
    """(gx, tile rows of the canvas, pad workgroup rows) of one launch: the same for every region of the call"""
    ch, cw = canvas_hw
    gx, gy = (cw + TILE_X - 1) // TILE_X, (ch + TILE_Y - 1) // TILE_Y
    lines = (3 * ch * cw * element_bytes + 15) // 16
    groups = (lines + CS.PAD_LINES_PER_GROUP - 1) // CS.PAD_LINES_PER_GROUP
    return gx, gy, (groups + gx - 1) // gx


def pad_line(line, size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """[(first byte, bytes)] of what pad_body stores of one 16-byte line of the tensor"""
    (oh, ow), (x, y), (ch, cw) = size_hw, origin_xy, canvas_hw
    eb, hwc = element_bytes, layout == "hwc"
    line_elems = 16 // eb
    row_elems = 3 * cw if hwc else cw
    total = 3 * cw * ch
    ix0 = (3 if hwc else 1) * x
    ix1 = ix0 + (3 if hwc else 1) * ow
    iy0, iy1 = y, y + oh
    e0 = line * line_elems
    row, q = divmod(e0, row_elems)
    plane, yrow = (0, row) if hwc else divmod(row, ch)
    if e0 + line_elems <= total and q + line_elems <= row_elems:
        image_row = iy0 <= yrow < iy1
        if image_row and q >= ix0 and q + line_elems <= ix1:
            return []
        if not image_row or q + line_elems <= ix0 or q >= ix1:
            return [(line * 16, 16)]
    skip = []
    qq, yy = q, yrow
    for k in range(line_elems):
        skip.append(e0 + k >= total or (iy0 <= yy < iy1 and ix0 <= qq < ix1))
        qq += 1
        if qq == row_elems:
            qq, yy = 0, yy + 1
            if not hwc and yy == ch:
                yy = 0
    if not any(skip):
        return [(line * 16, 16)]
    return [(line * 16 + k * eb, eb) for k in range(line_elems) if not skip[k]]


@functools.lru_cache(maxsize=None)
def region_facts(box_wh, canvas_hw, anchor, element_bytes, layout):
    """One region of a launch, workgroup by workgroup as k_fitted decides: blockIdx.y below the canvas's tile rows -- a tile of the
    image's own ceil(ow / 32) x ceil(oh / 8) runs resample_body, any other is idle; from there on pad_body, group (y - tile rows) * gx
    + x, lines group * 1024 + step * 256 + lane.  image_writers / pad_writers: per byte of the tensor how many image / pad stores cover
    it; idle: the idle workgroups; tiles: the image's (columns, rows); mask: per byte True where the definition has an image element"""
    import numpy as np
    X, Y, ow, oh = rect((0, 0) + box_wh, canvas_hw, anchor)
    ch, cw = canvas_hw
    eb = element_bytes
    nbytes = 3 * ch * cw * eb
    gx, gy, pad_rows = grid(canvas_hw, eb)
    tiles = ((ow + TILE_X - 1) // TILE_X, (oh + TILE_Y - 1) // TILE_Y)
    image_writers, pad_writers = np.zeros(nbytes, np.int32), np.zeros(nbytes, np.int32)
    in_bounds, idle, ran = True, [], []
    for by in range(gy):
        for bx in range(gx):
            (ran if bx * TILE_X < ow and by * TILE_Y < oh else idle).append((bx, by))
    # the tiles that run are exactly the image's, numbered from its origin: their stores are resample_body's with the region's canvas
    assert sorted(ran) == sorted((bx, by) for by in range(tiles[1]) for bx in range(tiles[0]))
    for a, n, _ in CS.image_stores((oh, ow), (X, Y), canvas_hw, eb, layout):
        in_bounds &= 0 <= a and a + n <= nbytes
        image_writers[a:a + n] += 1
    n_lines = (nbytes + 15) // 16
    for by in range(gy, gy + pad_rows):
        for bx in range(gx):
            group = (by - gy) * gx + bx
            for step in range(CS.PAD_LINES_PER_LANE):
                first = group * CS.PAD_LINES_PER_GROUP + step * BLOCK
                for line in range(first, min(first + BLOCK, n_lines)):
                    for a, n in pad_line(line, (oh, ow), (X, Y), canvas_hw, eb, layout):
                        in_bounds &= 0 <= a and a + n <= nbytes
                        pad_writers[a:a + n] += 1
    return dict(rect=(X, Y, ow, oh), grid=(gx, gy, pad_rows), tiles=tiles, idle=idle, image_writers=image_writers, pad_writers=pad_writers,
                in_bounds=in_bounds, mask=CS.image_mask((oh, ow), (X, Y), canvas_hw, eb, layout), bytes=nbytes)


class Call(RS.Call):
    """regions_structure.Call (stream, size = the canvas (h, w), boxes; regions() deals them over a window's frames) with, per box, the
    image rectangle the issue lists (w, h, X, Y), what the box is there for, and the boxes the fit refuses with their status names"""
    def __init__(self, stream, size, listed, refused=()):
        RS.Call.__init__(self, stream, size, [b for b, _, _ in listed])
        self.listed, self.refusals = listed, list(refused)


FILLS, FEWER_COLUMNS, FEWER_ROWS, ONE_COLUMN, RATIO_16 = "fills the canvas", "fewer tile columns", "fewer tile rows", "one-column image", "ratio exactly 16"
CALLS = {
    # 2 x 3 tiles, an odd row stride
    "96x64": Call("96x64", (19, 37), [
        ((0, 0, 96, 64), (29, 19, 4, 0), (FEWER_COLUMNS,)),
        ((0, 0, 74, 38), (37, 19, 0, 0), (FILLS,)),
        ((5, 3, 90, 9), (37, 4, 0, 7), (FEWER_ROWS,)),
        ((40, 0, 3, 60), (1, 19, 18, 0), (ONE_COLUMN, FEWER_COLUMNS)),
        ((95, 63, 1, 1), (19, 19, 9, 0), (FEWER_COLUMNS,)),
        ((63, 55, 33, 9), (37, 10, 0, 4), (FEWER_ROWS,)),
    ]),
    "608x57": Call("608x57", (13, 37), [
        ((0, 0, 592, 57), (37, 4, 0, 4), (RATIO_16, FEWER_ROWS)),
        ((5, 3, 37, 13), (37, 13, 0, 0), (FILLS,)),
        ((301, 20, 19, 7), (35, 13, 1, 0), ()),
        ((571, 0, 37, 57), (8, 13, 14, 0), (FEWER_COLUMNS,)),
        ((100, 0, 8, 57), (2, 13, 17, 0), (FEWER_COLUMNS,)),
    ], refused=[((0, 0, 600, 57), "REGION_RATIO_X", "REGION_RATIO_X"), ((16, 0, 592, 52), "REGION_RATIO_Y", "REGION_OK")]),          # (box, letterboxed, stretched)
    # the unfused road
    "100x57": Call("100x57", (16, 24), [
        ((0, 0, 100, 57), (24, 14, 0, 1), ()),
        ((3, 41, 49, 16), (24, 8, 0, 4), (FEWER_ROWS,)),
        ((75, 1, 25, 56), (7, 16, 8, 0), ()),
        ((50, 28, 24, 16), (24, 16, 0, 0), (FILLS,)),
        ((0, 0, 12, 8), (24, 16, 0, 0), (FILLS,)),
    ]),
}
