"""The structure of k_letterbox (csrc/leon_kernels.h: resample_body with a CanvasGeom, pad_body) and of its launch (launch_tensors,
csrc/leon_pipeline_impl.h), stated on the CPU as resample_structure.py states k_resample's: per frame the pad's byte runs in memory
order and, per 16-byte line of the tensor, who stores which of its bytes and how -- an image tile with one b128 store or element by
element, a pad workgroup with one b128 store or element by element.  The expressions are the kernel's; nothing here touches a device.

CASES is the list of geometries tests/test_canvas_structure.py (the facts) and tests/test_pipeline_tensor_canvas_gpu.py (the kernels)
share: each names a stream of resample_structure.STREAMS, a crop, the image's size and place and the canvas's size, and carries the
fact it exists for as a predicate.  A helper, not a test module."""
import functools

import leon_ctypes as L
from resample_structure import BICUBIC, BLOCK, STREAMS, TILE_X, TILE_Y, TRIANGLE

PAD_LINES_PER_LANE = 4                                  # kPadLinesPerLane
PAD_LINES_PER_GROUP = PAD_LINES_PER_LANE * BLOCK        # kPadLinesPerGroup
# (element bytes, layout) of the kernels: the four with the packed image store, then float CHW (one element store per lane and channel)
PACKED = [(1, "chw"), (1, "hwc"), (2, "hwc"), (4, "hwc")]
FLOAT_CHW = [(2, "chw"), (4, "chw")]
KERNELS = PACKED + FLOAT_CHW


def rows_of(canvas_hw, element_bytes, layout):
    """the tensor as a sequence of rows in memory order: (rows, elements a row, elements of the image's rows are [3x, 3(x + ow)) or [x, x + ow))"""
    ch, cw = canvas_hw
    return (ch, 3 * cw) if layout == "hwc" else (3 * ch, cw)


def image_mask(size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """per BYTE of the tensor in memory order: True where an image element lies -- from the definition, not from the kernel"""
    import numpy as np
    (oh, ow), (x, y), (ch, cw) = size_hw, origin_xy, canvas_hw
    m = np.zeros((ch, cw, 3), dtype=bool)
    m[y:y + oh, x:x + ow] = True
    if layout == "chw":
        m = m.transpose(2, 0, 1)
    return np.repeat(m.reshape(-1), element_bytes)


def pad_runs(size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """[(first byte, end byte)] of the pad in memory order, maximal: HWC -- the rows above the image, then per image row what lies between
    one row's image end and the next row's image start, then the rows below; CHW -- the same per plane, where the end of one plane's pad
    and the start of the next one's are one run"""
    import numpy as np
    m = image_mask(size_hw, origin_xy, canvas_hw, element_bytes, layout)
    edges = np.flatnonzero(np.diff(np.concatenate([[True], m, [True]]).astype(np.int8)))
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def image_stores(size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """[(first byte, bytes, "image b128" | "image elem")] of every store of the image tiles -- resample_body's store with the canvas's
    row stride and origin.  Packed kernels: per tile row the lines of [g0, g1); float CHW: one store per lane and channel."""
    (oh, ow), (x, y), (ch, cw) = size_hw, origin_xy, canvas_hw
    eb, hwc = element_bytes, layout == "hwc"
    plane = cw * ch
    out = []
    for oy0 in range(0, oh, TILE_Y):
        for ox0 in range(0, ow, TILE_X):
            nox, noy = min(TILE_X, ow - ox0), min(TILE_Y, oh - oy0)
            if (eb, layout) in FLOAT_CHW:
                for sub in range(noy):
                    for o in range(nox):
                        at = (oy0 + sub + y) * cw + (ox0 + o + x)
                        out.extend(((c * plane + at) * eb, eb, "image elem") for c in range(3))
                continue
            row_elems = 3 * TILE_X if hwc else TILE_X
            n_rows = TILE_Y if hwc else 3 * TILE_Y
            k_lines = (row_elems * eb + 15) // 16 + 1
            lines_p2 = 4 if k_lines <= 4 else 32
            for row in range(n_rows):
                if (row if hwc else row & 7) >= noy:
                    continue
                g0 = ((oy0 + row + y) * cw + ox0 + x) * 3 * eb if hwc else ((row >> 3) * plane + (oy0 + (row & 7) + y) * cw + ox0 + x) * eb
                g1 = g0 + nox * (3 if hwc else 1) * eb
                for line in range(lines_p2):
                    a0 = (g0 & ~15) + 16 * line
                    if a0 >= g0 and a0 + 16 <= g1:
                        out.append((a0, 16, "image b128"))
                    elif a0 + 16 > g0 and a0 < g1:
                        out.extend((a, eb, "image elem") for a in range(a0, a0 + 16, eb) if g0 <= a < g1)
    return out


def pad_groups(size_hw, canvas_hw, element_bytes, gx):
    """how many workgroup ROWS launch_tensors adds behind the image's tile rows, and how many pad workgroups have lines"""
    (oh, ow), (ch, cw) = size_hw, canvas_hw
    if (ch, cw) == (oh, ow):
        return 0, 0
    lines = (3 * ch * cw * element_bytes + 15) // 16
    groups = (lines + PAD_LINES_PER_GROUP - 1) // PAD_LINES_PER_GROUP
    return (groups + gx - 1) // gx, groups


def pad_stores(size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """[(first byte, bytes, "pad b128" | "pad elem", channel of each element)] of every store of the pad workgroups: pad_body, line by line"""
    (oh, ow), (x, y), (ch, cw) = size_hw, origin_xy, canvas_hw
    eb, hwc = element_bytes, layout == "hwc"
    gx = (ow + TILE_X - 1) // TILE_X
    extra_rows, _ = pad_groups(size_hw, canvas_hw, eb, gx)
    line_elems = 16 // eb
    row_elems = 3 * cw if hwc else cw
    total = 3 * cw * ch
    ix0 = (3 if hwc else 1) * x
    ix1 = ix0 + (3 if hwc else 1) * ow
    iy0, iy1 = y, y + oh
    n_lines = (total * eb + 15) // 16
    out = []
    for group in range(extra_rows * gx):
        for step in range(PAD_LINES_PER_LANE):
            for tid in range(BLOCK):
                line = group * PAD_LINES_PER_GROUP + step * BLOCK + tid
                if line >= n_lines:
                    continue
                e0 = line * line_elems
                row, q = divmod(e0, row_elems)
                plane, yrow = (0, row) if hwc else divmod(row, ch)
                whole = e0 + line_elems <= total
                if whole and q + line_elems <= row_elems:
                    image_row = iy0 <= yrow < iy1
                    if image_row and q >= ix0 and q + line_elems <= ix1:
                        continue
                    if not image_row or q + line_elems <= ix0 or q >= ix1:
                        out.append((line * 16, 16, "pad b128", [(q + k) % 3 if hwc else plane for k in range(line_elems)]))
                        continue
                chans, skip = [], []
                qq, pl, yy = q, plane, yrow
                for k in range(line_elems):
                    inside = e0 + k < total
                    chans.append(qq % 3 if hwc else pl)
                    skip.append(not inside or (iy0 <= yy < iy1 and ix0 <= qq < ix1))
                    qq += 1
                    if qq == row_elems:
                        qq, yy = 0, yy + 1
                        if not hwc and yy == ch:
                            yy, pl = 0, pl + 1
                if not any(skip):
                    out.append((line * 16, 16, "pad b128", chans))
                else:
                    out.extend((line * 16 + k * eb, eb, "pad elem", [chans[k]]) for k in range(line_elems) if not skip[k])
    return out


@functools.lru_cache(maxsize=None)
def frame_facts(size_hw, origin_xy, canvas_hw, element_bytes, layout):
    """What one frame's launch does to its tensor: writers = per byte how many stores cover it, kinds = per 16-byte line the set of store
    kinds that touch it, runs = pad_runs, grid = (gx, image tile rows, pad workgroup rows), channel_ok = every pad element carries
    the channel the definition gives its address, pad_bytes_ok = pad stores cover pad bytes only, image stores image bytes only"""
    import numpy as np
    (oh, ow), (ch, cw) = size_hw, canvas_hw
    eb = element_bytes
    nbytes = 3 * ch * cw * eb
    mask = image_mask(size_hw, origin_xy, canvas_hw, eb, layout)
    chan = np.broadcast_to(np.arange(3), (ch, cw, 3))
    chan = np.repeat((chan if layout == "hwc" else chan.transpose(2, 0, 1)).reshape(-1), eb)
    writers = np.zeros(nbytes, dtype=np.int32)
    n_lines = (nbytes + 15) // 16
    kinds = [set() for _ in range(n_lines)]
    sides_ok, channel_ok, in_bounds = True, True, True
    for a, n, kind in image_stores(size_hw, origin_xy, canvas_hw, eb, layout):
        in_bounds &= 0 <= a and a + n <= nbytes
        writers[a:a + n] += 1
        sides_ok &= bool(mask[a:a + n].all())
        kinds[a // 16].add(kind)
    for a, n, kind, chans in pad_stores(size_hw, origin_xy, canvas_hw, eb, layout):
        in_bounds &= 0 <= a and a + n <= nbytes
        writers[a:a + n] += 1
        sides_ok &= not mask[a:a + n].any()
        channel_ok &= bool((chan[a:a + n] == np.repeat(np.asarray(chans), eb)).all())
        kinds[a // 16].add(kind)
    gx = (ow + TILE_X - 1) // TILE_X
    extra_rows, groups = pad_groups(size_hw, canvas_hw, eb, gx)
    return dict(writers=writers, kinds=kinds, runs=pad_runs(size_hw, origin_xy, canvas_hw, eb, layout), sides_ok=sides_ok, channel_ok=channel_ok,
                in_bounds=in_bounds, grid=(gx, (oh + TILE_Y - 1) // TILE_Y, extra_rows), pad_groups=groups, bytes=nbytes,
                row_bytes=(3 * cw if layout == "hwc" else cw) * eb)


class Case:
    """stream: a key of STREAMS; crop: (x, y, w, h) or None; size: the image's (h, w); origin: (x, y); canvas: (h, w); fact: a predicate
    fact(case) over frame_facts that says what the case is here for; filters: the filters the GPU test runs it with"""
    def __init__(self, name, stream, crop, size, origin, canvas, why, fact, filters=(TRIANGLE,)):
        self.name, self.stream, self.crop, self.size, self.origin, self.canvas, self.why, self.fact, self.filters = name, stream, crop, size, origin, canvas, why, fact, filters

    @property
    def frame(self):
        return STREAMS[self.stream][4]

    @property
    def box(self):
        return self.crop or (0, 0) + self.frame

    def facts(self, element_bytes, layout):
        return frame_facts(self.size, self.origin, self.canvas, element_bytes, layout)

    def holds(self):
        return bool(self.fact(self))

    def __repr__(self):
        return self.name


def run_lengths(f):
    return [b - a for a, b in f["runs"]]


def every_kernel(pred, kernels=KERNELS):
    return lambda c: all(pred(c.facts(eb, layout), eb, layout) for eb, layout in kernels)


def image_row_starts(c, eb, layout):
    """the 16-byte classes of the image rows' first bytes"""
    (oh, ow), (x, y), (ch, cw) = c.size, c.origin, c.canvas
    if layout == "hwc":
        return {(((y + r) * cw + x) * 3 * eb) & 15 for r in range(oh)}
    return {((p * ch * cw + (y + r) * cw + x) * eb) & 15 for p in range(3) for r in range(oh)}


def _letterboxed(c):
    """the case's size and origin are leon_pipeline_letterbox's for its box and canvas"""
    return L.letterbox(c.box[2], c.box[3], c.canvas[1], c.canvas[0]) == (c.size[1], c.size[0]) + tuple(c.origin)


CASES = [
    Case("letterbox", "96x64", None, (27, 40), (0, 6), (40, 40),
         "pad above and below only, full-width runs, an odd image height, two tiles across",
         lambda c: (_letterboxed(c) and c.size[1] == c.canvas[1] and c.size[0] & 1 and c.facts(1, "hwc")["grid"][0] == 2
                    and len(c.facts(1, "hwc")["runs"]) == 2 and all(n % c.facts(1, "hwc")["row_bytes"] == 0 for n in run_lengths(c.facts(1, "hwc"))))),
    Case("pillarbox", "96x64", (0, 0, 32, 64), (40, 20), (10, 0), (40, 40),
         "pad left and right only, no full-row runs",
         lambda c: (_letterboxed(c) and c.size[0] == c.canvas[0]
                    and every_kernel(lambda f, eb, layout: all(n < f["row_bytes"] for n in run_lengths(f)), [(1, "hwc"), (2, "hwc"), (4, "hwc")])(c))),
    Case("all-start-classes", "96x64", None, (17, 33), (2, 1), (19, 37),
         "the row stride is 37 and odd: image rows start in every 16-byte class of every packed kernel (16, 8 and 4 classes); the second tile is one column wide",
         lambda c: all(image_row_starts(c, eb, layout) == set(range(0, 16, eb)) for eb, layout in PACKED) and c.size[1] % TILE_X == 1,
         filters=(TRIANGLE, BICUBIC)),
    Case("one-line", "96x64", (37, 22, 16, 16), (4, 3), (5, 2), (9, 12),
         "uint8 CHW: left pad, image and right pad of a row, and parts of the next row, share one 16-byte line; no b128 store anywhere in the image rows",
         lambda c: (c.canvas[1] < 16 and any({"image elem", "pad elem"} <= k for k in c.facts(1, "chw")["kinds"])
                    and not any("image b128" in k for k in c.facts(1, "chw")["kinds"])),
         filters=(TRIANGLE, BICUBIC)),
    Case("one-element-pad", "96x64", None, (8, 32), (1, 1), (10, 34),
         "the runs between rows are two elements long and cross a row border",
         every_kernel(lambda f, eb, layout: sorted(set(run_lengths(f)[1:-1]))[0] == 2 * eb * (3 if layout == "hwc" else 1) and len(f["runs"]) >= 9)),
    Case("small-image-big-canvas", "96x64", None, (8, 8), (190, 55), (64, 200),
         "one image tile, the pad covered by pad workgroups alone (several of them), the image in the last rows and columns",
         every_kernel(lambda f, eb, layout: f["grid"][:2] == (1, 1) and f["grid"][2] == f["pad_groups"] >= 3)
         ),
    Case("canvas-equals-image", "608x57", None, (4, 38), (0, 0), (4, 38),
         "no pad workgroup at all; equals the run without a canvas, bit for bit, for both filters",
         every_kernel(lambda f, eb, layout: f["grid"][2] == 0 and not f["runs"]), filters=(TRIANGLE, BICUBIC)),
    Case("unfused-road", "100x57", None, (27, 48), (0, 2), (32, 48),
         "a width that is no multiple of 8, an odd height; the fill row of 255 is in the image, not in the pad",
         lambda c: _letterboxed(c) and c.frame[0] % 8 and c.frame[1] & 1),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
