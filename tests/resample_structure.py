"""The structure of resample_body (csrc/leon_kernels.h) and plan_resize (csrc/leon_pipeline_impl.h), stated on the CPU: what a 32 x 8
tile derives from the tables of leon_ctypes.resize_weights -- staged footprint, chunks, seams, the fill row -- and what the packed store
of k_resample makes of a tile row: its start class, its bytes, the 16-byte lines that leave as one b128 store and
those that leave element by element.  The expressions are the kernel's, line for line; nothing here touches a device.

CASES is the list of geometries tests/test_resample_structure.py (the facts) and tests/test_resample_structure_gpu.py (the kernels) share:
each names one of three small streams, a crop, an output size and the filters, and carries the fact it exists for as a predicate
over tile_facts / store_facts.  A helper, not a test module."""
import functools

import leon_ctypes as L

TILE_X, TILE_Y, BLOCK, STAGE_PX = 32, 8, 256, 4096          # kResTileX, kResTileY, kRgbaBlock, kResStagePx
TRIANGLE, BICUBIC = L.RESIZE_TRIANGLE, L.RESIZE_BICUBIC
FILTER_NAMES = {TRIANGLE: "triangle", BICUBIC: "bicubic"}

# name: (coded width, coded height, GOPs, seed, (frame width, frame height)) for test_pipeline_gpu.ibbp_stream.  96 x 64: the plain
# frame.  608 x 57: the fused road, an odd height (the fill row of 255), ratio 16 across two tiles.  100 x 57: the unfused road, a
# width that is no multiple of 8, an odd height.  Two GOPs of unequal length each, 3 and 6 pictures: in one window their frame_ids
# skip ring positions.  synth.gop_ibbp writes no GOP shorter than 3 (I B B), and one of 4 or 5 ends in a P picture of display index 5,
# past the longest GOP of the stream, which the pipeline refuses ("temporal reference 5 outside the GOP"): 3 and 6 is the smallest
# unequal pair of whole GOPs (tests/test_resample_structure.py test_streams_are_whole_gops).
STREAMS = {
    "96x64": (96, 64, [3, 6], 9664, (96, 64)),
    "608x57": (608, 64, [3, 6], 60857, (608, 57)),
    "100x57": (112, 64, [3, 6], 10057, (100, 57)),
}
# (element bytes, layout) of the packed store: k_resample<1, chw>, <1, hwc>, <2, hwc>, <4, hwc>, either filter
PACKED = [(1, "chw"), (1, "hwc"), (2, "hwc"), (4, "hwc")]


def resample_col(c):
    return c + (c >> 4)


@functools.lru_cache(maxsize=None)
def weights(in_size, crop_start, crop_size, out_size, filter):
    return L.resize_weights(in_size, crop_start, crop_size, out_size, filter)


def axis_facts(in_size, crop_start, crop_size, out_size, filter):
    """per output sample of one axis: is its window cut by the axis' ends (the definition's lo < 0, hi > in_size), does it leave the crop"""
    first, count, _ = weights(in_size, crop_start, crop_size, out_size, filter)
    scale = float(crop_size) / float(out_size)
    support = (2.0 if filter == BICUBIC else 1.0) * max(scale, 1.0)
    centers = [crop_start + (o + 0.5) * scale for o in range(out_size)]
    end = first + count
    return dict(
        clipped_lo=any(int(c - support + 0.5) < 0 for c in centers), clipped_hi=any(int(c + support + 0.5) > in_size for c in centers),
        leaves_lo=bool((first < crop_start).any()), leaves_hi=bool((end > crop_start + crop_size).any()),
        max_taps=int(count.max()), min_taps=int(count.min()))


def tile_facts(frame_wh, crop, size_hw, filter):
    """[{...}] per 32 x 8 tile, in blockIdx order (y outer): the values resample_body computes before and inside its chunk loop"""
    fw, fh = frame_wh
    x, y, w, h = crop or (0, 0, fw, fh)
    oh, ow = size_hw
    first_x, count_x, wx = weights(fw, x, w, ow, filter)
    first_y, count_y, wy = weights(fh, y, h, oh, filter)
    tiles = []
    for oy0 in range(0, oh, TILE_Y):
        for ox0 in range(0, ow, TILE_X):
            nox, noy = min(TILE_X, ow - ox0), min(TILE_Y, oh - oy0)
            cx0 = int(first_x[ox0]) & ~7
            sw = (int(first_x[ox0 + nox - 1] + count_x[ox0 + nox - 1]) - cx0 + 7) & ~7
            ry0 = int(first_y[oy0]) & ~1
            ry1 = int(first_y[oy0 + noy - 1] + count_y[oy0 + noy - 1])
            sw8 = sw >> 3
            swp = resample_col(sw)
            rc = (STAGE_PX // swp) & ~1
            pair_step = BLOCK // sw8
            chunks = []          # (first row, rows, the last row pair holds the fill row)
            for r in range(ry0, ry1, rc):
                rows = min(rc, ry1 - r)
                n_pairs = (rows + 1) >> 1
                chunks.append((r, rows, r + 2 * (n_pairs - 1) + 1 >= fh))
            # the last row of an odd height is the fill row: which of the tile's output rows tap it, and with what weight
            fill_weights = [int(wy[o, fh - 1 - first_y[o]]) for o in range(oy0, oy0 + noy) if fh & 1 and first_y[o] + count_y[o] == fh]
            tiles.append(dict(
                ox0=ox0, oy0=oy0, nox=nox, noy=noy, cx0=cx0, sw=sw, sw8=sw8, swp=swp, rc=rc, pair_step=pair_step, col_step=BLOCK - pair_step * sw8,
                ry0=ry0, ry1=ry1, n_chunks=len(chunks), last_rows=chunks[-1][1], chunks=chunks,
                x_off=int(first_x[ox0]) - cx0, y_off=int(first_y[oy0]) - ry0,
                fill_in_last_chunk=chunks[-1][2], fill_weights=fill_weights,
                taps_x=(int(count_x[ox0:ox0 + nox].min()), int(count_x[ox0:ox0 + nox].max())),
                taps_y=(int(count_y[oy0:oy0 + noy].min()), int(count_y[oy0:oy0 + noy].max()))))
    return tiles


def store_facts(size_hw, element_bytes, layout):
    """[{...}] per row of every tile as the packed store walks it (HWC: the tile's rows; uint8 CHW: 3 x the tile's rows, one per channel):
    start = g0 & 15, bytes = g1 - g0, lines = per 16-byte line "b128" (one store) or "elem" (element by element)"""
    oh, ow = size_hw
    eb, hwc = element_bytes, layout == "hwc"
    assert (eb, layout) in PACKED
    row_elems = 3 * TILE_X if hwc else TILE_X
    n_rows = TILE_Y if hwc else 3 * TILE_Y
    k_lines = (row_elems * eb + 15) // 16 + 1
    lines_p2 = 4 if k_lines <= 4 else 32
    plane = ow * oh
    rows = []
    for oy0 in range(0, oh, TILE_Y):
        for ox0 in range(0, ow, TILE_X):
            nox, noy = min(TILE_X, ow - ox0), min(TILE_Y, oh - oy0)
            for row in range(n_rows):
                if (row if hwc else row & 7) >= noy:
                    continue
                g0 = ((oy0 + row) * ow + ox0) * 3 * eb if hwc else ((row >> 3) * plane + (oy0 + (row & 7)) * ow + ox0) * eb
                g1 = g0 + nox * (3 if hwc else 1) * eb
                lines = []
                for line in range(lines_p2):
                    a0 = (g0 & ~15) + 16 * line
                    if a0 >= g0 and a0 + 16 <= g1:
                        lines.append("b128")
                    elif a0 + 16 > g0 and a0 < g1:
                        lines.append("elem")
                assert (len(lines) - 1) * 16 < (g0 & 15) + g1 - g0 <= len(lines) * 16 and len(lines) <= k_lines          # the lines cover the row
                rows.append(dict(ox0=ox0, oy0=oy0, nox=nox, noy=noy, row=row, start=g0 & 15, end=g1 & 15, bytes=g1 - g0, lines=lines))
    return rows


def frame_wh(stream):
    return STREAMS[stream][4]


class Case:
    """stream: a key of STREAMS; crop: (x, y, w, h) or None; size: (out_h, out_w); kind: "staging" or "store"; fact: what the case is
    here for, a predicate fact(case, filter) over tile_facts / store_facts that must hold for every filter of the case"""
    def __init__(self, name, stream, crop, size, kind, why, fact, filters=(TRIANGLE, BICUBIC)):
        self.name, self.stream, self.crop, self.size, self.kind, self.why, self.fact, self.filters = name, stream, crop, size, kind, why, fact, filters

    @property
    def frame(self):
        return frame_wh(self.stream)

    @property
    def box(self):
        return self.crop or (0, 0) + self.frame

    def tiles(self, filter):
        return tile_facts(self.frame, self.crop, self.size, filter)

    def axes(self, filter):
        """(x axis facts, y axis facts)"""
        (fw, fh), (x, y, w, h) = self.frame, self.box
        return axis_facts(fw, x, w, self.size[1], filter), axis_facts(fh, y, h, self.size[0], filter)

    def store(self, element_bytes, layout):
        return store_facts(self.size, element_bytes, layout)

    def holds(self):
        return all(self.fact(self, f) for f in self.filters)

    def __repr__(self):
        return self.name


def any_tile(pred):
    return lambda c, f: any(pred(t) for t in c.tiles(f))


def every_tile(pred):
    return lambda c, f: all(pred(t) for t in c.tiles(f))


def both(*facts):
    return lambda c, f: all(fact(c, f) for fact in facts)


def every_packed(pred):
    """pred(rows of store_facts, element bytes) for each of the four packed kernels"""
    return lambda c, f: all(pred(c.store(eb, layout), eb) for eb, layout in PACKED)


def all_start_classes(rows, eb):
    return {r["start"] for r in rows} == set(range(0, 16, eb))


def short_rows_share_a_line(rows, eb):
    """rows shorter than a line with no b128 store, two of which lie in one 16-byte line"""
    short = [r for r in rows if r["bytes"] < 16 and "b128" not in r["lines"]]
    return bool(short) and any(r["start"] > 0 and r["start"] + r["bytes"] <= 16 for r in short)


def max_sw8(f):
    return 65 if f == TRIANGLE else 67


CASES = [
    # ---- staging ---------------------------------------------------------------------------------------------------------------------
    Case("one-group-1x1-crop", "96x64", (43, 21, 1, 1), (9, 33), "staging",
         "a 1 x 1 crop enlarged: every tile stages one 8-column group (sw8 == 1, pair_step 256, col_step 0, rc 512), the last tile is one column wide",
         every_tile(lambda t: t["sw8"] == 1 and t["pair_step"] == 256 and t["col_step"] == 0 and t["rc"] == 512)),
    Case("ratio16-two-tiles", "608x57", None, (4, 38), "staging",
         "608 -> 38: ratio 16 across two tiles, the widest footprint of the filter, 6 rows a chunk, 10 chunks, an odd last chunk of 3 rows with the fill row",
         lambda c, f: (c.tiles(f)[0]["sw8"] >= max_sw8(f) and (f != TRIANGLE or c.tiles(f)[0]["sw8"] == 65) and c.tiles(f)[0]["rc"] == 6
                       and c.tiles(f)[0]["n_chunks"] >= 3 and c.tiles(f)[0]["last_rows"] == 3 and c.tiles(f)[0]["fill_in_last_chunk"]
                       and 256 % c.tiles(f)[0]["sw8"] != 0 and c.tiles(f)[1]["nox"] == 6)),
    Case("one-pixel-ratio16", "96x64", (37, 22, 16, 16), (1, 1), "staging",
         "a 16 x 16 crop -> 1 x 1: ratio 16 on both axes, one lane of the tile valid, the taps leave the crop on all four sides",
         lambda c, f: (c.tiles(f)[0]["nox"] == 1 and c.tiles(f)[0]["noy"] == 1 and all(a["leaves_lo"] and a["leaves_hi"] for a in c.axes(f))
                       and c.tiles(f)[0]["taps_x"][1] >= (32 if f == TRIANGLE else 64))),
    Case("fill-row-starts-a-chunk", "608x57", (45, 13, 548, 44), (6, 39), "staging",
         "the chunk boundary falls on the fill row: the last chunk is the 255 row alone, its partner row of h is the spare row",
         any_tile(lambda t: t["last_rows"] == 1 and t["chunks"][-1][0] == 56 and t["fill_in_last_chunk"] and t["n_chunks"] >= 3)),
    Case("last-chunk-of-one-row", "608x57", (168, 5, 386, 40), (12, 60), "staging",
         "a last chunk of exactly one source row that is not the fill row: its partner row of h goes to the spare row",
         any_tile(lambda t: t["last_rows"] == 1 and t["n_chunks"] >= 2 and not t["fill_in_last_chunk"])),
    Case("seams-x7-y1", "100x57", (32, 30, 48, 5), (27, 63), "staging",
         "tiles whose first tap is 7 columns behind the staged group's start and 1 row behind the row pair's; nox 31, noy 3; taps leave the crop on all sides",
         lambda c, f: (any(t["x_off"] == 7 for t in c.tiles(f)) and any(t["y_off"] == 1 for t in c.tiles(f)) and any(t["nox"] == 31 for t in c.tiles(f))
                       and all(a["leaves_lo"] and a["leaves_hi"] for a in c.axes(f)))),
    Case("seams-x0-y0-clipped", "100x57", None, (15, 33), "staging",
         "the whole frame reduced: taps clipped by the frame on all four sides, the fill row tapped (bicubic: under a negative weight), offsets 0, nox 1, noy 7",
         lambda c, f: (all(a["clipped_lo"] and a["clipped_hi"] for a in c.axes(f)) and any(t["x_off"] == 0 and t["y_off"] == 0 for t in c.tiles(f))
                       and any(t["nox"] == 1 for t in c.tiles(f)) and any(t["noy"] == 7 for t in c.tiles(f))
                       and any(t["fill_in_last_chunk"] and t["fill_weights"] for t in c.tiles(f))
                       and (f != BICUBIC or any(w < 0 for t in c.tiles(f) for w in t["fill_weights"])))),
    Case("two-times", "96x64", (8, 6, 40, 28), (56, 80), "staging",
         "an exact 2x enlargement: sums on the rounding tie are common; three tiles across, seven down",
         lambda c, f: c.box[2] * 2 == c.size[1] and c.box[3] * 2 == c.size[0]),
    Case("four-times", "96x64", (50, 30, 17, 9), (36, 68), "staging",
         "an exact 4x enlargement",
         lambda c, f: c.box[2] * 4 == c.size[1] and c.box[3] * 4 == c.size[0]),
    Case("scale-one", "100x57", (9, 5, 64, 52), (52, 64), "staging",
         "scale 1 down to the fill row: one tap of 2^22 (bicubic: among zeros), a frame-size copy of the crop",
         lambda c, f: c.box[2:] == (c.size[1], c.size[0]) and c.tiles(f)[-1]["ry1"] == 57),
    Case("clamps-at-seam-and-fill-row", "100x57", (2, 20, 60, 37), (70, 90), "staging",
         "a bicubic enlargement over tile seams down to the fill row: undershoot and overshoot are clamped in both passes",
         lambda c, f: len({t["ox0"] for t in c.tiles(f)}) == 3 and c.tiles(f)[-1]["ry1"] == 57 and c.tiles(f)[-1]["fill_in_last_chunk"], filters=(BICUBIC,)),
    Case("two-chunks-odd-tail", "608x57", (100, 0, 300, 57), (16, 40), "staging",
         "a moderate reduction: a footprint whose groups do not divide 256, an odd last chunk",
         any_tile(lambda t: 256 % t["sw8"] != 0 and t["n_chunks"] >= 2 and t["last_rows"] >= 3 and t["last_rows"] & 1)),
    # ---- the packed store ------------------------------------------------------------------------------------------------------------
    Case("store-width-33", "96x64", None, (17, 33), "store",
         "an odd width: every start class of every element size; the second tile is one pixel wide (a row shorter than a line in all four kernels), noy 1",
         every_packed(lambda rows, eb: all_start_classes(rows, eb) and any(r["bytes"] < 16 for r in rows) and any(r["nox"] < 32 for r in rows)
                      and any(r["noy"] < 8 for r in rows))),
    Case("store-width-3", "96x64", (20, 10, 48, 40), (9, 3), "store",
         "rows of 3 pixels: no b128 store in the 1-byte kernels, rows that share a 16-byte line",
         lambda c, f: all(short_rows_share_a_line(c.store(eb, layout), eb) for eb, layout in PACKED[:2])),
    Case("store-width-1", "96x64", (40, 3, 16, 60), (10, 1), "store",
         "rows of one pixel (1, 3, 6 and 12 bytes): no b128 store in any kernel, rows that share a line, ratio 16 across",
         every_packed(lambda rows, eb: short_rows_share_a_line(rows, eb) and all(r["lines"] and "b128" not in r["lines"] for r in rows))),
    Case("store-width-64-aligned", "96x64", None, (9, 64), "store",
         "rows whose two ends are 16-byte aligned: b128 stores alone; a partial tile below",
         every_packed(lambda rows, eb: all(r["start"] == 0 and r["end"] == 0 and set(r["lines"]) == {"b128"} for r in rows) and any(r["noy"] < 8 for r in rows))),
    Case("store-width-45-bicubic-taps", "100x57", None, (23, 45), "store",
         "a partial tile of 13 columns and 7 rows in both store shapes, odd width, over the fill row",
         every_packed(lambda rows, eb: all_start_classes(rows, eb) and any(r["nox"] == 13 and r["noy"] == 7 for r in rows))),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
