"""ONE list of field tensor cases (include/leon_pipeline.h, leon_pipeline_field_tensors) for the CPU definition
(tests/test_fields_cases.py: leon_pipeline_field_tensor_record) and the kernel (tests/test_fields_kernel_gpu.py:
leon_pipeline_field_tensors_kernel); the oracle is leon_ctypes.field_tensor / field_record_status, the header's text in numpy.
A case is one call: a frame inside a coded picture, items, channels, an out size, an element type and records.  Everything is compared
for equality, bytes the call is to leave alone against the sentinel."""
import numpy as np

FILL, STATUS_FILL = 0xA5, -7
SHAPES = [(16, 16, 16, 16), (50, 38, 64, 48), (128, 32, 128, 32)]          # frame width, frame height, coded width, coded height
DTYPES = ("float16", "bfloat16", "float32")
# the kernel's tile is 32 x 8 output samples and its widest store 16 bytes (8 fp16 / bf16, 4 fp32 elements): one below, at and one above
# the tile, one above the store width
TILE_SIZES = [(7, 31), (8, 32), (9, 33), (3, 9), (2, 5), (2, 17)]          # (out_height, out_width)


def channel_end(c, fw, fh):
    """bytes from the item's start to the end of channel c's last element over a frame of fw x fh (the header's expression)"""
    return c[0] + 2 * (((fh - 1) >> c[3]) * c[1] + ((fw - 1) >> c[3]) * c[2]) + 2


def planes(L, fw, fh, specs):
    """channels for specs = [(shift, scale, bias), ...] laid out one after the other in an item: a shift-4 channel is word k (its index
    among the call's channels, mod 4) of vectors interleaved 4 apart, as a motion record's; the other planes' rows are 3 elements
    longer than their cells.  Returns (channels, item_bytes): the item ends with the last element of the channel that ends last."""
    channels, at = [], 0
    for q, (shift, scale, bias) in enumerate(specs):
        cells = ((fw - 1) >> shift) + 1
        c = L.field_channel(at + 2 * (q % 4), 4 * cells, 4, 4, scale, bias) if shift == 4 else L.field_channel(at, cells + 3, 1, shift, scale, bias)
        channels.append(c)
        at = channel_end(c, fw, fh) + 6
    return channels, max(channel_end(c, fw, fh) for c in channels)


def items_random(rng, n_items, item_bytes, gap=0):
    """int16 values over the whole range; `gap` bytes behind every item hold 0x5A"""
    items = np.full((n_items, item_bytes + gap), 0x5A, dtype=np.uint8)
    items[:, :item_bytes] = rng.integers(-32768, 32768, size=(n_items, item_bytes // 2), dtype=np.int64).astype(np.int16).view(np.uint8)
    return items


def boxes_of(fw, fh, n_items):
    """the whole frame, a box at every edge, a small box inside, and what a record can be refused for, a refused one between valid ones"""
    last = n_items - 1
    recs = [(last, 0, 0, fw, fh), (0, 0, 1, max(1, fw // 3), max(1, fh - 2)), (0, 0, 0, fw, fh, 0, 0, 1), (last, fw - max(1, fw // 2), 0, max(1, fw // 2), fh),
            (0, 1, 0, max(1, fw - 2), max(1, fh // 3)), (n_items, 0, 0, fw, fh), (last, 0, fh - max(1, fh // 2), fw, max(1, fh // 2)), (-1, 0, 0, 1, 1), (0, 0, 0, 0, 4), (0, 2, 2, fw - 1, 3),
            (0, 0, 0, 3, fh + 1), (0, -1, 0, 3, 3), (last, fw - 3, fh - 3, 3, 3), (0, 0, 0, fw, fh, 7, 0, 0)]
    return recs


def cases(L):
    rng = np.random.default_rng(20261021)
    out = []

    def add(what, shape, channels, items, records, size, dtype, **kw):
        fw, fh, cw, ch = shape
        records = [tuple(r) + (0,) * (8 - len(r)) for r in records]          # (whole records: frame, the box, three reserved words)
        out.append(dict(what=what, fw=fw, fh=fh, cw=cw, ch=ch, channels=channels, items=items, records=records, size=size, dtype=dtype, source=kw.pop("source", "buffer"), **kw))

    mixed = [(0, 1.0, 0.0), (1, 0.5, -3.0), (4, 0.25, 100.0)]
    # every shape and element type: mixed shifts in one call, every kind of box and of refusal, at 7 x 5, 1 x 1 and 16 x 16
    for shape in SHAPES:
        fw, fh = shape[:2]
        channels, nbytes = planes(L, fw, fh, mixed)
        for dtype in DTYPES:
            for size in ((5, 7), (1, 1), (16, 16)):
                add("window, %dx%d %s %dx%d" % (fw, fh, dtype, size[1], size[0]), shape, channels, items_random(rng, 3, nbytes), boxes_of(fw, fh, 3), size, dtype)
    # the tile's and the store's edges
    shape = SHAPES[1]
    fw, fh = shape[:2]
    channels, nbytes = planes(L, fw, fh, mixed)
    for dtype in ("float16", "float32"):
        for size in TILE_SIZES:
            add("tile, %s %dx%d" % (dtype, size[1], size[0]), shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, fw, fh), (0, 3, 4, 3, 3), (1, fw - 20, fh - 9, 20, 9)], size, dtype)
    # a ratio of exactly 16 on each axis, and one above it
    shape = SHAPES[2]
    channels, nbytes = planes(L, 128, 32, mixed)
    add("ratio, 16 and 17", shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, 112, 16), (0, 0, 0, 113, 16), (0, 16, 16, 112, 16), (1, 0, 0, 112, 17), (0, 15, 15, 113, 17)], (1, 7),
        "float16")
    add("ratio, the whole frame at 16", shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, 128, 32)], (2, 8), "float32")
    # a 3 x 3 box enlarged to 16 x 16 at every corner
    for shape in SHAPES:
        fw, fh = shape[:2]
        channels, nbytes = planes(L, fw, fh, mixed)
        add("enlarged, %dx%d" % (fw, fh), shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, 3, 3), (0, fw - 3, 0, 3, 3), (1, 0, fh - 3, 3, 3), (0, fw - 3, fh - 3, 3, 3)],
            (16, 16), "bfloat16")
    # 1, 3 and 8 channels with different shifts in one call
    shape = SHAPES[1]
    fw, fh = shape[:2]
    for n in (1, 3, 8):
        specs = [((0, 1, 4, 4, 2, 3, 0, 4)[q], 1.0 / (1 + q), q - 2.5) for q in range(n)]
        channels, nbytes = planes(L, fw, fh, specs)
        add("channels, %d" % n, shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, fw, fh), (0, 5, 6, 30, 20)], (5, 7), "float16")
    # an odd frame under shift 1 and shift 4: the last cell lies partly outside the frame
    shape = (49, 37, 64, 48)
    channels, nbytes = planes(L, 49, 37, [(1, 1.0, 0.0), (4, 1.0, 0.0), (0, 1.0, 0.0)])
    add("odd frame", shape, channels, items_random(rng, 2, nbytes), [(1, 0, 0, 49, 37), (0, 40, 30, 9, 7), (1, 48, 36, 1, 1)], (9, 33), "float32")
    # the int16 extremes, every element type
    shape = SHAPES[1]
    fw, fh = shape[:2]
    channels, nbytes = planes(L, fw, fh, [(0, 1.0, 0.0), (1, -1.0, 0.0), (4, 0.5, 0.25)])
    for dtype in DTYPES:
        items = np.stack([np.full(nbytes // 2, v, dtype=np.int16).view(np.uint8) for v in (-32768, 32767)])
        add("extremes, %s" % dtype, shape, channels, items, [(0, 0, 0, fw, fh), (1, 0, 0, fw, fh), (0, 7, 9, 20, 11), (1, 7, 9, 20, 11)], (5, 7), dtype)
    # scale and bias that land on rounding ties: constant planes (r is the constant) of 2049 and 2051 (fp16 ties at 1 and at 0.5 times
    # them), 257 and 259 (bf16) and their like with both signs.  fp32 holds every r exactly, so there the ties are the multiply's and the
    # add's own: r * (1 + 2^-23) and r * 3 * 2^-24 + 1 with r = 12289 and 24577
    shape = SHAPES[0]
    channels, nbytes = planes(L, 16, 16, [(0, 1.0, 0.0), (0, 0.5, 0.0), (0, 1.0 + 2.0 ** -23, 0.0), (0, 0.5, 0.5), (0, -1.0, 0.0), (0, 3.0 * 2.0 ** -24, 1.0)])
    for dtype in DTYPES:
        items = np.stack([np.full(nbytes // 2, v, dtype=np.int16).view(np.uint8) for v in (2049, 2051, 257, 259, 4099, 513, -2049, -257, 12289, 24577)])
        add("ties, %s" % dtype, shape, channels, items, [(i, 0, 0, 16, 16) for i in range(10)], (2, 3), dtype)
    # the record sources' layouts: a motion record's four interleaved words, a residual record's planes
    for shape in SHAPES[:2]:
        fw, fh, cw, ch = shape
        ml, rl = L.motion_layout(cw // 16, ch // 16), L.residual_layout(cw, ch)
        recs = [(1, 0, 0, fw, fh), (0, 1, 1, fw - 1, fh - 1), (2, 0, 0, 1, 1), (1, fw - 5, fh - 4, 5, 4)]
        add("motion record, %dx%d" % (fw, fh), shape, L.field_channels_motion(cw // 16, L.MOTION_FIELDS, (0.5, 0.5, 0.25, 0.25), 0.0), items_random(rng, 2, ml.record_pitch), recs, (5, 7),
            "float16", source="motion")
        add("residual record, %dx%d" % (fw, fh), shape, L.field_channels_residual(rl, scale=1.0 / 128), items_random(rng, 2, rl.record_pitch), recs, (5, 7), "float16", source="residual")
    # bytes left alone: between items, between tensors, a refused record between valid ones, no status; a limit that makes chunks
    shape = SHAPES[1]
    fw, fh = shape[:2]
    channels, nbytes = planes(L, fw, fh, mixed)
    recs = [(2, 0, 0, fw, fh), (0, 0, 0, fw + 1, fh), (1, 3, 3, 8, 8), (0, 0, 0, 1, 1, 0, 1, 0), (2, fw - 8, fh - 8, 8, 8)]
    add("alone, a gap behind every item", shape, channels, items_random(rng, 3, nbytes, gap=6), recs, (5, 7), "float16")
    add("alone, a pitch larger than the tensor", shape, channels, items_random(rng, 3, nbytes), recs, (5, 7), "float32", pitch=768)
    add("alone, no status", shape, channels, items_random(rng, 3, nbytes), recs, (5, 7), "bfloat16", status=False)
    add("alone, chunks of two", shape, channels, items_random(rng, 3, nbytes), recs, (5, 7), "float16", scratch_limit=2 * (4 * 35 * (5 + 7) + 64))
    add("alone, one record", shape, channels, items_random(rng, 3, nbytes), recs[:1], (5, 7), "float16")
    add("alone, one refused record", shape, channels, items_random(rng, 3, nbytes), recs[1:2], (5, 7), "float16")
    return out


def region_bytes(c):
    return len(c["channels"]) * c["size"][0] * c["size"][1] * (4 if c["dtype"] == "float32" else 2)


def pitch_of(c):
    return c.get("pitch") or -(-region_bytes(c) // 256) * 256


def expected(L, c):
    """(out uint8 [n, pitch], status [n]) as the header says them: a refused record's tensor and every gap hold FILL"""
    if "_want" not in c:
        n_items = c["items"].shape[0]
        out = np.full((len(c["records"]), pitch_of(c)), FILL, dtype=np.uint8)
        status = np.zeros(len(c["records"]), dtype=np.int32)
        for i, r in enumerate(c["records"]):
            status[i] = L.field_record_status(c["fw"], c["fh"], n_items, r, c["size"])
            if status[i] == 0:
                t = L.field_tensor(c["items"][r[0]].view(np.int16), c["fw"], c["fh"], r[1:5], c["size"], c["channels"], c["dtype"])
                out[i, :region_bytes(c)] = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
        c["_want"] = (out, status)
    return c["_want"]
