"""CPU: the definition of leon_pipeline_field_tensors (include/leon_pipeline.h) pinned to what the project already has, through the
library's CPU road (leon_pipeline_field_tensor_record) and the numpy text (leon_ctypes.field_tensor): a constant plane comes back as
the constant for every int16 value (the rows of the pixel road's tables sum to 2^22 within 11, far inside what the rounding absorbs); a
box resampled to its own size returns the plane's values; a plane that holds an 8-bit image gives the 8-bit values leon_ctypes.resize_rgb
gives for that box and size -- so a field tensor lines up with the pixel tensor sample for sample; and the call-level refusals, by
their message text.  No GPU."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def axes():
    """(in_size, start, size, out_size) the tables accept: every ratio class, boxes at both ends of the axis"""
    rng = np.random.default_rng(309)
    out = [(16, 0, 16, 1), (16, 0, 16, 16), (50, 0, 50, 7), (38, 0, 38, 5), (128, 0, 112, 7), (4096, 0, 4096, 256), (1920, 0, 1920, 224), (1080, 0, 1080, 224), (3, 0, 3, 16)]
    while len(out) < 309:
        in_size = int(rng.integers(1, 600))
        size = int(rng.integers(1, in_size + 1))
        start = int(rng.choice([0, in_size - size, rng.integers(0, in_size - size + 1)]))
        o = int(rng.integers(max(1, -(-size // 16)), 65))
        out.append((in_size, start, size, o))
    return out


def test_a_constant_plane_comes_back_for_every_int16_value(L):
    """on the tables: sat16((2^21 + v * sum W) >> 22) == v for every row of 309 axes and every v"""
    v = np.arange(-32768, 32768, dtype=np.int64)
    worst = 0
    for a in axes():
        first, count, w = L.resize_weights(*a)
        for s in np.unique(w.astype(np.int64).sum(axis=1)):
            worst = max(worst, abs(int(s) - (1 << 22)))
            assert np.array_equal(np.clip((v * int(s) + (1 << 21)) >> 22, -32768, 32767), v), (a, int(s))
    assert worst <= 11


def test_a_constant_plane_through_the_library(L):
    values = [-32768, -32767, -12345, -256, -1, 0, 1, 255, 256, 4097, 32766, 32767]
    fw, fh = 50, 38
    c = [L.field_channel(0, 16, 1, 2, 1.0, 0.0)]          # cells of 4 pixels, rows of 13 cells in a stride of 16
    nbytes = 2 * (((fh - 1) >> 2) * 16 + ((fw - 1) >> 2)) + 2
    items = np.stack([np.full(nbytes // 2, x, dtype=np.int16).view(np.uint8) for x in values])
    for i, x in enumerate(values):
        for box, size in (((0, 0, fw, fh), (5, 7)), ((3, 5, 40, 30), (2, 3)), ((47, 35, 3, 3), (16, 16))):
            st, t = L.field_tensor_record(fw, fh, 64, 48, items, (i,) + box, size, c, dtype="float32")
            assert st == 0 and (t == np.float32(x)).all(), (x, box, size)
            assert (L.field_tensor(items[i].view(np.int16), fw, fh, box, size, c, "float32") == np.float32(x)).all()


def test_a_box_at_its_own_size_returns_the_plane(L):
    rng = np.random.default_rng(5)
    fw, fh = 50, 38
    plane = rng.integers(-32768, 32768, size=(fh, 64), dtype=np.int64).astype(np.int16)
    items = plane.reshape(1, -1).view(np.uint8)
    c = [L.field_channel(0, 64, 1, 0, 1.0, 0.0)]
    for x, y, w, h in ((0, 0, fw, fh), (7, 3, 20, 11), (49, 37, 1, 1), (0, 30, 50, 8)):
        st, t = L.field_tensor_record(fw, fh, 64, 48, items, (0, x, y, w, h), (h, w), c, dtype="float32")
        assert st == 0 and np.array_equal(t[0], plane[y:y + h, x:x + w].astype(np.float32))
        assert np.array_equal(L.field_resample(plane.reshape(-1), fw, fh, (x, y, w, h), (h, w), c[0]), plane[y:y + h, x:x + w])


@pytest.mark.parametrize("box,size", [((0, 0, 50, 38), (5, 7)), ((0, 0, 50, 38), (38, 50)), ((10, 4, 33, 31), (9, 33)), ((47, 35, 3, 3), (16, 16)), ((1, 1, 48, 32), (2, 3)),
                                      ((0, 0, 50, 38), (64, 64))])
def test_a_plane_holding_an_image_gives_the_pixel_roads_values(L, box, size):
    rng = np.random.default_rng(11)
    fw, fh = 50, 38
    rgb = rng.integers(0, 256, size=(fh, fw, 3), dtype=np.uint8)
    rgb[:4, :4] = 255
    rgb[-4:, -4:] = 0
    items = np.ascontiguousarray(rgb.transpose(2, 0, 1)).astype(np.int16).reshape(1, -1).view(np.uint8)
    c = [L.field_channel(2 * k * fw * fh, fw, 1, 0, 1.0, 0.0) for k in range(3)]
    want = L.resize_rgb(rgb, box, size).transpose(2, 0, 1).astype(np.float32)
    st, t = L.field_tensor_record(fw, fh, 64, 48, items, (0,) + box, size, c, dtype="float32")
    assert st == 0 and np.array_equal(t, want)
    assert np.array_equal(L.field_tensor(items[0].view(np.int16), fw, fh, box, size, c, "float32"), want)


REFUSALS = [
    (dict(channel0=dict(scale=float("inf"))), "not finite"),
    (dict(channel0=dict(bias=float("nan"))), "not finite"),
    (dict(channel1=dict(scale=2.0)), "channel 1: scale 2, bias 0: 32768 * |scale| + |bias| is not finite in the element type"),
    (dict(channel0=dict(scale=1.0, bias=32768.0)), "is not finite in the element type"),
    (dict(channels=0), "0 channels (1 .. 8)"),
    (dict(channels=9), "9 channels (1 .. 8)"),
    (dict(channel0=dict(shift=5)), "channel 0: shift 5 (0 .. 4)"),
    (dict(channel0=dict(shift=-1)), "channel 0: shift -1 (0 .. 4)"),
    (dict(channel1=dict(elem_stride=0)), "channel 1: elem_stride 0 (1 .. 4)"),
    (dict(channel1=dict(elem_stride=5)), "channel 1: elem_stride 5 (1 .. 4)"),
    (dict(channel0=dict(row_stride=-1)), "channel 0: row_stride -1 is negative"),
    (dict(channel0=dict(offset_bytes=1)), "channel 0: offset_bytes 1 is not a multiple of 2"),
    (dict(out_width=0), "out_width 0 is outside 1 .. 4096"),
    (dict(out_height=4097), "out_height 4097 is outside 1 .. 4096"),
    (dict(filter=3), "filter 3 (LEON_RESIZE_TRIANGLE is the filter)"),
    (dict(dtype=8), "dtype 8 (LEON_TENSOR_F16, _BF16, _F32)"),
    (dict(dtype=0), "dtype 0 (LEON_TENSOR_F16, _BF16, _F32)"),
    (dict(source=3), "source 3 (LEON_FIELD_SOURCE_BUFFER, _MOTION, _RESIDUAL: 0 .. 2)"),
    (dict(reserved=1), "the reserved word of cfg is not 0"),
    (dict(channel1=dict(reserved=(0, 1))), "channel 1: a reserved word is not 0"),
    (dict(channel1=dict(offset_bytes=30)), "channel 1: its last element ends at byte 4866 of an item of 4864 bytes"),
    (dict(channel0=dict(row_stride=65)), "channel 0: its last element ends at byte"),
    (dict(source_bytes=2 * 4864 - 1), "source_bytes 9727 is below 2 items of 4864 bytes"),
    (dict(n_items=0), "0 items (1 .. 65535)"),
    (dict(item_pitch_bytes=4863), "item_pitch_bytes 4863 is not a multiple of 2"),
]


@pytest.mark.parametrize("over,text", REFUSALS)
def test_call_level_refusals_by_text(L, over, text):
    fw, fh = 50, 38
    # two luma-sized planes that fill the item to its last byte: 38 rows of 64, the second plane's last row cut at the frame's width
    channels = [L.field_channel(0, 64, 1, 0, 1.0, 0.0), L.field_channel(4864 - (2 * (37 * 64 + 49) + 2), 64, 1, 0, 1.0, 0.0)]
    items = np.zeros((2, 4864), dtype=np.uint8)
    st, t = L.field_tensor_record(fw, fh, 64, 48, items, (1, 0, 0, fw, fh), (5, 7), channels, fill=0xA5)
    assert st == 0
    with pytest.raises(L.LeonError) as e:
        L.field_tensor_record(fw, fh, 64, 48, items, (1, 0, 0, fw, fh), (5, 7), channels, fill=0xA5, over=over)
    assert text in str(e.value), str(e.value)


def test_refusals_of_the_sizes_and_pointers(L):
    channels = [L.field_channel(0, 64, 1, 0, 1.0, 0.0)]
    items = np.zeros((1, 2 * 64 * 48), dtype=np.uint8)
    for args, text in (((0, 38, 64, 48), "a frame of 0 x 38"), ((50, 4097, 64, 48), "a frame of 50 x 4097")):
        with pytest.raises(L.LeonError) as e:
            L.field_tensor_record(*args, items, (0, 0, 0, 1, 1), (1, 1), channels)
        assert text in str(e.value)
    # a record source asks for a coded size its layout accepts, and items no smaller than its records
    with pytest.raises(L.LeonError) as e:
        L.field_tensor_record(50, 38, 60, 48, items, (0, 0, 0, 1, 1), (1, 1), L.field_channels_motion(4), source="motion")
    assert "a coded size of 60 x 48" in str(e.value)
    with pytest.raises(L.LeonError) as e:
        L.field_tensor_record(50, 38, 64, 48, np.ascontiguousarray(items[:, :256]), (0, 0, 0, 1, 1), (1, 1), L.field_channels_motion(4), source="motion")
    assert "item_pitch_bytes 256 is below the record's" in str(e.value)
    # a channel that leaves a record: the fifth word of a macroblock's four
    rl = L.motion_layout(4, 3)
    rec = np.zeros((1, rl.record_pitch), dtype=np.uint8)
    with pytest.raises(L.LeonError) as e:
        L.field_tensor_record(50, 38, 64, 48, rec, (0, 0, 0, 1, 1), (1, 1), [L.field_channel(rl.record_bytes - 2 * (2 * 16 + 3 * 4), 16, 4, 4)], source="motion")
    assert "its last element ends at byte" in str(e.value)
    lib = L.load()
    cfg = L._field_config("buffer", "float16", (1, 1), channels, 1, items.shape[1], items.size)
    r = L._records_array([(0, 0, 0, 1, 1)])
    out = np.zeros(4, dtype=np.uint8)
    for bad in ((None, items.ctypes.data, r.ctypes.data, out.ctypes.data), (cfg, None, r.ctypes.data, out.ctypes.data), (cfg, items.ctypes.data, None, out.ctypes.data),
                (cfg, items.ctypes.data, r.ctypes.data, None), (cfg, items.ctypes.data + 1, r.ctypes.data, out.ctypes.data), (cfg, items.ctypes.data, r.ctypes.data, out.ctypes.data + 1)):
        assert lib.leon_pipeline_field_tensor_record(50, 38, 64, 48, bad[0], bad[1], bad[2], bad[3]) == L.ERR_INVALID
