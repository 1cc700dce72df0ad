"""CPU: field tensors (include/leon_pipeline.h, leon_pipeline_field_tensors) -- the structs' sizes and field offsets against the header
compiled as C, the constants, the exports, and the channel builders against the layouts they describe.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def test_struct_sizes_constants_and_symbols(L, tmp_path):
    chn, cfg, call = L.PipelineFieldChannel, L.PipelineFieldConfig, L.PipelineFieldTensorsCall
    assert C.sizeof(chn) == 32 and [getattr(chn, f).offset for f in ("offset_bytes", "row_stride", "elem_stride", "shift", "scale", "bias", "reserved")] == [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(cfg) == 304
    assert [getattr(cfg, f).offset for f in ("source", "dtype", "channels", "filter", "out_width", "out_height", "n_items", "reserved", "item_pitch_bytes", "source_bytes",
                                             "channel")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48]
    assert C.sizeof(call) == 64
    assert [getattr(call, f).offset for f in ("records", "n", "reserved0", "source", "device_out", "out_pitch_bytes", "device_status", "stream", "reserved")] == \
        [0, 8, 12, 16, 24, 32, 40, 48, 56]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", '
                   'sizeof(leon_pipeline_field_channel), sizeof(leon_pipeline_field_config), sizeof(leon_pipeline_field_tensors_call), '
                   'offsetof(leon_pipeline_field_config, channel), offsetof(leon_pipeline_field_config, source_bytes), offsetof(leon_pipeline_field_tensors_call, stream), '
                   'LEON_FIELD_SOURCE_BUFFER, LEON_FIELD_SOURCE_MOTION, LEON_FIELD_SOURCE_RESIDUAL, LEON_FIELD_MAX_CHANNELS, LEON_TENSOR_F16, LEON_TENSOR_BF16, LEON_TENSOR_F32);'
                   'return 0;}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["32", "304", "64", "48", "40", "48", "0", "1", "2", "8", "1", "2", "3"]
    assert (L.FIELD_SOURCE_BUFFER, L.FIELD_SOURCE_MOTION, L.FIELD_SOURCE_RESIDUAL, L.FIELD_MAX_CHANNELS) == (0, 1, 2, 8)
    assert (L.TENSOR_F16, L.TENSOR_BF16, L.TENSOR_F32) == (1, 2, 3)
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for sym in ("leon_pipeline_field_tensor_record", "leon_pipeline_field_tensors_device", "leon_pipeline_field_tensors", "leon_pipeline_field_tensors_kernel"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym


def test_the_header_says_what_is_not_in_the_definition():
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    at = header.index("Field tensors:")
    text = header[at:header.index("#define LEON_FIELD_SOURCE_BUFFER")]
    for word in ("NOT in this definition", "bicubic", "uint8", "HWC", "letterbox", "RGB differences", "rescaling"):
        assert word in text, word


def test_channel_builders_describe_the_layouts(L):
    cw, ch = 64, 48
    ml, rl = L.motion_layout(cw // 16, ch // 16), L.residual_layout(cw, ch)
    m = L.field_channels_motion(cw // 16, L.MOTION_FIELDS, scale=(0.5, 0.25, 1, 2), bias=1.5)
    assert m == [(0, 16, 4, 4, 0.5, 1.5), (2, 16, 4, 4, 0.25, 1.5), (4, 16, 4, 4, 1.0, 1.5), (6, 16, 4, 4, 2.0, 1.5)]
    r = L.field_channels_residual(rl)
    assert r == [(0, rl.luma_stride, 1, 0, 1.0, 0.0), (rl.cb_offset, rl.chroma_stride, 1, 1, 1.0, 0.0), (rl.cr_offset, rl.chroma_stride, 1, 1, 1.0, 0.0)]
    for parts in (1, 2, 3):
        lay = L.accumulate_layout(cw, ch, parts)
        names = L.accumulate_names(parts)
        a = L.field_channels_accumulate(lay, names)
        assert [c[0] for c in a] == [getattr(lay, n.lower() + "_offset") for n in names]
        assert [(c[1], c[3]) for c in a] == [(lay.chroma_stride, 1) if n in ("RCb", "RCr") else (lay.luma_stride, 0) for n in names]
    with pytest.raises(ValueError):
        L.field_channels_accumulate(L.accumulate_layout(cw, ch, 1), ("RY",))
    with pytest.raises(ValueError):
        L.field_channels_motion(4, ("fwd_h", "fwd_v"), scale=(1, 2, 3))
    # the channels read what the layouts' own views read: a residual record's planes and an accumulator's, value for value at a box's own size
    rng = np.random.default_rng(3)
    rec = rng.integers(0, 256, size=(1, rl.record_pitch), dtype=np.uint8)
    st, t = L.field_tensor_record(cw, ch, cw, ch, rec, (0, 0, 0, cw, ch), (ch, cw), r, source="residual", dtype="float32")
    y = np.lib.stride_tricks.as_strided(rec[0].view(np.int16), shape=(ch, cw), strides=(2 * rl.luma_stride, 2))
    cb = np.lib.stride_tricks.as_strided(rec[0, rl.cb_offset:].view(np.int16), shape=(ch // 2, cw // 2), strides=(2 * rl.chroma_stride, 2))
    assert st == 0 and np.array_equal(t[0], y.astype(np.float32)) and np.array_equal(t[1], np.repeat(np.repeat(cb, 2, axis=0), 2, axis=1).astype(np.float32))
    mrec = rng.integers(0, 256, size=(1, ml.record_pitch), dtype=np.uint8)
    st, t = L.field_tensor_record(cw, ch, cw, ch, mrec, (0, 0, 0, cw, ch), (ch, cw), L.field_channels_motion(cw // 16, L.MOTION_FIELDS), source="motion", dtype="float32")
    mv = mrec[0, :8 * ml.mbs].view(np.int16).reshape(ch // 16, cw // 16, 4)
    assert st == 0 and all(np.array_equal(t[k], np.repeat(np.repeat(mv[..., k], 16, axis=0), 16, axis=1).astype(np.float32)) for k in range(4))
