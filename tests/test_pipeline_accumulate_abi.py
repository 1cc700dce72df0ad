"""CPU: motion and residual accumulated along a GOP's chain (include/leon_pipeline.h, leon_pipeline_accumulate) -- the structs' sizes and
the exports against the header, and the layout call: the planes in their order on 256-byte boundaries, absent parts taking no room,
and with parts = 2 exactly a residual record's offsets.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def test_struct_sizes_and_symbols(L, tmp_path):
    cfg, lay, call = L.PipelineAccumulateConfig, L.PipelineAccumulateLayout, L.PipelineAccumulateCall
    assert C.sizeof(cfg) == 32 and [getattr(cfg, f).offset for f in ("parts", "n_slots", "reserved", "slot_pitch_bytes", "slots_bytes")] == [0, 4, 8, 16, 24]
    assert C.sizeof(lay) == 64
    assert [getattr(lay, f).offset for f in ("coded_width", "coded_height", "parts", "planes", "luma_stride", "chroma_stride", "ax_offset", "ay_offset", "age_offset", "ry_offset",
                                             "rcb_offset", "rcr_offset", "slot_bytes", "slot_pitch", "reserved")] == list(range(0, 60, 4))
    assert C.sizeof(call) == 64
    assert [getattr(call, f).offset for f in ("hops", "n", "reserved0", "slots", "device_via", "device_status", "stream", "reserved")] == [0, 8, 12, 16, 24, 32, 40, 48]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %zu %zu %d %d %zu %zu\\n", '
                   'sizeof(leon_pipeline_accumulate_config), sizeof(struct leon_pipeline_accumulate_layout), sizeof(leon_pipeline_accumulate_call), '
                   'sizeof(leon_pipeline_propagate_hop), LEON_ACCUMULATE_MOTION, LEON_ACCUMULATE_RESIDUAL, offsetof(struct leon_pipeline_accumulate_layout, slot_bytes), '
                   'offsetof(leon_pipeline_accumulate_call, stream));return 0;}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sizes"), str(src)])
    assert subprocess.check_output([str(tmp_path / "sizes")], text=True).split() == ["32", "64", "64", "32", "1", "2", "48", "40"]
    assert (L.ACCUMULATE_MOTION, L.ACCUMULATE_RESIDUAL) == (1, 2)
    header = open(os.path.join(ROOT, "include", "leon_pipeline.h")).read()
    for sym in ("leon_pipeline_accumulate_layout", "leon_pipeline_accumulate_record", "leon_pipeline_accumulate_device", "leon_pipeline_accumulate",
                "leon_pipeline_accumulate_kernel"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym


def pad(v, to):
    return -(-v // to) * to


@pytest.mark.parametrize("cw,ch", [(16, 16), (64, 48), (128, 32), (96, 64), (1920, 1088), (4096, 4096)])
def test_layout(L, cw, ch):
    ls, cs = pad(cw, 64), pad(cw // 2, 64)
    luma, chroma = 2 * ls * ch, 2 * cs * (ch // 2)
    res = L.residual_layout(cw, ch)
    assert (res.luma_stride, res.chroma_stride) == (ls, cs)
    for parts in (1, 2, 3):
        lay = L.accumulate_layout(cw, ch, parts)
        assert (lay.coded_width, lay.coded_height, lay.parts, lay.planes, lay.luma_stride, lay.chroma_stride) == (cw, ch, parts, 6 if parts == 3 else 3, ls, cs)
        offs = [getattr(lay, n.lower() + "_offset") for n in L.ACCUMULATE_PLANES]
        # from the header's text: the planes asked for in their order, each on a 256-byte boundary; 0 for an absent one
        at, want, end = 0, [], 0
        for i in range(6):
            if parts & (1 if i < 3 else 2):
                at = pad(at, 256)
                want.append(at)
                at += luma if i < 4 else chroma
                end = at
            else:
                want.append(0)
        assert offs == want and lay.slot_bytes == end and lay.slot_pitch == pad(end, 256) and list(lay.reserved) == [0, 0]
        assert L.accumulate_names(parts) == tuple(n for i, n in enumerate(L.ACCUMULATE_PLANES) if parts & (1 if i < 3 else 2))
    # parts = 2: exactly as a residual record's planes lie
    lay = L.accumulate_layout(cw, ch, 2)
    assert (lay.ry_offset, lay.rcb_offset, lay.rcr_offset, lay.slot_bytes, lay.slot_pitch) == (0, res.cb_offset, res.cr_offset, res.record_bytes, res.record_pitch)


def test_layout_refusals(L):
    for bad in ((0, 16, 1), (16, 0, 1), (60, 48, 1), (64, 40, 3), (4112, 16, 1), (64, 48, 0), (64, 48, 4), (64, 48, -1)):
        with pytest.raises(L.LeonError):
            L.accumulate_layout(*bad)
    with pytest.raises(L.LeonError):
        L._chk(L.load().leon_pipeline_accumulate_layout(64, 48, 1, None))


def test_views_lie_where_the_layout_says(L):
    import numpy as np
    lay = L.accumulate_layout(128, 32, 3)
    buf = np.zeros((2, lay.slot_bytes + 8), dtype=np.uint8)
    acc = L.accumulate_views(buf, lay)
    assert list(acc) == list(L.ACCUMULATE_PLANES)
    for name, v in acc.items():
        chroma = name in ("RCb", "RCr")
        assert v.shape == ((2, 16, 64) if chroma else (2, 32, 128)) and v.dtype == np.int16
        v[1, 1, 2] = 0x0102
        at = buf.shape[1] + getattr(lay, name.lower() + "_offset") + 2 * ((lay.chroma_stride if chroma else lay.luma_stride) + 2)
        assert buf.reshape(-1)[at] == 2 and buf.reshape(-1)[at + 1] == 1
    assert np.count_nonzero(buf) == 12
