"""CPU: the residual record of the pipeline's RESIDUAL output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_RESIDUAL) without a device
-- the bit, the symbols, the struct sizes as the binding and as the C compiler has them, the layout's values, and what
leon_pipeline_residual_layout refuses, each refusal leaving its output untouched."""
import ctypes as C
import os
import subprocess

import pytest

import leon_ctypes as L
from helpers import ROOT


def pad(v, to):
    return (v + to - 1) // to * to


def test_symbols_bit_and_struct_sizes():
    lib = L.load()
    for n in ("leon_pipeline_residual_layout", "leon_pipeline_residual_kernel", "leon_pipeline_get_residual_layout", "leon_pipeline_window_residual",
              "leon_pipeline_read_residual"):
        assert hasattr(lib, n) and n in L.PIPELINE_SYMBOLS
    assert L.PIPELINE_OUTPUT_RESIDUAL == 1 << 9 and L.PIPELINE_OUTPUT_ACTIVITY == 1 << 7 and L.PIPELINE_OUTPUT_MOTION == 1 << 5
    lay = L.PipelineResidualLayout
    assert C.sizeof(lay) == 64 and lay.luma_stride.offset == 8 and lay.cb_offset.offset == 16 and lay.record_pitch.offset == 40
    pic = L.PipelineResidualPicture
    assert C.sizeof(pic) == 56 and pic.intra.offset == 24 and pic.premultiplier.offset == 40 and pic.n_entries.offset == 48


def test_structs_have_the_size_the_c_compiler_gives_them(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %d\\n", sizeof(struct leon_pipeline_residual_layout), '
                   'sizeof(leon_pipeline_residual_picture), LEON_PIPELINE_OUTPUT_RESIDUAL);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["64", "56", "512"]


# (coded size) -> luma_stride, chroma_stride, cb_offset, cr_offset, record_bytes: worked out by hand from the header's text
LAYOUTS = {
    (16, 16): (64, 64, 2048, 3072, 4096),
    (48, 32): (64, 64, 4096, 6144, 8192),
    (128, 16): (128, 64, 4096, 5120, 6144),
    (144, 32): (192, 128, 12288, 16384, 20480),
    (592, 32): (640, 320, 40960, 51200, 61440),
    (4096, 4096): (4096, 2048, 33554432, 41943040, 50331648),
}


@pytest.mark.parametrize("cw,ch", sorted(LAYOUTS))
def test_layout(cw, ch):
    lay = L.residual_layout(cw, ch)
    assert (lay.coded_width, lay.coded_height) == (cw, ch)
    assert (lay.luma_stride, lay.chroma_stride, lay.cb_offset, lay.cr_offset, lay.record_bytes) == LAYOUTS[(cw, ch)]
    # ... and the header's formulas
    assert lay.luma_stride == pad(cw, 64) and lay.chroma_stride == pad(cw // 2, 64)
    assert lay.cb_offset == pad(2 * lay.luma_stride * ch, 256)
    assert lay.cr_offset == lay.cb_offset + pad(2 * lay.chroma_stride * (ch // 2), 256)
    assert lay.record_bytes == lay.cr_offset + 2 * lay.chroma_stride * (ch // 2)
    assert lay.record_pitch == pad(lay.record_bytes, 256)
    assert lay.cb_offset % 256 == 0 and lay.cr_offset % 256 == 0
    assert list(lay.reserved) == [0, 0]


def test_1080p_record_is_smaller_than_an_rgba_frame():
    lay = L.residual_layout(1920, 1088)
    assert lay.record_bytes == 6266880 < 1920 * 1080 * 4


def test_layout_refusals_leave_the_struct_alone():
    lib = L.load()
    for cw, ch in ((0, 64), (64, 0), (4112, 64), (64, 4112), (-16, 16), (24, 16), (16, 24), (15, 16), (8, 8)):
        with pytest.raises(L.LeonError) as e:
            L.residual_layout(cw, ch)
        assert e.value.code == L.ERR_INVALID
        out = L.PipelineResidualLayout()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        assert lib.leon_pipeline_residual_layout(cw, ch, C.byref(out)) == L.ERR_INVALID
        assert bytes(out) == b"\x5a" * 64
    assert lib.leon_pipeline_residual_layout(64, 64, None) == L.ERR_INVALID
