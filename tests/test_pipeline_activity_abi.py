"""CPU: the activity record of the pipeline's ACTIVITY output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_ACTIVITY) without a
device -- the bit, the symbols, the struct sizes as the binding and as the C compiler has them, the layout's values, and what
leon_pipeline_activity_layout and leon_pipeline_activity_record refuse, each refusal leaving its output untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import activity_cases as K
import leon_ctypes as L
from helpers import ROOT


def pad256(v):
    return (v + 255) // 256 * 256


def test_symbols_bit_and_struct_sizes():
    lib = L.load()
    for n in ("leon_pipeline_activity_layout", "leon_pipeline_activity_record", "leon_pipeline_activity_kernel", "leon_pipeline_get_activity_layout",
              "leon_pipeline_window_activity", "leon_pipeline_read_activity"):
        assert hasattr(lib, n) and n in L.PIPELINE_SYMBOLS
    assert L.PIPELINE_OUTPUT_ACTIVITY == 1 << 7 and L.PIPELINE_OUTPUT_MOTION == 1 << 5
    assert C.sizeof(L.PipelineActivityLayout) == 64 and L.PipelineActivityLayout.summary_offset.offset == 16 and L.PipelineActivityLayout.record_pitch.offset == 32
    assert C.sizeof(L.PipelineActivityPicture) == 32 and L.PipelineActivityPicture.qscale.offset == 16 and L.PipelineActivityPicture.n_entries.offset == 24
    cell = L.ACTIVITY_CELL
    assert cell.itemsize == 8 and [cell.fields[n][1] for n in ("ac_count", "ac_mag", "dc_mag", "blocks", "qscale")] == [0, 2, 4, 6, 7]


def test_structs_have_the_size_the_c_compiler_gives_them(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %d\\n", sizeof(struct leon_pipeline_activity_layout), '
                   'sizeof(leon_pipeline_activity_picture), LEON_PIPELINE_OUTPUT_ACTIVITY);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["64", "32", "128"]


@pytest.mark.parametrize("mbw,mbh", [(6, 4), (37, 2), (13, 7), (22, 15), (1, 1), (32, 1), (120, 68), (256, 256)])
def test_layout(mbw, mbh):
    lay = L.activity_layout(mbw, mbh)
    mbs = mbw * mbh
    assert (lay.mb_width, lay.mb_height, lay.mbs) == (mbw, mbh, mbs)
    assert lay.summary_offset == pad256(8 * mbs)
    assert lay.record_bytes == lay.summary_offset + 32
    assert lay.record_pitch == pad256(lay.record_bytes)
    assert lay.reserved0 == 0 and list(lay.reserved) == [0, 0, 0]


def test_layout_refusals_leave_the_struct_alone():
    lib = L.load()
    for mbw, mbh in ((0, 4), (4, 0), (257, 4), (4, 257), (-1, 1)):
        with pytest.raises(L.LeonError) as e:
            L.activity_layout(mbw, mbh)
        assert e.value.code == L.ERR_INVALID
        out = L.PipelineActivityLayout()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        assert lib.leon_pipeline_activity_layout(mbw, mbh, C.byref(out)) == L.ERR_INVALID
        assert bytes(out) == b"\x5a" * 64
    assert lib.leon_pipeline_activity_layout(4, 4, None) == L.ERR_INVALID


def test_record_refusals_leave_the_record_alone():
    mbw, mbh, (grp_off, entries, qscale) = K.named()["9x2"]
    n_groups = K.groups(mbw, mbh)[2] + 2 * K.groups(mbw, mbh)[3]

    def refused(**kw):
        args = dict(mbw=mbw, mbh=mbh, grp_off=grp_off, entries=entries, qscale=qscale, fill=K.SENTINEL)
        args.update(kw)
        with pytest.raises(L.LeonError) as e:
            L.activity_record(args.pop("mbw"), args.pop("mbh"), args.pop("grp_off"), args.pop("entries"), args.pop("qscale"), **args)
        assert e.value.code == L.ERR_INVALID, e.value
        assert (e.value.buffer == K.SENTINEL).all(), "a refused call wrote the record"

    for w, h in ((0, 2), (9, 0), (257, 2), (9, 257), (-1, 2)):
        refused(mbw=w, mbh=h)
    refused(grp_off=None)
    refused(qscale=None)
    refused(entries=None, n_entries=len(entries))
    refused(record=False)
    for g in (0, 1, n_groups // 2, n_groups - 1):          # grp_off not monotonic, at the first group, inside, at the last
        bad = grp_off.copy()
        if bad[g + 1] == 0:
            bad[g] = 1
        else:
            bad[g] = bad[g + 1] + 1
        refused(grp_off=bad)
    refused(n_entries=int(grp_off[n_groups]) - 1)            # the lists end behind the entries handed over
    # ... and the same arguments are accepted; a picture without entries may have a null list
    L.activity_record(mbw, mbh, grp_off, entries, qscale, fill=K.SENTINEL)
    e_off, e_ent, e_q = K.named()["empty_13x3"][2]
    cells, summary = L.activity_record(13, 3, e_off, None, e_q)
    assert not cells.view(np.uint8).any() and not summary.any()
