"""CPU: regions of delivered frames as a tensor batch (include/leon_pipeline.h: leon_pipeline_region, leon_pipeline_regions_config,
leon_pipeline_regions_check, leon_pipeline_resample_regions, leon_pipeline_read_regions) are additions to the C ABI -- two new structs
of 32 bytes, three new functions; every struct existing hosts pass keeps its size and the ABI its version.  leon_pipeline_regions_check
refuses, without a device, everything of a call that the host can decide, names the region in leon_last_error and reports its index;
it accepts the calls of tests/regions_structure.py."""
import ctypes as C
import os
import subprocess

import pytest

from helpers import ROOT
from regions_structure import CALLS, FILTERS


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    return leon_ctypes


def test_c_layout_equals_the_ctypes_mirror(tmp_path, L):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "leon.h"\n#include "leon_pipeline.h"\nint main(void){\n'
                   '#define R leon_pipeline_region\n#define G leon_pipeline_regions_config\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(R), offsetof(R, frame), offsetof(R, x), offsetof(R, y), offsetof(R, width), offsetof(R, height),'
                   ' offsetof(R, reserved));\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(G), offsetof(G, out_width), offsetof(G, out_height), offsetof(G, filter), offsetof(G, reserved));\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(leon_pipeline_config), sizeof(leon_pipeline_frame), sizeof(leon_pipeline_tensor_config),'
                   ' sizeof(leon_pipeline_tensor_resize), sizeof(leon_pipeline_tensor_geometry), sizeof(leon_pipeline_tensor_format), sizeof(leon_pipeline_tensor_shape),'
                   ' sizeof(leon_pipeline_info), sizeof(leon_pipeline_tensor_canvas), LEON_ABI_VERSION);\n'
                   'int (*a)(int32_t, int32_t, int32_t, const leon_pipeline_region*, int32_t, const leon_pipeline_regions_config*, int32_t*) = leon_pipeline_regions_check;\n'
                   'int (*b)(leon_pipeline*, int64_t, const leon_pipeline_region*, int32_t, const leon_pipeline_regions_config*, void*, uint64_t) = leon_pipeline_resample_regions;\n'
                   'int (*c)(leon_pipeline*, int64_t, const leon_pipeline_region*, int32_t, const leon_pipeline_regions_config*, void*) = leon_pipeline_read_regions;\n'
                   'R r[2] = {{0, 0, 0, 80, 64, {0, 0, 0}}, {1, 1, 44, 90, 13, {0, 0, 0}}}; G g = {5, 8, LEON_RESIZE_BICUBIC, {0, 0, 0, 0, 0}}; int32_t bad = 7;\n'
                   'int rc = a(96, 64, 2, r, 2, &g, &bad);\n'
                   'printf("%d %d\\n", rc, bad);\n'
                   'return b == 0 || c == 0;}\n')
    lib = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include"), "-L", lib, "-lleon_hip", "-Wl,-rpath," + lib])
    lines = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    R, G = L.PipelineRegion, L.PipelineRegionsConfig
    assert lines[0] == [C.sizeof(R), R.frame.offset, R.x.offset, R.y.offset, R.width.offset, R.height.offset, R.reserved.offset] == [32, 0, 4, 8, 12, 16, 20]
    assert lines[1] == [C.sizeof(G), G.out_width.offset, G.out_height.offset, G.filter.offset, G.reserved.offset] == [32, 0, 4, 8, 12]
    # the structs that existing hosts pass keep their size, the ABI its version
    assert lines[2] == [C.sizeof(L.PipelineConfig), C.sizeof(L.PipelineFrame), C.sizeof(L.PipelineTensorConfig), C.sizeof(L.PipelineTensorResize),
                        C.sizeof(L.PipelineTensorGeometry), C.sizeof(L.PipelineTensorFormat), C.sizeof(L.PipelineTensorShape), C.sizeof(L.PipelineInfo),
                        C.sizeof(L.PipelineTensorCanvas), 3]
    assert lines[2][:9] == [56, 64, 28, 28, 36, 32, 48, 112, 64] and L.load().leon_abi_version() == 3
    # from C: the second region reduces 90 columns to 5
    assert lines[3] == [L.ERR_INVALID, 1]


def test_names_of_the_binding(L):
    lib = L.load()
    for n in ("leon_pipeline_regions_check", "leon_pipeline_resample_regions", "leon_pipeline_read_regions"):
        assert hasattr(lib, n) and n in L.PIPELINE_SYMBOLS
    for m in ("resample_regions", "read_regions", "region_bytes"):
        assert callable(getattr(L.Pipeline, m))
    # no pipeline: refused, no device touched
    r, g = (L.PipelineRegion * 1)(L.PipelineRegion(0, 0, 0, 8, 8)), L.PipelineRegionsConfig(8, 8, 0)
    assert lib.leon_pipeline_resample_regions(None, 0, r, 1, C.byref(g), None, 0) == L.ERR_INVALID
    assert lib.leon_pipeline_read_regions(None, 0, r, 1, C.byref(g), None) == L.ERR_INVALID


@pytest.mark.parametrize("filt", FILTERS)
def test_the_shared_calls_are_accepted(L, filt):
    for call in CALLS.values():
        fw, fh = call.frame
        assert L.regions_check(fw, fh, 9, call.regions(9), call.size, filt) is None


def refused(L, bad, *words, frame=(608, 57), n_frames=9, regions=((0, 5, 3, 37, 13),), size=(13, 37), filt=0):
    with pytest.raises(L.LeonError) as e:
        L.regions_check(frame[0], frame[1], n_frames, regions, size, filt)
    assert e.value.code == L.ERR_INVALID and e.value.bad == bad, (str(e.value), e.value.bad)
    for w in words:
        assert w in str(e.value), str(e.value)
    if bad >= 0:
        assert "region %d" % bad in str(e.value)


def test_refusals_name_the_region(L):
    good = [(0, 5, 3, 37, 13), (8, 0, 0, 592, 57), (3, 571, 0, 37, 57)]
    assert L.regions_check(608, 57, 9, good, (13, 37)) is None
    at = lambda k, r: good[:k] + [r] + good[k + 1:]
    # n outside 1 .. 65535
    refused(L, -1, "1 .. 65535", regions=[])
    refused(L, -1, "1 .. 65535", regions=[good[0]] * 65536)
    assert L.regions_check(608, 57, 9, [good[0]] * 65535, (13, 37)) is None
    # a frame outside the window's frames
    refused(L, 1, "frame 9", regions=at(1, (9, 0, 0, 37, 13)))
    refused(L, 2, "frame -1", regions=at(2, (-1, 0, 0, 37, 13)))
    refused(L, 0, "frame 0", regions=good, n_frames=0)
    # an empty box, a box that leaves the frame
    for k, box in ((0, (0, 0, 0, 13)), (1, (0, 0, 37, 0)), (2, (0, 0, -4, 13)), (1, (-1, 0, 37, 13)), (0, (0, -1, 37, 13)), (2, (572, 0, 37, 13)), (1, (0, 45, 37, 13)),
                   (0, (2 ** 31 - 1, 0, 37, 13)), (1, (0, 0, 2 ** 31 - 1, 13)), (2, (0, 0, 609, 13))):
        refused(L, k, "empty or leaves the frame", regions=at(k, (0,) + box))
    # width / out_width or height / out_height above 16: the message of the tables' builder
    refused(L, 1, "width 600 -> 37 reduces by more than 16", regions=at(1, (0, 1, 44, 600, 13)))
    refused(L, 2, "height 57 -> 3 reduces by more than 16", regions=[(0, 5, 3, 37, 13), (1, 0, 0, 37, 48), (0, 0, 0, 37, 57)], size=(3, 37))
    assert L.regions_check(608, 57, 9, [(0, 0, 0, 592, 48)], (3, 37)) is None          # exactly 16 on both axes
    # an out size outside 1 .. 4096
    for size, word in (((0, 37), "out_height"), ((13, 0), "out_width"), ((4097, 37), "out_height"), ((13, 4097), "out_width"), ((-1, 37), "out_height")):
        refused(L, -1, word, size=size)
    assert L.regions_check(608, 57, 9, [(0, 0, 0, 608, 57)], (4096, 4096)) is None
    # a filter other than 0 or 3
    for filt in (1, 2, 4, -1):
        refused(L, -1, "filter %d" % filt, filt=filt)
    # a non-zero reserved word, of the config and of a region
    for k in range(5):
        cfg = L.PipelineRegionsConfig(37, 13, 0)
        cfg.reserved[k] = 1
        refused(L, -1, "reserved word %d" % k, size=cfg)
    for k in range(3):
        r = L.PipelineRegion(0, 5, 3, 37, 13)
        r.reserved[k] = -7
        refused(L, 1, "reserved word %d" % k, regions=[good[0], r])
    # the first offending region is the one reported
    refused(L, 0, "reduces by more than 16", regions=[(0, 1, 44, 600, 13), (9, 0, 0, 37, 13)])
    # null arguments
    lib = L.load()
    assert lib.leon_pipeline_regions_check(608, 57, 9, None, 1, C.byref(L.PipelineRegionsConfig(37, 13, 0)), None) == L.ERR_INVALID
    assert lib.leon_pipeline_regions_check(608, 57, 9, (L.PipelineRegion * 1)(), 1, None, None) == L.ERR_INVALID


def test_the_refused_box_of_the_shared_call(L):
    call = CALLS["608x57"]
    regs = call.regions(9)
    regs.insert(4, (2,) + call.refused)
    refused(L, 4, "reduces by more than 16", regions=regs, size=call.size)
