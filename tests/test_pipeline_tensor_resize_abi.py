"""CPU: the resized tensor output (include/leon_pipeline.h, leon_pipeline_tensor_resize) is part of the C ABI -- its structs and
functions -- and its definition is a pair of integer tables per axis computed on the host: leon_pipeline_resize_weights must equal
leon_ctypes.resize_weights, the Python statement of the same definition, entry for entry.  Where Pillow is installed it is an
independent witness: leon_ctypes.resize_rgb equals Image.resize(size, BILINEAR, box, reducing_gap=None), 0 differing bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

# (frame (w, h), crop (x, y, w, h) or None, size (w, h))
GEOMETRIES = [((352, 240), None, (224, 224)), ((1920, 1080), None, (224, 224)), ((1920, 1080), (419, 0, 1080, 1079), (224, 224)),
              ((96, 64), None, (96, 64)), ((96, 64), (3, 5, 40, 31), (80, 62)), ((360, 199), (1, 1, 357, 197), (23, 13)),
              ((1920, 1080), None, (120, 68)), ((1920, 1080), None, (384, 216))]
# (in_size, crop_start, crop_size, out_size): ratio exactly 16, enlargements
EXTRA_AXES = [(1920, 0, 1920, 120), (4096, 0, 4096, 256), (64, 0, 64, 4), (33, 1, 32, 2), (96, 0, 96, 200), (64, 5, 31, 62), (10, 9, 1, 7), (2, 0, 2, 4096)]


def axes():
    out = list(EXTRA_AXES)
    for (fw, fh), crop, (ow, oh) in GEOMETRIES:
        x, y, w, h = crop or (0, 0, fw, fh)
        out += [(fw, x, w, ow), (fh, y, h, oh)]
    return out


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    return leon_ctypes


def c_weights(L, in_size, crop_start, crop_size, out_size, filt=0, max_taps=None):
    max_taps = L.RESIZE_MAX_TAPS if max_taps is None else max_taps
    n = max(1, min(out_size, 4096))
    first, count, w = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full((n, max(1, max_taps)), -7, np.int32)
    rc = L.load().leon_pipeline_resize_weights(in_size, crop_start, crop_size, out_size, filt, first.ctypes.data, count.ctypes.data, w.ctypes.data, max_taps)
    return rc, first, count, w


def test_c_layout_equals_the_ctypes_mirrors(tmp_path, L):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "leon.h"\n#include "leon_pipeline.h"\nint main(void){\n'
                   '#define R leon_pipeline_tensor_resize\n#define G leon_pipeline_tensor_geometry\n'
                   'printf("%d %d\\n", LEON_RESIZE_TRIANGLE, LEON_RESIZE_MAX_TAPS);\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(R), offsetof(R, crop_x), offsetof(R, crop_y), offsetof(R, crop_width), offsetof(R, crop_height),'
                   ' offsetof(R, out_width), offsetof(R, out_height), offsetof(R, filter));\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(G), offsetof(G, width), offsetof(G, height), offsetof(G, crop_x), offsetof(G, crop_y),'
                   ' offsetof(G, crop_width), offsetof(G, crop_height), offsetof(G, taps_x), offsetof(G, taps_y), offsetof(G, resized));\n'
                   'printf("%zu %zu %zu %zu %d\\n", sizeof(leon_pipeline_config), sizeof(leon_pipeline_frame), sizeof(leon_pipeline_tensor_config), sizeof(leon_pipeline_info),'
                   ' LEON_ABI_VERSION);\n'
                   'int (*a)(const leon_pipeline_config*, const leon_pipeline_tensor_config*, const leon_pipeline_tensor_resize*, const uint8_t*, size_t, size_t,'
                   ' leon_pipeline_callback, void*, leon_pipeline**) = leon_pipeline_create_tensor_resized;\n'
                   'int (*b)(int32_t, int32_t, int32_t, int32_t, int32_t, int32_t*, int32_t*, int32_t*, int32_t) = leon_pipeline_resize_weights;\n'
                   'int (*c)(leon_pipeline*, leon_pipeline_tensor_geometry*) = leon_pipeline_get_tensor_geometry;\n'
                   'return a == 0 || b == 0 || c == 0;}\n')
    lib = os.path.join(ROOT, "mpeg1video-decoder-webgl_amd", "lib")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-o", str(exe), str(src), "-I", os.path.join(ROOT, "include"), "-L", lib, "-lleon_hip", "-Wl,-rpath," + lib])
    lines = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert lines[0] == [L.RESIZE_TRIANGLE, L.RESIZE_MAX_TAPS] == [0, 33]
    R, G = L.PipelineTensorResize, L.PipelineTensorGeometry
    assert lines[1] == [C.sizeof(R), R.crop_x.offset, R.crop_y.offset, R.crop_width.offset, R.crop_height.offset, R.out_width.offset, R.out_height.offset,
                        R.filter.offset] == [28, 0, 4, 8, 12, 16, 20, 24]
    assert lines[2] == [C.sizeof(G), G.width.offset, G.height.offset, G.crop_x.offset, G.crop_y.offset, G.crop_width.offset, G.crop_height.offset,
                        G.taps_x.offset, G.taps_y.offset, G.resized.offset]
    # the structs that existing hosts pass keep their size, the ABI its version
    assert lines[3] == [C.sizeof(L.PipelineConfig), C.sizeof(L.PipelineFrame), C.sizeof(L.PipelineTensorConfig), C.sizeof(L.PipelineInfo), 3]
    assert lines[3][:4] == [56, 64, 28, 112] and L.load().leon_abi_version() == 3
    assert [n for n, _ in L.PipelineInfo._fields_][-5:] == ["tensor_dtype", "tensor_element_bytes", "tensor_frame_bytes", "tensor_frame_pitch", "tensor_gop_pitch"]


def test_names_of_the_binding(L):
    lib = L.load()
    for n in ("leon_pipeline_create_tensor_resized", "leon_pipeline_resize_weights", "leon_pipeline_get_tensor_geometry"):
        assert hasattr(lib, n) and n in L.PIPELINE_SYMBOLS
    assert lib.leon_pipeline_get_tensor_geometry(None, C.byref(L.PipelineTensorGeometry())) == L.ERR_INVALID
    assert lib.leon_pipeline_resize_weights(10, 0, 10, 5, 0, None, None, None, 33) == L.ERR_INVALID


@pytest.mark.parametrize("axis", axes(), ids=lambda a: "%d[%d+%d]to%d" % a)
def test_weights_equal_the_python_definition(L, axis):
    in_size, c0, cs, out = axis
    rc, first, count, w = c_weights(L, *axis)
    assert rc == L.OK, L.load().leon_last_error()
    pf, pn, pw = L.resize_weights(*axis)
    assert pw.shape == (out, int(pn.max())) and pn.max() <= L.RESIZE_MAX_TAPS
    assert np.array_equal(first, pf) and np.array_equal(count, pn)
    assert np.array_equal(w[:, :pw.shape[1]], pw) and not w[:, pw.shape[1]:].any()
    # what the definition promises: taps inside the axis, non-negative weights that sum to 2^22 within a few units
    assert (pf >= 0).all() and (pf + pn <= in_size).all() and (pn >= 1).all() and (pw >= 0).all()
    assert (np.abs(pw.sum(axis=1) - (1 << 22)) <= L.RESIZE_MAX_TAPS).all()
    assert all(not pw[o, pn[o]:].any() for o in range(out))
    # the same rows with max_taps = the largest count; one less is refused
    rc, f2, n2, w2 = c_weights(L, *axis, max_taps=int(pn.max()))
    assert rc == L.OK and np.array_equal(w2, pw) and np.array_equal(f2, pf) and np.array_equal(n2, pn)
    assert c_weights(L, *axis, max_taps=int(pn.max()) - 1)[0] == L.ERR_INVALID


def test_same_size_is_one_tap_of_full_weight(L):
    for axis in ((96, 0, 96, 96), (64, 5, 31, 31), (1920, 419, 1080, 1080)):
        first, count, w = L.resize_weights(*axis)
        rc, cf, cn, cw = c_weights(L, *axis)
        assert rc == L.OK and np.array_equal(cw[:, :w.shape[1]], w)
        assert ((w != 0).sum(axis=1) == 1).all() and (w.max(axis=1) == 1 << 22).all()
        assert np.array_equal(first + w.argmax(axis=1), axis[1] + np.arange(axis[3]))       # output o is sample crop_start + o
    img = np.random.default_rng(7).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(L.resize_rgb(img, None, (64, 96)), img)
    assert np.array_equal(L.resize_rgb(img, (3, 5, 40, 31), (31, 40)), img[5:36, 3:43])


def test_refusals(L):
    lib = L.load()
    assert c_weights(L, 1601, 0, 1601, 100)[0] == L.ERR_INVALID                # ratio 16.01
    assert c_weights(L, 1600, 0, 1600, 100)[0] == L.OK                         # ratio 16
    for axis in ((100, 90, 20, 10), (100, -1, 20, 10), (100, 0, 0, 10), (100, 100, 1, 10), (100, 0, 101, 10)):      # the crop leaves the axis, or is empty
        assert c_weights(L, *axis)[0] == L.ERR_INVALID
        with pytest.raises(ValueError):
            L.resize_weights(*axis)
    assert c_weights(L, 100, 0, 100, 0)[0] == L.ERR_INVALID and c_weights(L, 100, 0, 100, 4097)[0] == L.ERR_INVALID and c_weights(L, 100, 0, 100, -3)[0] == L.ERR_INVALID
    assert c_weights(L, 4096, 0, 4096, 4096)[0] == L.OK
    assert c_weights(L, 100, 0, 100, 50, filt=1)[0] == L.ERR_INVALID           # another filter
    assert b"filter" in lib.leon_last_error()
    for bad in ((1601, 0, 1601, 100), (100, 0, 100, 0), (100, 0, 100, 4097)):
        with pytest.raises(ValueError):
            L.resize_weights(*bad)
    # resize settings without the TENSOR bit: refused by create before any device is touched (so is a resize the limits refuse)
    data = open(os.path.join(ROOT, "tests", "golden", "streams", "ibbp_96x64.jsv"), "rb").read()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    cb = L.PIPELINE_CB(lambda *a: None)
    for output, rz in ((L.PIPELINE_OUTPUT_RGBA, (0, 0, 0, 0, 40, 40, 0)), (L.PIPELINE_OUTPUTS["both"], (0, 0, 0, 0, 40, 40, 0)), (0, (0, 0, 0, 0, 40, 40, 0)),
                       (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 40, 3, 0)), (L.PIPELINE_OUTPUT_TENSOR, (90, 0, 40, 40, 40, 40, 0)),
                       (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 40, 40, 2)), (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 0, 40, 0)),
                       (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 0, 0, 4097, 40, 0)), (L.PIPELINE_OUTPUT_TENSOR, (0, 0, 10, 10, 0, 0, 0))):
        cfg = L.PipelineConfig()
        cfg.output = output
        h = C.c_void_p()
        r = L.PipelineTensorResize(*rz)
        assert lib.leon_pipeline_create_tensor_resized(C.byref(cfg), None, C.byref(r), buf, len(data), len(data), cb, None, C.byref(h)) == L.ERR_INVALID, (output, rz)
        assert b"resize" in lib.leon_last_error() and not h.value


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d-%s-%dx%d" % (g[0] + ("crop" if g[1] else "whole",) + g[2]))
def test_resize_rgb_equals_pillow(L, geometry):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    (fw, fh), crop, (ow, oh) = geometry
    x, y, w, h = crop or (0, 0, fw, fh)
    rng = np.random.default_rng(fw * 31 + ow)
    img = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:fh, 0:fw]
    img[::2] = ((((yy + xx) & 1) * 255).astype(np.uint8))[::2, :, None]       # saturated checkerboard rows between random ones
    got = L.resize_rgb(img, crop, (oh, ow))
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR, box=(x, y, x + w, y + h), reducing_gap=None))
    assert got.shape == ref.shape == (oh, ow, 3)
    assert int((got != ref).sum()) == 0, "%d bytes differ from Pillow %s" % (int((got != ref).sum()), PIL.__version__)
