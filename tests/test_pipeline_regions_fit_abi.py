"""CPU: the fit of a regions call (include/leon_pipeline.h, leon_pipeline_regions_fit) as the host judges it, no device: the struct's
size, the all-zero fit against leon_pipeline_regions_check region by region, the refusals of the settings, the rectangle against
leon_pipeline_letterbox, and the status words of the boxes that letterboxing refuses -- with check and status agreeing."""
import ctypes as C
import re

import pytest

import fitted_structure as F
import regions_structure as S
from fitted_structure import CALLS
from helpers import ROOT
from regions_structure import BICUBIC, FILTERS, TRIANGLE
from resample_structure import FILTER_NAMES

N_FRAMES = 9


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def test_struct_size_symbols_and_constants(L):
    assert C.sizeof(L.PipelineRegionsFit) == 32
    assert C.sizeof(L.PipelineRegion) == 32 and C.sizeof(L.PipelineRegionsConfig) == 32 and C.sizeof(L.PipelineRegionsDevice) == 64
    header = open(ROOT + "/include/leon_pipeline.h").read()
    for sym in ("leon_pipeline_region_fit_rect", "leon_pipeline_regions_fit_check", "leon_pipeline_region_fit_status", "leon_pipeline_resample_regions_fit",
                "leon_pipeline_read_regions_fit", "leon_pipeline_resample_regions_device_fit"):
        assert hasattr(L.load(), sym) and sym in L.PIPELINE_SYMBOLS and re.search(r"\b%s\(" % sym, header), sym
    for name, value in (("LEON_REGIONS_FIT_STRETCH", L.REGIONS_FIT_STRETCH), ("LEON_REGIONS_FIT_LETTERBOX", L.REGIONS_FIT_LETTERBOX),
                        ("LEON_REGIONS_ANCHOR_CENTRE", L.REGIONS_ANCHOR_CENTRE), ("LEON_REGIONS_ANCHOR_TOP_LEFT", L.REGIONS_ANCHOR_TOP_LEFT)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), header), name
    assert L.load().leon_abi_version() == 3


def outcome(fn, *a, **kw):
    try:
        fn(*a, **kw)
        return None
    except Exception as e:          # LeonError: its code, its region and its message
        return (e.code, getattr(e, "bad", None), str(e))


def test_an_all_zero_fit_is_regions_check_region_by_region(L):
    """the stretch calls of regions_structure and the letterbox calls' boxes, refused ones included: the same verdict, index and message
    with fit NULL, with an all-zero fit and from leon_pipeline_regions_check; the same status word from the three status calls"""
    zero = L.PipelineRegionsFit()
    for calls in (S.CALLS, CALLS):
        for name, call in calls.items():
            fw, fh = call.frame
            boxes = list(call.boxes) + ([call.refused] if getattr(call, "refused", None) else []) + [b for b, _, _ in getattr(call, "refusals", [])]
            boxes += [(0, 0, 0, 8), (fw - 3, 0, 8, 8), (0, 0, 8, fh + 1)]
            for filt in FILTERS:
                for i, box in enumerate(boxes):
                    for frame in (i % N_FRAMES, N_FRAMES):
                        reg = (frame,) + tuple(box)
                        want = outcome(L.regions_check, fw, fh, N_FRAMES, [reg], call.size, filt)
                        assert outcome(L.regions_fit_check, fw, fh, N_FRAMES, [reg], call.size, filt, fit=None) == want
                        assert outcome(L.regions_fit_check, fw, fh, N_FRAMES, [reg], call.size, filt, fit=zero) == want
                        st = L.region_status(fw, fh, N_FRAMES, reg, call.size, filt)
                        assert L.region_fit_status(fw, fh, N_FRAMES, reg, call.size, filt, fit=None) == st
                        assert L.region_fit_status(fw, fh, N_FRAMES, reg, call.size, filt, fit=zero) == st
                        assert (st == 0) == (want is None)
                # the whole list at once: the first offender's index
                regs = [(i % N_FRAMES,) + tuple(b) for i, b in enumerate(boxes)]
                want = outcome(L.regions_check, fw, fh, N_FRAMES, regs, call.size, filt)
                assert want is not None and outcome(L.regions_fit_check, fw, fh, N_FRAMES, regs, call.size, filt, fit=zero) == want


def fit_of(L, mode=1, anchor=0, pad=(0, 0, 0), reserved=(0, 0, 0)):
    return L.PipelineRegionsFit(mode, anchor, (C.c_int32 * 3)(*pad), (C.c_int32 * 3)(*reserved))


BAD_FITS = [("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("anchor 2", dict(anchor=2)), ("anchor -1", dict(anchor=-1)),
            ("pad value 0 is 256", dict(pad=(256, 0, 0))), ("pad value 2 is -1", dict(pad=(0, 0, -1))), ("pad value 1 is 1000", dict(pad=(0, 1000, 0))),
            ("reserved word 0", dict(reserved=(1, 0, 0))), ("reserved word 2", dict(reserved=(0, 0, -5))),
            ("LEON_REGIONS_FIT_STRETCH", dict(mode=0, anchor=1)), ("LEON_REGIONS_FIT_STRETCH", dict(mode=0, pad=(0, 7, 0)))]


@pytest.mark.parametrize("word,fields", BAD_FITS, ids=[w.replace(" ", "-") + str(i) for i, (w, _) in enumerate(BAD_FITS)])
def test_refused_settings(L, word, fields):
    lib, f = L.load(), fit_of(L, **fields)
    cfg, reg, rect, bad = L.PipelineRegionsConfig(37, 19, TRIANGLE), L.PipelineRegion(0, 0, 0, 96, 64), (C.c_int32 * 4)(-7, -7, -7, -7), C.c_int32(5)
    assert lib.leon_pipeline_region_fit_rect(96, 64, C.byref(cfg), C.byref(f), rect) == L.ERR_INVALID
    assert word.encode() in lib.leon_last_error() and list(rect) == [-7] * 4
    assert lib.leon_pipeline_regions_fit_check(96, 64, N_FRAMES, C.byref(reg), 1, C.byref(cfg), C.byref(f), C.byref(bad)) == L.ERR_INVALID
    assert word.encode() in lib.leon_last_error() and bad.value == -1
    assert lib.leon_pipeline_region_fit_status(96, 64, N_FRAMES, C.byref(reg), C.byref(cfg), C.byref(f)) == L.ERR_INVALID
    assert word.encode() in lib.leon_last_error()
    # no pipeline is looked at before the settings are
    assert lib.leon_pipeline_resample_regions_fit(None, 0, C.byref(reg), 1, C.byref(cfg), C.byref(f), None, 0) == L.ERR_INVALID


def test_accepted_settings_and_other_refusals_of_fit_rect(L):
    lib = L.load()
    cfg, rect = L.PipelineRegionsConfig(37, 19, TRIANGLE), (C.c_int32 * 4)()
    for f in (fit_of(L, 1, 0, (255, 0, 255)), fit_of(L, 1, 1, (0, 0, 0)), fit_of(L, 0)):
        assert lib.leon_pipeline_region_fit_rect(96, 64, C.byref(cfg), C.byref(f), rect) == L.OK
    assert lib.leon_pipeline_region_fit_rect(96, 64, C.byref(cfg), None, rect) == L.OK and list(rect) == [0, 0, 37, 19]
    f = fit_of(L)
    for w, h in ((0, 64), (96, 0), (-1, 5)):
        assert lib.leon_pipeline_region_fit_rect(w, h, C.byref(cfg), C.byref(f), rect) == L.ERR_INVALID
    assert lib.leon_pipeline_region_fit_rect(96, 64, None, C.byref(f), rect) == L.ERR_INVALID
    assert lib.leon_pipeline_region_fit_rect(96, 64, C.byref(cfg), C.byref(f), None) == L.ERR_INVALID
    assert lib.leon_pipeline_region_fit_rect(96, 64, C.byref(L.PipelineRegionsConfig(4097, 19, TRIANGLE)), C.byref(f), rect) == L.ERR_INVALID


def test_fit_rect_is_the_letterbox_and_top_left_its_size_at_the_origin(L):
    for name, call in CALLS.items():
        ch, cw = call.size
        for box, (w, h, x, y), _ in call.listed:
            ow, oh, lx, ly = L.letterbox(box[2], box[3], cw, ch)
            assert (ow, oh, lx, ly) == (w, h, x, y), (name, box)
            assert L.region_fit_rect(box[2], box[3], call.size) == (lx, ly, ow, oh)
            assert L.region_fit_rect(box[2], box[3], call.size, anchor="centre", pad_value=(1, 2, 3)) == (lx, ly, ow, oh)
            assert L.region_fit_rect(box[2], box[3], call.size, anchor="top_left") == (0, 0, ow, oh)


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: FILTER_NAMES[f])
def test_the_listed_boxes_pass_and_the_refused_get_their_words(L, filt):
    for name, call in CALLS.items():
        fw, fh = call.frame
        regs = call.regions(N_FRAMES)
        for anchor in F.ANCHORS:
            assert outcome(L.regions_fit_check, fw, fh, N_FRAMES, regs, call.size, filt, anchor=anchor) is None, (name, anchor)
            assert [L.region_fit_status(fw, fh, N_FRAMES, r, call.size, filt, anchor=anchor) for r in regs] == [0] * len(regs)
        for box, boxed, stretched in call.refusals:
            reg = (4,) + box
            assert L.region_fit_status(fw, fh, N_FRAMES, reg, call.size, filt) == getattr(L, boxed), (name, box)
            assert L.region_status(fw, fh, N_FRAMES, reg, call.size, filt) == getattr(L, stretched), (name, box)
            got = outcome(L.regions_fit_check, fw, fh, N_FRAMES, regs[:3] + [reg] + regs[3:], call.size, filt)
            assert got is not None and got[0] == L.ERR_INVALID and got[1] == 3 and "region 3" in got[2] and "reduces by more than 16" in got[2], got
            assert (outcome(L.regions_check, fw, fh, N_FRAMES, regs[:3] + [reg] + regs[3:], call.size, filt) is None) == (stretched == "REGION_OK")
    assert sum(len(c.refusals) for c in CALLS.values()) == 2


def test_status_order_with_a_fit(L):
    """reserved, frame, then x before y; a box without a size is judged against the canvas"""
    fw, fh, size = 608, 57, (13, 37)
    st = lambda reg, **kw: L.region_fit_status(fw, fh, N_FRAMES, reg, size, TRIANGLE, **kw)
    rec = L.PipelineRegion(99, 0, 0, 600, 99)
    rec.reserved[1] = 1
    assert st(rec) == L.REGION_RESERVED
    assert st((9, 0, 0, 600, 99)) == L.REGION_FRAME and st((-1, 0, 0, 8, 8)) == L.REGION_FRAME
    assert st((0, 0, 0, 0, 8)) == L.REGION_BOX and st((0, 0, 0, 8, 0)) == L.REGION_BOX and st((0, 600, 0, 9, 8)) == L.REGION_BOX
    assert st((0, 0, 0, 600, 0)) == L.REGION_RATIO_X          # no letterbox: the canvas, and x comes first
    assert st((0, 0, 0, 592, 0)) == L.REGION_BOX
    assert st((0, 0, 0, 600, 58)) == L.REGION_RATIO_X         # x before the y box
    assert st((0, 0, 0, 8, 58)) == L.REGION_BOX
    assert st((0, 16, 0, 592, 52)) == L.REGION_RATIO_Y == st((0, 16, 0, 592, 52), anchor="top_left")
