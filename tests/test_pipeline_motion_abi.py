"""CPU: the motion record of the pipeline's MOTION output (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_MOTION) without a device --
its layout, its definition held against the tensors that were WRITTEN into tools/syntax_streams.py's streams (the record is the
stream-carried part of a picture's maps: parser state in the maps must not show), the library's CPU evaluation
(leon_pipeline_motion_record, the text k_motion compiles too) against the numpy statement, and anchors written by hand."""
import ctypes as C
import functools

import numpy as np
import pytest

import leon_ctypes as L
import leon_vlc_ctypes as V
import syntax_streams as X
import synth as S
import jsv_writer as W

NAMES = list(X.CASES)


def pad256(v):
    return (v + 255) // 256 * 256


@functools.lru_cache(maxsize=None)
def case(name):
    """(written pictures, parsed pictures, (mbw, mbh)), built and parsed once per process and left unchanged"""
    pics, data, _ = X.build_case(X.CASES[name])
    cw, ch = X.CASES[name]["size"]
    return pics, parse(data), (cw // 16, ch // 16)


def parse(data):
    st = V.Stream(data, threads=1)
    out = []
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        out.append(p)
    st.close()
    return out


def maps_of(p):
    return dict(repadd=p.get("repadd"), mb_dir=p.get("mb_dir"), mv_fwd=p.get("mv_fwd"), mv_bwd=p.get("mv_bwd"))


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


def test_symbols_and_struct_sizes():
    lib = L.load()
    for n in ("leon_pipeline_motion_layout", "leon_pipeline_motion_record", "leon_pipeline_get_motion_layout", "leon_pipeline_window_motion",
              "leon_pipeline_read_motion", "leon_pipeline_motion_kernel"):
        assert hasattr(lib, n) and n in L.PIPELINE_SYMBOLS
    assert L.PIPELINE_OUTPUT_MOTION == 1 << 5
    assert C.sizeof(L.PipelineMotionFrame) == 32 and L.PipelineMotionFrame.fwd_gop.offset == 8 and L.PipelineMotionFrame.fwd_display.offset == 16
    assert L.PipelineMotionFrame.bwd_display.offset == 20
    assert C.sizeof(L.PipelineMotionLayout) == 64
    assert C.sizeof(L.PipelineMotionPicture) == 40 and L.PipelineMotionPicture.repadd.offset == 8 and L.PipelineMotionPicture.mv_bwd.offset == 32


def test_structs_have_the_size_the_c_compiler_gives_them(tmp_path):
    import os
    import subprocess
    from helpers import ROOT
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "leon_pipeline.h"\nint main(void){printf("%zu %zu %d %zu %zu\\n", sizeof(leon_pipeline_motion_frame), '
                   'sizeof(struct leon_pipeline_motion_layout), LEON_PIPELINE_OUTPUT_MOTION, sizeof(leon_pipeline_motion_picture), '
                   'sizeof(leon_pipeline_motion_kernel_frame));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "64", "32", "40", "8"]


@pytest.mark.parametrize("mbw,mbh", [(6, 4), (37, 2), (13, 7), (22, 15), (1, 1), (256, 256)])
def test_layout(mbw, mbh):
    lay = L.motion_layout(mbw, mbh)
    mbs = mbw * mbh
    assert (lay.mb_width, lay.mb_height, lay.mbs) == (mbw, mbh, mbs)
    assert lay.info_offset == pad256(8 * mbs)
    assert lay.summary_offset == lay.info_offset + pad256(mbs)
    assert lay.record_bytes == lay.summary_offset + 32
    assert lay.record_pitch == pad256(lay.record_bytes)
    assert lay.reserved0 == 0 and list(lay.reserved) == [0, 0]


def test_layout_refusals():
    for mbw, mbh in ((0, 4), (4, 0), (257, 4), (4, 257), (-1, 1)):
        with pytest.raises(L.LeonError) as e:
            L.motion_layout(mbw, mbh)
        assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.LeonError):
        L.motion_record(1, 0, 4)
    with pytest.raises(L.LeonError):
        L.motion_record(4, 2, 2)                                              # no such picture type
    with pytest.raises(L.LeonError):
        L.motion_record(3, 2, 1, repadd=np.zeros(2, np.uint8), mv_fwd=np.zeros(4, np.int16))      # a B picture without its backward maps


@pytest.mark.parametrize("name", NAMES)
def test_record_is_the_stream_carried_part_of_the_maps(name):
    """motion_from_maps(parser maps) == motion_from_maps(written tensors) == leon_pipeline_motion_record(parser maps), byte for byte,
    for every picture; the C buffer's unspecified bytes keep their 0xA5"""
    pics, got, (mbw, mbh) = case(name)
    assert len(pics) == len(got)
    lay = L.motion_layout(mbw, mbh)
    mbs = mbw * mbh
    for i, (t, p) in enumerate(zip(pics, got)):
        assert (p["type"], p["temporal_reference"]) == (t["type"], t["display"]), i
        from_parser = L.motion_from_maps(p["type"], mbw, mbh, **maps_of(p))
        from_written = L.motion_from_maps(t["type"], mbw, mbh, **maps_of(t))
        assert same(from_parser, from_written), (name, i, t["type"])
        mv, info, summary, buf = L.motion_record(p["type"], mbw, mbh, fill=0xA5, **maps_of(p))
        assert same((mv, info, summary), from_written), (name, i, t["type"])
        assert mv.dtype == np.int16 and info.dtype == np.uint8 and summary.dtype == np.uint32
        assert len(buf) == lay.record_bytes
        assert (buf[8 * mbs:lay.info_offset] == 0xA5).all() and (buf[lay.info_offset + mbs:lay.summary_offset] == 0xA5).all()
        assert not (info & ~np.uint8(7)).any()


def test_premise_the_maps_hold_parser_state_and_the_record_ignores_it():
    """over the cases: a B macroblock whose UNUSED direction's map entry is not zero (the predictor), and a skipped P macroblock whose
    `intra` flag is stale (the picture before's) -- the record shows neither"""
    unused, stale = 0, 0
    for name in NAMES:
        pics, got, (mbw, mbh) = case(name)
        for t, p in zip(pics, got):
            rec = L.motion_from_maps(p["type"], mbw, mbh, **maps_of(p))
            mv, info = rec[0].reshape(-1, 4), rec[1].reshape(-1)
            if p["type"] == 3:
                d = np.where(np.asarray(p["repadd"]) >= 128, 0, np.asarray(p["mb_dir"]) & 3)
                fwd, bwd = np.asarray(p["mv_fwd"]).reshape(-1, 2), np.asarray(p["mv_bwd"]).reshape(-1, 2)
                hit_f = ((d & 1) == 0) & (info != 4) & fwd.any(axis=1)
                hit_b = ((d & 2) == 0) & (info != 4) & bwd.any(axis=1)
                unused += int(hit_f.sum()) + int(hit_b.sum())
                assert not mv[hit_f, 0:2].any() and not mv[hit_b, 2:4].any()
            if p["type"] == 2:
                # stale: the parser's flag says intra where the written picture has an inter (skipped) macroblock
                hit = (np.asarray(p["intra"]) != 0) & (np.asarray(t["intra"]) == 0)
                stale += int(hit.sum())
                assert (info[hit] == 1).all() and (np.asarray(p["repadd"])[hit] < 128).all()
    assert unused > 0, "no B macroblock of the cases has a predictor in its unused direction's map"
    assert stale > 0, "no skipped P macroblock of the cases has a stale intra flag"


def test_stale_intra_flag_behind_an_i_picture():
    """built here: a P picture directly behind an I picture whose macroblocks 1 .. 4 are skipped -- the parser's `intra` map keeps the I
    picture's 1 there, the record says forward with a zero vector"""
    cw, ch = 96, 64
    mbw, mbh = cw // 16, ch // 16
    rng = np.random.default_rng(5)
    i_pic = S.make_picture(rng, cw, ch, S.PIC_I)
    p_pic = S.make_picture(rng, cw, ch, S.PIC_P, in_picture=False)
    for mb in range(0, 6):
        p_pic["intra"][mb] = 0
        p_pic["repadd"][mb] = 0
    for mb in range(1, 5):                                       # nothing coded, zero vector: skipped
        p_pic["coef_y"][0:16, 16 * mb:16 * mb + 16] = 0
        p_pic["coef_cb"][0:8, 8 * mb:8 * mb + 8] = 0
        p_pic["coef_cr"][0:8, 8 * mb:8 * mb + 8] = 0
        p_pic["mv_fwd"][2 * mb:2 * mb + 2] = 0
    i_pic["display"], p_pic["display"] = 0, 1
    data, _ = W.write_stream([i_pic, p_pic], cw, ch, cw, ch, gop_starts=[0])
    got = parse(data)
    assert [p["type"] for p in got] == [1, 2]
    p = got[1]
    assert (np.asarray(p["intra"])[1:5] != 0).all(), "the premise: the skipped macroblocks keep the I picture's flag"
    mv, info, summary = L.motion_record(2, mbw, mbh, **maps_of(p))
    assert same((mv, info, summary), L.motion_from_maps(2, mbw, mbh, **maps_of(p_pic)))
    assert (info.reshape(-1)[1:5] == 1).all() and not mv.reshape(-1, 4)[1:5].any()


def test_hand_written_anchors():
    """2 x 1 pictures of each type: every info value, a vector of -2048, the summary by hand"""
    for fn in (L.motion_from_maps, L.motion_record):
        # I: both intra, whatever maps are (not) given
        mv, info, s = fn(1, 2, 1)
        assert info.tolist() == [[4, 4]] and not mv.any() and s.tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
        # P: macroblock 0 forward (-2048, 3), macroblock 1 intra (repadd 255; its map entry holds a vector that must not show)
        mv, info, s = fn(2, 2, 1, repadd=np.array([0, 255], np.uint8), mv_fwd=np.array([-2048, 3, 7, 7], np.int16))
        assert info.tolist() == [[1, 4]] and mv.tolist() == [[[-2048, 3, 0, 0], [0, 0, 0, 0]]]
        assert s.tolist() == [1, 0, 1, 1, 2048, 3, 0, 0]
        # P: repadd 127 is not intra, 128 is; a forward macroblock with the zero vector counts as forward and not as moving
        mv, info, s = fn(2, 2, 1, repadd=np.array([127, 128], np.uint8), mv_fwd=np.array([0, 0, 5, 5], np.int16))
        assert info.tolist() == [[1, 4]] and not mv.any() and s.tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
        # B: backward only (the forward entry holds the predictor), then both directions
        mv, info, s = fn(3, 2, 1, repadd=np.array([0, 0], np.uint8), mb_dir=np.array([2, 3], np.uint8),
                         mv_fwd=np.array([9, -9, 1, -2], np.int16), mv_bwd=np.array([-2048, 2046, -3, 4], np.int16))
        assert info.tolist() == [[2, 3]] and mv.tolist() == [[[0, 0, -2048, 2046], [1, -2, -3, 4]]]
        assert s.tolist() == [1, 2, 0, 2, 1, 2, 2051, 2050]
        # B: forward only (the backward entry holds the predictor), then intra (direction bits and vectors in the maps do not show);
        # bits of mb_dir above the low two are not the record's
        mv, info, s = fn(3, 2, 1, repadd=np.array([0, 200], np.uint8), mb_dir=np.array([1 | 4, 3], np.uint8),
                         mv_fwd=np.array([-5, 6, 8, 8], np.int16), mv_bwd=np.array([11, 12, 8, 8], np.int16))
        assert info.tolist() == [[1, 4]] and mv.tolist() == [[[-5, 6, 0, 0], [0, 0, 0, 0]]]
        assert s.tolist() == [1, 0, 1, 1, 5, 6, 0, 0]
        # B: a macroblock without a direction (d = 0) is neither predicted nor intra
        mv, info, s = fn(3, 2, 1, repadd=np.array([0, 0], np.uint8), mb_dir=np.array([0, 0], np.uint8),
                         mv_fwd=np.array([1, 1, 1, 1], np.int16), mv_bwd=np.array([1, 1, 1, 1], np.int16))
        assert info.tolist() == [[0, 0]] and not mv.any() and not s.any()
