"""CPU: open GOPs (closed_gop = 0) from the writer to the front ends, and the expected frames of a pipeline that decodes
them (include/leon_pipeline.h "Open GOPs"): the leading B pictures of an open GOP predict forward from the last anchor of
the GOP before it; without that GOP -- first of a run, first of a loop pass, broken_link -- they are dropped.

open_gop_frames() is what tests/test_pipeline_open_gop_gpu.py holds the pipeline against.  It parses with the native front
end; here it is held once against the oracle run on the writer's own tensors, so that no parser stands alone as the witness."""
import os
import shutil

import numpy as np
import pytest

from helpers import ROOT, oracle_frames_from_tensors

STREAMS = os.path.join(ROOT, "tests", "golden", "streams")

# GOP lengths in pictures and which GOPs are open: GOP 1 is a lone I picture; GOP 2 is only B B I behind it; GOP 3 is closed
# between two open ones and ends in P; GOP 4 predicts from that P and ends in B pictures behind its last P; GOP 5 predicts
# from GOP 4's last P; GOP 6 has broken_link and loses its leading B pictures.  (A GOP cut behind a P skips display positions:
# the last GOP is a whole IBBP-12, so that every temporal reference lies below the longest GOP's picture count, which is what
# a pipeline sizes its frame ring by.)
GOPS = (7, 1, 3, 10, 6, 4, 12)
OPEN = (1, 2, 4, 5, 6)
BROKEN = (6,)


def gop_entries(n):
    """synth.gop_ibbp cut to n pictures in coded order (I B B P B B P ...); a lone I picture is display position 0"""
    import synth as S
    return [(S.PIC_I, 0, None, None)] if n == 1 else S.gop_ibbp(max(n, 3))[:n]


def open_stream(cw, ch, seed, gops=GOPS, open_gops=OPEN, broken=BROKEN, frame=None, backward_only=False):
    """(stream bytes, the tensors in coded order, the index of each GOP's first picture): built as test_pipeline_gpu.ibbp_stream
    builds its streams, the leading B pictures of OPEN GOPs left to predict forward and bidirectionally (backward_only: open
    by flag only)"""
    import jsv_writer as W
    import synth as S
    rng = np.random.default_rng(seed)
    pics, starts = [], []
    for g, n in enumerate(gops):
        starts.append(len(pics))
        for ptype, disp, f, b in gop_entries(n):
            leading = ptype == S.PIC_B and f is None
            t = S.make_picture(rng, cw, ch, ptype, force_dir=2 if leading and (g not in open_gops or backward_only) else None)
            t["display"] = disp
            pics.append(t)
    fw, fh = frame or (cw, ch)
    data = W.write_stream(pics, cw, ch, fw, fh, gop_starts=starts, closed_gop=open_gops, broken_link=broken)[0]
    return data, pics, starts


def open_gop_frames(data, first_gop=0):
    """({(gop, display_index): RGBA}, {(gop, display_index): (Y, Cb, Cr) cropped to the frame}) of a run that starts at key-map
    entry first_gop: the walk of test_pipeline_gpu.oracle_frames, with older / newer kept across the border of an open GOP
    that has its predecessor, and the leading B pictures of an open GOP that has not left out"""
    import leon_vlc_ctypes as V
    from oracle import oracle_py as O
    st = V.Stream(data, threads=1)
    info = st.info
    cw, ch, fw, fh = info.coded_width, info.coded_height, info.frame_width, info.frame_height
    matrices = lambda i: np.concatenate([np.frombuffer(bytes(i.intra_qm), np.uint8), np.frombuffer(bytes(i.non_intra_qm), np.uint8)])
    qm = matrices(info)
    rgba, planes_out = {}, {}
    gop, older, newer, dropping = -1, None, None, False
    while True:
        p = st.next_picture(dense=True)
        if p is None:
            break
        if p["new_sequence"]:
            qm = matrices(st.refresh_info())
        if p["type"] == 1:
            gop += 1
            has_predecessor = p["open_gop"] and not p["broken_link"] and gop > first_gop
            if not has_predecessor:
                older = newer = None
            dropping = p["open_gop"] and not has_predecessor
        fwd = bwd = None
        if p["type"] == 2:
            fwd = newer
        elif p["type"] == 3:
            if older is None and dropping:
                continue
            bwd, fwd = newer, (older if older is not None else newer)
        planes = O.decode_picture(p["type"], cw, ch, p["coef_y"], p["coef_cb"], p["coef_cr"], p["qscale"], p["intra"],
                                  repadd=p.get("repadd"), mb_dir=p.get("mb_dir"), mv_fwd=p.get("mv_fwd"), mv_bwd=p.get("mv_bwd"),
                                  qm=qm, ref_fwd=fwd, ref_bwd=bwd)
        if p["type"] != 3:
            older, newer = newer, planes
        if gop < first_gop:
            continue
        y, cb, cr = O.split_planes(planes, cw, ch)
        key = (gop, p["temporal_reference"])
        rgba[key] = O.ycbcr_to_rgba(y, cb, cr, cw, fw, fh, "cpu")
        y, cb, cr = y.reshape(ch, cw), cb.reshape(ch // 2, cw // 2), cr.reshape(ch // 2, cw // 2)
        cwid, chh = (fw + 1) // 2, (fh + 1) // 2
        planes_out[key] = tuple(np.ascontiguousarray(a) for a in (y[:fh, :fw], cb[:chh, :cwid], cr[:chh, :cwid]))
    return rgba, planes_out


def dropped_positions(gops, open_gops, broken, first_gop=0):
    """{(gop, display_index)} a run from first_gop on does not deliver: the leading B pictures of open GOPs without predecessor"""
    import synth as S
    out = set()
    for g, n in enumerate(gops):
        if g >= first_gop and g in open_gops and (g == first_gop or g in broken):
            out |= {(g, disp) for ptype, disp, f, b in gop_entries(n) if ptype == S.PIC_B and f is None}
    return out


def frames_from_tensors(pics, starts, cw, ch, gops, open_gops, broken, first_gop=0):
    """{(gop, display_index): RGBA} by helpers.oracle_frames_from_tensors -- the oracle on what went INTO the writer, no parser.
    Its bookkeeping starts over at every entry of gop_starts and carries older / newer through everything between two of
    them: it is given the GOPs WITHOUT predecessor as starts (a closed GOP's leading B pictures predict backward only, so it
    may be one), the dropped pictures taken out, and the GOP number folded into "display" (1000 * gop + display index)."""
    dropped = dropped_positions(gops, open_gops, broken, first_gop)
    feed, chain_starts = [], []
    for g in range(first_gop, len(gops)):
        if g == first_gop or g not in open_gops or g in broken:
            chain_starts.append(len(feed))
        for t in pics[starts[g]:starts[g] + gops[g]]:
            if (g, t["display"]) not in dropped:
                feed.append(dict(t, display=1000 * g + t["display"]))
    out = oracle_frames_from_tensors(feed, cw, ch, gop_starts=tuple(chain_starts))
    return {(d // 1000, d % 1000): v["rgba"] for (_, d), v in out.items()}


def test_writer_defaults_write_the_fixture_byte_for_byte():
    """closed_gop / broken_link left alone: the stream tools/make_streams.py wrote for ibbp_96x64.jsv, rewritten from its tensors"""
    import jsv_writer as W
    import synth as S
    rng = np.random.default_rng(7)
    pics, starts = [], []
    for gop in (S.gop_ibbp(12), S.gop_ibbp(6)):
        starts.append(len(pics))
        for ptype, disp, f, b in gop:
            t = S.make_picture(rng, 96, 64, ptype, force_dir=2 if (ptype == S.PIC_B and f is None) else None)
            t["display"] = disp
            pics.append(t)
    fixture = open(os.path.join(STREAMS, "ibbp_96x64.jsv"), "rb").read()
    assert W.write_stream(pics, 96, 64, 90, 60, gop_starts=starts)[0] == fixture
    assert W.write_stream(pics, 96, 64, 90, 60, gop_starts=starts, closed_gop=True, broken_link=())[0] == fixture
    assert W.write_stream(pics, 96, 64, 90, 60, gop_starts=starts, closed_gop=())[0] == fixture
    # the flags change two bits of a GOP header and nothing else
    opened = W.write_stream(pics, 96, 64, 90, 60, gop_starts=starts, closed_gop=(1,), broken_link=(1,))[0]
    diff = [i for i in range(len(fixture)) if opened[i] != fixture[i]]
    assert len(opened) == len(fixture) and len(diff) == 1
    assert fixture[diff[0]] & 0x60 == 0x40 and opened[diff[0]] & 0x60 == 0x20 and fixture[diff[0]] ^ opened[diff[0]] == 0x60
    assert W.write_stream(pics, 96, 64, 90, 60, gop_starts=starts, closed_gop=False)[0] != fixture


def test_merge_gops_keeps_each_gop_headers_flags():
    """merged single-GOP streams: a closed body stays closed (byte for byte what write_stream writes for the whole), an open or
    broken one keeps its bits"""
    import jsv_writer as W
    import leon_vlc_ctypes as V
    import synth as S
    rng = np.random.default_rng(5)
    gops = [[dict(S.make_picture(rng, 48, 32, ptype), display=disp) for ptype, disp, f, b in S.gop_ibbp(4)] for _ in range(3)]
    whole = W.write_stream(sum(gops, []), 48, 32, gop_starts=[0, 4, 8], closed_gop=(1, 2), broken_link=(2,))[0]
    parts = [W.write_stream(g, 48, 32, gop_starts=[0], closed_gop=i == 0, broken_link=(0,) if i == 2 else ())[0] for i, g in enumerate(gops)]
    assert W.merge_gops(parts, 48, 32)[0] == whole
    st = V.Stream(whole, threads=1)
    flags = []
    while True:
        p = st.next_picture()
        if p is None:
            break
        if p["type"] == 1:
            flags.append((p["open_gop"], p["broken_link"]))
    assert flags == [(False, False), (True, False), (True, True)]


def gop_flags(data, scan):
    """[(open_gop, broken_link)] of every picture, through the host parser or the scan entry"""
    import leon_vlc_ctypes as V
    st = V.Stream(data, threads=1, scan_only=True) if scan else V.Stream(data, threads=1)
    out = []
    while True:
        p = st.scan_picture() if scan else st.next_picture()
        if p is None:
            return out
        out.append((p["type"], p["open_gop"], p["broken_link"]))


@pytest.mark.parametrize("scan", [False, True], ids=["host-parser", "scan"])
def test_flags_round_trip_through_the_front_end(scan):
    """open_gop and broken_link come with the first picture behind the GOP header and with no other; a CLOSED GOP whose header
    sets broken_link reports neither (bit 1 only together with bit 0)"""
    data, pics, starts = open_stream(48, 32, 11, gops=(4, 3, 4, 1, 4), open_gops=(1, 2, 3), broken=(2, 4))
    got = gop_flags(data, scan)
    assert len(got) == len(pics)
    want = {starts[0]: (False, False), starts[1]: (True, False), starts[2]: (True, True), starts[3]: (True, False), starts[4]: (False, False)}
    for i, (ptype, is_open, is_broken) in enumerate(got):
        assert ptype == pics[i]["type"]
        assert (is_open, is_broken) == want.get(i, (False, False)), "picture %d" % i


def test_the_raw_field_is_a_bit_set():
    """leon_vlc_picture.open_gop: bit 0 closed_gop = 0, bit 1 broken_link (include/leon_vlc.h LEON_VLC_GOP_*); the ABI version stays 2"""
    import ctypes as C
    import leon_vlc_ctypes as V
    data, pics, starts = open_stream(48, 32, 11, gops=(4, 3, 4), open_gops=(1, 2), broken=(0, 2))
    st = V.Stream(data, threads=1)
    raw = []
    for _ in pics:
        p = V.Picture()
        assert st.lib.leon_vlc_next_picture(st.h, C.byref(p)) == 1
        raw.append(p.open_gop)
    assert [raw[s] for s in starts] == [0, 1, 3] and sum(raw) == 4
    assert st.lib.leon_vlc_abi_version() == 2


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_the_js_parser_still_parses_the_stream(tmp_path):
    from test_js_parser import run_cli
    data, pics, _ = open_stream(48, 32, 12)
    path = tmp_path / "open.jsv"
    path.write_bytes(data)
    got = run_cli("tensors", str(path))
    assert [p["type"] for p in got["pictures"]] == [t["type"] for t in pics]


def test_expected_frames_agree_with_the_oracle_on_the_writers_tensors():
    """open_gop_frames (native parser + oracle) against helpers.oracle_frames_from_tensors (the writer's tensors + oracle) with
    the same bookkeeping: from the start and from an open GOP in the middle"""
    data, pics, starts = open_stream(48, 32, 13)
    for first in (0, 4):
        got, _ = open_gop_frames(data, first)
        want = frames_from_tensors(pics, starts, 48, 32, GOPS, OPEN, BROKEN, first)
        all_positions = {(g, t["display"]) for g in range(first, len(GOPS)) for t in pics[starts[g]:starts[g] + GOPS[g]]}
        assert set(got) == set(want) == all_positions - dropped_positions(GOPS, OPEN, BROKEN, first)
        for k in want:
            assert np.array_equal(got[k], want[k]), (first, k)
    assert dropped_positions(GOPS, OPEN, BROKEN) == {(6, 0), (6, 1)} and dropped_positions(GOPS, OPEN, BROKEN, 4) == {(4, 0), (4, 1), (6, 0), (6, 1)}
    # the forward reference across the border matters: the frames differ from a decode that starts every GOP over
    from test_pipeline_gpu import oracle_frames
    closed_walk = oracle_frames(data)
    assert any(not np.array_equal(got_all, closed_walk[k]) for k, got_all in open_gop_frames(data)[0].items())


def test_open_by_flag_only_gives_the_closed_frames():
    """an open GOP whose leading B pictures predict backward only decodes to what test_pipeline_gpu.oracle_frames makes of it
    (both references = the I picture) -- wherever it has its predecessor; the dropped positions are the only difference"""
    from test_pipeline_gpu import oracle_frames
    data, pics, starts = open_stream(48, 32, 14, backward_only=True)
    got, _ = open_gop_frames(data)
    want = oracle_frames(data)
    assert set(want) - set(got) == dropped_positions(GOPS, OPEN, BROKEN) and set(got) <= set(want)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
