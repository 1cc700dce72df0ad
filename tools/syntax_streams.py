#!/usr/bin/env python3
"""syntax_streams.py -- small streams that carry the WHOLE slice-layer syntax (test tooling).

The content of synth.make_picture, written with jsv_writer's defaults, leaves most of ISO/IEC 11172-2's slice layer
unused: one f_code, no full_pel, no stuffing, no address escape, no skipped B macroblocks, the long escape forms and the
large dct_dc_size only by accident.  The cases here start from the same pictures and then force those elements in; the
tensors they return are what went INTO the writer, so whatever a parser reads back is held against them, not against
another parser (tests/test_vlc_syntax.py, tests/test_vlc_syntax_gpu.py).

    pics, data, stats = build_case(CASES[name])
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "mpeg1video-decoder-webgl_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import synth as S           # noqa: E402
import jsv_writer as W      # noqa: E402

# name: size, GOP ("ibbp" / "ippp", pictures), seed, then what the case exists for.  f_code / full_pel: one (forward,
# backward) pair for the stream or a list of pairs handed out to its pictures in turn.  slice_mbs "all": one slice per picture.
CASES = {
    # --- f_code 1 (no residual bits at all) ... 7, forward and backward not the same, full_pel per direction
    "f1":            dict(size=(96, 64), gop=("ibbp", 9), seed=11, f_code=(1, 1), full_pel=(0, 0)),
    "f3_f5_stuffed": dict(size=(96, 64), gop=("ibbp", 9), seed=12, f_code=(3, 5), full_pel=(0, 1), stuffing=1, slice_mbs=5),
    "f7_f4_fullpel": dict(size=(96, 64), gop=("ibbp", 6), seed=13, f_code=(7, 4), full_pel=(1, 0)),
    # slices of one macroblock: the predictor is reset in front of every vector, so nothing can wrap -- the case for f_code 1
    "f1_fullpel_slices1": dict(size=(96, 64), gop=("ibbp", 6), seed=19, f_code=(1, 1), full_pel=(1, 0), slice_mbs=1),
    "f6_f7_fullpel_one_slice": dict(size=(96, 64), gop=("ibbp", 9), seed=14, f_code=(6, 7), full_pel=(1, 1), stuffing=2,
                                    slice_mbs="all", extra_slice=3),
    "f2_f6_yuva":    dict(size=(96, 64), gop=("ibbp", 6), seed=15, f_code=(2, 6), full_pel=(0, 0), alpha=True, stuffing=4),
    "per_picture":   dict(size=(96, 64), gop=("ibbp", 9), seed=16, slice_mbs=5,
                          # one pair per picture, I B B P B B P B B: the two leading B pictures predict backward only, so
                          # their forward code (1) has no vector to wrap
                          f_code=[(1, 2), (1, 3), (1, 5), (2, 7), (6, 6), (3, 4), (7, 5), (4, 6), (5, 2)],
                          full_pel=[(0, 0), (0, 0), (0, 1), (1, 1), (0, 0), (1, 1), (0, 1), (1, 0), (0, 1)]),
    # --- macroblock_escape: 37 macroblocks in a row; slices of 36 start at columns 0, 36 and 35 (an escape in the first
    #     increment of a slice) and P pictures skip 34 macroblocks in a run (an escape between two coded macroblocks)
    "escape_592x32": dict(size=(592, 32), gop=("ibbp", 6), seed=17, f_code=(4, 4), full_pel=(0, 0), slice_mbs=36, long_skip=True),
    # --- I and P only: what the reference parser reads too (the fixtures tests/golden/streams/syntax_*.jsv)
    "f1_ip":         dict(size=(96, 64), gop=("ippp", 4), seed=21, f_code=(1, 1), full_pel=(0, 0), stuffing=5),
    "f5_fullpel_ip": dict(size=(96, 64), gop=("ippp", 4), seed=22, f_code=(5, 5), full_pel=(1, 1), slice_mbs=5, extra_slice=6),
    "f7_one_slice_ip": dict(size=(96, 64), gop=("ippp", 4), seed=23, f_code=(7, 7), full_pel=(0, 0), slice_mbs="all", stuffing=7),
    "escape_ip_592x32": dict(size=(592, 32), gop=("ippp", 3), seed=24, f_code=(4, 4), full_pel=(0, 0), slice_mbs=36, long_skip=True,
                             stuffing=8),
}
# the long ring walk of the GPU parser (VlcWin refills): one slice per picture, dense content, more than one workgroup's rows
CASES["dense_one_slice_208x112"] = dict(size=(208, 112), gop=("ibbp", 6), seed=18, f_code=(3, 2), full_pel=(0, 0), slice_mbs="all",
                                        dense=True)
FIXTURES = ["f1_ip", "f5_fullpel_ip", "f7_one_slice_ip", "escape_ip_592x32"]
# Written WITHOUT the writer's keep_last_mb: P pictures whose slices of 5 end in a macroblock of 6 bits (the vector of the
# macroblock before it, no coefficients), some of which fit into the byte their predecessor ended in.  What the reference
# does with those (it never reads them) is recorded in tests/golden/parser_syntax_lastmb_ip_96x64.json.
QUIRK_CASES = {"lastmb_ip": dict(size=(96, 64), gop=("ippp", 6), seed=31, f_code=(3, 3), full_pel=(0, 0), slice_mbs=5,
                                 repeat_last=5, keep_last_mb=False)}


def fixture_name(case):
    w, h = (CASES.get(case) or QUIRK_CASES[case])["size"]
    return "syntax_%s" % case if case.endswith("x%d" % h) else "syntax_%s_%dx%d" % (case, w, h)


def _block(t, plane, by, bx):
    """view of the 8x8 block (by, bx) of a coefficient plane"""
    return t[plane][8 * by:8 * by + 8, 8 * bx:8 * bx + 8]


def _set_zz(blk, k, level):
    z = int(W.ZIGZAG[k])
    blk[z >> 3, z & 7] = level


def _clear_mb(t, mb, mbw):
    my, mx = divmod(mb, mbw)
    for k in ("coef_y", "coef_a"):
        if k in t:
            t[k][16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = 0
    for k in ("coef_cb", "coef_cr"):
        t[k][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = 0


def _make_inter(t, mb):
    t["intra"][mb] = 0
    t["repadd"][mb] = 0


def syntax_picture(rng, cw, ch, ptype, f_code, full_pel, force_dir=None, alpha=False, long_skip=False, dense=False,
                   repeat_last=None):
    """synth.make_picture, then: vectors over the whole range of the picture's f_code (twice that, even, with full_pel),
    a few quantiser changes, and the rare syntax elements planted where the picture type has room for them"""
    kw = dict(intra_frac=0.15, skip_frac=0.0, uncoded_frac=0.05) if dense else {}
    t = S.make_picture(rng, cw, ch, ptype, in_picture=False, force_dir=force_dir, alpha=alpha, **kw)
    mbw, mbh = cw // 16, ch // 16
    nmb = mbw * mbh
    t["f_code"], t["full_pel"] = tuple(f_code), tuple(full_pel)
    if ptype != S.PIC_I:
        for key, fc, fp in (("mv_fwd", f_code[0], full_pel[0]), ("mv_bwd", f_code[1], full_pel[1])):
            if key not in t:
                continue
            r = 16 << (fc - 1)
            v = rng.integers(-r, r, size=2 * nmb)
            v[:8] = [-r, r - 1, r - 1, -r, -r, -r, r - 1, r - 1]          # the ends of the range, next to each other: wraps
            v = (v * (2 if fp else 1)).astype(np.int16)
            if ptype == S.PIC_P:                                           # skipped P macroblocks keep their zero vector
                v.reshape(-1, 2)[~t[key].reshape(-1, 2).any(axis=1)] = 0
            t[key] = v
    # quantiser changes inside slices
    change = rng.random(nmb) < 0.2
    t["qscale"] = np.where(change, rng.integers(1, 32, size=nmb), t["qscale"]).astype(np.uint8)
    planes = ["coef_y", "coef_cb", "coef_cr"] + (["coef_a"] if alpha else [])

    # levels of +-128 .. +-255 (the long escape forms; 128 and -128 are their first values) and a few coefficients
    # behind long zero runs (an escape carries runs above 31; the table's longest codes runs of 10 .. 31)
    def coded_blocks(plane):
        bh, bw_ = t[plane].shape[0] // 8, t[plane].shape[1] // 8
        return [(by, bx) for by in range(bh) for bx in range(bw_) if _block(t, plane, by, bx).any()]
    for plane in planes:
        blocks = coded_blocks(plane)
        if not blocks:
            continue
        pick = [blocks[int(i)] for i in rng.choice(len(blocks), size=min(10, len(blocks)), replace=False)]
        for n, (by, bx) in enumerate(pick):
            blk = _block(t, plane, by, bx)
            if n < 4:
                _set_zz(blk, int(rng.integers(1, 12)), [128, -128, 255, -255][n])
            elif n < 6:
                _set_zz(blk, int(rng.integers(1, 30)), int(rng.integers(129, 255)) * (1 if n == 4 else -1))
            else:
                dc = blk[0, 0]
                blk[:] = 0
                blk[0, 0] = dc                                             # the DC of an intra block stays; elsewhere the run starts at 0
                if n == 6:
                    _set_zz(blk, 63, -3)                                   # run 62 (or 63): escape, run > 31
                elif n == 7:
                    _set_zz(blk, 40, 1)                                    # run 39 (or 40): escape, run > 31, short form
                    _set_zz(blk, 62, 2)                                    # run 21, level 2: not in the table, short escape
                elif n == 8:
                    _set_zz(blk, 1, 20)                                    # run 0 level 20: a 14-bit code
                    _set_zz(blk, 12, 2)                                    # run 10 level 2: a 16-bit code
                    _set_zz(blk, 40, 1)                                    # run 27 level 1: a 16-bit code
                else:
                    _set_zz(blk, 33, 200)                                  # run 32 (or 33) and a long escape at once
    # intra DC 0 -> 255 -> 0: dct_dc_size 8 with both signs (the predictor starts at 128), 64 and 0 steps for sizes 7 and 0
    intra_mbs = np.nonzero(t["intra"])[0]
    if ptype == S.PIC_I:
        for m, mb in enumerate(intra_mbs[:4]):
            my, mx = divmod(int(mb), mbw)
            lum = [[0, 255, 0, 0], [64, 128, 128, 250], [0, 255, 0, 255], [255, 255, 191, 127]][m]
            for b in range(4):
                _block(t, "coef_y", 2 * my + (b >> 1), 2 * mx + (b & 1))[0, 0] = lum[b]
                if alpha:
                    _block(t, "coef_a", 2 * my + (b >> 1), 2 * mx + (b & 1))[0, 0] = lum[b]
            _block(t, "coef_cb", my, mx)[0, 0] = [0, 255, 0, 64][m]
            _block(t, "coef_cr", my, mx)[0, 0] = [255, 0, 255, 255][m]
    elif len(intra_mbs):
        my, mx = divmod(int(intra_mbs[0]), mbw)
        for b in range(4):
            _block(t, "coef_y", 2 * my + (b >> 1), 2 * mx + (b & 1))[0, 0] = [255, 0, 255, 192][b]
        _block(t, "coef_cb", my, mx)[0, 0] = 0
        _block(t, "coef_cr", my, mx)[0, 0] = 255
    if ptype == S.PIC_B:
        # runs of macroblocks that repeat the one before them, vectors and direction, and carry nothing: skipped in B
        for start, length in ((1, 3), (mbw + 2, 1), (2 * mbw + 1, min(mbw - 3, 6))):
            if start + length >= nmb:
                continue
            _make_inter(t, start)
            for mb in range(start + 1, start + 1 + length):
                _make_inter(t, mb)
                _clear_mb(t, mb, mbw)
                t["mb_dir"][mb] = t["mb_dir"][start]
                t["mv_fwd"][2 * mb:2 * mb + 2] = t["mv_fwd"][2 * start:2 * start + 2]
                t["mv_bwd"][2 * mb:2 * mb + 2] = t["mv_bwd"][2 * start:2 * start + 2]
    if alpha and ptype != S.PIC_I:
        # the yuva syntax has macroblock_quant only together with coded_block_pattern: a macroblock whose only coded blocks
        # are alpha blocks could not say which scale they were quantised with -- give each of those a luma coefficient
        def mb_any(plane, n):
            return t[plane].reshape(mbh, n, mbw, n).transpose(0, 2, 1, 3).reshape(nmb, -1).any(axis=1)
        only_a = mb_any("coef_a", 16) & ~(mb_any("coef_y", 16) | mb_any("coef_cb", 8) | mb_any("coef_cr", 8)) & (t["intra"] == 0)
        for mb in np.nonzero(only_a)[0]:
            t["coef_y"][16 * (int(mb) // mbw), 16 * (int(mb) % mbw) + 1] = 1
    if ptype == S.PIC_P and long_skip:
        # 34 skipped macroblocks in a run, inside a slice of 36: increment 35 = one escape + 2
        for first in range(0, nmb, 36):
            if first + 36 <= nmb:
                for mb in range(first + 1, first + 35):
                    _make_inter(t, mb)
                    _clear_mb(t, mb, mbw)
                    t["mv_fwd"][2 * mb:2 * mb + 2] = 0
        # the two macroblocks of the last, short slice: vectors at opposite ends of the range, so the second one wraps
        r = 16 << (f_code[0] - 1)
        for mb, v in ((nmb - 2, (-r, r - 1)), (nmb - 1, (r - 1, -r))):
            _make_inter(t, mb)
            t["mv_fwd"][2 * mb:2 * mb + 2] = np.array(v) * (2 if full_pel[0] else 1)
    if ptype == S.PIC_P and repeat_last:
        # the last macroblock of every slice of `repeat_last`: the vector of the one before it and nothing else --
        # '1' (increment) '001' (vectors, no pattern) '1' '1' (both differences zero), six bits
        for mb in range(repeat_last - 1, nmb, repeat_last):
            _make_inter(t, mb - 1)
            if not t["mv_fwd"][2 * mb - 2:2 * mb].any():
                t["mv_fwd"][2 * mb - 2:2 * mb] = (2, -2)
            _make_inter(t, mb)
            _clear_mb(t, mb, mbw)
            t["mv_fwd"][2 * mb:2 * mb + 2] = t["mv_fwd"][2 * mb - 2:2 * mb]
    return t


def build_case(case, keep_last_mb=None):
    """(pictures in coded order -- the tensors handed to the writer --, stream bytes, the writer's stats)"""
    c = dict(case)
    if keep_last_mb is None:
        keep_last_mb = c.get("keep_last_mb", True)
    cw, ch = c["size"]
    kind, n = c["gop"]
    gop = S.gop_ibbp(n) if kind == "ibbp" else S.gop_ippp(n)
    rng = np.random.default_rng(c["seed"])
    fcs = c["f_code"] if isinstance(c["f_code"], list) else [c["f_code"]]
    fps = c["full_pel"] if isinstance(c["full_pel"], list) else [c["full_pel"]]
    pics = []
    for i, (ptype, disp, f, b) in enumerate(gop):
        t = syntax_picture(rng, cw, ch, ptype, fcs[i % len(fcs)], fps[i % len(fps)],
                           force_dir=2 if (ptype == S.PIC_B and f is None) else None, alpha=c.get("alpha", False),
                           long_skip=c.get("long_skip", False), dense=c.get("dense", False), repeat_last=c.get("repeat_last"))
        t["display"] = disp
        pics.append(t)
    slice_mbs = c.get("slice_mbs")
    if slice_mbs == "all":
        slice_mbs = (cw // 16) * (ch // 16)
    stats = W.new_stats()
    data, _ = W.write_stream(pics, cw, ch, cw, ch, gop_starts=[0], slice_mbs=slice_mbs, stuffing=c.get("stuffing"),
                             extra_slice=c.get("extra_slice"), b_skip=True, keep_last_mb=keep_last_mb, stats=stats)
    return pics, data, stats
