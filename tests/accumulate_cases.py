"""Accumulators, hops and the expected result for the tests of leon_pipeline_accumulate (tests/test_accumulate_cases.py on the CPU through
leon_pipeline_accumulate_record, tests/test_accumulate_kernel_gpu.py on the device through leon_pipeline_accumulate_kernel): ONE list
of cases for both, so the definition is pinned without a GPU on exactly what the kernel is run on.  The oracle of all of them is
leon_ctypes.accumulate_hop: the header's text in numpy integers.

A case is a dict: cw, ch, parts, motion, residual (records per window frame, None where there is none), hops, buf (uint8 [S, pitch]:
the slots as the caller hands them over, SENTINEL in the bytes between them) and, where they differ from the usual, n (the count
handed over when it is not len(hops)), n_frames, via / status (False: NULL).  In every case the hops of one call name distinct
destinations and no hop's destination as a source, as the header asks; sources are slots 0 .. 2 unless the case says otherwise."""
import numpy as np

import carry_cases as K

SHAPES = ((16, 16), (64, 48), (128, 32))          # one macroblock; luma stride = width; chroma stride = width
PARTS = (1, 2, 3)
VIA_FILL = 0xEE          # what a via map holds where nothing was written (not a via value)
STATUS_FILL = -77
SENTINEL = 0xA5
# sources in slots 0 .. 2, destinations 3 .. 9, over the six frames of window()
HOPS = [(0, 3, 0, 1), (1, 4, 1, 2), (2, 5, 0, -1), (2, 6, -1, 1), (3, 7, 2, 0), (4, 8, 1, 2), (5, 9, 0, 1)]


def slots(L, rng, cw, ch, parts, S, gap=0, value=None):
    """uint8 [S, slot_bytes + gap]: random bits in every plane (the whole int16 range: saturation happens by itself), or `value` in
    every element; SENTINEL between the slots"""
    lay = L.accumulate_layout(cw, ch, parts)
    assert gap % 4 == 0 and lay.slot_bytes % 256 == 0
    buf = np.full((S, lay.slot_bytes + gap), SENTINEL, dtype=np.uint8)
    if value is None:
        buf[:, :lay.slot_bytes] = rng.integers(0, 256, size=(S, lay.slot_bytes), dtype=np.uint8)
    else:
        buf[:, :lay.slot_bytes].view("<i2")[...] = value
    return buf


def residuals(rng, cw, ch, n, lo=-600, hi=600):
    return [tuple(rng.integers(lo, hi + 1, size=s).astype(np.int16) for s in ((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2))) for _ in range(n)]


def window(mbw, mbh, seed):
    """six frames: two seeded records (vectors that leave the picture at every edge; small ones), the int16 extremes, out at the bottom
    right / top left, out at the left / bottom, an I picture"""
    return [K.varied(mbw, mbh, seed, limit=60), K.varied(mbw, mbh, seed + 1, limit=3), K.uniform(mbw, mbh, (-32768, 32767, 32767, -32768), 3),
            K.uniform(mbw, mbh, (12, 12, -12, -12), 3), K.uniform(mbw, mbh, (-12, 0, 0, 12), 3), K.uniform(mbw, mbh, (0, 0, 0, 0), 4)]


def case(L, what, cw, ch, parts, motion, hops, S=10, gap=0, seed=0, residual=True, value=None, **kw):
    rng = np.random.default_rng(seed)
    res = residuals(rng, cw, ch, len(motion)) if residual is True else residual
    if isinstance(res, list):
        res = [r if m is not None else None for r, m in zip(res, motion)]
    return dict(what=what, cw=cw, ch=ch, parts=parts, motion=motion, residual=res, hops=hops, buf=slots(L, rng, cw, ch, parts, S, gap, value), **kw)


def cases(L):
    out = []
    for cw, ch in SHAPES:
        mbw, mbh = cw // 16, ch // 16
        for parts in PARTS:
            tag = "%dx%d parts %d" % (cw, ch, parts)
            out.append(case(L, "window, " + tag, cw, ch, parts, window(mbw, mbh, 50 + parts), HOPS, seed=cw + parts))
            # sources in the LAST slot of a buffer of exactly n_slots * slot_pitch, vectors into its bottom-right corner: the funnel's spare dword
            vecs = [(32767, 32767), (2 * (cw - 4), 2 * (ch - 1)), (2 * (cw - 5), 2 * (ch - 1)), (2 * (cw - 4) - 1, 2 * ch), (4 * (cw // 2 - 4) - 2, 4 * (ch // 2 - 1))]
            hops = [(f, 2 * f + d, -1 if d else 2 * len(vecs), 2 * len(vecs) if d else -1) for f in range(len(vecs)) for d in (0, 1)]
            out.append(case(L, "last slot, " + tag, cw, ch, parts, [K.uniform(mbw, mbh, v + v, 3) for v in vecs], hops, S=2 * len(vecs) + 1, seed=7 * cw + parts))
            for gap in (4, 256):
                out.append(case(L, "gap %d, %s" % (gap, tag), cw, ch, parts, window(mbw, mbh, 90 + gap), HOPS, gap=gap, seed=gap + parts))
        # the ties of both roundings, (v + 1) >> 1 and (v + 2) >> 2, of both signs: forward with (v, -v), backward with (-v, v)
        ties = (1, -1, 2, -2, 3, -3)
        hops = [(f, 3 + 2 * f + d, -1 if d else 0, 1 if d else -1) for f in range(len(ties)) for d in (0, 1)]
        out.append(case(L, "ties, %dx%d" % (cw, ch), cw, ch, 3, [K.uniform(mbw, mbh, (v, -v, -v, v), 3) for v in ties], hops, S=15, seed=cw))
        # saturation both ways in every plane: sources of 32767 / -32767, the residual and the displacement of the same sign
        for sign in (1, -1):
            rng = np.random.default_rng(3)
            res = [tuple(np.full_like(p, sign * 5000) for p in residuals(rng, cw, ch, 1)[0])]
            out.append(case(L, "saturation %+d, %dx%d" % (sign, cw, ch), cw, ch, 3, [K.uniform(mbw, mbh, (sign * 8, sign * 6, sign * 8, sign * 6), 3)],
                            [(0, 3, 0, -1), (0, 4, -1, 1)], S=5, residual=res, value=sign * 32767))
    cw, ch, mbw, mbh = 64, 48, 4, 3
    # info 0 .. 4 against forward only, backward only, both, neither, and one slot for both
    info = np.array([[0, 1, 2, 3], [4, 3, 2, 1], [1, 4, 0, 2]], dtype=np.uint8)
    mv = np.empty((mbh, mbw, 4), dtype=np.int16)
    mv[:, :] = (12, -8, -20, 4)
    for parts in PARTS:
        out.append(case(L, "info, parts %d" % parts, cw, ch, parts, [(mv, info)], [(0, 3, 0, -1), (0, 4, -1, 1), (0, 5, 0, 1), (0, 6, -1, -1), (0, 7, 2, 2)], seed=11))
    # counts: one hop, one refused hop, refused hops between valid ones, hops behind the call's count
    bad = [(0, 3, 0, 1, 0, 0, 1, 0), (6, 4, 0, 1), (0, 10, 0, 1), (0, 4, 4, 1), (0, 5, 1, -2), (-1, 6, 0, 1), (0, 7, 0, 7)]
    for n in (1, 2, 5):
        hops = []
        for i in range(n):
            hops += [HOPS[i] + (0, 0, 0, 0), bad[i] + (0,) * (8 - len(bad[i]))]
        out.append(case(L, "%d hops, refused ones between" % len(hops), cw, ch, 3, window(mbw, mbh, 70), hops + [(1, 9, 0, 1, 0, 0, 0, 0)] * 2, n=len(hops), seed=n))
    out.append(case(L, "one hop", cw, ch, 3, window(mbw, mbh, 71), HOPS[:1], seed=1))
    out.append(case(L, "one refused hop", cw, ch, 3, window(mbw, mbh, 71), [bad[2]], seed=2))
    for via, status in ((False, True), (True, False), (False, False)):
        out.append(case(L, "via %s, status %s" % (via, status), cw, ch, 3, window(mbw, mbh, 72), HOPS + [(6, 9, 0, 1)], via=via, status=status, seed=3))
    out.append(case(L, "a window of no frames", cw, ch, 3, window(mbw, mbh, 73), HOPS[:2], n_frames=0, seed=4))
    # one macroblock, and a window whose other frames have no record: the rings have one slot, which is not the target's index
    for parts in PARTS:
        out.append(case(L, "only the target's records, parts %d" % parts, 16, 16, parts, [None, K.uniform(1, 1, (4, -6, -8, 2), 3), None], [(1, 3, 0, 2)], S=4, seed=5))
    return out


def expected(L, c):
    """(the buffer after the hops, via [m, mbh, mbw] with VIA_FILL and status [m] with STATUS_FILL where nothing is to be written, the
    set of slots a valid hop writes) by accumulate_hop on a copy; m = len(hops), of which the first n are the call's"""
    want = c["buf"].copy()
    lay = L.accumulate_layout(c["cw"], c["ch"], c["parts"])
    acc = L.accumulate_views(want, lay)
    hops, m = c["hops"], len(c["hops"])
    n = m if c.get("n") is None else c["n"]
    via = np.full((m, c["ch"] // 16, c["cw"] // 16), VIA_FILL, dtype=np.uint8)
    status = np.full(m, STATUS_FILL, dtype=np.int64)
    written = set()
    for i, h in enumerate(hops[:n]):
        st, v = L.accumulate_hop(c["cw"], c["ch"], c.get("n_frames", len(c["motion"])), c["motion"], c["residual"], h, acc)
        status[i] = st
        if st == 0:
            via[i] = v
            written.add(int(h[1]))
    if not c.get("via", True):
        via[:] = VIA_FILL
    if not c.get("status", True):
        status[:] = STATUS_FILL
    return want, via, status, written


def assert_equal(L, c, got, want):
    """got = (buf, via, status), want = what expected() gives.  Every slot exactly: each plane inside the coded size (the pad columns of a destination are
    unspecified), the whole bytes of a slot that no valid hop writes -- sources, slots the call does not name, refused hops' -- and the
    bytes between the slots; via and status exactly, what lies behind the call's count included."""
    what = c["what"]
    lay = L.accumulate_layout(c["cw"], c["ch"], c["parts"])
    gv, wv = L.accumulate_views(got[0], lay), L.accumulate_views(want[0], lay)
    for name in wv:
        if not np.array_equal(gv[name], wv[name]):
            at = np.argwhere(gv[name] != wv[name])
            raise AssertionError("%s: plane %s differs in %d places, first at (slot, y, x) %s: %d, expected %d" % (
                what, name, len(at), at[0].tolist(), gv[name][tuple(at[0])], wv[name][tuple(at[0])]))
    for s in range(c["buf"].shape[0]):
        if s not in want[3]:
            assert np.array_equal(got[0][s], c["buf"][s]), "%s: slot %d, which no valid hop writes, changed" % (what, s)
    assert (got[0][:, lay.slot_bytes:] == SENTINEL).all(), "%s: bytes between the slots were written" % what
    for name, g, w in (("via", got[1], want[1]), ("status", np.asarray(got[2]).astype(np.int64), want[2])):
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            raise AssertionError("%s: %s differs in %d places, first at %s: %s, expected %s" % (what, name, len(at), at[0].tolist(), g[tuple(at[0])], w[tuple(at[0])]))
