"""Crafted group lists, shapes and the ring checks for the tests of the ACTIVITY record on lists of the test's own choosing
(tests/test_activity_cases.py on the CPU against leon_pipeline_activity_record, tests/test_activity_kernel_gpu.py through
leon_pipeline_activity_kernel on the device).  The oracle is leon_ctypes.activity_from_lists: the header's text in numpy, independent of
the C code.

k_activity (csrc/leon_kernels.h) cuts a picture into tasks of the 8 macroblocks under one chroma group of one macroblock row; a task
reads two chroma lists and two or four luma lists, 64 entries per trip of its wave.  WIDTHS are the macroblock widths at which that
differs: one luma group per chroma group and a partly filled one (1), a full luma group (4), a second, partly filled luma group (5), a
full chroma group (8), a second task whose chroma group has one luma group, the missing 2c + 1 (9, 12), and with two (13), and five
tasks a row with a partly filled last group of each kind (37).  HEIGHTS 1, 2, 3: one block-row pair, two, three."""
import functools

import numpy as np

from record_cases import SENTINEL, permutation  # noqa: F401  (K.SENTINEL, K.permutation in the tests)

WIDTHS = (1, 4, 5, 8, 9, 12, 13, 37)
HEIGHTS = (1, 2, 3)
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS]
GROUP_SIZES = (0, 1, 63, 64, 65, 129, 512)          # no trip, one lane, a trip less one, a full trip, a trip and one lane, two and one, eight
LEVELS = (0, 1, -1, 255, -255, -32768)


def groups(mbw, mbh):
    gy, gc = -(-mbw // 4), -(-mbw // 8)
    return gy, gc, 2 * mbh * gy, mbh * gc


def entry(level, b, r, c, junk=0):
    """an entry of include/leon_vlc.h: level in bits 0..15, the tile offset r * 128 + b * 16 + c * 2 in bits 16..25; junk: bits 26..31"""
    return (int(level) & 0xffff) | ((r * 128 + b * 16 + c * 2) << 16) | ((junk & 63) << 26)


def lists(mbw, mbh, seed, extra_groups=0):
    """(grp_off, entries, qscale) of a crafted picture: every group's size from GROUP_SIZES (each size at least once where the picture
    has seven groups), every entry's block 0 .. 7 whatever mbw is -- a partly filled last group holds entries whose mx >= mbw --, one in
    six at DC, levels from LEVELS or anything, junk in the bits no field uses of every fourth entry; qscale 1 .. 31 everywhere, so a
    macroblock that codes nothing shows whether the map leaks.  extra_groups: groups behind Cr (the A groups of a yuva picture), full of
    entries that count nothing."""
    rng = np.random.default_rng([seed, mbw, mbh])
    gy, gc, n_y, n_c = groups(mbw, mbh)
    n = n_y + 2 * n_c + extra_groups
    sizes = rng.choice(np.array(GROUP_SIZES), size=n)
    sizes[rng.permutation(n)[:len(GROUP_SIZES)]] = GROUP_SIZES[:min(n, len(GROUP_SIZES))]
    grp_off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(sizes, out=grp_off[1:])
    total = int(grp_off[-1])
    level = rng.integers(-2047, 2048, size=total)
    pick = rng.random(total) < 0.5
    level[pick] = rng.choice(np.array(LEVELS), size=int(pick.sum()))
    b, r, c = rng.integers(0, 8, size=total), rng.integers(0, 8, size=total), rng.integers(0, 8, size=total)
    dc = rng.random(total) < 1 / 6
    r[dc], c[dc] = 0, 0
    junk = np.where(np.arange(total) % 4 == 3, rng.integers(0, 64, size=total), 0)
    entries = ((level & 0xffff) | ((r * 128 + b * 16 + c * 2) << 16) | (junk << 26)).astype(np.uint32)
    qscale = rng.integers(1, 32, size=mbw * mbh).astype(np.uint8)
    return grp_off, entries, qscale


def empty(mbw, mbh):
    """a picture that codes nothing, with a qscale map that holds something everywhere"""
    gy, gc, n_y, n_c = groups(mbw, mbh)
    return np.zeros(n_y + 2 * n_c + 1, np.uint32), np.zeros(0, np.uint32), np.full(mbw * mbh, 9, np.uint8)


def one_macroblock(per_block, level, dc_level=0):
    """a 1 x 1 picture whose six blocks hold per_block AC entries of `level` each (and a DC entry of dc_level where that is not 0):
    groups Y row 0, Y row 1, Cb, Cr; luma blocks b = 0, 1 of each row"""
    def block(b):
        at = np.arange(per_block, dtype=np.int64) % 63 + 1          # the 63 AC positions (r, c) = (at >> 3, at & 7), over and over
        ac = (int(level) & 0xffff) | (((at >> 3) * 128 + b * 16 + (at & 7) * 2) << 16)
        return np.concatenate([ac, np.array([entry(dc_level, b, 0, 0)] if dc_level else [], dtype=np.int64)])
    grp = [np.concatenate([block(0), block(1)]), np.concatenate([block(1), block(0)]), block(0), block(0)]
    grp_off = np.cumsum([0] + [len(g) for g in grp]).astype(np.uint32)
    return grp_off, np.concatenate(grp).astype(np.uint32), np.array([31], np.uint8)


@functools.lru_cache(maxsize=None)
def named():
    """{name: (mbw, mbh, (grp_off, entries, qscale))}: built once per process and left unchanged"""
    out = {"%dx%d" % s: s + (lists(s[0], s[1], 3),) for s in SHAPES}
    out["empty_13x3"] = (13, 3, empty(13, 3))
    out["empty_1x1"] = (1, 1, empty(1, 1))
    out["saturated_378x255"] = (1, 1, one_macroblock(63, 255, dc_level=200))          # 378 AC entries of 255: 96390 in ac_mag
    out["saturated_dc"] = (1, 1, one_macroblock(0, 1, dc_level=-32768))               # six DC entries of 32768: 196608 in dc_mag
    out["past_2_to_the_32"] = (1, 1, one_macroblock(22000, -32768))                   # 132000 entries of 32768: 2^32 + 30 million before it saturates
    out["a_groups_9x2"] = (9, 2, lists(9, 2, 5, extra_groups=2 * 2 * 3))              # a yuva picture's A groups are not read
    return out


def expected(L, case):
    mbw, mbh, (grp_off, entries, qscale) = case
    return L.activity_from_lists(mbw, mbh, grp_off, entries, qscale)


def assert_record(buf, lay, want, what="", sentinel=SENTINEL):
    """buf: a record's bytes (record_bytes or the pitch) that held the sentinel beforehand; want = (cells, summary).  The two specified
    parts equal, every other byte still the sentinel."""
    cells, summary = want
    mbs, so, rb = int(lay.mbs), int(lay.summary_offset), int(lay.record_bytes)
    got_s = buf[so:so + 32].view(np.uint32)
    got_c = buf[:8 * mbs].view(cells.dtype)
    bad = np.flatnonzero(got_c != cells.reshape(-1))
    assert not len(bad), "%s: cells differ at macroblocks %s: %s, expected %s" % (what, bad[:6].tolist(), got_c[bad[:6]].tolist(), cells.reshape(-1)[bad[:6]].tolist())
    assert got_s.tolist() == summary.tolist(), "%s: summary %s, expected %s" % (what, got_s.tolist(), summary.tolist())
    assert (buf[8 * mbs:so] == sentinel).all(), "%s: bytes behind the cells were written" % what
    assert (buf[rb:] == sentinel).all(), "%s: bytes behind the summary were written" % what


def assert_ring(ring, lay, frames, want, what="", sentinel=SENTINEL):
    """ring: uint8 [ring_frames, record_pitch] as it came back; frames: [(picture, ring index)]; want[picture] = (cells, summary).  Every
    named record is its picture's (assert_record); every record no frame names still holds the sentinel.  Vectorised over the frames of
    a picture."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1, 2)
    assert ring.shape[1] == lay.record_pitch
    named_ = np.zeros(len(ring), dtype=bool)
    named_[frames[:, 1]] = True
    assert named_.sum() == len(frames)
    rest = ring[~named_]
    assert (rest == sentinel).all(), "%s: records no frame names were written: ring indices %s" % (what, np.flatnonzero(~named_)[(rest != sentinel).any(axis=1)][:8].tolist())
    for p in np.unique(frames[:, 0]):
        idx = frames[frames[:, 0] == p, 1]
        rec = ring[idx]
        same = (rec == rec[0]).all(axis=1)
        assert same.all(), "%s: picture %d: the records at ring indices %s differ from the one at %d" % (what, p, idx[~same][:6].tolist(), idx[0])
        assert_record(rec[0], lay, want[int(p)], "%s: picture %d at ring index %d" % (what, p, idx[0]), sentinel)
