"""Crafted pictures, their group lists and the ring checks for the tests of the RESIDUAL record on lists of the test's own choosing
(tests/test_residual_cases.py checks the table's premises on the CPU, tests/test_residual_kernel_gpu.py runs it through
leon_pipeline_residual_kernel on the device).  The arithmetic's definition is the oracle: lo_pass1_plane followed by
lo_pass2_residual_plane on the picture's DENSE coefficient planes.

A case is made dense first (planes whose groups hold a chosen number of coefficients in chosen columns), turned into lists by
leon_vlc_ctypes.sparsify and then edited by hand where it needs what no parser writes: entries with level 0 (some on cells another
entry fills) and entries of blocks at or behind the plane's block width.  Neither changes the record, so the dense planes stay the
reference; both count towards a group's length, which is how every group reaches exactly the length chosen for it.

k_residual (csrc/leon_kernels.h) cuts a picture into the reconstruction kernels' tasks: two block groups of 8 blocks each, 64 entries
per trip of its wave.  SIZES are the coded sizes at which that differs: one task per plane with 2 of 8 luma and 1 of 8 chroma blocks
valid (16x16), two block-row pairs (48x32), groups exactly full (128x16), a third luma group and a second chroma group with one valid
block (144x32).  COLUMNS 2, 4, 8: tiles whose live columns take the row pass's three forms."""
import ctypes as C
import functools

import numpy as np

from record_cases import SENTINEL, permutation  # noqa: F401  (K.SENTINEL, K.permutation in the tests)

SIZES = ((16, 16), (48, 32), (128, 16), (144, 32))
COLUMNS = (2, 4, 8)
GROUP_SIZES = (0, 1, 63, 64, 65, 129, 512)          # no trip, one lane, a trip less one, a full trip, a trip and one lane, two and one, eight
LEVELS = (1, -1, 255, -255, 2047, -2047, 32767, -32768)          # the last two: the hand-off's wrap path


def groups(cw, ch):
    mbw, mbh = cw // 16, ch // 16
    gy, gc = -(-mbw // 4), -(-mbw // 8)
    return gy, gc, 2 * mbh * gy, mbh * gc


def plane_groups(cw, ch):
    """[(plane 0 Y 1 Cb 2 Cr, block row R, group g, valid blocks)] in the order of the group ids"""
    gy, gc, n_y, n_c = groups(cw, ch)
    out = []
    for plane, W, H, G in ((0, cw, ch, gy), (1, cw // 2, ch // 2, gc), (2, cw // 2, ch // 2, gc)):
        out += [(plane, R, g, min(8, W // 8 - 8 * g)) for R in range(H // 8) for g in range(G)]
    return out


def dense(cw, ch, sizes, columns, rng, levels=LEVELS, mixed=True):
    """(coef_y, coef_cb, coef_cr) int16: group i (plane_groups) holds min(sizes[i], what its valid blocks' first `columns` columns take)
    coefficients, none of them 0; levels: half from `levels`, half anything in -2047 .. 2047 (mixed), or from `levels` alone"""
    planes = [np.zeros((ch, cw), np.int16), np.zeros((ch // 2, cw // 2), np.int16), np.zeros((ch // 2, cw // 2), np.int16)]
    for (plane, R, g, nb), size in zip(plane_groups(cw, ch), sizes):
        cells = nb * 8 * columns
        n = min(int(size), cells)
        at = rng.permutation(cells)[:n]
        b, r, c = at // (8 * columns), (at // columns) % 8, at % columns
        v = rng.choice(np.array(levels), size=n)
        if mixed:
            some = rng.integers(-2047, 2048, size=n)
            some[some == 0] = 7
            v = np.where(rng.random(n) < 0.5, v, some)
        planes[plane][8 * R + r, 64 * g + 8 * b + c] = v.astype(np.int16)
    return planes


def entry(level, b, r, c):
    """an entry of include/leon_vlc.h: level in bits 0..15, the tile offset r * 128 + b * 16 + c * 2 in bits 16..25"""
    return (int(level) & 0xffff) | ((r * 128 + b * 16 + c * 2) << 16)


def top_up(cw, ch, grp_off, entries, sizes, rng):
    """every group filled up to sizes[i] entries with what does not change the record: entries of blocks at or behind the block width
    (any level, where the group has such blocks) and entries with level 0 (any cell, also one that another entry fills), shuffled into
    the group's own entries.  Returns (grp_off, entries, number of level-0 entries, number behind the width)."""
    out, n_zero, n_behind = [], 0, 0
    for i, ((plane, R, g, nb), size) in enumerate(zip(plane_groups(cw, ch), sizes)):
        own = entries[grp_off[i]:grp_off[i + 1]]
        more = []
        for k in range(max(0, int(size) - len(own))):
            if nb < 8 and k % 2 == 0:
                more.append(entry(rng.choice(np.array(LEVELS)), rng.integers(nb, 8), rng.integers(0, 8), rng.integers(0, 8)))
                n_behind += 1
            else:
                more.append(entry(0, rng.integers(0, 8), rng.integers(0, 8), rng.integers(0, 8)))
                n_zero += 1
        both = np.concatenate([own, np.array(more, dtype=np.uint32)]).astype(np.uint32)
        out.append(both[rng.permutation(len(both))])
    new_off = np.zeros(len(out) + 1, np.uint32)
    np.cumsum([len(x) for x in out], out=new_off[1:])
    return new_off, np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32), n_zero, n_behind


def maps(cw, ch, rng, qscales=(1, 31)):
    mbs = (cw // 16) * (ch // 16)
    return rng.choice(np.array(qscales), size=mbs).astype(np.uint8), (rng.random(mbs) < 0.5).astype(np.uint8)


def default_matrices():
    from oracle import oracle_py as O
    return O.default_qm(), O.premultiplier()


def custom_matrices(rng):
    from oracle import oracle_py as O
    return rng.integers(1, 256, size=128).astype(np.uint8), O.premultiplier()


def make(cw, ch, columns, seed, custom, sizes=None, levels=LEVELS, mixed=True, qscales=(1, 31)):
    """a case: dict(cw, ch, coef (y, cb, cr), grp_off, entries, qscale, intra, qm, pm, sizes, n_zero, n_behind)"""
    import leon_vlc_ctypes as V
    rng = np.random.default_rng([seed, cw, ch, columns])
    n = len(plane_groups(cw, ch))
    if sizes is None:
        sizes = rng.choice(np.array(GROUP_SIZES), size=n)
        sizes[rng.permutation(n)[:len(GROUP_SIZES)]] = GROUP_SIZES[:min(n, len(GROUP_SIZES))]
    coef = dense(cw, ch, sizes, columns, rng, levels, mixed)
    grp_off, entries = V.sparsify(coef[0], coef[1], coef[2], cw, ch)
    grp_off, entries, n_zero, n_behind = top_up(cw, ch, grp_off, entries, sizes, rng)
    qscale, intra = maps(cw, ch, rng, qscales)
    qm, pm = custom_matrices(rng) if custom else default_matrices()
    return dict(cw=cw, ch=ch, coef=coef, grp_off=grp_off, entries=entries, qscale=qscale, intra=intra, qm=qm, pm=pm, sizes=np.asarray(sizes), n_zero=n_zero,
                n_behind=n_behind)


def empty(cw, ch):
    """a picture that codes nothing, with maps that hold something everywhere"""
    mbs = (cw // 16) * (ch // 16)
    qm, pm = default_matrices()
    n = len(plane_groups(cw, ch))
    return dict(cw=cw, ch=ch, coef=[np.zeros((ch, cw), np.int16), np.zeros((ch // 2, cw // 2), np.int16), np.zeros((ch // 2, cw // 2), np.int16)],
                grp_off=np.zeros(n + 1, np.uint32), entries=np.zeros(0, np.uint32), qscale=np.full(mbs, 9, np.uint8), intra=np.ones(mbs, np.uint8), qm=qm, pm=pm,
                sizes=np.zeros(n, np.int64), n_zero=0, n_behind=0)


def one_block(level):
    """16x16, the DC of the first luma block alone: five small pictures with different records for the launch-chunk test"""
    c = make(16, 16, 8, 1, False, sizes=[0, 0, 0, 0])
    c["coef"][0][0, 0] = level
    c["grp_off"], c["entries"] = np.array([0, 1, 1, 1, 1], np.uint32), np.array([entry(level, 0, 0, 0)], np.uint32)
    c["qscale"][:], c["intra"][:] = 8, 0
    return c


@functools.lru_cache(maxsize=None)
def named():
    """{name: case}: built once per process and left unchanged"""
    out = {}
    for i, (cw, ch) in enumerate(SIZES):
        for j, columns in enumerate(COLUMNS):
            out["%dx%d_c%d" % (cw, ch, columns)] = make(cw, ch, columns, 3, (i + j) % 2 == 1)
    # an empty half beside a full one: the upper luma block row and Cb full, the lower row and Cr without a coefficient
    n = len(plane_groups(128, 16))
    half = [512 if (p == 0 and R == 0) or p == 1 else 0 for p, R, g, nb in plane_groups(128, 16)]
    assert len(half) == n
    out["empty_half_128x16"] = make(128, 16, 8, 4, True, sizes=half)
    out["empty_48x32"] = empty(48, 32)
    # every coefficient of every valid block at one of the two extreme levels: the hand-off's wrap path in every column
    out["extremes_48x32"] = make(48, 32, 8, 5, False, sizes=[512] * len(plane_groups(48, 32)), levels=(32767, -32768), mixed=False)
    out["dense_2047_144x32"] = make(144, 32, 8, 6, True, sizes=[512] * len(plane_groups(144, 32)), levels=(2047, -2047), mixed=False)
    return out


def picture(case, n_entries=None):
    """the case as residual_kernel takes a picture"""
    p = (case["grp_off"], case["entries"], case["qscale"], case["intra"], case["qm"], case["pm"])
    return p if n_entries is None else p + (n_entries,)


def oracle_residual(case):
    """(y, cb, cr) int32 of the case's dense planes: lo_pass1_plane, then lo_pass2_residual_plane"""
    from oracle import oracle_py as O
    cw, ch = case["cw"], case["ch"]
    out = []
    for k, (W, H) in enumerate(((cw, ch), (cw // 2, ch // 2), (cw // 2, ch // 2))):
        scratch = np.ascontiguousarray(O.pass1_plane(case["coef"][k], W, H, k > 0, case["qscale"], case["intra"], cw // 16, case["qm"], case["pm"]))
        res = np.zeros((H, W), dtype=np.int32)
        O.lib().lo_pass2_residual_plane(scratch.ctypes.data_as(C.c_void_p), W, H, res.ctypes.data_as(C.c_void_p))
        out.append(res)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the record's planes of a named case, int16 (the CPU test checks that the oracle's values lie inside int16); computed once"""
    return tuple(np.clip(p, -32768, 32767).astype(np.int16) for p in oracle_residual(named()[name]))


def expected_of(case):
    return tuple(np.clip(p, -32768, 32767).astype(np.int16) for p in oracle_residual(case))


def assert_record(L, buf, lay, want, what="", sentinel=SENTINEL):
    """buf: a record's bytes up to the pitch, which held the sentinel beforehand; want = (y, cb, cr).  Every specified element equal;
    the bytes between record_bytes and the pitch still the sentinel.  (The pad columns are unspecified: not looked at.)"""
    got = L.residual_planes(buf, lay)
    for name, g, w in zip(("Y", "Cb", "Cr"), got, want):
        bad = np.argwhere(g != w)
        assert not len(bad), "%s: %s differs in %d elements, first at (y, x) %s: %d, expected %d" % (what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert (buf[int(lay.record_bytes):] == sentinel).all(), "%s: bytes behind record_bytes were written" % what


def assert_ring(L, ring, lay, frames, want, what="", sentinel=SENTINEL):
    """ring: uint8 [ring_frames, record_pitch] as it came back; frames: [(picture, ring index)]; want[picture] = (y, cb, cr).  Every
    named record is its picture's; every record no frame names still holds the sentinel in every byte."""
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
        assert_record(L, rec[0], lay, want[int(p)], "%s: picture %d at ring index %d" % (what, p, idx[0]), sentinel)
