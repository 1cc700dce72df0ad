"""The structure of recon_task, column_pass and recon_luma_pair (csrc/leon_kernels.h), stated on the CPU: what a wave derives from
where the non-zero coefficients of its task lie -- the list of live columns and its rounds of 64, the butterfly form each round and
each half's row pass takes, which tile's quantiser scale a column of a two-tile front is dequantised with, the scatter-loop trips of
the sparse road, how many hand-off values leave the int16 range, how many stored samples depend on truncation against floor.
task_facts() follows the kernels' expressions; the arithmetic (dequantiser, butterfly, hand-off) is the reference's, in numpy.

CASES is the list of pictures tests/test_recon_structure.py (the facts) and tests/test_recon_structure_gpu.py (the kernels) share:
each is built at one of five widths, 32 rows high, has an I, a P and a B form over two seeded reference pictures, and carries the
facts it exists for as predicates over task_facts.  ITEMS is the list of edges those predicates must cover between them.
A helper, not a test module."""
import functools

import numpy as np

PIC_I, PIC_P, PIC_B = 1, 2, 3
HEIGHT = 32
WIDTHS = (48, 64, 80, 128, 144)
ROADS = ("plain-dense", "plain-sparse", "display-dense", "display-sparse",
         "yuva-plain-dense", "yuva-plain-sparse", "yuva-display-dense", "yuva-display-sparse")

# the matrices every decoder of these tests runs with: the default intra matrix, and a non-intra matrix with three small entries --
# with 16 everywhere (the default) no non-intra product (2 l + sign) q Q / 16 can floor to 0
QM_INTRA = np.array([
    8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
    22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83], np.uint8)
QM_NON = np.full(64, 16, np.uint8)
QM_NON[0 * 8 + 1], QM_NON[1 * 8 + 0], QM_NON[2 * 8 + 2] = 1, 2, 3
QM = np.concatenate([QM_INTRA, QM_NON])
PREMULTIPLIER = np.array([
    32, 44, 42, 38, 32, 25, 17, 9, 44, 62, 58, 52, 44, 35, 24, 12, 42, 58, 55, 49, 42, 33, 23, 12, 38, 52, 49, 44, 38, 30, 20, 10,
    32, 44, 42, 38, 32, 25, 17, 9, 25, 35, 33, 30, 25, 20, 14, 7, 17, 24, 23, 20, 17, 14, 9, 5, 9, 12, 12, 10, 9, 7, 5, 2], np.int64)


def pair_task(ptype, sparse, alpha):
    """leon_kernels.h pair_task: the two luma parts of a display task share one front"""
    return not sparse and not alpha and ptype != PIC_I


def road_flags(road):
    return dict(display="display" in road, sparse=road.endswith("sparse"), alpha=road.startswith("yuva"))


# ---- the reference's arithmetic, vectorised ---------------------------------------------------------------------------------------

def tdiv256(a):
    """GLSL int '/' 256: truncation toward zero"""
    a = np.asarray(a, np.int64)
    return np.where(a >= 0, a >> 8, -((-a) >> 8))


def butterfly8(X):
    """X[..., 8] -> (o[..., 8], the eight col_final inputs): mpeg1video.js:23 / :26, the text of oracle lo_butterfly8"""
    X = np.asarray(X, np.int64)
    x = [X[..., i] for i in range(8)]
    b1, b3, b4 = x[4], x[2] + x[6], x[5] - x[3]
    tmp1, tmp2, b6 = x[1] + x[7], x[3] + x[5], x[1] - x[7]
    b7, m0 = tmp1 + tmp2, x[0]
    x4 = tdiv256(b6 * 473 - b4 * 196 + 128) - b7
    x0 = x4 - tdiv256((tmp1 - tmp2) * 362 + 128)
    x1 = m0 - b1
    x2 = tdiv256((x[2] - x[6]) * 362 + 128) - b3
    x3 = m0 + b1
    y3, y4, y5, y6 = x1 + x2, x3 + b3, x1 - x2, x3 - b3
    y7 = -x0 - tdiv256(b4 * 473 + b6 * 196 + 128)
    o = np.stack([b7 + y4, x4 + y3, y5 - x0, y6 - y7, y6 + y7, x0 + y5, y3 - x4, y4 - b7], axis=-1)
    return o, np.stack([y4, b7, y3, x4, y5, x0, y6, y7], axis=-1)


def dequant(X, q, intra, c):
    """X[n, 8] raw levels of n columns (rows i), q / intra / c per column -> the butterfly inputs (COL_INT_3, COL_4)"""
    X = np.asarray(X, np.int64)
    q, c = np.asarray(q, np.int64)[:, None], np.asarray(c, np.int64)
    ia = np.asarray(intra, bool)[:, None]
    i = np.arange(8)[None, :]
    Q = np.where(ia, QM_INTRA.astype(np.int64)[i * 8 + c[:, None]], QM_NON.astype(np.int64)[i * 8 + c[:, None]])
    x = 2 * X + np.where(ia, 0, np.sign(X))
    f = (x * q * Q) // 16                                   # floor
    f = np.where(f % 2 == 0, np.where(f > 0, f - 1, f + 1), f)
    f = np.clip(f, -2048, 2047) * PREMULTIPLIER[i * 8 + c[:, None]]
    f = np.where(X == 0, 0, f)
    dc = ia[:, 0] & (c == 0)
    f[:, 0] = np.where(dc, X[:, 0] * 256, f[:, 0])
    return f


def handoff_store(w):
    """_B / UNORM8 store / _E (mpeg1video.js:18): w mod 2^16 with the high byte saturating"""
    w = np.asarray(w, np.int64)
    v = np.where(w < 0, w + 65536, w)
    hi = np.clip(v >> 8, 0, 255)
    u = hi * 256 + (v - (v >> 8) * 256)
    return np.where(u >= 32768, u - 65536, u)


# ---- task_facts -------------------------------------------------------------------------------------------------------------------

def _tile(plane, W, Rb, g):
    """[r][b][c] of block row Rb, blocks 8 g .. 8 g + 7 (blocks past the plane: zeros, what the kernel's bounded loads return)"""
    t = np.zeros((8, 8, 8), np.int64)
    n = min(8, W // 8 - 8 * g)
    if n > 0:
        t[:, :n, :] = np.asarray(plane, np.int64).reshape(-1, W)[8 * Rb:8 * Rb + 8, 64 * g:64 * g + 8 * n].reshape(8, n, 8)
    return t


def _front(tiles, qia, ptype, pred_halves):
    """One front: tiles [tile][half][r][b][c] (changed in place like the kernel's LDS tile), qia [tile][b] = (q, intra) of block b.
    scan_tile's list, column_pass round by round, then the row pass of each half."""
    n_tiles = len(tiles)
    ids, colbits = [], []
    for t in range(n_tiles):
        for h in range(2):
            live = tiles[t][h].any(axis=0).T.reshape(64)              # lane = c * 8 + b
            colbits.append(sum(1 << int(l) for l in np.nonzero(live)[0]))
            ids += [(t << 7) + 64 * h + int(l) for l in np.nonzero(live)[0]]
    n_cols = len(ids)
    rounds, n_sat, below, max_pair = [], 0, 0.0, 0
    for base in range(0, n_cols, 64):
        act = ids[base:base + 64]
        lanes = act + [0] * (64 - len(act))              # idle lanes redo column id 0 (tile 0, half 0, c 0, b 0) and write nothing
        X = np.stack([tiles[i >> 7][(i >> 6) & 1][:, i & 7, (i >> 3) & 7] for i in lanes])
        nz = (X != 0)
        rl = lambda m: 1 + max([i for i in range(8) if m[:, i].any()], default=0)
        # rows_live over the active lanes alone, and over all 64 lanes as lanes_nonzero sees them.  They differ when column 0 is live
        # and an EARLIER round has transformed it in place: the idle lanes then read its eight hand-off values, not coefficients,
        # and usually raise rows_live to 8.  A larger rows_live only picks a fuller butterfly form whose extra inputs are zero in
        # every active lane: conservative (slower), never wrong.  In the first round column 0, if live, is lane 0's own column.
        rows_active, rows_seen = rl(nz[:len(act)]), rl(nz)
        q = np.array([qia[i >> 7][i & 7][0] for i in act])
        ia = np.array([qia[i >> 7][i & 7][1] for i in act])
        c = np.array([(i >> 3) & 7 for i in act])
        o, fin = butterfly8(dequant(X[:len(act)], q, ia, c))
        pairs = np.concatenate([np.abs(fin), np.abs(fin[:, 0::2] + fin[:, 1::2]), np.abs(fin[:, 0::2] - fin[:, 1::2])], axis=1)
        max_pair = max(max_pair, int(pairs.max()))
        s = o.astype(np.float32) * np.float32(0.4)
        sat = np.abs(s) >= np.float32(32768.0)
        n_sat += int(sat.sum())
        if (~sat).any():
            below = max(below, float(np.abs(s)[~sat].max()))
        w = handoff_store(np.floor(s).astype(np.int64))
        for k, i in enumerate(act):
            tiles[i >> 7][(i >> 6) & 1][:, i & 7, (i >> 3) & 7] = w[k]
        rounds.append(dict(active=len(act), rows_live_active=rows_active, rows_live=rows_seen,
                           rows=[i for i in range(8) if nz[:len(act), i].any()],
                           form="lo2" if rows_seen <= 2 else "lo4" if rows_seen <= 4 else "full",
                           lanes_saturating=int(sat.any(axis=1).sum())))
    halves, trunc_differs = [], 0
    for t in range(n_tiles):
        for h in range(2):
            bits = colbits[2 * t + h]
            cols_live = 0 if bits == 0 else (bits.bit_length() + 7) >> 3            # 8 - (clzll(colbits | 1) >> 3)
            form = "skip" if bits == 0 else "lo2" if cols_live <= 2 else "lo4" if cols_live <= 4 else "full"
            halves.append(dict(tile=t, half=h, colbits=bits, cols_live=cols_live, form=form,
                               cols=[c for c in range(8) if (bits >> (8 * c)) & 255]))
            pred = pred_halves[2 * t + h]
            if ptype != PIC_I and pred is not None:
                # row n of block b: Y[c] = trunc(w * 2.5), t = butterfly + 128, sample = clamp(t / 256 + prediction)
                w = tiles[t][h].astype(np.float32) * np.float32(2.5)
                tt = butterfly8(np.trunc(w).astype(np.int64))[0] + 128              # [n][b][m]
                tr, fl = np.clip(tdiv256(tt) + pred, 0, 255), np.clip((tt >> 8) + pred, 0, 255)
                trunc_differs += int((tr != fl).sum())
    return dict(ids=ids, n_cols=n_cols, n_rounds=len(rounds), rounds=rounds, halves=halves,
                qia_tile=[i >> 7 for i in ids],
                dc_lane=[bool(qia[i >> 7][i & 7][1]) and (i & 56) == 0 for i in ids],
                qia_differs=[n_tiles == 2 and qia[0][i & 7] != qia[1][i & 7] for i in ids],
                saturating=n_sat, largest_below=below, largest_col_final=max_pair, trunc_differs=trunc_differs)


def _prediction(pic, cw, ch, refs):
    """the predicted planes (Y, Cb, Cr, A) of a P / B picture: None for an I picture or without references"""
    if pic["type"] == PIC_I or refs is None:
        return None
    from oracle import oracle_py as O
    mbw = cw // 16
    n, n3 = cw * ch, cw * ch * 3 // 2
    fwd, bwd = refs
    cut = lambda buf: [(buf[:n], cw, ch, False), (buf[n:n + n // 4], cw // 2, ch // 2, True), (buf[n + n // 4:n3], cw // 2, ch // 2, True)] + \
        ([(buf[n3:], cw, ch, False)] if len(buf) > n3 else [])
    out = []
    for k, (pf, W, H, chroma) in enumerate(cut(fwd)):
        p = O.predict_plane(pf, W, H, chroma, pic["mv_fwd"], mbw).astype(np.int64)
        mbs = 8 if chroma else 16
        up = lambda m: np.kron(np.asarray(m).reshape(ch // 16, mbw), np.ones((mbs, mbs), np.int64))
        if pic["type"] == PIC_B:
            pb = O.predict_plane(cut(bwd)[k][0], W, H, chroma, pic["mv_bwd"], mbw).astype(np.int64)
            d = up(pic["mb_dir"]) & 3
            p = np.where(d == 0, 0, np.where(d == 1, p, np.where(d == 2, pb, (p + pb + 1) >> 1)))
        out.append(np.where(up(pic["repadd"]) >= 128, 0, p))
    return out


def task_facts(pic, cw, ch, road, refs=None):
    """One record per front of the road's kernel, in task order.  A front is what one scan_tile / column_pass pair covers: a part
    (kind "luma", "chroma", "alpha") or the two luma parts of a dense P / B display task (kind "pair").  refs = (forward, backward)
    flat planes: with them P / B records count the samples whose stored byte depends on truncation against floor."""
    f = road_flags(road)
    ptype = pic["type"]
    mbw, mbh = cw // 16, ch // 16
    bw = cw // 8
    gY, gC = (bw + 7) // 8, (mbw + 7) // 8
    q, ia = np.asarray(pic["qscale"]).reshape(mbh, mbw) & 31, np.asarray(pic["intra"]).reshape(mbh, mbw) != 0
    pred = _prediction(pic, cw, ch, refs)
    planes = {"y": pic["coef_y"], "a": pic.get("coef_a")}

    def mbs_of(Rt, g, chroma):
        """(q, intra) of block b of the part: luma block Q's macroblock is Q >> 1"""
        out = []
        for b in range(8):
            m = min(8 * g + b, (mbw if chroma else bw) - 1)
            m = m if chroma else m >> 1
            out.append((int(q[Rt, m]), bool(ia[Rt, m])))
        return out

    def pred_tile(k, W, Rb, g):
        return None if pred is None else _tile(pred[k], W, Rb, g)          # [n][b][m]

    def luma(kind, Rt, g):
        key, k = ("a", 3) if kind == "alpha" else ("y", 0)
        tiles = [[_tile(planes[key], cw, 2 * Rt + h, g) for h in range(2)]]
        counts = [int((t != 0).sum()) for t in tiles[0]]
        r = _front(tiles, [mbs_of(Rt, g, False)], ptype, [pred_tile(k, cw, 2 * Rt + h, g) for h in range(2)])
        r.update(kind=kind, Rt=Rt, g=g, blocks=min(8, bw - 8 * g), has_right=None, entries=counts)
        return r

    def chroma(Rt, g):
        tiles = [[_tile(pic["coef_cb"], cw // 2, Rt, g), _tile(pic["coef_cr"], cw // 2, Rt, g)]]
        counts = [int((t != 0).sum()) for t in tiles[0]]
        r = _front(tiles, [mbs_of(Rt, g, True)], ptype, [pred_tile(1, cw // 2, Rt, g), pred_tile(2, cw // 2, Rt, g)])
        r.update(kind="chroma", Rt=Rt, g=g, blocks=min(8, mbw - 8 * g), has_right=None, entries=counts)
        return r

    def pair(Rt, gc):
        has_right = 2 * gc + 1 < gY
        gs = [2 * gc, 2 * gc + 1][:2 if has_right else 1]
        tiles = [[_tile(pic["coef_y"], cw, 2 * Rt + h, g) for h in range(2)] for g in gs]
        r = _front(tiles, [mbs_of(Rt, g, False) for g in gs], ptype, [pred_tile(0, cw, 2 * Rt + h, g) for g in gs for h in range(2)])
        r.update(kind="pair", Rt=Rt, g=2 * gc, blocks=min(16, bw - 16 * gc), has_right=has_right, entries=None)
        return r

    recs = []
    if not f["display"]:
        recs += [luma("luma", Rt, g) for Rt in range(mbh) for g in range(gY)]
        recs += [chroma(Rt, g) for Rt in range(mbh) for g in range(gC)]
        if f["alpha"]:
            recs += [luma("alpha", Rt, g) for Rt in range(mbh) for g in range(gY)]
    else:
        for Rt in range(mbh):
            for gc in range(gC):
                recs.append(chroma(Rt, gc))
                if pair_task(ptype, f["sparse"], f["alpha"]):
                    recs.append(pair(Rt, gc))
                    continue
                for g in (2 * gc, 2 * gc + 1):
                    if g < gY:
                        if f["alpha"]:
                            recs.append(luma("alpha", Rt, g))
                        recs.append(luma("luma", Rt, g))
                        recs[-1]["has_right"] = 2 * gc + 1 < gY
    for r in recs:
        if f["sparse"]:
            # the scatter loop: for (k = 64; k < count; k += 64)
            r["scatter_trips"] = [max(0, (n - 1) // 64) for n in r["entries"]]
        else:
            r["entries"] = None
    return recs


def owner(recs, plane, y, x):
    """the record of the front that reconstructs sample (y, x) of plane "y", "cb", "cr" or "a" """
    for r in recs:
        if plane in ("cb", "cr"):
            if r["kind"] == "chroma" and y // 8 == r["Rt"] and 8 * r["g"] <= x // 8 < 8 * r["g"] + 8:
                return r
        elif r["kind"] == {"y": "luma", "a": "alpha"}[plane] or (plane == "y" and r["kind"] == "pair"):
            if y // 16 == r["Rt"] and 8 * r["g"] <= x // 8 < 8 * r["g"] + (16 if r["kind"] == "pair" else 8):
                return r
    return None


def brief(r):
    """a record without its long lists, for a failure message"""
    return {k: v for k, v in r.items() if k not in ("ids", "qia_tile", "dc_lane", "qia_differs")}


# ---- the cases a stream can carry: the road to k_recon_display_out ---------------------------------------------------------------

GOP = ((PIC_I, 2, None, None), (PIC_B, 0, None, 2), (PIC_B, 1, None, 2), (PIC_P, 5, 2, None), (PIC_B, 3, 2, 5), (PIC_B, 4, 2, 5))   # synth.gop_ibbp(6)


def codable(case):
    """can tools/jsv_writer.py code the case's levels?  An AC level of +-255 at most, an intra DC within 255 of its predictor (any
    DC in 0 .. 255, and the small negative ones of these cases)"""
    return all(int(np.abs(case.picture(t)[k]).max()) <= 255 for t in (PIC_I, PIC_P, PIC_B) for k in ("coef_y", "coef_cb", "coef_cr"))


def stream_pictures(width):
    """(pictures in coded order, GOP starts, case names): one closed GOP of six pictures, I B B P B B, per codable case of the width.
    The I picture is the case's with every macroblock intra (an I picture codes no other), the two leading B pictures predict
    backward only, the P and the last two B pictures are the case's own forms.  No A component: the streams are not yuva."""
    pics, starts, names = [], [], []
    for c in CASES:
        if c.width != width or not codable(c):
            continue
        starts.append(len(pics))
        names.append(c.name)
        for ptype, disp, f, b in GOP:
            t = {k: v for k, v in c.picture(ptype, all_intra=ptype == PIC_I).items() if k != "coef_a"}
            if ptype == PIC_B and f is None:
                t["mb_dir"] = np.full_like(t["mb_dir"], 2)
            t["display"] = disp
            pics.append(t)
    return pics, starts, names


@functools.lru_cache(maxsize=None)
def stream(width):
    """(stream bytes, pictures, GOP starts, case names) with the matrices QM in its sequence headers"""
    import jsv_writer as W
    pics, starts, names = stream_pictures(width)
    data = W.write_stream(pics, width, HEIGHT, gop_starts=starts, qm_intra=QM_INTRA, qm_non_intra=QM_NON)[0]
    return data, pics, starts, names


STREAM_ROAD = {"plain-dense": "display-sparse", "plain-sparse": "display-sparse", "display-sparse": "display-sparse", "display-dense": "display-dense"}


def stream_items():
    """the items of ITEMS the streams still show: every fact of a codable case, asked of the picture the stream carries (the I form
    all intra) on the display road that has the same fronts -- single-tile fronts are those of display-sparse, pair fronts those of
    display-dense; the yuva roads have no stream"""
    seen = set()
    for c in CASES:
        if not codable(c):
            continue
        for item, road, ptype, fact in c.facts:
            if road in STREAM_ROAD:
                t = {k: v for k, v in c.picture(ptype, all_intra=ptype == PIC_I).items()}
                if fact(task_facts(t, c.width, HEIGHT, STREAM_ROAD[road])):
                    seen.add(item)
    return seen


# what only the direct ABI roads reach: levels no stream can code, and the fourth component
ABI_ONLY = ("intra DC at -32768, -1, 1 and 32767 with the largest ACs", "each of the DCs -32768, -1, 1 and 32767 in a DC lane",
            "a lane just below |s| = 32768 and a lane at it", "a round in which exactly one lane is beyond |s| = 32768",
            "yuva: A live, Y empty", "yuva: Y live, A empty")


# ---- the pictures -----------------------------------------------------------------------------------------------------------------

def blank(cw, ptype, all_intra=False):
    """no coefficients; every macroblock its own quantiser scale; intra in every third macroblock column, so that the macroblocks of
    block b of the two tiles of a pair (columns m and m + 4) differ in scale everywhere and in the intra flag for three b of four;
    small vectors of odd and even phase, inside the picture; the three directions of a B picture in turn"""
    ch = HEIGHT
    mbw, mbh = cw // 16, ch // 16
    my, mx = np.mgrid[0:mbh, 0:mbw]
    t = {"type": ptype, "qscale": (2 + (3 * mx + 7 * my) % 29).astype(np.uint8).reshape(-1),
         "intra": np.where(((mx + my) % 3 == 0) | all_intra, 255, 0).astype(np.uint8).reshape(-1)}
    for k, (W, H) in (("coef_y", (cw, ch)), ("coef_cb", (cw // 2, ch // 2)), ("coef_cr", (cw // 2, ch // 2)), ("coef_a", (cw, ch))):
        t[k] = np.zeros((H, W), np.int16)
    if ptype != PIC_I:
        import synth as S
        hv = np.array([-3, -2, -1, 0, 1, 2, 3])
        mv = np.stack([hv[(mx + 2 * my) % 7], hv[(3 * mx + my + 2) % 7]], axis=-1)
        t["mv_fwd"] = S.clip_vectors(mv.reshape(-1).astype(np.int16), mbw, mbh, cw, ch)
        if ptype == PIC_B:
            t["mv_bwd"] = S.clip_vectors(mv[..., ::-1].reshape(-1).astype(np.int16), mbw, mbh, cw, ch)
            t["mb_dir"] = (1 + (mx + my) % 3).astype(np.uint8).reshape(-1)
    return t


def finish(t):
    if t["type"] != PIC_I:
        t["repadd"] = np.where(t["intra"] != 0, 255, 0).astype(np.uint8)
    return t


def put(t, Rt, ids, level=lambda j, i: 1 + j % 3, rows=(0,), plane="coef_y", g0=0):
    """levels into the columns `ids` (kernel ids: tile << 7 | half << 6 | c << 3 | b) of the luma front (Rt, g0) -- chroma: plane
    "chroma", half 0 = Cb, half 1 = Cr -- at `rows` (a tuple, or a function of the column's position j in the list)"""
    for j, i in enumerate(ids):
        tile, h, c, b = i >> 7, (i >> 6) & 1, (i >> 3) & 7, i & 7
        Q = 8 * (g0 + tile) + b
        for r in (rows(j) if callable(rows) else rows):
            if plane == "chroma":
                t["coef_cr" if h else "coef_cb"][8 * Rt + r, 8 * Q + c] = level(j, r)
            else:
                t[plane][8 * (2 * Rt + h) + r, 8 * Q + c] = level(j, r)


def scatter(t, seed, density=0.08, planes=("coef_y", "coef_cb", "coef_cr")):
    """seeded sparse content: levels of +-1..6, a DC of 40..200 in every intra block of the luma and chroma planes"""
    rng = np.random.default_rng(seed)
    mbw = t["coef_y"].shape[1] // 16
    for k in planes:
        p = t[k]
        lv = rng.integers(1, 7, p.shape) * rng.choice([-1, 1], p.shape)
        p[...] = np.where(rng.random(p.shape) < density, lv, 0)
        mbs = 8 if k in ("coef_cb", "coef_cr") else 16
        ia = np.kron(t["intra"].reshape(-1, mbw) != 0, np.ones((mbs // 8, mbs // 8), bool))
        p[::8, ::8] = np.where(ia, rng.integers(40, 201, ia.shape), p[::8, ::8])


def oddify_products(t):
    """the floored products (2 l + sign) q Q / 16 of a picture's non-intra luma levels: is there a 0 (which becomes +1), a positive
    and a negative even value (which step toward zero)?"""
    mbw = t["coef_y"].shape[1] // 16
    y = t["coef_y"].astype(np.int64)
    q = np.kron(t["qscale"].reshape(-1, mbw).astype(np.int64), np.ones((16, 16), np.int64))
    non = np.kron(t["intra"].reshape(-1, mbw) == 0, np.ones((16, 16), bool))
    Q = np.tile(QM_NON.reshape(8, 8).astype(np.int64), (y.shape[0] // 8, y.shape[1] // 8))
    f = ((2 * y + np.sign(y)) * q * Q // 16)[non & (y != 0)]
    return bool((f == 0).any() and ((f > 0) & (f % 2 == 0)).any() and ((f < 0) & (f % 2 == 0)).any())


SIGN = lambda j, i: (1 + j % 3) * (-1 if j & 1 else 1)
ALL0 = list(range(128))                        # a whole tile in list order
ALL2 = list(range(256))                        # both tiles of a pair


class Case:
    def __init__(self, name, width, build, facts):
        """build(t): fills a blank picture; facts: [(item of ITEMS, road, ptype, predicate over task_facts' records)]"""
        self.name, self.width, self.build, self.facts = name, width, build, facts

    @functools.lru_cache(maxsize=None)
    def picture(self, ptype, all_intra=False):
        """all_intra: every macroblock intra whatever the case's map says -- the only I picture a stream can carry"""
        t = blank(self.width, ptype, all_intra)
        self.build(t)
        if all_intra:
            t["intra"][:] = 255
        return finish(t)

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def references(cw):
    """the two reference pictures every P and B form predicts from: flat [Y | Cb | Cr | A], seeded"""
    rng = np.random.default_rng(7000 + cw)
    n = cw * HEIGHT * 5 // 2
    return tuple(rng.integers(16, 236, n).astype(np.uint8) for _ in range(2))


def single(recs, kind="luma"):
    return [r for r in recs if r["kind"] == kind]


def pairs(recs):
    return [r for r in recs if r["kind"] == "pair"]


def n_cols_are(kind, *ns):
    return lambda recs: set(ns) <= {r["n_cols"] for r in recs if r["kind"] == kind}


def _cases():
    C = []
    PD, DD, DS = "plain-dense", "display-dense", "display-sparse"

    # -- the list's length on a single-tile front ----------------------------------------------------------------------------------
    def b(t):
        put(t, 0, ALL0[:63], SIGN)
        put(t, 1, ALL0[:65], SIGN)
    C.append(Case("single-63-65", 64, b, [
        ("single n_cols 63", PD, PIC_I, n_cols_are("luma", 63)), ("single n_cols 65", PD, PIC_P, n_cols_are("luma", 65)),
        ("exactly one full left part", DD, PIC_P, lambda R: all(r["blocks"] == 8 and r["has_right"] is False for r in pairs(R))),
        ("column 0 live with a short last round", PD, PIC_I, lambda R: any(
            r["ids"][0] == 0 and r["n_rounds"] == 2 and r["rounds"][1]["active"] == 1 and r["rounds"][1]["rows_live"] > r["rounds"][1]["rows_live_active"]
            for r in single(R)))]))

    def b(t):
        put(t, 0, ALL0[:64], SIGN)
        put(t, 0, [0], lambda j, i: -2, plane="chroma")            # Cb, one column; Cr empty
        put(t, 1, [64 + 9], lambda j, i: 3, rows=(1,), plane="chroma")       # Cr, one column; Cb empty
    C.append(Case("single-64-0-1", 64, b, [
        ("single n_cols 64", PD, PIC_B, n_cols_are("luma", 64)), ("single n_cols 0", PD, PIC_I, n_cols_are("luma", 0)),
        ("single n_cols 1", PD, PIC_P, n_cols_are("chroma", 1)),
        ("Cb live, Cr empty", DS, PIC_B, lambda R: any([h["form"] for h in r["halves"]] == ["lo2", "skip"] for r in single(R, "chroma"))),
        ("Cb empty, Cr live", DS, PIC_B, lambda R: any([h["form"] for h in r["halves"]] == ["skip", "lo2"] for r in single(R, "chroma")))]))

    def b(t):
        put(t, 0, ALL0[1:64], SIGN, rows=(5,))                     # column 0 dead; first round: row 5
        put(t, 0, ALL0[64:], SIGN, rows=(0,))                      # second round: row 0, and an idle lane that reads zeros
        put(t, 1, ALL0[:64], SIGN, rows=(0,))
        put(t, 1, ALL0[64:], SIGN, rows=(7,))
    C.append(Case("single-127-128", 64, b, [
        ("single n_cols 127", PD, PIC_I, n_cols_are("luma", 127)), ("single n_cols 128", PD, PIC_P, n_cols_are("luma", 128)),
        ("column 0 dead with a short last round", PD, PIC_B, lambda R: any(
            r["n_cols"] == 127 and r["ids"][0] != 0 and r["rounds"][1]["active"] == 63 for r in single(R))),
        ("later round with a smaller rows_live", PD, PIC_I, lambda R: any(
            r["n_rounds"] == 2 and (r["rounds"][0]["rows_live"], r["rounds"][1]["rows_live"]) == (6, 1) for r in single(R))),
        ("later round with a larger rows_live", PD, PIC_I, lambda R: any(
            r["n_rounds"] == 2 and (r["rounds"][0]["rows_live"], r["rounds"][1]["rows_live"]) == (1, 8) and r["rounds"][1]["rows_live_active"] == 8
            for r in single(R)))]))

    # -- the list's length on a two-tile front (dense P / B display) ---------------------------------------------------------------
    def pair_case(name, n0, ids0, n1, ids1, extra=()):
        def b(t):
            put(t, 0, ids0, SIGN, rows=lambda j: (j // 64 % 4,))
            put(t, 1, ids1, SIGN, rows=lambda j: (7 - j // 64 % 4,))
        C.append(Case(name, 128, b, [("pair n_cols %d" % n0, DD, PIC_P, n_cols_are("pair", n0)),
                                     ("pair n_cols %d" % n1, DD, PIC_B, n_cols_are("pair", n1))] + list(extra)))
    right_h0 = [128 + l for l in range(64)]
    pair_case("pair-64-65", 64, right_h0, 65, [64 + l for l in range(64)] + [128 + 64 + 10], [
        ("live columns only in the right tile", DD, PIC_P, lambda R: any(r["n_cols"] == 64 and set(r["qia_tile"]) == {1} for r in pairs(R))),
        ("live columns only in half 0", DD, PIC_P, lambda R: any(r["n_cols"] == 64 and not any(i & 64 for i in r["ids"]) for r in pairs(R))),
        ("live columns only in half 1", DD, PIC_B, lambda R: any(r["n_cols"] == 65 and all(i & 64 for i in r["ids"]) for r in pairs(R))),
        ("a full pair", DD, PIC_P, lambda R: all(r["has_right"] and r["blocks"] == 16 for r in pairs(R))),
        ("a right-tile column whose quantiser scale and intra flag differ from the left tile's", DD, PIC_P, lambda R: any(
            any(d and tl for d, tl in zip(r["qia_differs"], r["qia_tile"])) for r in pairs(R)))])
    pair_case("pair-128-129", 128, ALL0, 129, ALL0 + [128 + 37], [
        ("live columns only in the left tile", DD, PIC_P, lambda R: any(r["n_cols"] == 128 and r["has_right"] and set(r["qia_tile"]) == {0} for r in pairs(R)))])
    pair_case("pair-192-193", 192, ALL2[:192], 193, ALL2[:193])
    pair_case("pair-255-256", 255, ALL2[1:], 256, ALL2, [
        ("pair: column 0 dead with a short last round", DD, PIC_P, lambda R: any(
            r["n_cols"] == 255 and r["n_rounds"] == 4 and r["rounds"][3]["active"] == 63 for r in pairs(R))),
        ("pair: four full rounds, the id list filled to its last byte", DD, PIC_B, lambda R: any(
            r["n_cols"] == 256 and [x["active"] for x in r["rounds"]] == [64] * 4 and r["ids"][-1] == 255 for r in pairs(R)))])

    # -- widths --------------------------------------------------------------------------------------------------------------------
    C.append(Case("w48-partial-left", 48, lambda t: scatter(t, 48), [
        ("a lone partial left part", DD, PIC_P, lambda R: all(r["blocks"] == 6 and r["has_right"] is False and r["n_cols"] > 0 for r in pairs(R)))]))
    C.append(Case("w80-partial-right-alpha-empty", 80, lambda t: scatter(t, 80), [
        ("a partial right part", DD, PIC_B, lambda R: all(
            r["blocks"] == 10 and r["has_right"] and {i & 7 for i in r["ids"] if i & 128} == {0, 1} for r in pairs(R))),
        ("yuva: Y live, A empty", "yuva-display-dense", PIC_P, lambda R: all(r["n_cols"] == 0 for r in single(R, "alpha")) and all(r["n_cols"] > 0 for r in single(R))),
        ("a wrong-tile scale changes a column: both tiles live, scales differ", DD, PIC_P, lambda R: any(
            any(d and tl for d, tl in zip(r["qia_differs"], r["qia_tile"])) for r in pairs(R)))]))

    def b(t):
        scatter(t, 144, planes=("coef_y", "coef_cb", "coef_cr", "coef_a"))
        t["coef_y"][:16, :128] = 0                                   # the first pair of the upper row: nothing live, has_right true
    C.append(Case("w144-left-only-second-task", 144, b, [
        ("a second task with only a left part", DD, PIC_P, lambda R: [r["has_right"] for r in pairs(R)] == [True, False] * 2 and all(
            r["blocks"] == 2 and r["n_cols"] > 0 for r in pairs(R)[1::2])),
        ("pair n_cols 0", DD, PIC_B, n_cols_are("pair", 0))]))

    def b(t):
        scatter(t, 81, planes=("coef_a",))
    C.append(Case("yuva-a-only", 80, b, [
        ("yuva: A live, Y empty", "yuva-display-sparse", PIC_B, lambda R: all(r["n_cols"] == 0 for r in single(R)) and all(r["n_cols"] > 0 for r in single(R, "alpha")))]))

    # -- rows_live and cols_live: every value, and the inputs at the edge of each short form ---------------------------------------
    def rows_case(name, ks):
        def b(t):
            cols = [0, 9, 18, 27, 64 + 36, 64 + 45, 64 + 54, 64 + 63, 3, 64 + 12]
            for Rt, k in enumerate(ks[:2]):
                put(t, Rt, cols, SIGN, rows=(0, k - 1))
            for Rt, k in enumerate(ks[2:]):
                put(t, Rt, sorted({i & ~4 for i in cols}), SIGN, rows=(0, k - 1), plane="chroma")      # four chroma blocks at this width
        first = lambda k: lambda R: any(r["n_rounds"] == 1 and r["rounds"][0]["rows_live"] == k and r["rounds"][0]["rows_live_active"] == k for r in R)
        only = lambda k: lambda R: any(r["n_rounds"] == 1 and r["rounds"][0]["rows"] == [0, k - 1] for r in R)
        C.append(Case(name, 64, b, [("rows_live %d in a first round" % k, DD, (PIC_I, PIC_P, PIC_B)[k % 3], first(k)) for k in ks] + [
            ("only rows 0 and %d live in a round" % (k - 1), PD, PIC_P, only(k)) for k in ks if k in (3, 4, 5)]))
    rows_case("rows-live-1-3-5-7", (1, 3, 5, 7))
    rows_case("rows-live-2-4-6-8", (2, 4, 6, 8))

    def b(t):
        for Rt, (k0, k1) in enumerate(((1, 3), (2, 5))):
            put(t, Rt, [b_ for b_ in (0, 3, 7)] + [8 * (k0 - 1) + b_ for b_ in (1, 3)], SIGN, rows=(0, 2))
            put(t, Rt, [64 + b_ for b_ in (2, 5)] + [64 + 8 * (k1 - 1) + b_ for b_ in (0, 6)], SIGN, rows=(1, 6))
        for Rt, (k0, k1) in enumerate(((4, 6), (7, 8))):
            put(t, Rt, [0, 2] + [8 * (k0 - 1) + 1], SIGN, rows=(0, 3), plane="chroma")
            put(t, Rt, [64 + 1] + [64 + 8 * (k1 - 1) + 3], SIGN, rows=(0, 4), plane="chroma")
    halves_of = lambda R: [h for r in R for h in r["halves"]]
    C.append(Case("cols-live-1-to-8", 64, b, [("cols_live %d" % k, DS, (PIC_I, PIC_P, PIC_B)[k % 3],
                                               (lambda k: lambda R: any(h["cols_live"] == k for h in halves_of(R)))(k)) for k in range(1, 9)] + [
        ("only columns 0 and %d live in a half" % (k - 1), PD, PIC_B, (lambda k: lambda R: any(h["cols"] == [0, k - 1] for h in halves_of(R)))(k))
        for k in (3, 4, 5)] + [
        ("the two halves of a task on different row-pass forms", PD, PIC_P, lambda R: {tuple(h["form"] for h in r["halves"]) for r in R} >= {
            ("lo2", "lo4"), ("lo2", "full"), ("lo4", "full")})]))

    def b(t):
        put(t, 0, [64 + 8 * c + b_ for c in (0, 5) for b_ in (1, 4)], SIGN, rows=(0, 3))        # luma: half 0 empty, half 1 live
        put(t, 1, [8 * c + b_ for c in (1, 7) for b_ in (0, 7)], SIGN, rows=(2,))               # half 0 live, half 1 empty
        put(t, 0, [64 + 8 * 2 + 1], SIGN, rows=(0, 1), plane="chroma")
        put(t, 1, [8 * 6 + 2], SIGN, rows=(4,), plane="chroma")
    forms = lambda R, kind: {tuple(h["form"] == "skip" for h in r["halves"]) for r in single(R, kind)}
    C.append(Case("empty-halves", 64, b, [
        ("colbits 0 in half 0 next to a live half 1", DS, PIC_P, lambda R: (True, False) in forms(R, "luma")),
        ("colbits 0 in half 1 next to a live half 0", DS, PIC_B, lambda R: (False, True) in forms(R, "luma")),
        ("chroma: Cb empty next to Cr", PD, PIC_P, lambda R: (True, False) in forms(R, "chroma")),
        ("chroma: Cr empty next to Cb", PD, PIC_B, lambda R: (False, True) in forms(R, "chroma"))]))

    # -- one coefficient at each of the 64 positions -------------------------------------------------------------------------------
    def b(t):
        for k in range(64):
            R, Q = k // 16, k % 16
            t["coef_y"][8 * R + (k >> 3), 8 * Q + (k & 7)] = (3 + k % 5) * (-1 if k % 3 == 0 else 1)
            if k < 16:
                R, Q = k // 8, k % 8
                t["coef_cb"][8 * R + (k >> 1), 8 * Q + 7 - (k & 7)] = 2 + k % 3
                t["coef_cr"][8 * R + 7 - (k >> 1), 8 * Q + (k & 7)] = -2 - k % 3
    C.append(Case("every-position", 128, b, [
        ("a single coefficient at each of the 64 positions", PD, PIC_I, lambda R: sum(r["n_cols"] for r in single(R)) == 64),
        ("an intra block with a level in row 0 of a column other than 0", PD, PIC_P, lambda R: any(
            any(lane for lane in r["dc_lane"]) and r["n_cols"] > sum(r["dc_lane"]) for r in single(R)))]))

    # -- magnitudes ----------------------------------------------------------------------------------------------------------------
    def b(t):
        t["intra"][:] = np.tile([255, 255, 255, 0], 2)              # the last macroblock column stays predicted
        t["qscale"][:] = 31
        t["coef_y"][9, 56 + 2] = 1
        for Q, (dc, ac) in enumerate(((-32768, -32768), (-1, 32767), (1, -32768), (32767, 32767), (32767, -32768), (-32768, 32767))):
            for Rb in (0, 3):
                t["coef_y"][8 * Rb, 8 * Q] = dc
                t["coef_y"][8 * Rb + 1:8 * Rb + 8, 8 * Q] = ac               # the largest ACs of the DC's own column
                t["coef_y"][8 * Rb + 1, 8 * Q + 1] = ac                      # and the largest product of all: 2047 * 62
        t["coef_cb"][0, 0], t["coef_cr"][8, 8] = 32767, -32768
    C.append(Case("dc-extremes", 64, b, [
        ("intra DC at -32768, -1, 1 and 32767 with the largest ACs", PD, PIC_I, lambda R: any(
            r["saturating"] > 0 and r["largest_col_final"] >= 32767 * 256 + 2047 * 44 for r in single(R))),
        ("each of the DCs -32768, -1, 1 and 32767 in a DC lane", PD, PIC_B, lambda R: any(sum(r["dc_lane"]) >= 6 for r in single(R)) and (
            lambda t: {-32768, -1, 1, 32767} <= set(t["coef_y"][::8, ::8][np.kron(t["intra"].reshape(2, -1), np.ones((2, 2), np.uint8)) != 0].tolist()))(
                BY_NAME["dc-extremes"].picture(PIC_B)))]))

    def b(t):
        t["intra"][:] = np.tile([255, 255, 255, 0], 2)              # the last macroblock column stays predicted
        t["qscale"][:] = 1
        y = t["coef_y"]
        y[0, 0], y[1, 0] = 319, 3                # level 3 -> 5, 319 * 256 + 5 * 44 = 81884: s = 32753.6, the largest below
        y[0, 8] = 320                            # 81920 * 0.4f = 32768.0 exactly: at the edge
        y[0, 16], y[0, 24] = -319, -320          # -32665.6 (floor -32666) and -32768.0
        put(t, 1, ALL0[:40], SIGN, rows=(1,))    # a round of small columns ...
        y[16, 8 * 5] = 400                       # ... in which exactly one lane is beyond: 40960 wraps to -24576
    C.append(Case("handoff-edge", 64, b, [
        ("a lane just below |s| = 32768 and a lane at it", PD, PIC_I, lambda R: any(
            r["saturating"] == 16 and 32750 < r["largest_below"] < 32768 and r["rounds"][0]["lanes_saturating"] == 2 for r in single(R))),
        ("a round in which exactly one lane is beyond |s| = 32768", PD, PIC_P, lambda R: any(
            r["rounds"] and r["rounds"][0]["active"] == 40 and r["rounds"][0]["lanes_saturating"] == 1 for r in single(R)))]))

    def b(t):
        t["intra"][:] = 0
        t["qscale"][:] = np.array([1, 5, 2, 1, 3, 4], np.uint8)
        y = t["coef_y"]
        for Q in range(6):
            for Rb in range(4):
                y[8 * Rb, 8 * Q + 1] = (1, -1, 2, -2)[(Q + Rb) % 4]       # Q[0][1] = 1: (2 l + 1) q / 16 floors to 0 -> +1 for q <= 5
                y[8 * Rb, 8 * Q + 3] = (2, -3, 4, -5)[(Q + Rb) % 4]       # Q = 16: even products step toward zero
        t["coef_cb"][0, 1], t["coef_cr"][8, 9] = 1, -1
    C.append(Case("oddify-w48", 48, b, [
        ("a non-intra product that floors to 0, in a round with rows_live 1", PD, PIC_P, lambda R: all(
            r["n_rounds"] == 1 and r["rounds"][0]["rows_live"] == 1 for r in R) and oddify_products(BY_NAME["oddify-w48"].picture(PIC_P)))]))

    # -- the sparse road's groups --------------------------------------------------------------------------------------------------
    def b(t):
        t["qscale"][:] = 2
        rng = np.random.default_rng(512)
        y = t["coef_y"]
        y[:8, :] = rng.choice([-2, -1, 1, 2], (8, 64))                         # 512 entries
        y[8:16, :].reshape(-1)[rng.choice(512, 65, replace=False)] = 1          # 65
        y[16:24, :].reshape(-1)[rng.choice(512, 64, replace=False)] = -1        # 64
        y[24 + 3, 8 * 5 + 2] = 2                                                # 1
    ent = lambda R: {n for r in R for n in r["entries"]}
    C.append(Case("sparse-groups", 64, b, [
        ("sparse groups of 0, 1, 64, 65 and 512 entries", "plain-sparse", PIC_P, lambda R: ent(R) >= {0, 1, 64, 65, 512} and {
            tr for r in R for tr in r["scatter_trips"]} >= {0, 1, 7})]))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
SATURATING = ("dc-extremes", "handoff-edge")      # the cases whose hand-off values leave the int16 range; no other case's do

# the edges the cases' predicates must cover between them (tests/test_recon_structure.py: a dropped case fails there)
ITEMS = (
    ["single n_cols %d" % n for n in (0, 1, 63, 64, 65, 127, 128)] +
    ["pair n_cols %d" % n for n in (0, 64, 65, 128, 129, 192, 193, 255, 256)] +
    ["live columns only in the right tile", "live columns only in the left tile", "live columns only in half 1", "live columns only in half 0",
     "column 0 live with a short last round", "column 0 dead with a short last round",
     "later round with a larger rows_live", "later round with a smaller rows_live"] +
    ["rows_live %d in a first round" % k for k in range(1, 9)] + ["only rows 0 and %d live in a round" % k for k in (2, 3, 4)] +
    ["only columns 0 and %d live in a half" % k for k in (2, 3, 4)] + ["each of the DCs -32768, -1, 1 and 32767 in a DC lane"] + ["cols_live %d" % k for k in range(1, 9)] +
    ["the two halves of a task on different row-pass forms",
     "colbits 0 in half 0 next to a live half 1", "colbits 0 in half 1 next to a live half 0", "chroma: Cb empty next to Cr", "chroma: Cr empty next to Cb",
     "a single coefficient at each of the 64 positions", "an intra block with a level in row 0 of a column other than 0",
     "intra DC at -32768, -1, 1 and 32767 with the largest ACs", "a lane just below |s| = 32768 and a lane at it",
     "a round in which exactly one lane is beyond |s| = 32768", "a non-intra product that floors to 0, in a round with rows_live 1",
     "sparse groups of 0, 1, 64, 65 and 512 entries", "yuva: A live, Y empty", "yuva: Y live, A empty",
     "a lone partial left part", "exactly one full left part", "a partial right part", "a full pair", "a second task with only a left part",
     "a right-tile column whose quantiser scale and intra flag differ from the left tile's",
     "a wrong-tile scale changes a column: both tiles live, scales differ", "Cb live, Cr empty", "Cb empty, Cr live",
     "pair: column 0 dead with a short last round", "pair: four full rounds, the id list filled to its last byte"])


@functools.lru_cache(maxsize=None)
def expected(name, ptype, alpha):
    """the oracle's picture of a case's form over references(): flat [Y | Cb | Cr (| A)]"""
    from oracle import oracle_py as O
    c = BY_NAME[name]
    t = c.picture(ptype)
    cw, n3 = c.width, c.width * HEIGHT * 3 // 2
    fwd, bwd = (r if alpha else r[:n3] for r in references(cw))
    return O.decode_picture(ptype, cw, HEIGHT, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"], repadd=t.get("repadd"),
                            mb_dir=t.get("mb_dir"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"), qm=QM,
                            ref_fwd=None if ptype == PIC_I else fwd, ref_bwd=bwd if ptype == PIC_B else None,
                            coef_a=t["coef_a"] if alpha else None)


@functools.lru_cache(maxsize=None)
def facts_of(name, ptype, road):
    c = BY_NAME[name]
    return task_facts(c.picture(ptype), c.width, HEIGHT, road, refs=references(c.width))
