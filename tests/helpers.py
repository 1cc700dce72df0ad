"""Shared test plumbing: run the same boundary tensors through the oracle (CPU) and
through libleon_hip.so (C ABI, GPU) and compare planes bit for bit."""
import base64
import json
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def b64(s, dtype=np.uint8):
    return np.frombuffer(base64.b64decode(s), dtype=dtype)


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def oracle_decode_sequence(O, cw, ch, pics, refs, qm=None):
    """pics: list of tensors dicts in coded order, each with keys 'slot', 'ref_fwd', 'ref_bwd'
    (indices into the `out` dict).  Returns {slot: flat [Y|Cb|Cr] uint8}."""
    out = dict(refs)
    for t in pics:
        out[t["slot"]] = O.decode_picture(
            t["type"], cw, ch, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"],
            repadd=t.get("repadd"), mb_dir=t.get("mb_dir"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"),
            qm=qm, ref_fwd=None if t.get("ref_fwd") is None else out[t["ref_fwd"]],
            ref_bwd=None if t.get("ref_bwd") is None else out[t["ref_bwd"]])
    return out


def hip_submit(L, dec, t, keep, rgba_out=None):
    """rgba_out (a device pointer): the fused path, k_recon_display -- planes AND the RGBA frame from one launch"""
    extra = {} if rgba_out is None else dict(rgba_out=rgba_out, no_planes=False)
    p = L.make_picture(t["type"], t["slot"], t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"],
                       repadd=t.get("repadd"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"),
                       mb_dir=t.get("mb_dir"),
                       ref_fwd_slot=-1 if t.get("ref_fwd") is None else t["ref_fwd"],
                       ref_bwd_slot=-1 if t.get("ref_bwd") is None else t["ref_bwd"], keep=keep, **extra)
    dec.submit_picture(p)


def planes_flat(y, cb, cr):
    return np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])


def hip_submit_sparse(L, dec, t, keep, cw, ch, rgba_out=None):
    """The same picture through the sparse boundary (include/leon_vlc.h lists)."""
    extra = {} if rgba_out is None else dict(rgba_out=rgba_out, no_planes=False)
    import leon_vlc_ctypes as V
    if "grp_off" in t and t.get("entries") is not None:
        grp_off, entries = t["grp_off"], t["entries"]
    else:
        grp_off, entries = V.sparsify(t["coef_y"], t["coef_cb"], t["coef_cr"], cw, ch)
    p = L.make_sparse_picture(t["type"], t["slot"], grp_off, entries, len(entries), t["qscale"], t["intra"],
                              repadd=t.get("repadd"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"),
                              mb_dir=t.get("mb_dir"),
                              ref_fwd_slot=-1 if t.get("ref_fwd") is None else t["ref_fwd"],
                              ref_bwd_slot=-1 if t.get("ref_bwd") is None else t["ref_bwd"], keep=keep, **extra)
    dec.submit_sparse([p], L.MEM_HOST)


# ---- the tensors handed to tools/jsv_writer.py as the reference of whatever parses its stream ------------------------------

def stream_carried_masks(t, cw, ch):
    """{tensor name: boolean mask over its entries} -- the entries of a written picture `t` that its STREAM carries, i.e.
    where a parser's output has to equal what went into the writer.  Everything else a parser reports is state it keeps,
    not something the stream says, and no decoder reads it:
      coefficients   all of them: a block that is not coded is a block of zeros on both sides
      intra          coded macroblocks: a skipped one has no macroblock_type; the parsers leave the map entry of the
                     picture before in place there (as the reference does, decoders/jsv.js:794-795), and with no
                     coefficients the flag changes nothing
      repadd         all of it (cleared per picture, 255 at intra macroblocks outside I pictures)
      mv_fwd         P: non-intra macroblocks (a skipped one has the zero vector it was reset to); B: where mb_dir has the
                     forward bit -- a macroblock predicted backward only keeps the forward PREDICTOR in that entry
      mv_bwd         B: where mb_dir has the backward bit, for the same reason
      mb_dir         B: non-intra macroblocks (an intra one has no direction; the parsers write 0)
      qscale         macroblocks with at least one coded block: macroblock_quant exists only together with a pattern or
                     intra, so a macroblock of vectors alone cannot change the scale and inherits the one in force --
                     which no dequantiser then uses"""
    mbw, mbh = cw // 16, ch // 16
    nmb = mbw * mbh
    ptype = t["type"]
    intra = np.asarray(t["intra"]).astype(bool)

    def mb_any(plane, n):
        return np.asarray(plane).reshape(mbh, n, mbw, n).transpose(0, 2, 1, 3).reshape(nmb, -1).any(axis=1)
    pattern = intra | mb_any(t["coef_y"], 16) | mb_any(t["coef_cb"], 8) | mb_any(t["coef_cr"], 8)
    coded = pattern | mb_any(t["coef_a"], 16) if "coef_a" in t else pattern
    m = {k: np.ones(np.asarray(t[k]).shape, bool) for k in ("coef_y", "coef_cb", "coef_cr", "coef_a") if k in t}
    m["qscale"] = pattern                              # (the alpha_pattern of a yuva stream brings no macroblock_quant with it)
    if ptype == 1:
        m["intra"] = np.ones(nmb, bool)
        return m
    m["repadd"] = np.ones(nmb, bool)
    if ptype == 2:
        zero_mv = ~np.asarray(t["mv_fwd"]).reshape(-1, 2).any(axis=1)
        m["intra"] = coded | ~zero_mv                  # every macroblock that is not skipped (the first and last of a slice
        m["mv_fwd"] = np.repeat(~intra, 2)             # never are, but a test need not know the slices: they agree anyway)
        return m
    d = np.asarray(t["mb_dir"])
    # B: a macroblock without coefficients is skipped at most when it repeats the direction and both vectors of the one
    # before it; one that does not is coded whatever the slices are, and both sides say non-intra there
    state = np.concatenate([d.reshape(-1, 1), np.asarray(t["mv_fwd"]).reshape(-1, 2), np.asarray(t["mv_bwd"]).reshape(-1, 2)], axis=1)
    repeats = np.zeros(nmb, bool)
    repeats[1:] = (state[1:] == state[:-1]).all(axis=1) & ~intra[:-1]
    m["intra"] = coded | ~repeats
    m["mb_dir"] = ~intra
    m["mv_fwd"] = np.repeat(~intra & ((d & 1) != 0), 2)
    m["mv_bwd"] = np.repeat(~intra & ((d & 2) != 0), 2)
    return m


def oracle_frames_from_tensors(pics, cw, ch, fw=None, fh=None, gop_starts=(0,), qm=None):
    """{(gop, display_index): {"planes": (Y, Cb, Cr[, A]) cropped to the frame, "rgba": RGBA}} by running the oracle on the
    tensors that were handed to the writer (pics, coded order, each with "display"): the reference bookkeeping of
    oracle_frames (tests/test_pipeline_gpu.py), and no parser anywhere."""
    from oracle import oracle_py as O
    fw, fh = fw or cw, fh or ch
    out, gop, older, newer = {}, -1, None, None
    n3 = cw * ch * 3 // 2
    for i, t in enumerate(pics):
        if i in gop_starts:
            gop += 1
            older = newer = None
        fwd = bwd = None
        if t["type"] == 2:
            fwd = newer
        elif t["type"] == 3:
            bwd, fwd = newer, (older if older is not None else newer)
        planes = O.decode_picture(t["type"], cw, ch, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"],
                                  repadd=t.get("repadd"), mb_dir=t.get("mb_dir"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"),
                                  qm=qm, ref_fwd=fwd, ref_bwd=bwd, coef_a=t.get("coef_a"))
        if t["type"] != 3:
            older, newer = newer, planes
        y, cb, cr = O.split_planes(planes[:n3], cw, ch)
        a = planes[n3:] if t.get("coef_a") is not None else None
        cwid, chh = (fw + 1) // 2, (fh + 1) // 2
        crop = [y[:fh, :fw], cb[:chh, :cwid], cr[:chh, :cwid]] + ([a.reshape(ch, cw)[:fh, :fw]] if a is not None else [])
        out[(gop, t["display"])] = {"planes": tuple(np.ascontiguousarray(p) for p in crop),
                                    "rgba": O.ycbcr_to_rgba(y, cb, cr, cw, fw, fh, "cpu", a=a)}
    return out
