"""GPU: dense P and B pictures through the fused display kernels whose tasks run ONE front -- the chroma tile and both luma
tiles scanned into one list of live columns, one column pass (recon_task FRONT3, leon_kernels.h) -- against the oracle: planes
where they are written and RGBA, equal.  The cases are the places where the one list can go wrong: a last chroma group without
a right part, a workgroup with idle waves and a cropped frame, the common dozen of live columns per part, a list that just
fills one round of the pass (64) and one that needs a second (65), parts without any live column, the full list (384 ids),
quantiser scale and intra flag differing from macroblock to macroblock, and a B launch with an odd number of pictures."""
import numpy as np
import pytest

from helpers import planes_flat
from test_fused_display_gpu import L, O, S, _check_fused_gop, _decode_oracle, _gop  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu


def _columns(rng, plane_rows, candidates, n):
    """n of the candidate columns (plane, first row, x) get one to three small non-zero coefficients"""
    for k in rng.choice(len(candidates), size=n, replace=False):
        plane, y0, x = candidates[k]
        rows = rng.choice(8, size=int(rng.integers(1, 4)), replace=False)
        plane_rows[plane][y0 + rows, x] = rng.choice([-3, -2, -1, 1, 2, 3], size=rows.size)


def _craft(rng, t, cw, ch, n_c, n_l, n_r):
    """replaces the coefficients of picture t: every task (8 macroblocks: a chroma tile, a left and a right luma tile) gets
    exactly n_c, n_l and n_r live columns (a right tile the picture does not have gets none)"""
    planes = {k: np.zeros_like(t[k]) for k in ("coef_y", "coef_cb", "coef_cr")}
    for Rt in range(ch // 16):
        for gc in range((cw // 16 + 7) // 8):
            chroma = [(p, 8 * Rt, x) for p in ("coef_cb", "coef_cr") for x in range(64 * gc, min(64 * gc + 64, cw // 2))]
            left = [("coef_y", 16 * Rt + 8 * h, x) for h in range(2) for x in range(128 * gc, min(128 * gc + 64, cw))]
            right = [("coef_y", 16 * Rt + 8 * h, x) for h in range(2) for x in range(128 * gc + 64, min(128 * gc + 128, cw))]
            for cand, n in ((chroma, n_c), (left, n_l), (right, n_r)):
                if cand:
                    assert n <= len(cand)
                    _columns(rng, planes, cand, n)
    t.update(planes)


def _live_columns(t, cw, ch):
    """live columns of every task of picture t, (chroma, left, right)"""
    out = []
    for Rt in range(ch // 16):
        for gc in range((cw // 16 + 7) // 8):
            c = sum(int((t[p][8 * Rt:8 * Rt + 8, 64 * gc:64 * gc + 64] != 0).any(axis=0).sum()) for p in ("coef_cb", "coef_cr"))
            lr = [sum(int((t["coef_y"][16 * Rt + 8 * h:16 * Rt + 8 * h + 8, 128 * gc + 64 * s:128 * gc + 64 * s + 64] != 0).any(axis=0).sum()) for h in range(2))
                  for s in range(2)]
            out.append((c, lr[0], lr[1]))
    return out


# name -> (coded and frame size, live columns per tile of every task or None for the generator's own coefficients)
CASES = {
    "192x64_last_group_without_right_part": ((192, 64, 192, 64), None),
    "320x48_frame_312x40_idle_waves_and_crop": ((320, 48, 312, 40), None),
    "a_dozen_per_part": ((256, 32, 256, 32), (12, 12, 12)),
    "64_columns_one_round": ((256, 32, 256, 32), (20, 22, 22)),
    "65_columns_second_round": ((256, 32, 256, 32), (21, 22, 22)),
    "chroma_live_luma_dead": ((256, 32, 256, 32), (30, 0, 0)),
    "luma_live_chroma_dead": ((256, 32, 256, 32), (0, 25, 27)),
    "every_coefficient_nonzero": ((256, 32, 256, 32), "full"),
    "scale_and_intra_per_macroblock": ((256, 48, 256, 48), "per_mb"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_single_front_equals_oracle(L, O, S, case):
    (cw, ch, fw, fh), cols = CASES[case]
    gop = S.gop_ibbp(6)                      # I B B P B B: both P and B kernels, B pictures one per launch (an odd count)
    rng = np.random.default_rng(sum(map(ord, case)))
    tens = _gop(S, rng, cw, ch, gop, in_picture=False, uncoded_frac=0.0 if cols == "per_mb" else 0.3)
    for ptype, disp, f, b in gop:
        t = tens[disp]
        if ptype == S.PIC_I:
            continue
        if isinstance(cols, tuple):
            _craft(rng, t, cw, ch, *cols)
            want = [(cols[0], cols[1], cols[2] if 128 * gc + 64 < cw else 0) for Rt in range(ch // 16) for gc in range((cw // 16 + 7) // 8)]
            assert _live_columns(t, cw, ch) == want
        elif cols == "full":
            for k in ("coef_y", "coef_cb", "coef_cr"):
                t[k] = rng.choice(np.array([-2, -1, 1, 2], dtype=t[k].dtype), size=t[k].shape)
            assert all(n == (128, 128, 128) for n in _live_columns(t, cw, ch))
        elif cols == "per_mb":
            nmb = (cw // 16) * (ch // 16)
            t["qscale"] = rng.integers(1, 32, size=nmb).astype(np.uint8)
            t["intra"] = np.where(rng.random(nmb) < 0.5, 255, 0).astype(np.uint8)
            t["repadd"] = t["intra"].copy()
            # every task has macroblocks of both kinds and more than one scale, and columns in all three tiles
            for Rt in range(ch // 16):
                row = slice(Rt * (cw // 16), Rt * (cw // 16) + 8)
                assert len(set(t["qscale"][row])) > 1 and 0 < int((t["intra"][row] != 0).sum()) < 8
            assert all(min(n) > 0 for n in _live_columns(t, cw, ch))
    _check_fused_gop(L, O, S, (cw, ch, fw, fh), False, gop, tens)


def test_b_launch_with_three_pictures(L, O, S):
    """one device batch of three B pictures behind their anchors: the workgroups of B pictures alternate in pairs (pic_of_wg), the
    third picture's partner is idle"""
    import torch
    cw, ch = 192, 64
    gop = S.gop_ibbp(6)
    rng = np.random.default_rng(333)
    tens = _gop(S, rng, cw, ch, gop, in_picture=False)
    exp = _decode_oracle(O, cw, ch, gop, tens)
    dec = L.Decoder(cw, ch, n_slots=7)
    try:
        rgba = torch.zeros((6, ch, cw, 4), dtype=torch.uint8, device="cuda")
        keep, batch = [], []
        dev = lambda a: None if a is None else (keep.append(torch.from_numpy(np.ascontiguousarray(a)).cuda()), keep[-1].data_ptr())[1]
        for ptype, disp, f, b in gop:
            t = tens[disp]
            fwd = f if f is not None else b
            kw = dict(ref_fwd_slot=-1 if fwd is None else fwd, ref_bwd_slot=-1 if b is None else b, rgba_out=rgba[disp].data_ptr())
            if ptype != S.PIC_B:
                dec.submit_picture(L.make_picture(ptype, disp, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"], repadd=t.get("repadd"),
                                                  mv_fwd=t.get("mv_fwd"), keep=keep, **kw))
            elif len(batch) < 3:
                batch.append(L.make_picture(ptype, disp, dev(t["coef_y"]), dev(t["coef_cb"]), dev(t["coef_cr"]), dev(t["qscale"]), dev(t["intra"]),
                                            repadd=dev(t["repadd"]), mv_fwd=dev(t["mv_fwd"]), mv_bwd=dev(t["mv_bwd"]), mb_dir=dev(t["mb_dir"]),
                                            device=True, no_planes=True, **kw))
        assert len(batch) == 3
        dec.submit_batch(batch, L.MEM_DEVICE)
        dec.sync()
        got = rgba.cpu().numpy()
        for p in batch:
            disp = p.out_slot
            y, cb, cr = O.split_planes(exp[disp], cw, ch)
            assert np.array_equal(got[disp], O.ycbcr_to_rgba(y, cb, cr, cw, cw, ch, "cpu")), "RGBA of B picture %d" % disp
        for disp in (2, 5):
            assert np.array_equal(planes_flat(*dec.read_planes(disp)), exp[disp])
    finally:
        dec.close()
