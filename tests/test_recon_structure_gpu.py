"""GPU: the reconstruction kernels (k_recon, k_recon_display, dense and sparse, yuva) at the pictures of tests/recon_structure.py --
every length of the live-column list, every butterfly form of both passes, both tiles of the pair front, the scatter loop's trips, the
hand-off's int16 edge -- each case on each road, bit for bit against the oracle.  k_recon_display_out is reached through the pipeline:
the cases a stream can carry (recon_structure.stream), one stream per width, with planes and with tensor output.
tests/test_recon_structure.py shows on the CPU that the cases reach those edges.  One decoder per (width, road): all pictures of the road are submitted before its one sync."""
import numpy as np
import pytest

import recon_structure as R
from recon_structure import CASES, HEIGHT, PIC_B, PIC_I, PIC_P, ROADS

pytestmark = pytest.mark.gpu
TYPES = (PIC_I, PIC_P, PIC_B)
MARKER = 0xA5


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    oracle_py.lib()
    return oracle_py


def _run_road(L, O, cw, road):
    """{(case name, type): {"planes": flat [Y | Cb | Cr (| A)], "rgba": the fused frame or the converted slot}}"""
    import torch
    import leon_vlc_ctypes as V
    f = R.road_flags(road)
    ch, alpha = HEIGHT, f["alpha"]
    cases = [c for c in CASES if c.width == cw]
    n, n3 = cw * ch, cw * ch * 3 // 2
    dec = L.Decoder(cw, ch, n_slots=2 + 3 * len(cases), alpha=alpha)
    try:
        dec.set_quant_matrices(R.QM[:64], R.QM[64:])
        for slot, ref in enumerate(R.references(cw)):
            dec.write_planes(slot, *O.split_planes(ref[:n3], cw, ch))
            if alpha:
                dec.write_alpha_plane(slot, ref[n3:].reshape(ch, cw))
        frames = torch.zeros((3 * len(cases), ch, cw, 4), dtype=torch.uint8, device="cuda") if f["display"] else None
        keep, slots = [], {}
        for k, (c, ptype) in enumerate((c, t) for c in cases for t in TYPES):
            t = c.picture(ptype)
            slot = slots[(c.name, ptype)] = 2 + k
            no_planes = f["display"] and ptype == PIC_B
            if no_planes:          # a display B picture writes no planes: the marker must stay
                mark = np.full(n3, MARKER, np.uint8)
                dec.write_planes(slot, *O.split_planes(mark, cw, ch))
                if alpha:
                    dec.write_alpha_plane(slot, np.full((ch, cw), MARKER, np.uint8))
            kw = dict(repadd=t.get("repadd"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"), mb_dir=t.get("mb_dir"),
                      ref_fwd_slot=-1 if ptype == PIC_I else 0, ref_bwd_slot=1 if ptype == PIC_B else -1, keep=keep)
            if f["display"]:
                kw.update(rgba_out=frames[k].data_ptr(), no_planes=no_planes)
            if f["sparse"]:
                go, en = V.sparsify(t["coef_y"], t["coef_cb"], t["coef_cr"], cw, ch, coef_a=t["coef_a"] if alpha else None)
                dec.submit_sparse([L.make_sparse_picture(ptype, slot, go, en, len(en), t["qscale"], t["intra"], **kw)], L.MEM_HOST)
            else:
                if alpha:
                    kw["coef_a"] = t["coef_a"]
                dec.submit_picture(L.make_picture(ptype, slot, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"], **kw))
        dec.sync()
        got_frames = frames.cpu().numpy() if f["display"] else None
        out = {}
        for k, key in enumerate(slots):
            planes = [p.ravel() for p in dec.read_planes(slots[key])] + ([dec.read_alpha_plane(slots[key]).ravel()] if alpha else [])
            rgba = got_frames[k] if f["display"] else (dec.convert_rgba(slots[key]) if alpha else None)
            out[key] = {"planes": np.concatenate(planes), "rgba": rgba}
        return out
    finally:
        dec.close()


@pytest.fixture(scope="module")
def runs(L, O):
    made = {}

    def get(cw, road):
        if (cw, road) not in made:
            made[(cw, road)] = _run_road(L, O, cw, road)
        return made[(cw, road)]
    return get


def _where(cw, i):
    """flat sample index -> (plane, y, x)"""
    n = cw * HEIGHT
    for name, start, W in (("y", 0, cw), ("cb", n, cw // 2), ("cr", n + n // 4, cw // 2), ("a", n + n // 2, cw)):
        size = n if name in ("y", "a") else n // 4
        if i < start + size:
            return name, (i - start) // W, (i - start) % W
    raise IndexError(i)


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(L, O, runs, case, road):
    f = R.road_flags(road)
    cw, ch, alpha = case.width, HEIGHT, f["alpha"]
    n3 = cw * ch * 3 // 2
    got = runs(cw, road)
    for ptype in TYPES:
        want = R.expected(case.name, ptype, alpha)
        have = got[(case.name, ptype)]
        if f["display"] and ptype == PIC_B:
            assert (have["planes"] == MARKER).all(), "%s %s: a no_planes picture wrote its planes" % (case.name, road)
        else:
            bad = np.nonzero(have["planes"] != want)[0]
            if bad.size:
                plane, y, x = _where(cw, int(bad[0]))
                rec = R.owner(R.facts_of(case.name, ptype, road), plane, y, x)
                pytest.fail("%s %s type %d: %d samples differ, first in plane %s at row %d col %d: got %d, oracle %d; its front: %s" % (
                    case.name, road, ptype, bad.size, plane, y, x, have["planes"][bad[0]], want[bad[0]], R.brief(rec)))
        if have["rgba"] is not None:
            rgba = O.ycbcr_to_rgba(*O.split_planes(want[:n3], cw, ch), cw, cw, ch, "cpu", a=want[n3:] if alpha else None)
            bad = np.argwhere(have["rgba"] != rgba)
            if bad.size:
                y, x, comp = (int(v) for v in bad[0])
                # R, G and B come from the pixel's Y and from its quad's Cb and Cr: the fronts of both; the A byte from the A front
                recs = R.facts_of(case.name, ptype, road)
                fronts = [("a", R.owner(recs, "a", y, x))] if comp == 3 else [("y", R.owner(recs, "y", y, x)), ("cb/cr", R.owner(recs, "cb", y // 2, x // 2))]
                pytest.fail("%s %s type %d: %d RGBA bytes differ, first at row %d col %d component %d: got %d, oracle %d; the fronts behind it: %s" % (
                    case.name, road, ptype, len(bad), y, x, comp, have["rgba"][y, x, comp], rgba[y, x, comp],
                    [(n, R.brief(r) if r else None) for n, r in fronts]))


# ---- k_recon_display_out: the codable cases as streams through the pipeline -------------------------------------------------------

@pytest.fixture(scope="module")
def stream_frames():
    """width -> (stream bytes, {(gop, display index): the oracle's planes and RGBA of the WRITTEN tensors}, case names)"""
    from helpers import oracle_frames_from_tensors
    made = {}

    def get(cw):
        if cw not in made:
            data, pics, starts, names = R.stream(cw)
            made[cw] = (data, oracle_frames_from_tensors(pics, cw, HEIGHT, gop_starts=starts, qm=R.QM), names)
        return made[cw]
    return get


PARSERS = pytest.mark.parametrize("gpu_parser", [True, False], ids=["gpu-parser", "host-parser"])


@PARSERS
@pytest.mark.parametrize("output", ["ycbcr", "both"])
@pytest.mark.parametrize("cw", R.WIDTHS)
def test_streams_planes_output(L, stream_frames, cw, output, gpu_parser):
    from test_pipeline_planes_gpu import run_planes
    data, want, names = stream_frames(cw)
    got, rgba, _ = run_planes(L, data, output, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)
    assert set(got) == set(want)
    for (gop, disp) in sorted(want):
        for name, g, w in zip(("Y", "Cb", "Cr"), got[(gop, disp)], want[(gop, disp)]["planes"]):
            bad = np.argwhere(g != w)
            assert bad.size == 0, "%s (GOP %d) display %d: plane %s differs in %d samples, first at %s" % (names[gop], gop, disp, name, len(bad), bad[0])
        if output == "both":
            assert np.array_equal(rgba[(gop, disp)], want[(gop, disp)]["rgba"]), "%s (GOP %d) display %d: RGBA" % (names[gop], gop, disp)


@PARSERS
@pytest.mark.parametrize("cw", R.WIDTHS)
def test_streams_tensor_output(L, stream_frames, cw, gpu_parser):
    from test_pipeline_tensor_format_gpu import assert_tensors, expected, run_format
    data, want, names = stream_frames(cw)
    exp = expected(L, {k: v["rgba"] for k, v in want.items()}, "uint8", "hwc")
    got = run_format(L, data, "uint8", "hwc", parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser)[0]
    assert_tensors(got, exp, "width %d: %s" % (cw, names))
