"""GPU: what a pipeline and a decoder own comes and goes with them (csrc/leon_owned.h), cycle after cycle in one process.  Each test
makes, uses and closes its object four times; every cycle must deliver the first cycle's bytes, and the contiguous pool must have as
much handed out after a close as before the cycle began.  Nothing here provokes a failure: the paths are the ordinary ones, among them
those that make resources at first use (the regions stream and scratch, the device roads' events and staging, the conversion stream and
its events, a staging entry, the timing events) and one that grows a scratch buffer inside a live pipeline."""
import os

import numpy as np
import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu

CYCLES = 4
STREAM = os.path.join(ROOT, "tests", "golden", "streams", "slices5_ip_96x64.jsv")
SMALL, LARGE = (13, 37), (64, 64)          # (h, w) of the two regions calls
PAD = (114, 7, 250)
MIB = 1 << 20


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def table_words(L, fw, fh, box, size):
    """int32 words of a region's tables as the host road lays them out (resize_tables_layout): first | count | W of both axes, rows of
    the region's largest tap counts, the rows of Wx an odd number of words"""
    _, x, y, w, h = box
    tx = int(L.resize_weights(fw, x, w, size[1])[1].max()) | 1
    ty = int(L.resize_weights(fh, y, h, size[0])[1].max())
    return 2 * size[1] + size[1] * tx + 2 * size[0] + size[0] * ty


def boxes_past_the_first_mib(L, fw, fh, first):
    """`first`, then whole-frame boxes of alternating frames until [descriptors | tables] of the call pass 1 MiB, the size the regions
    scratch starts at, and a few more: the call has to grow the scratch"""
    boxes, words = list(first), sum(table_words(L, fw, fh, b, LARGE) for b in first)
    per_filler = table_words(L, fw, fh, (0, 0, 0, fw, fh), LARGE)
    upload = lambda n, w: (64 * n + 255) // 256 * 256 + 4 * w
    while upload(len(boxes), words) <= MIB:
        boxes.append((len(boxes) & 1, 0, 0, fw, fh))
        words += per_filler
    return boxes + [(i & 1, 0, 0, fw, fh) for i in range(8)]


def pipeline_cycle(L, data, gpu_parser):
    """one pipeline from create to close: {what: bytes} of everything it delivered and of the calls made in its callback"""
    import torch
    got = {}

    def on_window(window, frames):
        fl = list(frames)
        p = fl[0]["_pipe"]
        fw, fh = p.info.frame_width, p.info.frame_height
        for f in fl:
            key = (window, f["gop"], f["display_index"])
            got[("rgba",) + key] = L.read_frame(f)
            got[("planes",) + key] = np.concatenate([a.ravel() for a in p.read_planes(f)])
            got[("tensor",) + key] = p.read_tensor(f)
        assert len(fl) >= 2
        two = [(0, 8, 4, 60, 40), (1, 30, 10, 40, 30)]
        got[("small", window)] = p.read_regions(window, two, SMALL)
        many = boxes_past_the_first_mib(L, fw, fh, two)
        large = p.read_regions(window, many, LARGE)          # grows the regions scratch of the live pipeline
        got[("large", window)] = large
        got[("large's first two", window)] = large[:2].copy()
        got[("two at the large size", window)] = p.read_regions(window, two, LARGE)
        got[("small again", window)] = p.read_regions(window, two, SMALL)
        m = L.warp_matrix_rotated_box(fw / 2.0, fh / 2.0, 40, 24, 30, (24, 40))
        got[("warp", window)] = p.read_warp_regions(window, [(1, m)], (24, 40), PAD)
        side = torch.cuda.Stream()
        dev_boxes = torch.tensor(two, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        batch, status = p.resample_regions_device(window, dev_boxes, SMALL, stream=side)
        side.synchronize()
        got[("device road", window)] = batch.cpu().numpy()
        got[("device status", window)] = status.cpu().numpy()
    pipe = L.Pipeline(data, parser_threads=2, gops_per_window=2, gpu_parser=gpu_parser, on_window=on_window, output="all", tensor_dtype="uint8",
                      tensor_layout="hwc")
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
    finally:
        pipe.close()
    return got


def assert_same_bytes(got, want, what):
    assert sorted(got, key=repr) == sorted(want, key=repr), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def test_pipeline_cycles_deliver_the_same_bytes_and_return_the_pool(L):
    """Test A.  Four pipelines in turn, output "all" with uint8 HWC tensors, the slice layer parsed on the GPU and on the host
    alternately.  The regions of the large call are (64, 64) tensors where the small call's are (13, 37): its first two boxes are
    the small call's, and its first two tensors are compared with a call of those two boxes alone at the large size."""
    data = open(STREAM, "rb").read()
    first = None
    for cycle in range(CYCLES):
        before = L.pool_stats()["in_use_bytes"]
        got = pipeline_cycle(L, data, gpu_parser=cycle % 2 == 0)
        assert L.pool_stats()["in_use_bytes"] == before, "cycle %d: the pool has %d bytes handed out after close, %d before the cycle" % (
            cycle, L.pool_stats()["in_use_bytes"], before)
        windows = sorted(k[1] for k in got if k[0] == "small")
        assert windows and any(k[0] == "rgba" for k in got)
        for w in windows:
            assert np.array_equal(got[("large's first two", w)], got[("two at the large size", w)]), (cycle, w)
            assert np.array_equal(got[("small again", w)], got[("small", w)]), (cycle, w)
            assert np.array_equal(got[("device road", w)], got[("small", w)]) and (got[("device status", w)] == 0).all(), (cycle, w)
            assert got[("large", w)].nbytes > MIB and got[("small", w)].shape == (2,) + SMALL + (3,)
        # window ids count on inside a pipeline only: every cycle's keys are the first cycle's
        if first is None:
            first = got
        else:
            assert_same_bytes(got, first, "cycle %d against cycle 0" % cycle)


def decoder_cycle(L, S, pics):
    """one decoder from create to close: the host-memory I picture (a staging entry), the P picture as a device batch that writes its
    slot and a fused RGBA frame, the B picture as a prepared batch, conversions to the host and (on the conversion stream) to the device"""
    import torch
    cw, ch = 96, 64
    dec = L.Decoder(cw, ch, n_slots=13, device_id=0)
    out, keep = {}, []
    try:
        dec.set_overlap_convert(True)
        dec.timing_enable(True)
        (ti, si, _, _), (tp, sp, fp, _), (tb, sb, fb, bb) = pics
        dec.submit_picture(L.make_picture(S.PIC_I, si, ti["coef_y"], ti["coef_cb"], ti["coef_cr"], ti["qscale"], ti["intra"], keep=keep))

        def on_device(t):
            d = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int16 if k.startswith(("coef", "mv")) else np.uint8)).cuda()
                 for k, v in t.items() if isinstance(v, np.ndarray)}
            keep.append(d)
            return {k: v.data_ptr() for k, v in d.items()}
        frame = torch.zeros((ch, cw, 4), dtype=torch.uint8, device="cuda")
        d = on_device(tp)
        torch.cuda.synchronize()
        dec.submit_batch([L.make_picture(S.PIC_P, sp, d["coef_y"], d["coef_cb"], d["coef_cr"], d["qscale"], d["intra"], repadd=d["repadd"], mv_fwd=d["mv_fwd"],
                                         ref_fwd_slot=fp, device=True, rgba_out=frame.data_ptr())], L.MEM_DEVICE)
        d = on_device(tb)
        torch.cuda.synchronize()
        b = dec.batch_create([L.make_picture(S.PIC_B, sb, d["coef_y"], d["coef_cb"], d["coef_cr"], d["qscale"], d["intra"], repadd=d["repadd"], mv_fwd=d["mv_fwd"],
                                             mv_bwd=d["mv_bwd"], mb_dir=d["mb_dir"], ref_fwd_slot=fb, ref_bwd_slot=bb, device=True)])
        dec.batch_run(b)
        dec.batch_destroy(b)
        out["rgba of P to the host"] = dec.convert_rgba(sp)
        both = torch.zeros((2, ch, cw, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dec.convert_rgba_batch([sb, si], both.data_ptr())          # on the conversion stream, behind the reconstruction
        dec.sync()
        out["rgba of B and I on the device"] = both.cpu().numpy()
        out["fused frame of P"] = frame.cpu().numpy()
        for name, slot in (("I", si), ("P", sp), ("B", sb)):
            out["planes of " + name] = np.concatenate([a.ravel() for a in dec.read_planes(slot)])
        out["timed launches"] = np.asarray([dec.timing_get(0)["launches"], dec.timing_get(1)["launches"]])
        dec.timing_reset()
        assert dec.timing_get(0)["launches"] == 0
        # the yardsticks' buffers and events are temporaries of the call (1 MiB each: from the contiguous pool, and back)
        assert dec.measure_copy_bandwidth(MIB, 1) > 0 and dec.measure_stream_bandwidth(MIB, 1, reads=2, writes=2) > 0
    finally:
        dec.close()
    return out


def test_decoder_cycles_equal_the_oracle_and_return_the_pool(L):
    """Test B.  (The decoder's own calls have no frame-planes output -- only a pipeline sets one, and Test A's pipelines do: the
    device batch here writes a fused RGBA frame beside its slot.)"""
    import synth as S
    from oracle import oracle_py as O
    cw, ch = 96, 64
    rng = np.random.default_rng(123)
    pics, planes = [], {}
    for ptype, slot, f, b in [(S.PIC_I, 0, None, None), (S.PIC_P, 2, 0, None), (S.PIC_B, 1, 0, 2)]:
        t = S.make_picture(rng, cw, ch, ptype)
        pics.append((t, slot, f, b))
        planes[slot] = O.decode_picture(ptype, cw, ch, t["coef_y"], t["coef_cb"], t["coef_cr"], t["qscale"], t["intra"], repadd=t.get("repadd"),
                                        mb_dir=t.get("mb_dir"), mv_fwd=t.get("mv_fwd"), mv_bwd=t.get("mv_bwd"), ref_fwd=planes.get(f), ref_bwd=planes.get(b))
    rgba = {slot: O.ycbcr_to_rgba(*O.split_planes(p, cw, ch), cw, cw, ch, "cpu") for slot, p in planes.items()}
    want = {"rgba of P to the host": rgba[2], "rgba of B and I on the device": np.stack([rgba[1], rgba[0]]), "fused frame of P": rgba[2],
            "planes of I": planes[0], "planes of P": planes[2], "planes of B": planes[1]}
    first = None
    for cycle in range(CYCLES):
        before = L.pool_stats()["in_use_bytes"]
        got = decoder_cycle(L, S, pics)
        assert L.pool_stats()["in_use_bytes"] == before, cycle
        launches = got.pop("timed launches")
        assert launches[0] == 3 and launches[1] == 2, launches          # I, P, B reconstructed; two conversions
        for k, w in want.items():
            assert got[k].shape == w.shape and np.array_equal(got[k], w), (cycle, k)
        if first is None:
            first = got
        else:
            assert_same_bytes(got, first, "cycle %d against cycle 0" % cycle)
