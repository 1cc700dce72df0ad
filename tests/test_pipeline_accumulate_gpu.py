"""GPU: motion and residual accumulated along the chains of delivered windows (include/leon_pipeline.h, leon_pipeline_accumulate;
k_accumulate) -- for every delivered frame of a window, with random accumulators in the reference slots: the host road, the device
road on a caller's stream and the device road on the pipeline's own stream, all three exactly equal to leon_ctypes.accumulate_hop (the
header's text in numpy integers) on what read_motion and read_residual give.  Then the chain a user runs: accumulate_gop against the
same hops done on the host, with the invariant of the displacement on every frame.  Then the refusals of the whole call.  Last the
decoder's own reconstruction as the oracle: in a stream without intra macroblocks in its P and B pictures, with one direction per B
picture, full-pel vectors and coded residual, I_luma[y + AY][x + AX] + RY[y][x] IS the delivered luma of every frame, in every sample."""
import ctypes as C
import functools

import numpy as np
import pytest

import accumulate_cases as A
from test_open_gop import open_stream
from test_pipeline_carry_gpu import run_windows
from test_pipeline_gpu import ibbp_stream
from test_pipeline_motion_gpu import stream

pytestmark = pytest.mark.gpu

PARSERS = pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def coded(pipe):
    return pipe.info.coded_width, pipe.info.coded_height


def accumulate_window(L, pipe, window, frames, roads=("host", "stream", "null"), parts_list=A.PARTS):
    """everything of one delivered window: every frame as a target, with both reference slots, with the forward one alone and with
    the backward one alone, then two refused hops, on each road"""
    import torch
    n = len(frames)
    cw, ch = coded(pipe)
    motion = [pipe.read_motion(window, i)[:2] for i in range(n)]
    residual = [pipe.read_residual(window, i) for i in range(n)]
    r = dict(n=n, keys=[(f["gop"], f["display_index"], f["type"]) for f in frames], runs=[])
    # slots 0 and 1: the references; 2 + 3 i .. 4 + 3 i: frame i's accumulator with both, forward only, backward only
    hops = [h for i in range(n) for h in ((i, 2 + 3 * i, 0, 1), (i, 3 + 3 * i, 0, -1), (i, 4 + 3 * i, -1, 1))] + [(n, 2, 0, 1), (0, 2, 2, 1)]
    full = L._records_array(hops)
    for parts in parts_list:
        c = dict(what="window %d, parts %d" % (window, parts), cw=cw, ch=ch, parts=parts, motion=motion, residual=residual, hops=hops,
                 buf=A.slots(L, np.random.default_rng(window * 10 + parts), cw, ch, parts, 2 + 3 * n, gap=4 if parts == 2 else 0))
        run = dict(case=c, want=A.expected(L, c))
        if "host" in roads:
            buf = c["buf"].copy()
            via, status = pipe.accumulate(window, buf, hops, parts, via_fill=A.VIA_FILL)
            run["host"] = (buf, via, status)

        def tensors():
            return (torch.from_numpy(c["buf"].copy()).cuda(), torch.tensor(full, dtype=torch.int32, device="cuda"),
                    torch.full((len(hops), ch // 16, cw // 16), A.VIA_FILL, dtype=torch.uint8, device="cuda"), torch.full((len(hops),), A.STATUS_FILL, dtype=torch.int32, device="cuda"))
        if "stream" in roads:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                s, h, via, status = tensors()
                got = pipe.accumulate_device(window, s, h, parts, via=via, status=status)
                assert got[0].data_ptr() == via.data_ptr() and got[1].data_ptr() == status.data_ptr()
            st.synchronize()
            run["stream"] = (s.cpu().numpy(), via.cpu().numpy(), status.cpu().numpy())
        if "null" in roads:          # stream NULL: the pipeline's regions stream, and the call waits
            s, h, via, status = tensors()
            torch.cuda.synchronize()
            cfg = L._accumulate_config(c["buf"], parts)
            call = L.PipelineAccumulateCall(h.data_ptr(), len(hops), 0, s.data_ptr(), via.data_ptr(), status.data_ptr(), None)
            assert pipe.lib.leon_pipeline_accumulate_device(pipe.h, window, C.byref(cfg), C.byref(call)) == L.OK, pipe.lib.leon_last_error()
            run["null"] = (s.cpu().numpy(), via.cpu().numpy(), status.cpu().numpy())
        r["runs"].append(run)
    return r


def assert_window(L, r, what):
    assert r["runs"]
    for run in r["runs"]:
        want = run["want"]
        assert want[2][:-2].tolist() == [0] * (3 * r["n"]) and want[2][-2:].tolist() == [L.REGION_FRAME, L.REGION_SLOT]
        for road in ("host", "stream", "null"):
            if road in run:
                c = dict(run["case"], what="%s, %s, %s road" % (what, run["case"]["what"], road))
                A.assert_equal(L, c, run[road], want)
        # an I picture is all restart; a P picture never goes backward
        for i, k in enumerate(r["keys"]):
            if k[2] == 1:
                assert (want[1][3 * i:3 * i + 3] == 0).all()
            if k[2] == 2:
                assert (want[1][3 * i + 2] == 0).all() and (want[1][3 * i] != 2).all()


@PARSERS
@pytest.mark.parametrize("name", ["ibbp_96x64_coded", "cropped_61x45"])
def test_every_delivered_frame_of_a_window(L, name, gpu_parser):
    """closed IBBP GOPs; cropped_61x45 is a frame smaller than its coded picture: the accumulators lie over the CODED 64 x 48"""
    data, kw = stream(name)
    got = run_windows(L, data, functools.partial(accumulate_window, L), gops_per_window=2, gpu_parser=gpu_parser, residual=True, **kw)
    assert got
    for window, r in got.items():
        assert_window(L, r, "%s window %d" % (name, window))
        assert {0, 1, 2} <= set(np.unique(r["runs"][0]["want"][1]).tolist())


@PARSERS
def test_open_gops(L, gpu_parser):
    data = open_stream(96, 64, 31)[0]
    got = run_windows(L, data, functools.partial(accumulate_window, L, parts_list=(3,)), gops_per_window=1, gpu_parser=gpu_parser, residual=True)
    assert got
    for window, r in got.items():
        assert_window(L, r, "open GOPs, window %d" % window)


def gop_chain_on_the_host(L, cw, ch, motion, residual, refs, keys, src, parts):
    """accumulate_gop's contract with accumulate_hop: src written as a restart, the levels of propagate_plan in order, a frame out of
    reach all zero, via 0, NO_REFERENCE.  Slot = window frame; the rows of the result are the GOP's frames."""
    n = len(keys)
    group = [i for i, k in enumerate(keys) if k[0] == keys[src][0]]
    levels, unreachable = L.propagate_plan(refs, keys, src)
    lay = L.accumulate_layout(cw, ch, parts)
    buf = np.full((n, lay.slot_bytes), 0x77, dtype=np.uint8)
    acc = L.accumulate_views(buf, lay)
    via, status = np.zeros((n, ch // 16, cw // 16), dtype=np.uint8), np.zeros(n, dtype=np.int64)
    for u in unreachable:
        buf[u] = 0
        status[u] = L.REGION_NO_REFERENCE
    for hops in [[(src, -1, -1)]] + levels:
        for t, f, b in hops:
            st, v = L.accumulate_hop(cw, ch, n, motion, residual, (t, t, f, b), acc)
            assert st == 0
            via[t] = v
    return {name: a[group] for name, a in acc.items()}, via[group], status[group], levels, unreachable, group


@pytest.mark.parametrize("start", ["I", "first P", "last P"])
@pytest.mark.parametrize("name,parts", [("ibbp_96x64_coded", None), ("ibbp_96x64_coded", 1), ("cropped_61x45", 2)])
def test_accumulate_gop_against_the_chain_on_the_host(L, name, parts, start):
    import torch
    data, kw = stream(name)

    def work(pipe, window, frames):
        frames = list(frames)
        cw, ch = coded(pipe)
        keys = [(f["gop"], f["display_index"], f["type"]) for f in frames]
        anchors = [i for i, k in enumerate(keys) if k[2] == (1 if start == "I" else 2)]
        src = anchors[-1] if start != "first P" else anchors[0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = pipe.accumulate_gop(window, src, parts)
            inside = None
            if "AX" in got:          # the invariant, asked on the stream: no host wait between the chain and its reader
                yy, xx = torch.meshgrid(torch.arange(ch, device="cuda"), torch.arange(cw, device="cuda"), indexing="ij")
                sx, sy = xx[None] + got["AX"].to(torch.int32), yy[None] + got["AY"].to(torch.int32)
                inside = ((sx >= 0) & (sx < cw) & (sy >= 0) & (sy < ch)).all(dim=(1, 2))
        st.synchronize()
        motion = [pipe.read_motion(window, i)[:2] for i in range(len(frames))]
        residual = [pipe.read_residual(window, i) for i in range(len(frames))]
        refs = [a.tolist() for a in pipe.carry_refs(window)]
        want = gop_chain_on_the_host(L, cw, ch, motion, residual, refs, keys, src, 3 if parts is None else parts)
        host = {k: v.cpu().numpy() for k, v in got.items() if k not in ("layout", "slots")}
        return host, want, pipe.gop_frames(window, src), keys, src, None if inside is None else inside.cpu().numpy()
    for (got, want, rows, keys, src, inside) in run_windows(L, data, work, gops_per_window=2, gpu_parser=True, residual=True, **kw).values():
        acc, via, status, levels, unreachable, group = want
        assert rows == group and len(group) < len(keys)
        assert set(got) == set(acc) | {"via", "status"} and set(acc) == set(L.accumulate_names(3 if parts is None else parts))
        for name_, a in acc.items():
            assert got[name_].shape == a.shape and np.array_equal(got[name_], a), "%s from %s: plane %s differs in %d places" % (name, start, name_, (got[name_] != a).sum())
        assert np.array_equal(got["via"], via) and np.array_equal(got["status"].astype(np.int64), status)
        assert (unreachable == []) == (start == "I") and sum(len(h) for h in levels) + len(unreachable) == len(group) - 1
        assert (via[group.index(src)] == 0).all() and all((a[group.index(src)] == 0).all() for a in acc.values())
        if inside is not None:
            assert inside.all()
            cw, ch = acc["AX"].shape[2], acc["AX"].shape[1]
            yy, xx = np.mgrid[0:ch, 0:cw]
            assert ((xx + acc["AX"] >= 0) & (xx + acc["AX"] < cw) & (yy + acc["AY"] >= 0) & (yy + acc["AY"] < ch)).all()
            assert acc["AGE"].max() == len(levels) and acc["AGE"].min() == 0


def test_the_call_is_refused_as_a_whole(L):
    import torch
    data = ibbp_stream(96, 64, [6], 47)
    seen = []

    def work(pipe, window, frames):
        lay = pipe.accumulate_layout(3)
        n_slots = 4
        slots = torch.full((n_slots, lay.slot_bytes), 0x12, dtype=torch.uint8, device="cuda")
        hops = torch.tensor([[1, 2, 0, 1, 0, 0, 0, 0], [2, 3, 0, 1, 0, 0, 0, 0]], dtype=torch.int32, device="cuda")
        via = torch.full((2, 4, 6), A.VIA_FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((2,), -55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ok_cfg = dict(parts=3, n_slots=n_slots, reserved=(0, 0), slot_pitch_bytes=lay.slot_bytes, slots_bytes=n_slots * lay.slot_bytes)
        ok = dict(hops=hops.data_ptr(), n=2, reserved0=0, slots=slots.data_ptr(), device_via=via.data_ptr(), device_status=status.data_ptr())

        def config(**kw):
            c = dict(ok_cfg, **kw)
            return L.PipelineAccumulateConfig(c["parts"], c["n_slots"], (C.c_int32 * 2)(*c["reserved"]), c["slot_pitch_bytes"], c["slots_bytes"])

        def refused(word, window_=window, reserved=(0, 0), cfg=None, null_cfg=False, **kw):
            a = dict(ok, **kw)
            call = L.PipelineAccumulateCall(a["hops"], a["n"], a["reserved0"], a["slots"], a["device_via"], a["device_status"], None, (C.c_uint64 * 2)(*reserved))
            rc = pipe.lib.leon_pipeline_accumulate_device(pipe.h, window_, None if null_cfg else C.byref(config(**(cfg or {}))), C.byref(call))
            assert rc == L.ERR_INVALID and word.encode() in pipe.lib.leon_last_error(), (word, rc, pipe.lib.leon_last_error())
            torch.cuda.synchronize()
            assert bool((slots == 0x12).all()) and bool((via == A.VIA_FILL).all()) and bool((status == -55).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        refused("not out for delivery", window_=window + 7)
        refused("null hops", hops=None)
        refused("null slots", slots=None)
        refused("4-byte aligned", hops=hops.data_ptr() + 2)
        refused("4-byte aligned", slots=slots.data_ptr() + 2)
        refused("4-byte aligned", device_status=status.data_ptr() + 3)
        refused("0 hops", n=0)
        refused("65536 hops", n=65536)
        refused("-1 hops", n=-1)
        refused("reserved word of the call", reserved0=1)
        refused("reserved word of the call", reserved=(1, 0))
        refused("reserved word of the call", reserved=(0, 1))
        refused("null cfg", null_cfg=True)
        for parts in (0, 4, -1):
            refused("parts", cfg=dict(parts=parts))
        for n in (0, 65536):
            refused("slots", cfg=dict(n_slots=n))
        refused("slot_pitch_bytes", cfg=dict(slot_pitch_bytes=lay.slot_bytes - 4))
        refused("slot_pitch_bytes", cfg=dict(slot_pitch_bytes=lay.slot_bytes + 2))
        refused("slots_bytes", cfg=dict(slots_bytes=n_slots * lay.slot_bytes - 1))
        refused("slots_bytes", cfg=dict(slot_pitch_bytes=lay.slot_bytes + 4))
        refused("reserved word of cfg", cfg=dict(reserved=(1, 0)))
        refused("reserved word of cfg", cfg=dict(reserved=(0, 1)))
        assert pipe.lib.leon_pipeline_accumulate_device(pipe.h, window, C.byref(config()), None) == L.ERR_INVALID
        # the host road refuses the same; a hop's fault is no refusal
        host = np.full((n_slots, lay.slot_bytes), 0x12, dtype=np.uint8)
        hh = L._records_array([(1, 2, 0, 1)])
        for args in ((window + 7, C.byref(config()), hh.ctypes.data, 1, host.ctypes.data), (window, None, hh.ctypes.data, 1, host.ctypes.data),
                     (window, C.byref(config()), None, 1, host.ctypes.data), (window, C.byref(config()), hh.ctypes.data, 1, None),
                     (window, C.byref(config()), hh.ctypes.data, 0, host.ctypes.data), (window, C.byref(config()), hh.ctypes.data, 65536, host.ctypes.data),
                     (window, C.byref(config(parts=4)), hh.ctypes.data, 1, host.ctypes.data)):
            assert pipe.lib.leon_pipeline_accumulate(pipe.h, *args, None, None) == L.ERR_INVALID
        assert (host == 0x12).all()
        v, st_ = pipe.accumulate(window, host, [(99, 2, 0, 1), (1, 2, 2, 1), (1, 2, 0, 1)], 3, via_fill=A.VIA_FILL)
        assert st_.tolist() == [L.REGION_FRAME, L.REGION_SLOT, 0] and (v[:2] == A.VIA_FILL).all() and (v[2] != A.VIA_FILL).all() and (host[3] == 0x12).all()
        assert not (host[2] == 0x12).all()
        # via and status may be NULL
        call = L.PipelineAccumulateCall(hops.data_ptr(), 2, 0, slots.data_ptr(), None, None, None)
        assert pipe.lib.leon_pipeline_accumulate_device(pipe.h, window, C.byref(config()), C.byref(call)) == L.OK
        assert bool((via == A.VIA_FILL).all()) and bool((status == -55).all()) and bool((slots[:2] == 0x12).all()) and not bool((slots[2:] == 0x12).all())
        return True
    assert all(run_windows(L, data, work, gops_per_window=1, gpu_parser=True, residual=True).values()) and len(seen) == 24

    # a pipeline without the RESIDUAL bit: the motion part runs, the residual part is refused as gauge refuses a missing output
    def no_residual(pipe, window, frames):
        lay1, lay3 = L.accumulate_layout(96, 64, 1), L.accumulate_layout(96, 64, 3)
        assert pipe.accumulate_layout().parts == 1          # parts=None: every part the outputs allow
        got = pipe.accumulate_gop(window, [i for i, f in enumerate(frames) if f["type"] == 1][0])
        torch.cuda.synchronize()
        assert set(got) == {"AX", "AY", "AGE", "via", "status", "slots", "layout"} and bool((got["status"] == 0).all())
        z = np.zeros((2, lay3.slot_bytes), dtype=np.uint8)
        for parts in (2, 3):
            with pytest.raises(L.LeonError, match="residual"):
                pipe.accumulate(window, z, [(0, 1, 0, -1)], parts)
        assert pipe.accumulate(window, z[:, :lay1.slot_bytes].copy(), [(0, 1, 0, -1)], 1)[1].tolist() == [0]
        return True
    assert all(run_windows(L, data, no_residual, gops_per_window=1, gpu_parser=True).values())
    # a pipeline without the MOTION bit
    refusals = []

    def no_motion(window, frames):
        pipe = frames[0]["_pipe"]
        lay = L.accumulate_layout(96, 64, 2)
        z = np.zeros((2, lay.slot_bytes), dtype=np.uint8)
        h = L._records_array([(0, 1, 0, -1)])
        cfg = L._accumulate_config(z, 2)
        call = L.PipelineAccumulateCall(h.ctypes.data, 1, 0, z.ctypes.data, None, None, None)
        refusals.append((pipe.lib.leon_pipeline_accumulate_device(pipe.h, window, C.byref(cfg), C.byref(call)), pipe.lib.leon_last_error()))
        refusals.append((pipe.lib.leon_pipeline_accumulate(pipe.h, window, C.byref(cfg), h.ctypes.data, 1, z.ctypes.data, None, None), pipe.lib.leon_last_error()))
    pipe = L.Pipeline(data, on_window=no_motion, gops_per_window=1, residual=True)
    try:
        pipe.wait()
        assert pipe.error is None, pipe.error
    finally:
        pipe.close()
    assert refusals and all(rc == L.ERR_INVALID and b"motion" in msg for rc, msg in refusals)


def residual_stream(cw, ch, gops, seed, scene=(88.0, 168.0), amp=10.0, pics_out=None):
    """like copy_stream (tests/test_pipeline_propagate_gpu.py), with coded residual: no intra macroblock in P and B pictures, one
    direction per B picture, every vector full-pel, uncoded_frac 0.3 -- and the coefficients made anew from synth's parts: the I
    picture a scene inside `scene` (well away from 0 and 255), the P and B pictures a residual of amplitude `amp`, so that no sum along
    a chain reaches the clamp.  pics_out: a list that receives the pictures' tensors (the oracle decodes them on the CPU)."""
    import jsv_writer as W
    import synth as S
    rng = np.random.default_rng(seed)
    mbw, mbh = cw // 16, ch // 16
    pics, starts = [], []
    for n in gops:
        starts.append(len(pics))
        k = 0
        for ptype, disp, f, b in S.gop_ibbp(n):
            if ptype == S.PIC_I:
                t = S.make_picture(rng, cw, ch, ptype)
            else:
                force = None
                if ptype == S.PIC_B:
                    force = 2 if f is None else 1 + k % 2
                    k += 1
                t = S.make_picture(rng, cw, ch, ptype, intra_frac=0, uncoded_frac=0.3, force_dir=force)
                for key in ("mv_fwd", "mv_bwd"):
                    if key in t:
                        t[key] &= ~1
            for key, (w, h), chroma in (("coef_y", (cw, ch), False), ("coef_cb", (cw // 2, ch // 2), True), ("coef_cr", (cw // 2, ch // 2), True)):
                if ptype == S.PIC_I:
                    content = S.smooth_scene(rng, w, h, lo=scene[0], hi=scene[1], noise=2.0)
                else:
                    content = S.smooth_scene(rng, w, h, lo=-amp, hi=amp, noise=amp / 4)
                lv = S.quantise_plane(S.fdct_plane(content.astype(np.float32)), t["qscale"], t["intra"], mbw, mbh, chroma, S.DEFAULT_INTRA_QUANT, S.DEFAULT_NON_INTRA_QUANT)
                if ptype != S.PIC_I:          # the blocks make_picture left uncoded (cbp, skipped macroblocks) stay uncoded
                    was = t[key].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
                    lv[~was.any(axis=(2, 3))] = 0
                t[key] = np.ascontiguousarray(S.blocks_to_plane(lv))
            t["display"] = disp
            pics.append(t)
    if pics_out is not None:
        pics_out.extend(pics)
    return W.write_stream(pics, cw, ch, cw, ch, gop_starts=starts)[0]


def chain_luma(L, cw, ch, keys, refs, motion, residual, luma, src):
    """[(t, type, counts...)] for every frame of src's GOP: the accumulators of the whole chain by accumulate_hop, then
    I_luma[y + AY][x + AX] + RY[y][x] against the frame's own luma"""
    n = len(keys)
    lay = L.accumulate_layout(cw, ch, 3)
    buf = np.zeros((n, lay.slot_bytes), dtype=np.uint8)
    acc = L.accumulate_views(buf, lay)
    levels, unreachable = L.propagate_plan(refs, keys, src)
    assert unreachable == []
    for hops in [[(src, -1, -1)]] + levels:
        for t, f, b in hops:
            assert L.accumulate_hop(cw, ch, n, motion, residual, (t, t, f, b), acc)[0] == 0
    return acc


def identity_counts(acc, luma, t, src):
    ch, cw = luma[t].shape
    yy, xx = np.mgrid[0:ch, 0:cw]
    rebuilt = luma[src].astype(np.int64)[yy + acc["AY"][t], xx + acc["AX"][t]] + acc["RY"][t]
    return int((rebuilt != luma[t]).sum())


@pytest.mark.parametrize("cw,ch,gop,seed", [(96, 64, 6, 61), (64, 48, 9, 62), (352, 240, 6, 63)])
def test_the_decoders_own_reconstruction_is_the_oracle(L, cw, ch, gop, seed):
    """Without intra macroblocks, with one direction per B picture and full-pel vectors the decoder's luma of a P or B picture is its
    reference's samples along the vectors plus the residual, and as long as no clamp to 0 .. 255 acts that holds along the whole chain:
    I_luma[y + AY][x + AX] + RY[y][x] equals the delivered luma in EVERY sample of every frame of the GOP.  The accumulators come from
    accumulate_gop on the device.  The test asserts its premise itself.  (Checked on the CPU against the oracle's planes and residual
    when this was written, with accumulate_hop on motion_from_maps' records: 96 x 64 IBBP-6, 64 x 48 IBBP-9 and 352 x 240 IBBP-6 gave 0
    differing samples over 18 P and B pictures with 1809 of 1866 macroblocks moving, every P and B picture with a non-zero residual
    record, chains of up to 3 hops, and luma between 86 and 177.)"""
    import torch
    data = residual_stream(cw, ch, [gop], seed)

    def work(pipe, window, frames):
        frames = list(frames)
        n = len(frames)
        luma = [pipe.read_planes(f)[0] for f in frames]
        motion = [pipe.read_motion(window, i) for i in range(n)]
        residual = [pipe.read_residual(window, i) for i in range(n)]
        (src,) = [i for i, f in enumerate(frames) if f["type"] == 1]
        got = pipe.accumulate_gop(window, src)
        torch.cuda.synchronize()
        acc = {k: got[k].cpu().numpy() for k in ("AX", "AY", "AGE", "RY")}
        via = got["via"].cpu().numpy()
        assert pipe.gop_frames(window, src) == list(range(n)) and bool((got["status"] == 0).all())
        out = []
        for t in range(n):
            mv, info, _ = motion[t]
            out.append(dict(t=t, type=frames[t]["type"], intra=int((info & 4).astype(bool).sum()), restart=int((via[t] == 0).sum()),
                            moving=int((mv != 0).any(axis=2).sum()), odd=int((mv & 1).astype(bool).sum()), residual=int(np.count_nonzero(residual[t][0])),
                            lo=int(luma[t].min()), hi=int(luma[t].max()), age=int(acc["AGE"][t].max()), differ=identity_counts(acc, luma, t, src)))
        return out
    (out,) = run_windows(L, data, work, gops_per_window=1, gpu_parser=True, output="ycbcr", residual=True).values()
    assert len(out) == gop and sorted({o["type"] for o in out}) == [1, 2, 3]
    rest = [o for o in out if o["type"] != 1]
    for o in out:
        print("frame %d (type %d): %d moving macroblocks, age %d, %d residual samples, luma %d .. %d, %d samples differ" % (
            o["t"], o["type"], o["moving"], o["age"], o["residual"], o["lo"], o["hi"], o["differ"]))
    # the premise: no intra macroblock (so no restart), full-pel vectors, macroblocks that move, a residual on every picture, no clamp
    assert all(o["intra"] == 0 and o["restart"] == 0 and o["odd"] == 0 and o["residual"] > 0 for o in rest), out
    assert sum(o["moving"] for o in rest) > len(rest) * (cw // 16) * (ch // 16) // 2, out
    assert all(0 < o["lo"] and o["hi"] < 255 for o in out), out
    assert max(o["age"] for o in out) >= 2          # a chain, not single hops
    assert all(o["differ"] == 0 for o in out), out
