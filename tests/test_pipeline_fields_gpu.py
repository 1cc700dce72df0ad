"""GPU: field tensors of delivered windows (include/leon_pipeline.h, leon_pipeline_field_tensors; k_box_tables and k_fields) on the
project's small synthetic streams -- motion_tensors against leon_ctypes.field_tensor applied to what read_motion gives, residual_tensors
against it applied to read_residual, accumulate_tensors against it applied to accumulate_gop's views, each from a dense item the test
lays out itself; the host road with a refused record's tensor left alone; carry_regions_gop's [F, N, 8] rows going in unchanged, the
rows carry refused coming back as status words; a call on a side stream ordered against torch's work on it; and the refusals of the
whole call: a pipeline without the source's output, a released window, a buffer where there is none to give."""
import ctypes as C

import numpy as np
import pytest

from test_pipeline_motion_gpu import stream

pytestmark = pytest.mark.gpu

SIZE = (5, 7)
FILL = 0xA5


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def records_of(n, fw, fh):
    recs = [r for i in range(n) for r in ((i, 0, 0, fw, fh), (i, 5, 3, 30, 20), (i, fw - 7, fh - 5, 7, 5))]
    recs += [(n, 0, 0, 4, 4), (0, 0, 0, fw + 1, 4), (0, 1, 1, 4, 4, 0, 0, 9)]
    return [tuple(r) + (0,) * (8 - len(r)) for r in recs]


def want_batch(L, fw, fh, items, recs, channels, dtype):
    """(tensors [n, C, h, w] with FILL in the bytes of a refused record, status) from dense items: items[i] the int16 elements of item i"""
    dt = L.FIELD_NP_DTYPES[dtype]
    out = np.zeros((len(recs), len(channels)) + SIZE, dtype=dt)
    out.view(np.uint8)[...] = FILL
    status = np.zeros(len(recs), dtype=np.int32)
    for k, r in enumerate(recs):
        status[k] = L.field_record_status(fw, fh, len(items), r, SIZE)
        if status[k] == 0:
            out[k] = L.field_tensor(items[r[0]], fw, fh, r[1:5], SIZE, channels, dtype)
    return out, status


def bits(t):
    """a batch on the device as host bit patterns"""
    import torch
    t = t.contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


def same(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def window_work(L, pipe, window, frames):
    import torch
    n, fw, fh, cw, ch = len(frames), pipe.info.frame_width, pipe.info.frame_height, pipe.info.coded_width, pipe.info.coded_height
    mbw = cw // 16
    checks = {}
    recs = records_of(n, fw, fh)
    full = L._records_array(recs)
    # dense items of the test's own: a frame's four vector words interleaved; its three residual planes one after the other
    motion = [np.ascontiguousarray(pipe.read_motion(window, i)[0], dtype=np.int16).reshape(-1) for i in range(n)]
    residual = [np.concatenate([np.ascontiguousarray(p, dtype=np.int16).reshape(-1) for p in pipe.read_residual(window, i)]) for i in range(n)]
    m_dense = L.field_channels_motion(mbw, L.MOTION_FIELDS, (0.5, 0.5, 0.25, 0.25), (0.0, 1.0, 0.0, -1.0))
    r_dense = [L.field_channel(0, cw, 1, 0, 1.0 / 128, 0.0), L.field_channel(2 * cw * ch, cw // 2, 1, 1, 1.0 / 64, 0.5), L.field_channel(2 * cw * ch + 2 * (cw // 2) * (ch // 2), cw // 2, 1, 1, 1.0, 0.0)]
    side = torch.cuda.Stream()
    for dtype in ("float16", "bfloat16", "float32"):
        want_m, want_st = want_batch(L, fw, fh, motion, recs, m_dense, dtype)
        want_r, _ = want_batch(L, fw, fh, residual, recs, r_dense, dtype)
        nbytes = want_m[0].nbytes
        pitch = -(-nbytes // 256) * 256
        # the device road on a side stream, behind a fill of the output and the records' upload on that stream, in front of the copies back
        with torch.cuda.stream(side):
            out = torch.full((len(recs) * pitch,), FILL, dtype=torch.uint8, device="cuda")
            st = torch.full((len(recs),), -3, dtype=torch.int32, device="cuda")
            dev = torch.from_numpy(full).pin_memory().to("cuda", non_blocking=True)
            batch, status = pipe.motion_tensors(window, dev, SIZE, L.MOTION_FIELDS, (0.5, 0.5, 0.25, 0.25), (0.0, 1.0, 0.0, -1.0), dtype=dtype, out=out, status=st, stream=side)
            got_m, got_st, raw = bits(batch), status.cpu().numpy(), out.cpu().numpy().reshape(len(recs), pitch)
        side.synchronize()
        checks["motion %s" % dtype] = same(got_m, want_m) and got_st.tolist() == want_st.tolist() and bool((raw[:, nbytes:] == FILL).all()) and status.data_ptr() == st.data_ptr()
        # ... on torch's current stream, buffers of the method's own: a refused record's tensor is not compared
        batch, status = pipe.residual_tensors(window, torch.from_numpy(full).cuda(), SIZE, scale=(1.0 / 128, 1.0 / 64, 1.0), bias=(0.0, 0.5, 0.0), dtype=dtype)
        ok = want_st == 0
        checks["residual %s" % dtype] = same(bits(batch)[ok], want_r[ok]) and status.cpu().numpy().tolist() == want_st.tolist()
        # the host road: everything comes back whole
        got, st_h = pipe.field_tensors(window, recs, SIZE, L.field_channels_motion(mbw, L.MOTION_FIELDS, (0.5, 0.5, 0.25, 0.25), (0.0, 1.0, 0.0, -1.0)), source="motion", dtype=dtype,
                                       fill=FILL, status_fill=-3)
        checks["host road %s" % dtype] = same(got, want_m) and st_h.tolist() == want_st.tolist()
    # accumulators: the GOP of the window's first I picture; a record's frame word is the row of the planes
    src = [i for i, f in enumerate(frames) if f["type"] == L.PIC_I][0]
    acc = pipe.accumulate_gop(window, src)
    rows = pipe.gop_frames(window, src)
    names = ("AX", "AY", "AGE", "RY", "RCb", "RCr")
    planes = {k: acc[k].cpu().numpy() for k in names}
    items = [np.concatenate([planes[k][i].reshape(-1) for k in names]) for i in range(len(rows))]
    a_dense, at = [], 0
    for k in names:
        h, w = planes[k].shape[1:]
        a_dense.append(L.field_channel(at, w, 1, 1 if k in ("RCb", "RCr") else 0, 0.25, 2.0))
        at += 2 * h * w
    arecs = records_of(len(rows), fw, fh)
    want_a, want_st = want_batch(L, fw, fh, items, arecs, a_dense, "float32")
    batch, status = pipe.accumulate_tensors(acc, torch.from_numpy(L._records_array(arecs)).cuda(), SIZE, names, 0.25, 2.0, dtype="float32")
    ok = want_st == 0
    checks["accumulate"] = same(bits(batch)[ok], want_a[ok].view(np.uint32)) and status.cpu().numpy().tolist() == want_st.tolist()
    checks["accumulate moved"] = bool((planes["AX"] != 0).any() or (planes["AY"] != 0).any())
    # the rows carry_regions_gop writes go in as they are, [F, N, 8]; a row carry refused is an empty box: a status word, nothing written
    boxes = torch.tensor([[8, 8, 20, 16], [0, 0, fw, fh], [fw - 9, fh - 9, 9, 9]], dtype=torch.int32, device="cuda")
    carried, _, cst = pipe.carry_regions_gop(window, boxes, src)
    batch, status = pipe.motion_tensors(window, carried, SIZE, ("fwd_h", "fwd_v"), 0.5, dtype="float16")
    crecs = [tuple(r) for r in carried.cpu().numpy().reshape(-1, 8).tolist()]
    want_c, want_st = want_batch(L, fw, fh, motion, crecs, L.field_channels_motion(mbw, ("fwd_h", "fwd_v"), 0.5), "float16")
    ok = want_st == 0
    cst = cst.cpu().numpy().reshape(-1)
    checks["carried"] = tuple(batch.shape) == (len(crecs), 2) + SIZE and same(bits(batch)[ok], want_c[ok]) and status.cpu().numpy().tolist() == want_st.tolist()
    checks["carried refused"] = bool(ok.any() and (~ok).any() and (want_st[cst != 0] == L.REGION_BOX).all() and (want_st[cst == 0] == 0).all())
    # a buffer with a record source, and none with the buffer source
    for kw in (dict(source="motion", buffer=acc["slots"]), dict(source="buffer")):
        try:
            pipe.field_tensors_device(window, carried, SIZE, m_dense, **kw)
            checks["buffer %s" % kw["source"]] = False
        except ValueError:
            checks["buffer %s" % kw["source"]] = True
    return checks


def run(L, data, work, **kw):
    """work(pipe, window, frames) in every window's callback; then after(pipe) with every window released and the pipeline still open"""
    got, last = {}, {}

    def on_window(window, frames):
        got[window] = work(frames[0]["_pipe"], window, frames)
        last["window"], last["n"] = window, len(frames)
    pipe = L.Pipeline(data, on_window=on_window, parser_threads=2, gops_per_window=2, **kw)
    try:
        pipe.wait()
        assert pipe.ended and pipe.error is None, pipe.error
        return got, last, pipe
    except BaseException:
        pipe.close()
        raise


@pytest.mark.parametrize("gpu_parser", [False, True], ids=["host-parser", "gpu-parser"])
def test_every_source_and_road_on_a_frame_smaller_than_its_coded_picture(L, gpu_parser):
    import torch
    data, kw = stream("cropped_61x45")
    got, last, pipe = run(L, data, lambda pipe, window, frames: window_work(L, pipe, window, frames), gpu_parser=gpu_parser, motion=True, residual=True, **kw)
    try:
        assert got
        for window, checks in got.items():
            assert all(checks.values()), (window, [k for k, v in checks.items() if not v])
        # a released window is refused, on both roads
        recs = records_of(last["n"], pipe.info.frame_width, pipe.info.frame_height)
        with pytest.raises(L.LeonError, match="not out for delivery"):
            pipe.motion_tensors(last["window"], torch.from_numpy(L._records_array(recs)).cuda(), SIZE)
        with pytest.raises(L.LeonError, match="not out for delivery"):
            pipe.field_tensors(last["window"], recs, SIZE, L.field_channels_motion(pipe.info.coded_width // 16), source="motion")
    finally:
        pipe.close()


def test_a_pipeline_without_the_sources_output_is_refused(L):
    import torch
    data, kw = stream("cropped_61x45")
    seen = []

    def work(pipe, window, frames):
        fw, fh, cw, ch = pipe.info.frame_width, pipe.info.frame_height, pipe.info.coded_width, pipe.info.coded_height
        dev = torch.from_numpy(L._records_array([(0, 0, 0, fw, fh)])).cuda()
        out = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
        has_motion = pipe.motion_layout is not None
        source, word = (L.FIELD_SOURCE_RESIDUAL, b"no residual output") if has_motion else (L.FIELD_SOURCE_MOTION, b"no motion output")
        channels = L.field_channels_residual(L.residual_layout(cw, ch)) if has_motion else L.field_channels_motion(cw // 16)
        cfg = L._field_config(source, "float16", SIZE, channels)
        call = L.PipelineFieldTensorsCall(dev.data_ptr(), 1, 0, None, out.data_ptr(), 0, None, None, 0)
        rc = pipe.lib.leon_pipeline_field_tensors_device(pipe.h, window, C.byref(cfg), C.byref(call))
        ok = rc == L.ERR_INVALID and word in pipe.lib.leon_last_error()
        torch.cuda.synchronize()
        try:
            (pipe.residual_tensors if has_motion else pipe.motion_tensors)(window, dev, SIZE)
            ok = False
        except L.LeonError:
            pass
        # the source it has works, and the call touched nothing of the refused one's output
        batch, status = (pipe.motion_tensors if has_motion else pipe.residual_tensors)(window, dev, SIZE)
        seen.append(ok and bool((out == FILL).all()) and status.cpu().numpy().tolist() == [0])
        return True
    for outputs in (dict(motion=True), dict(residual=True)):
        got, last, pipe = run(L, data, work, gpu_parser=True, **outputs, **kw)
        pipe.close()
        assert got
    assert len(seen) >= 2 and all(seen)
