"""GPU: regions letterboxed into the batch's tensor size from boxes in device memory (include/leon_pipeline.h,
leon_pipeline_resample_regions_device_fit) -- k_fit_tables judges each region against its own image size and lays its tables out for
it, k_fitted runs behind the status word.  The expected bytes are the HOST path's of the same build, which
tests/test_pipeline_regions_fit_gpu.py pins to the oracle; the status words are leon_pipeline_region_fit_status's and the rectangles
leon_pipeline_region_fit_rect's (pinned on the CPU by tests/test_pipeline_regions_fit_abi.py and tests/test_fitted_structure.py).
Equality everywhere, no tolerance."""
import numpy as np
import pytest

import fitted_structure as F
import regions_structure as S
from fitted_structure import CALLS, CENTRE, TOP_LEFT
from regions_structure import BICUBIC, FILTERS, TRIANGLE
from resample_structure import FILTER_NAMES, STREAMS
from test_pipeline_gpu import ibbp_stream
from test_pipeline_regions_device_gpu import records, side_stream, slot_bytes, ubits
from test_pipeline_regions_gpu import CANARY, run

pytestmark = pytest.mark.gpu

PAD = (114, 7, 250)
FORMATS = [("uint8", "hwc"), ("float16", "chw"), ("float32", "hwc"), ("uint8", "chw")]
RUNS = [(c, f, d, l) for c in sorted(CALLS) for f in FILTERS for d, l in FORMATS]
UNTOUCHED = -9


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.fixture(scope="module")
def streams():
    made = {}

    def get(name):
        if name not in made:
            cw, ch, gops, seed, (fw, fh) = STREAMS[name]
            made[name] = ibbp_stream(cw, ch, gops, seed=seed, frame=(fw, fh))
        return made[name]
    return get


def assert_same(out, want, what):
    assert out.shape == want.shape and out.dtype == want.dtype, what
    if not np.array_equal(out, want):
        bad = np.argwhere(out != want)
        raise AssertionError("%s: %d of %d elements differ from the host path in regions %s, first at %s" % (
            what, len(bad), out.size, sorted({int(b[0]) for b in bad})[:10], bad[0].tolist()))


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join([r[0], FILTER_NAMES[r[1]], r[2], r[3]]))
def test_call(L, streams, run_):
    """bytes = the host path's, status 0 everywhere, rects = region_fit_rect -- for the anchor the run takes (they alternate)"""
    import torch
    name, filt, dtype, layout = run_
    call = CALLS[name]
    anchor = (CENTRE, TOP_LEFT)[RUNS.index(run_) % 2]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        got["regs"] = regs
        got["want"] = ubits(p.read_regions(window, regs, call.size, filt, fit="letterbox", anchor=anchor, pad_value=PAD))
        st = side_stream()
        with torch.cuda.stream(st):
            boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
            view, status, rects = p.resample_regions_device(window, boxes, call.size, filt, fit="letterbox", anchor=anchor, pad_value=PAD, rects=True)
        st.synchronize()
        got["out"], got["status"], got["rects"] = ubits(view), status.cpu().numpy(), rects.cpu().numpy()
    run(L, streams(name), dtype, layout, on_frames).close()
    what = "%s %s %s %s %s" % (name, FILTER_NAMES[filt], dtype, layout, anchor)
    assert (got["status"] == 0).all(), (what, got["status"])
    assert_same(got["out"], got["want"], what)
    assert got["rects"].tolist() == [list(L.region_fit_rect(r[3], r[4], call.size, anchor=anchor)) for r in got["regs"]]
    assert got["rects"].tolist() == [list(F.rect(r[1:], call.size, anchor)) for r in got["regs"]]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refused_regions_among_good_ones(L, streams, name):
    """non-zero status exactly at the refused positions and equal to region_fit_status; their whole tensors -- pad included -- the gaps up
    to an explicit pitch and everything behind the last region still the canary's; their rects untouched; the good regions equal the
    host path and have their rects"""
    import torch
    call, filt, dtype, layout, e = CALLS[name], BICUBIC, "float16", "hwc", 2
    fw, fh = call.frame
    nbytes, dflt = S.placement(call.size, e)
    pitch = dflt + 256
    got = {}

    def on_frames(p, window, keys, frames):
        good = call.regions(len(frames))
        bad = [(2,) + b for b, _, _ in call.refusals] + [(len(frames), 0, 0, 8, 8), (0, 0, 0, 8, 8), (1, 4, 4, 0, 8), (-1, 0, 0, 8, 8), (3, fw - 7, 0, 8, 8), (3, 0, 0, 8, 0)]
        rec, at = [], []
        for i, g in enumerate(good):
            rec.append(g)
            if i < len(bad):
                at.append(len(rec))
                rec.append(bad[i])
        full = records(rec)
        reserved_at = at[len(call.refusals) + 1]
        full[reserved_at, 6] = 5          # a reserved word
        n = len(rec)
        want_status = []
        for r in full:
            reg = L.PipelineRegion(*[int(v) for v in r[:5]])
            reg.reserved[0], reg.reserved[1], reg.reserved[2] = int(r[5]), int(r[6]), int(r[7])
            want_status.append(L.region_fit_status(fw, fh, len(frames), reg, call.size, filt, pad_value=PAD))
        assert [i for i in range(n) if want_status[i]] == at
        assert set(want_status) >= {0, L.REGION_RESERVED, L.REGION_FRAME, L.REGION_BOX} | ({L.REGION_RATIO_X, L.REGION_RATIO_Y} if call.refusals else set())
        got["want"] = ubits(p.read_regions(window, good, call.size, filt, fit="letterbox", pad_value=PAD))
        st = side_stream()
        with torch.cuda.stream(st):
            buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
            status = torch.full((n + 4,), UNTOUCHED, dtype=torch.int32, device="cuda")
            rects = torch.full((n + 2, 4), UNTOUCHED, dtype=torch.int32, device="cuda")
            view, ret, rr = p.resample_regions_device(window, torch.from_numpy(full).cuda(), call.size, filt, out=buf, pitch=pitch, status=status,
                                                      fit="letterbox", pad_value=PAD, rects=rects)
        st.synchronize()
        assert view.data_ptr() == buf.data_ptr() and ret.data_ptr() == status.data_ptr() and rr.data_ptr() == rects.data_ptr() and tuple(rr.shape) == (n, 4)
        got.update(n=n, at=at, rec=rec, raw=buf.cpu().numpy(), status=status.cpu().numpy(), rects=rects.cpu().numpy(), want_status=want_status)
    run(L, streams(name), dtype, layout, on_frames).close()
    n, at, raw = got["n"], got["at"], got["raw"]
    assert got["status"][:n].tolist() == got["want_status"] and (got["status"][n:] == UNTOUCHED).all()
    assert (got["rects"][n:] == UNTOUCHED).all()
    k = 0
    for i in range(n):
        if i in at:
            assert (raw[i * pitch:(i + 1) * pitch] == CANARY).all(), "the refused region %d was written" % i
            assert (got["rects"][i] == UNTOUCHED).all(), "the rect of the refused region %d was written" % i
        else:
            assert raw[i * pitch:i * pitch + nbytes].tobytes() == got["want"][k].tobytes(), "region %d" % i
            assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
            assert got["rects"][i].tolist() == list(F.rect(got["rec"][i][1:], call.size)), i
            k += 1
    assert k == len(got["want"]) and (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: FILTER_NAMES[f])
def test_chunks_of_one_and_of_three_regions(L, streams, filt):
    """the slot is the stretch call's worst case for out = the canvas: the same limits give the same chunks, and the same bytes"""
    import torch
    name = "96x64"
    call = CALLS[name]
    per = slot_bytes(call.size, filt)
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        assert len(regs) == 10
        st = side_stream()
        with torch.cuda.stream(st):
            boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
            outs = [p.resample_regions_device(window, boxes, call.size, filt, scratch_limit=limit, fit="letterbox", pad_value=PAD, rects=True)
                    for limit in (None, per, 2 * per - 1, 3 * per, 4 * per - 1)]
        st.synchronize()
        got["outs"] = [(ubits(v), s.cpu().numpy(), r.cpu().numpy()) for v, s, r in outs]
        got["want"] = ubits(p.read_regions(window, regs, call.size, filt, fit="letterbox", pad_value=PAD))
        got["rects"] = [list(F.rect(r[1:], call.size)) for r in regs]
        with pytest.raises(L.LeonError, match="scratch_limit_bytes") as e:
            p.resample_regions_device(window, boxes, call.size, filt, scratch_limit=per - 1, fit="letterbox")
        assert e.value.code == L.ERR_INVALID
    run(L, streams(name), "uint8", "chw", on_frames).close()
    for out, status, rects in got["outs"]:
        assert np.array_equal(out, got["want"]) and (status == 0).all() and rects.tolist() == got["rects"]


def test_boxes_written_on_a_side_stream_right_before_the_call(L, streams):
    """the boxes are the result of torch kernels on a side stream, the call is queued behind them and a torch reduction of its output
    behind the call: nothing waits on the host in between"""
    import torch
    name, filt = "608x57", TRIANGLE
    call = CALLS[name]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        got["want"] = ubits(p.read_regions(window, regs, call.size, filt, fit="letterbox", pad_value=PAD))
        jitter = torch.tensor([0.0, 0.25, -0.25, 0.125, -0.375], dtype=torch.float32)
        st = side_stream()
        with torch.cuda.stream(st):
            fb = (torch.tensor(regs, dtype=torch.float32) + jitter).to("cuda", non_blocking=True)
            boxes = fb.round().to(torch.int32)
            view, status, rects = p.resample_regions_device(window, boxes, call.size, filt, fit="letterbox", pad_value=PAD, rects=True)
            red = view.to(torch.int64).sum(dim=(1, 2, 3))
            area = rects[:, 2] * rects[:, 3]
        st.synchronize()
        got.update(out=ubits(view), status=status.cpu().numpy(), red=red.cpu().numpy(), area=area.cpu().numpy(), regs=regs)
    run(L, streams(name), "uint8", "hwc", on_frames).close()
    assert (got["status"] == 0).all()
    assert_same(got["out"], got["want"], "behind torch's kernels")
    assert np.array_equal(got["red"], got["want"].reshape(len(got["want"]), -1).astype(np.int64).sum(axis=1))
    assert got["area"].tolist() == [F.rect(r[1:], call.size)[2] * F.rect(r[1:], call.size)[3] for r in got["regs"]]


def test_without_a_fit_the_device_call_is_the_one_it_was_and_rects_need_the_letterbox(L, streams):
    import torch
    name = "100x57"
    call = S.CALLS[name]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
        st = side_stream()
        with torch.cuda.stream(st):
            plain = p.resample_regions_device(window, boxes, call.size, BICUBIC)
            stretch = p.resample_regions_device(window, boxes, call.size, BICUBIC, fit="stretch")
        st.synchronize()
        assert len(plain) == 2 and len(stretch) == 2
        got["plain"], got["stretch"] = ubits(plain[0]), ubits(stretch[0])
        assert (plain[1] == 0).all() and (stretch[1] == 0).all()
        buf = torch.full((len(regs) * 4096,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for kw in (dict(rects=True), dict(fit="stretch", rects=True), dict(fit="letterbox", anchor=3), dict(fit="letterbox", pad_value=(0, 0, 300))):
            with pytest.raises(L.LeonError) as e:
                p.resample_regions_device(window, boxes, call.size, BICUBIC, out=buf, stream=st, **kw)
            assert e.value.code == L.ERR_INVALID
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()), kw
    run(L, streams(name), "float16", "chw", on_frames).close()
    assert np.array_equal(got["plain"], got["stretch"])
