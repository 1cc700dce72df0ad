"""GPU: warp regions whose records lie in device memory (include/leon_pipeline.h, leon_pipeline_warp_regions_device) -- k_warp judges
its own record and one workgroup of the region writes the status word.  The records arrive as a CUDA tensor on a non-default torch
stream; the expected bytes are the HOST path's of the same build, which tests/test_pipeline_warp_gpu.py pins to the oracle; the status
words are leon_pipeline_warp_region_status's (pinned on the CPU by tests/test_pipeline_warp_abi.py).  Equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import warp_structure as W
from resample_structure import STREAMS
from test_pipeline_gpu import ibbp_stream
from test_pipeline_regions_device_gpu import side_stream, ubits
from test_pipeline_regions_gpu import CANARY, run

pytestmark = pytest.mark.gpu

FORMATS = [("uint8", "hwc"), ("float16", "chw"), ("float32", "hwc"), ("uint8", "chw")]
RUNS = [(name, d, l) for name in sorted(W.SIZES) for d, l in FORMATS]


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


def records(regs):
    """[N, 8] int32 leon_pipeline_warp_region records of [(frame, m)] or [(frame, m, reserved)]"""
    return np.array([[r[0]] + list(r[1]) + [r[2] if len(r) > 2 else 0] for r in regs], dtype=np.int32)


def assert_same(out, want, what):
    assert out.shape == want.shape and out.dtype == want.dtype, what
    if not np.array_equal(out, want):
        bad = np.argwhere(out != want)
        raise AssertionError("%s: %d of %d elements differ from the host path in regions %s, first at %s" % (
            what, len(bad), out.size, sorted({int(b[0]) for b in bad})[:10], bad[0].tolist()))


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join(r))
def test_stream(L, streams, run_):
    """bytes = the host path's, status 0 everywhere; two calls on two streams share the scratch behind its event"""
    import torch
    name, dtype, layout = run_
    got = {}

    def on_frames(p, window, keys, frames):
        for size in W.SIZES[name]:
            regs = W.regions(W.frame_wh(name), size, len(frames))
            want = ubits(p.read_warp_regions(window, regs, size, W.PAD))
            st, st2 = side_stream(), side_stream()
            with torch.cuda.stream(st):
                rec = torch.tensor(records(regs), dtype=torch.int32, device="cuda")
                view, status = p.warp_regions_device(window, rec, size, W.PAD)
            with torch.cuda.stream(st2):
                rec2 = torch.tensor(records(regs[::-1]), dtype=torch.int32, device="cuda")
                view2, status2 = p.warp_regions_device(window, rec2, size, W.PAD, stream=st2)
            st.synchronize()
            st2.synchronize()
            got[size] = (want, ubits(view), status.cpu().numpy(), ubits(view2), status2.cpu().numpy())
    run(L, streams(name), dtype, layout, on_frames).close()
    for size, (want, out, status, out2, status2) in got.items():
        what = "%s %s %s %s" % (name, size, dtype, layout)
        assert (status == 0).all() and (status2 == 0).all(), (what, status, status2)
        assert_same(out, want, what)
        assert_same(out2, want[::-1], what + " (reversed, second stream)")


def test_refused_regions_among_good_ones(L, streams):
    """non-zero status exactly at the refused positions and equal to warp_region_status; their bytes, the gaps up to an explicit pitch
    and everything behind the last region still the canary's; the good regions equal the host path"""
    import torch
    name, size, dtype, layout, e = "608x57", (13, 37), "float16", "hwc", 2
    fw, fh = W.frame_wh(name)
    nbytes = 3 * size[0] * size[1] * e
    pitch = (nbytes + 255) // 256 * 256 + 256
    got = {}

    def on_frames(p, window, keys, frames):
        good = W.regions((fw, fh), size, len(frames))
        bad = [r for _, r, _, _ in W.refused_records(len(frames))] + [(-1, good[0][1], 0)]
        rec, at = [], []
        for i, g in enumerate(good):
            rec.append(g)
            if i < len(bad):
                at.append(len(rec))
                rec.append(bad[i])
        full = records(rec)
        n = len(rec)
        want_status = [L.warp_region_status(fw, fh, len(frames), L.PipelineWarpRegion(int(r[0]), (C.c_int32 * 6)(*[int(v) for v in r[1:7]]), int(r[7])), size) for r in full]
        want_good = ubits(p.read_warp_regions(window, good, size, W.PAD))
        st = side_stream()
        with torch.cuda.stream(st):
            buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
            status = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
            view, stat = p.warp_regions_device(window, torch.tensor(full, dtype=torch.int32, device="cuda"), size, W.PAD, out=buf, pitch=pitch, status=status)
        st.synchronize()
        got.update(at=at, n=n, want_status=want_status, want_good=want_good, raw=buf.cpu().numpy(), status=status.cpu().numpy(), view=ubits(view), n_bad=len(bad))
    run(L, streams(name), dtype, layout, on_frames).close()
    at, n, raw = got["at"], got["n"], got["raw"]
    assert got["status"][:n].tolist() == got["want_status"] and got["status"][n:].tolist() == [-9, -9]
    assert [i for i in range(n) if got["want_status"][i]] == at and len(at) == got["n_bad"] == 5
    assert [got["want_status"][i] for i in at] == [L.REGION_SCALE, L.REGION_FRAME, L.REGION_RESERVED, L.REGION_OFFSET, L.REGION_FRAME]
    good_at = [i for i in range(n) if i not in at]
    assert_same(got["view"][good_at], got["want_good"], "the good regions")
    for i in range(n):
        if i in at:
            assert (raw[i * pitch:(i + 1) * pitch] == CANARY).all(), "refused region %d was written" % i
        else:
            assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d was written" % i
    assert (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"


def test_the_call_is_refused_as_a_whole(L, streams):
    import torch
    name, size = "96x64", (8, 32)
    seen = []

    def on_frames(p, window, keys, frames):
        regs = W.regions(W.frame_wh(name), size, len(frames))
        rec = torch.tensor(records(regs), dtype=torch.int32, device="cuda")
        buf = torch.full((len(regs) * 2048 + 512,), CANARY, dtype=torch.uint8, device="cuda")
        status = torch.full((len(regs),), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def refused(word, **kw):
            args = dict(window=window, records=rec, size=size, out=buf, status=status)
            args.update(kw)
            with pytest.raises(L.LeonError) as e:
                p.warp_regions_device(args.pop("window"), args.pop("records"), args.pop("size"), W.PAD, **args)
            assert e.value.code == L.ERR_INVALID and word in str(e.value), str(e.value)
            torch.cuda.synchronize()
            assert bool((buf == CANARY).all()) and bool((status == -9).all()), "a refused call wrote (%s)" % word
            seen.append(word)
        refused("not out for delivery", window=window + 7)
        refused("out_pitch_bytes", pitch=1000)
        refused("not 256-byte aligned", out=buf[8:])
        refused("out_height", size=(0, 8))
        call = L.PipelineWarpRegionsCall(rec.data_ptr(), len(regs), 1, buf.data_ptr(), 0, status.data_ptr(), None)
        cfg = L.PipelineWarpConfig(32, 8)
        assert p.lib.leon_pipeline_warp_regions_device(p.h, window, C.byref(cfg), C.byref(call)) == L.ERR_INVALID and b"reserved word" in p.lib.leon_last_error()
        call = L.PipelineWarpRegionsCall(rec.data_ptr() + 2, len(regs), 0, buf.data_ptr(), 0, status.data_ptr(), None)
        assert p.lib.leon_pipeline_warp_regions_device(p.h, window, C.byref(cfg), C.byref(call)) == L.ERR_INVALID and b"4-byte aligned" in p.lib.leon_last_error()
        call = L.PipelineWarpRegionsCall(rec.data_ptr(), 0, 0, buf.data_ptr(), 0, status.data_ptr(), None)
        assert p.lib.leon_pipeline_warp_regions_device(p.h, window, C.byref(cfg), C.byref(call)) == L.ERR_INVALID and b"0 regions" in p.lib.leon_last_error()
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all())
        # stream NULL: the regions stream, and the call waits
        call = L.PipelineWarpRegionsCall(rec.data_ptr(), len(regs), 0, buf.data_ptr(), 0, status.data_ptr(), None)
        assert p.lib.leon_pipeline_warp_regions_device(p.h, window, C.byref(cfg), C.byref(call)) == L.OK
        assert bool((status == 0).all()) and not bool((buf[:256] == CANARY).all())
    run(L, streams(name), "float16", "chw", on_frames).close()
    assert len(seen) == 4
