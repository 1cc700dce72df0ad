"""GPU: the two device roads against each other.  leon_pipeline_resample_regions_device (stretch and letterbox) and
leon_pipeline_warp_regions_device share one enqueue bracket over one scratch (boxes_dev behind boxes_done, the staged frame ids): four
calls, alternating between the roads and between two side streams, are enqueued with no host wait between them, each into a buffer of
its own, and both streams are synchronised once at the end.  Then one host-road call, which must still return its bytes.  The expected
bytes are the host road's of the same build, taken before the enqueues -- tests/test_pipeline_regions_gpu.py,
test_pipeline_regions_fit_gpu.py and test_pipeline_warp_gpu.py pin those to the oracle.  Bit patterns, equality; every status word 0."""
import numpy as np
import pytest

import warp_structure as W
from regions_structure import CALLS, TRIANGLE
from resample_structure import STREAMS
from test_pipeline_gpu import ibbp_stream
from test_pipeline_regions_device_gpu import side_stream, ubits
from test_pipeline_regions_gpu import run
from test_pipeline_warp_device_gpu import assert_same, records

pytestmark = pytest.mark.gpu

NAME, DTYPE, LAYOUT, FILT = "96x64", "uint8", "hwc", TRIANGLE
ANGLE = 7.0          # degrees: the out size's box about each region's centre, turned a little


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def warp_regions(L, regs, size):
    """[(frame, m)]: per region (frame, x, y, w, h) the box of the out size about the region's centre, rotated by ANGLE"""
    return [(f, L.warp_matrix_rotated_box(x + w / 2.0, y + h / 2.0, size[1], size[0], ANGLE, size)) for f, x, y, w, h in regs]


def test_the_roads_interleaved_on_two_streams(L):
    import torch
    call = CALLS[NAME]
    size = call.size
    cw, ch, gops, seed, (fw, fh) = STREAMS[NAME]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = call.regions(len(frames))
        warps = warp_regions(L, regs, size)
        want = dict(stretch=ubits(p.read_regions(window, regs, size, FILT)),
                    fit=ubits(p.read_regions(window, regs, size, FILT, fit="letterbox", pad_value=W.PAD)),
                    warp=ubits(p.read_warp_regions(window, warps, size, W.PAD)))
        s1, s2 = side_stream(), side_stream()
        boxes = torch.tensor(regs, dtype=torch.int32, device="cuda")
        recs = torch.tensor(records(warps), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # the inputs are there; from here on no host wait until both streams are synchronised
        a = p.resample_regions_device(window, boxes, size, FILT, stream=s1)
        b = p.warp_regions_device(window, recs, size, W.PAD, stream=s2)
        c = p.resample_regions_device(window, boxes, size, FILT, stream=s2, fit="letterbox", pad_value=W.PAD)
        d = p.warp_regions_device(window, recs, size, W.PAD, stream=s1)
        s1.synchronize()
        s2.synchronize()
        assert len({t[0].data_ptr() for t in (a, b, c, d)}) == 4
        got.update(want=want, out=[(ubits(v), s.cpu().numpy()) for v, s in (a, b, c, d)], after=ubits(p.read_regions(window, regs, size, FILT)))
    run(L, ibbp_stream(cw, ch, gops, seed=seed, frame=(fw, fh)), DTYPE, LAYOUT, on_frames).close()
    want = got["want"]
    assert not np.array_equal(want["stretch"], want["fit"]) and not np.array_equal(want["stretch"], want["warp"])
    for (out, status), road, what in zip(got["out"], ("stretch", "warp", "fit", "warp"),
                                         ("1: stretch on s1", "2: warp on s2", "3: letterbox on s2", "4: warp on s1")):
        assert status.shape == (len(want[road]),) and (status == 0).all(), (what, status)
        assert_same(out, want[road], what)
    assert_same(got["after"], want["stretch"], "the host road behind the device roads")
