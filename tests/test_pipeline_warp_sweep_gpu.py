"""GPU: k_warp<element bytes, layout> across the legal record set -- tests/warp_structure.py: sweep, about 100 records per stream and
out size: shear, anisotropic scale, rank 1 and rank 0, reflections, records on the thresholds of warp_supersample, footprints 21
groups wide and 81 row pairs high, footprints of more than one staging pass at every width from 4 groups on, pieces cut by two frame
edges at S = 2 and 4, the offset limits, seeded random records (tests/test_warp_sweep_structure.py proves on the CPU what they hold).  Built like tests/test_pipeline_warp_gpu.py, whose helpers
these are: expected values are the ORACLE's RGBA of the region's frame through leon_ctypes.warp_rgb and the element table, compared
as bit patterns, no tolerance, no record skipped; the device road's bytes are the host road's, its status words
leon_pipeline_warp_region_status's."""
import ctypes as C

import pytest

import warp_structure as W
from test_pipeline_regions_device_gpu import side_stream, ubits
from test_pipeline_regions_gpu import CANARY, FORMATS, run
from test_pipeline_tensor_format_gpu import bits
from test_pipeline_warp_device_gpu import records
from test_pipeline_warp_gpu import L, assert_named_regions, check_stream, streams, want_regions          # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

SWEEP = (W.sweep, W.sweep_regions)
RUNS = [(name, d, l) for name in sorted(W.SIZES) for d, l in FORMATS]


@pytest.mark.parametrize("run_", RUNS, ids=lambda r: "-".join(r))
def test_sweep(L, streams, run_):
    """one read_warp_regions call per out size with the whole sweep, S = 1, 2 and 4 and both levels side by side in one launch"""
    name, dtype, layout = run_
    check_stream(L, streams, name, dtype, layout, regions=SWEEP)


def test_sweep_bfloat16(L, streams):
    check_stream(L, streams, "100x57", "bfloat16", "chw", regions=SWEEP)


@pytest.mark.parametrize("name,dtype,layout", [(n, d, l) for n in ("608x57", "100x57") for d, l in (("uint8", "hwc"), ("float16", "chw"))],
                         ids=lambda v: str(v))
def test_sweep_from_device_records(L, streams, name, dtype, layout):
    """the sweep's records interleaved with the refused side of the thresholds (W.sweep_refused), from device memory into a canary
    buffer at an explicit pitch: the status words are warp_region_status's for every record, a refused region's whole pitch is still
    the canary's, the good regions are the host road's bytes, the gaps and the tail untouched"""
    import torch
    fw, fh = W.frame_wh(name)
    e = 1 if dtype == "uint8" else 2
    got = {}

    def on_frames(p, window, keys, frames):
        for size in W.SIZES[name]:
            nbytes = 3 * size[0] * size[1] * e
            pitch = (nbytes + 255) // 256 * 256 + 256
            good = W.sweep_regions((fw, fh), size, len(frames))
            bad = W.sweep_refused(len(frames))
            rec, at, stated = [], [], []
            for i, g in enumerate(good):          # a refused record behind every ninth good one
                rec.append(g)
                if i % 9 == 4 and len(at) < len(bad):
                    at.append(len(rec))
                    rec.append(bad[len(at) - 1][1])
                    stated.append(bad[len(at) - 1][2])
            assert len(at) == len(bad)
            full = records(rec)
            n = len(rec)
            want_status = [L.warp_region_status(fw, fh, len(frames), L.PipelineWarpRegion(int(r[0]), (C.c_int32 * 6)(*[int(v) for v in r[1:7]]), int(r[7])), size) for r in full]
            want_good = ubits(p.read_warp_regions(window, good, size, W.PAD))
            st = side_stream()
            with torch.cuda.stream(st):
                buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
                status = torch.full((n + 2,), -9, dtype=torch.int32, device="cuda")
                view, _ = p.warp_regions_device(window, torch.tensor(full, dtype=torch.int32, device="cuda"), size, W.PAD, out=buf, pitch=pitch, status=status)
            st.synchronize()
            got[size] = dict(at=at, n=n, stated=stated, want_status=want_status, want_good=want_good, raw=buf.cpu().numpy(), status=status.cpu().numpy(),
                             view=ubits(view), nbytes=nbytes, pitch=pitch)
    run(L, streams(name)[0], dtype, layout, on_frames).close()
    assert sorted(got) == sorted(W.SIZES[name])
    for size, r in got.items():
        at, n, raw, nbytes, pitch = r["at"], r["n"], r["raw"], r["nbytes"], r["pitch"]
        what = "%s %s %s %s" % (name, size, dtype, layout)
        assert r["status"][:n].tolist() == r["want_status"] and r["status"][n:].tolist() == [-9, -9], what
        assert [i for i in range(n) if r["want_status"][i]] == at and [r["want_status"][i] for i in at] == r["stated"] and len(at) == 10, what
        good_at = [i for i in range(n) if i not in at]
        names = [nm for nm, _ in W.sweep((fw, fh), size)]
        assert_named_regions(r["view"][good_at], r["want_good"], names, layout, what + " against the host road")
        for i in range(n):
            if i in at:
                assert (raw[i * pitch:(i + 1) * pitch] == CANARY).all(), "%s: refused region %d was written" % (what, i)
            else:
                assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "%s: the gap behind region %d was written" % (what, i)
        assert (raw[n * pitch:] == CANARY).all(), "%s: bytes behind the last region were written" % what


@pytest.mark.parametrize("dtype,layout", [("uint8", "chw"), ("float16", "hwc")])
def test_caller_pitch_and_canary_on_the_widest_and_tallest(L, streams, dtype, layout):
    """the widest and the tallest level-0 footprints (21 groups of 8 columns by 2 row pairs; 81 row pairs by 2 groups: one staging pass
    each, the one that uses the most lanes of a row and the one that uses the most rows) and the rank-0 records into a caller's buffer
    filled with a canary, regions default pitch + 256 apart: each region's bytes are the expected ones, every byte between region_bytes and the pitch and behind the last region is the canary's"""
    import torch
    name, size = "100x57", (24, 70)
    data, rgba = streams(name)
    e = 1 if dtype == "uint8" else 2
    nbytes = 3 * size[0] * size[1] * e
    dflt = (nbytes + 255) // 256 * 256
    assert nbytes < dflt
    pitch = dflt + 256
    sweep = dict(W.sweep(W.frame_wh(name), size))
    names = ["widest", "tallest", "rank0_inside", "rank0_corner"]
    got = {}

    def on_frames(p, window, keys, frames):
        regs = [((3 * i + 2) % len(frames), sweep[n]) for i, n in enumerate(names)]
        n = len(regs)
        assert p.region_bytes(size) == (nbytes, dflt)
        buf = torch.full((n * pitch + 512,), CANARY, dtype=torch.uint8, device="cuda")
        view = p.warp_regions(window, regs, size, W.PAD, out=buf, pitch=pitch)
        shape = (n,) + ((size[0], size[1], 3) if layout == "hwc" else (3, size[0], size[1]))
        assert tuple(view.shape) == shape and view.dtype == getattr(torch, dtype) and view.data_ptr() == buf.data_ptr() and view.stride(0) * e == pitch
        got.update(keys=keys, regs=regs, view=bits(view.cpu().numpy()), raw=buf.cpu().numpy())
    run(L, data, dtype, layout, on_frames).close()
    want = want_regions(L, name, rgba, got["keys"], got["regs"], size, dtype, layout)
    assert len({w.tobytes() for w in want}) == len(names)          # four different images, none of them all pad
    assert_named_regions(got["view"], want, names, layout, "the view over the caller's buffer")
    raw, n = got["raw"], len(names)
    for i in range(n):
        assert raw[i * pitch:i * pitch + nbytes].tobytes() == want[i].tobytes(), names[i]
        assert (raw[i * pitch + nbytes:(i + 1) * pitch] == CANARY).all(), "the gap behind region %d (%s) was written" % (i, names[i])
    assert (raw[n * pitch:] == CANARY).all(), "bytes behind the last region were written"
