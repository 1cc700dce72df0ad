"""CPU: what leon_pipeline_carry_device, leon_pipeline_gauge_kernel and leon_pipeline_propagate_kernel refuse before any device call,
by code AND text.  The GPU tests of the three (test_carry_kernel_gpu.py, test_gauge_kernel_gpu.py, test_propagate_kernel_gpu.py)
compare codes only; a caller sees the message.  The expected strings are literals, recorded from the library as it stood before the
three calls shared one stager and one table builder.  Every call is through the library itself (the wrappers ask motion_layout for the
grid first) on a 5 x 2 grid with an 80 x 32 frame and a window of three frames, with one good region or hop; every output array holds
a fill beforehand and afterwards."""
import ctypes as C

import numpy as np
import pytest

import carry_cases as K
import gauge_cases as G

FW, FH, MBW, MBH, N_FRAMES = 80, 32, 5, 2, 3
STRIDE, PLANES, ELEM, SLOTS = 2, 2, 2, 4
SLOT_BYTES = PLANES * (FH // STRIDE) * (FW // STRIDE) * ELEM


def geometry(a):
    """the arguments every call starts with"""
    a.update(device_id=0, fw=FW, fh=FH, mbw=MBW, mbh=MBH, n_frames=N_FRAMES)


def carry_good(L):
    """(the call's arguments by name, in the call's order; the names of its outputs)"""
    a = {}
    geometry(a)
    a["fwd"], a["bwd"] = np.array(K.FWD, dtype=np.int32), np.array(K.BWD, dtype=np.int32)
    a["records"], a["keep"] = L._carry_records(K.window(MBW, MBH, 31), MBW, MBH)
    a.update(regions=L._records_array([(0, 1, 1, 8, 8, 1)]), n=1, out=np.full((1, 8), -77, np.int32), votes=np.full((1, 4), -77, np.int32), status=np.full(1, -77, np.int32))
    return a, ("out", "votes", "status")


def gauge_good(L):
    a = {}
    geometry(a)
    motion, activity = G.window(MBW, MBH, 31)
    a["motion"], a["activity"], a["keep"] = L._gauge_records(motion, activity, MBW, MBH, N_FRAMES)
    a.update(cfg=L.PipelineGaugeConfig(3), regions=L._records_array([(1, 1, 1, 8, 8)]), n=1, stats=np.full((1, 16), -77, np.int64), status=np.full(1, -77, np.int32))
    return a, ("stats", "status")


def propagate_good(L):
    a = {}
    geometry(a)
    a["records"], a["keep"] = L._carry_records(K.window(MBW, MBH, 31), MBW, MBH)
    a["cfg"] = L.PipelinePropagateConfig(STRIDE, PLANES, ELEM, SLOTS, 0, 0, SLOT_BYTES, SLOTS * SLOT_BYTES)
    a.update(hops=L._records_array([(0, 3, 0, 1)]), n=1, maps=np.full(SLOTS * SLOT_BYTES + 4, 0xA5, np.uint8), via=np.full((1, FH // STRIDE, FW // STRIDE), 0xEE, np.uint8),
             status=np.full(1, -77, np.int32))
    return a, ("maps", "via", "status")


FAMILIES = {"carry": ("leon_pipeline_carry_device", carry_good), "gauge": ("leon_pipeline_gauge_kernel", gauge_good),
            "propagate": ("leon_pipeline_propagate_kernel", propagate_good)}


def put(**kw):
    return lambda a: a.update(kw)


def item(name, index, value):
    """one element of an array argument (a record pointer, a reference, a reserved word)"""
    def change(a):
        a[name][index] = value
    return change


def field(name, value):
    def change(a):
        setattr(a["cfg"], name, value)
    return change


def both(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


def cfg_reserved(a):
    a["cfg"].reserved[6] = 1


def odd_maps(a):
    a["maps_offset"] = 2


# ---- what the three calls refuse alike: {name: a change of the good arguments} -----------------------------------------------------
COMMON = {
    "n_0": put(n=0),
    "n_minus_1": put(n=-1),
    "n_65536": put(n=65536),
    "frame_81x32": put(fw=FW + 1),
    "frame_80x33": put(fh=FH + 1),
    "mbw_0": put(mbw=0),
    "mbw_257": put(mbw=257),
    "n_frames_minus_1": put(n_frames=-1),
}
CASES = {
    "carry": dict(COMMON, **{
        "null_fwd": put(fwd=None), "null_bwd": put(bwd=None), "null_records": put(records=None), "null_regions": put(regions=None), "null_out": put(out=None),
        "fwd_3": item("fwd", 1, 3), "fwd_minus_2": item("fwd", 2, -2), "bwd_3": item("bwd", 2, 3), "bwd_minus_2": item("bwd", 0, -2),
        "voter_missing": item("records", 1, None),
    }),
    "gauge": dict(COMMON, **{
        "null_cfg": put(cfg=None), "null_regions": put(regions=None), "null_stats": put(stats=None), "null_motion": put(motion=None), "null_activity": put(activity=None),
        "sources_0": field("sources", 0), "sources_4": field("sources", 4), "cfg_reserved": cfg_reserved,
        "no_motion_sources_1": both(field("sources", 1), item("motion", 1, None)),
        "no_motion_sources_3": item("motion", 1, None),
        "no_activity_sources_2": both(field("sources", 2), item("activity", 1, None)),
    }),
    "propagate": dict(COMMON, **{
        "null_records": put(records=None), "null_cfg": put(cfg=None), "null_hops": put(hops=None), "null_maps": put(maps=None),
        "stride_3": field("stride", 3), "elem_bytes_3": field("elem_bytes", 3), "planes_0": field("planes", 0), "n_slots_0": field("n_slots", 0),
        "n_slots_65536": field("n_slots", 65536), "slot_pitch_below": field("slot_pitch_bytes", SLOT_BYTES - 4), "slot_pitch_odd": field("slot_pitch_bytes", SLOT_BYTES + 2),
        "maps_bytes_below": field("maps_bytes", SLOTS * SLOT_BYTES - 4), "cfg_reserved0": field("reserved0", 1), "maps_not_aligned": odd_maps,
        "target_missing": item("records", 0, None),
    }),
}

EXPECTED = {
    "carry": {
        "n_0": "carry regions: 0 regions (a call takes 1 .. 65535)",
        "n_minus_1": "carry regions: -1 regions (a call takes 1 .. 65535)",
        "n_65536": "carry regions: 65536 regions (a call takes 1 .. 65535)",
        "frame_81x32": "carry: a frame of 81 x 32 in a grid of 5 x 2 macroblocks",
        "frame_80x33": "carry: a frame of 80 x 33 in a grid of 5 x 2 macroblocks",
        "mbw_0": "carry: 0 x 2 macroblocks (1 .. 256 each)",
        "mbw_257": "carry: 257 x 2 macroblocks (1 .. 256 each)",
        "n_frames_minus_1": "carry: -1 frames",
        "null_fwd": "null argument",
        "null_bwd": "null argument",
        "null_records": "null argument",
        "null_regions": "null argument",
        "null_out": "null argument",
        "fwd_3": "carry: frame 1 points into frames 3 and -1 of 3",
        "fwd_minus_2": "carry: frame 2 points into frames -2 and 0 of 3",
        "bwd_3": "carry: frame 2 points into frames 0 and 3 of 3",
        "bwd_minus_2": "carry: frame 0 points into frames -1 and -2 of 3",
        "voter_missing": "carry: frame 1 votes (frame 0 to 1) and has no record",
    },
    "gauge": {
        "n_0": "gauge regions: 0 regions (a call takes 1 .. 65535)",
        "n_minus_1": "gauge regions: -1 regions (a call takes 1 .. 65535)",
        "n_65536": "gauge regions: 65536 regions (a call takes 1 .. 65535)",
        "frame_81x32": "carry: a frame of 81 x 32 in a grid of 5 x 2 macroblocks",
        "frame_80x33": "carry: a frame of 80 x 33 in a grid of 5 x 2 macroblocks",
        "mbw_0": "carry: 0 x 2 macroblocks (1 .. 256 each)",
        "mbw_257": "carry: 257 x 2 macroblocks (1 .. 256 each)",
        "n_frames_minus_1": "carry: -1 frames",
        "null_cfg": "null argument",
        "null_regions": "null argument",
        "null_stats": "null argument",
        "null_motion": "null argument",
        "null_activity": "null argument",
        "sources_0": "gauge regions: sources 0 (LEON_GAUGE_MOTION | LEON_GAUGE_ACTIVITY: 1 .. 3)",
        "sources_4": "gauge regions: sources 4 (LEON_GAUGE_MOTION | LEON_GAUGE_ACTIVITY: 1 .. 3)",
        "cfg_reserved": "gauge regions: a reserved word of the config is not 0",
        "no_motion_sources_1": "gauge: frame 1 has no motion record",
        "no_motion_sources_3": "gauge: frame 1 has no motion record",
        "no_activity_sources_2": "gauge: frame 1 has no activity record",
    },
    "propagate": {
        "n_0": "propagate maps: 0 hops (a call takes 1 .. 65535)",
        "n_minus_1": "propagate maps: -1 hops (a call takes 1 .. 65535)",
        "n_65536": "propagate maps: 65536 hops (a call takes 1 .. 65535)",
        "frame_81x32": "carry: a frame of 81 x 32 in a grid of 5 x 2 macroblocks",
        "frame_80x33": "carry: a frame of 80 x 33 in a grid of 5 x 2 macroblocks",
        "mbw_0": "carry: 0 x 2 macroblocks (1 .. 256 each)",
        "mbw_257": "carry: 257 x 2 macroblocks (1 .. 256 each)",
        "n_frames_minus_1": "carry: -1 frames",
        "null_records": "null argument",
        "null_cfg": "null argument",
        "null_hops": "null argument",
        "null_maps": "null argument",
        "stride_3": "propagate: stride 3 (1, 2, 4, 8, 16), 2 planes (1 .. 4096), elem_bytes 2 (1, 2, 4)",
        "elem_bytes_3": "propagate: stride 2 (1, 2, 4, 8, 16), 2 planes (1 .. 4096), elem_bytes 3 (1, 2, 4)",
        "planes_0": "propagate: stride 2 (1, 2, 4, 8, 16), 0 planes (1 .. 4096), elem_bytes 2 (1, 2, 4)",
        "n_slots_0": "propagate: 0 slots (1 .. 65535)",
        "n_slots_65536": "propagate: 65536 slots (1 .. 65535)",
        "slot_pitch_below": "propagate: slot_pitch_bytes 2556 (a multiple of 4 not below the map's 2560 bytes)",
        "slot_pitch_odd": "propagate: slot_pitch_bytes 2562 (a multiple of 4 not below the map's 2560 bytes)",
        "maps_bytes_below": "propagate: maps_bytes 10236 is below 4 slots of 2560 bytes",
        "cfg_reserved0": "propagate: a reserved word of cfg is not 0",
        "maps_not_aligned": "propagate: maps MAPS is not 4-byte aligned",          # MAPS: the pointer the call was given, as %p prints it
        "target_missing": "propagate: frame 0 is the target of hop 0 and has no record",
    },
}


def call(L, family, change=None):
    """one call -> (code, message, {output: (array, what it held beforehand)})"""
    symbol, good = FAMILIES[family]
    a, outputs = good(L)
    before = {name: a[name].copy() for name in outputs}
    arrays = {name: a[name] for name in outputs}
    if change:
        change(a)
    args = []
    for name, v in a.items():
        if name == "keep" or name == "maps_offset":
            continue
        if isinstance(v, np.ndarray):
            v = v.ctypes.data + (a.get("maps_offset", 0) if name == "maps" else 0)
        elif isinstance(v, C.Structure):
            v = C.byref(v)
        args.append(v)
    lib = L.load()
    rc = getattr(lib, symbol)(*args)
    return rc, lib.leon_last_error().decode(), {name: (arrays[name], before[name]) for name in outputs}


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


@pytest.mark.parametrize("family,name", [(f, n) for f in EXPECTED for n in EXPECTED[f]])
def test_refusal(L, family, name):
    code, message, outputs = call(L, family, CASES[family][name])
    assert code == L.ERR_INVALID
    assert message == EXPECTED[family][name].replace("MAPS", "0x%x" % (outputs["maps"][0].ctypes.data + 2) if family == "propagate" else "")
    for what, (now, before) in outputs.items():
        assert np.array_equal(now, before), "a refused call wrote %s" % what


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_good_call_is_not_refused(L, family):
    """with a device it runs; without one it fails at the first device call, behind every refusal"""
    code, message, _ = call(L, family)
    assert code in (L.OK, L.ERR_HIP), message


def test_every_case_has_its_text():
    assert all(set(EXPECTED[f]) == set(CASES[f]) for f in CASES) and set(EXPECTED) == set(CASES)
