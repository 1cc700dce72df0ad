"""CPU: what leon_pipeline_accumulate_kernel refuses before any device call, by code AND text, in the manner of
tests/test_table_kernel_refusals.py.  Every call is through the library itself on a coded picture of 80 x 32 (a 5 x 2 grid) and a
window of three frames, with one good hop; every output array holds a fill beforehand and afterwards."""
import ctypes as C

import numpy as np
import pytest

import accumulate_cases as A
import carry_cases as K

CW, CH, MBW, MBH, N_FRAMES, SLOTS = 80, 32, 5, 2, 3, 4


@pytest.fixture(scope="module")
def L():
    import leon_ctypes
    leon_ctypes.load()
    return leon_ctypes


def good(L):
    """the call's arguments by name, in the call's order"""
    lay = L.accumulate_layout(CW, CH, 3)
    a = dict(device_id=0, cw=CW, ch=CH, n_frames=N_FRAMES)
    a["motion"], k1 = L._carry_records(K.window(MBW, MBH, 31), MBW, MBH)
    a["residual"], k2 = L._residual_records(A.residuals(np.random.default_rng(1), CW, CH, N_FRAMES), CW, CH)
    a["keep"] = (k1, k2)
    a["cfg"] = L.PipelineAccumulateConfig(3, SLOTS, (C.c_int32 * 2)(0, 0), lay.slot_bytes, SLOTS * lay.slot_bytes)
    a.update(hops=L._records_array([(1, 3, 0, 1)]), n=1, slots=np.full(SLOTS * lay.slot_bytes + 4, 0xA5, np.uint8), via=np.full((1, MBH, MBW), 0xEE, np.uint8),
             status=np.full(1, -77, np.int32))
    return a, lay


def put(**kw):
    return lambda a: a.update(kw)


def item(name, index, value):
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
    a["cfg"].reserved[1] = 1


SLOT_BYTES = 3 * 2 * 128 * 32 + 2 * 128 * 32 + 2 * 2 * 64 * 16          # 80 pads to 128, 40 to 64
CASES = {
    "n_0": (put(n=0), "accumulate: 0 hops (a call takes 1 .. 65535)"),
    "n_minus_1": (put(n=-1), "accumulate: -1 hops (a call takes 1 .. 65535)"),
    "n_65536": (put(n=65536), "accumulate: 65536 hops (a call takes 1 .. 65535)"),
    "size_81x32": (put(cw=CW + 1), "accumulate: a coded size of 81 x 32 (multiples of 16)"),
    "size_80x40": (put(ch=40), "accumulate: a coded size of 80 x 40 (multiples of 16)"),
    "size_0x32": (put(cw=0), "accumulate: a coded size of 0 x 32 (multiples of 16)"),
    "size_4112x32": (put(cw=4112), "accumulate: 257 x 2 macroblocks (1 .. 256 each)"),
    "n_frames_minus_1": (put(n_frames=-1), "accumulate: -1 frames"),
    "null_motion": (put(motion=None), "null argument"),
    "null_cfg": (put(cfg=None), "null argument"),
    "null_hops": (put(hops=None), "null argument"),
    "null_slots": (put(slots=None), "null argument"),
    "null_residual_parts_3": (put(residual=None), "accumulate: null residual records with LEON_ACCUMULATE_RESIDUAL"),
    "parts_0": (field("parts", 0), "accumulate: parts 0 (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3)"),
    "parts_4": (field("parts", 4), "accumulate: parts 4 (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3)"),
    "cfg_reserved": (cfg_reserved, "accumulate: a reserved word of cfg is not 0"),
    "n_slots_0": (field("n_slots", 0), "accumulate: 0 slots (1 .. 65535)"),
    "n_slots_65536": (field("n_slots", 65536), "accumulate: 65536 slots (1 .. 65535)"),
    "slot_pitch_below": (field("slot_pitch_bytes", SLOT_BYTES - 4), "accumulate: slot_pitch_bytes %d (a multiple of 4 not below the accumulator's %d bytes)" % (SLOT_BYTES - 4, SLOT_BYTES)),
    "slot_pitch_odd": (field("slot_pitch_bytes", SLOT_BYTES + 2), "accumulate: slot_pitch_bytes %d (a multiple of 4 not below the accumulator's %d bytes)" % (SLOT_BYTES + 2, SLOT_BYTES)),
    "slots_bytes_below": (field("slots_bytes", SLOTS * SLOT_BYTES - 4), "accumulate: slots_bytes %d is below 4 slots of %d bytes" % (SLOTS * SLOT_BYTES - 4, SLOT_BYTES)),
    "slots_not_aligned": (put(slots_offset=2), "accumulate: slots SLOTS is not 4-byte aligned"),          # SLOTS: the pointer the call was given, as %p prints it
    "motion_missing": (item("motion", 1, None), "accumulate: frame 1 is the target of hop 0 and has no motion record"),
    "residual_missing": (item("residual", 1, None), "accumulate: frame 1 is the target of hop 0 and has no residual record"),
}


def call(L, change=None):
    """one call -> (code, message, {output: (array, what it held beforehand)})"""
    a, lay = good(L)
    assert lay.slot_bytes == SLOT_BYTES
    outputs = ("slots", "via", "status")
    before = {name: a[name].copy() for name in outputs}
    arrays = {name: a[name] for name in outputs}
    if change:
        change(a)
    args = []
    for name, v in a.items():
        if name in ("keep", "slots_offset"):
            continue
        if isinstance(v, np.ndarray):
            v = v.ctypes.data + (a.get("slots_offset", 0) if name == "slots" else 0)
        elif isinstance(v, C.Structure):
            v = C.byref(v)
        args.append(v)
    lib = L.load()
    rc = lib.leon_pipeline_accumulate_kernel(*args)
    return rc, lib.leon_last_error().decode(), {name: (arrays[name], before[name]) for name in outputs}


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(L, name):
    change, text = CASES[name]
    code, message, outputs = call(L, change)
    assert code == L.ERR_INVALID
    assert message == text.replace("SLOTS", "0x%x" % (outputs["slots"][0].ctypes.data + 2))
    for what, (now, before) in outputs.items():
        assert np.array_equal(now, before), "a refused call wrote %s" % what


def test_a_refused_hop_needs_no_record(L):
    """a hop whose status is not 0 reads nothing: its target's records may be missing, and the call gets as far as the device"""
    code, message, _ = call(L, both(item("motion", 1, None), item("residual", 1, None), lambda a: a.update(hops=L._records_array([(1, 3, 3, 1)]))))
    assert code in (L.OK, L.ERR_HIP), message


def test_the_motion_part_needs_no_residual_records(L):
    def change(a):
        a["cfg"].parts = 1
        a["residual"] = None
    code, message, _ = call(L, change)
    assert code in (L.OK, L.ERR_HIP), message


def test_the_good_call_is_not_refused(L):
    """with a device it runs; without one it fails at the first device call, behind every refusal"""
    code, message, _ = call(L)
    assert code in (L.OK, L.ERR_HIP), message
