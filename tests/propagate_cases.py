"""Maps, hops and the expected result for the tests of leon_pipeline_propagate_maps (tests/test_pipeline_propagate_abi.py on the CPU,
tests/test_propagate_kernel_gpu.py and tests/test_pipeline_propagate_gpu.py on the device).  The oracle of all of them is
leon_ctypes.propagate_map: the header's text in numpy integers.  Elements are opaque bytes, so the maps are random bits of an
unsigned type of the element's size and everything is compared as such."""
import numpy as np

STRIDES = (1, 2, 4, 8, 16)
ELEMS = (1, 2, 4)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
VIA_FILL = 0xEE          # what a via map holds where nothing was written (not a via value)


def cells(fw, fh, s):
    return -(-fh // s), -(-fw // s)


def rand_maps(rng, slots, planes, fw, fh, s, e):
    """[slots, planes, mh, mw] of random bits"""
    mh, mw = cells(fw, fh, s)
    return rng.integers(0, 1 << (8 * e), size=(slots, planes, mh, mw), dtype=np.uint64).astype(UINT[e])


def pitched(maps, gap=0, sentinel=0xA5):
    """(a view [S, P, mh, mw] like `maps` whose slots lie apart by the map's bytes rounded up to a multiple of 4, plus gap; the byte
    buffer [S, pitch] under it, `sentinel` between the maps).  gap = 0: the least pitch the library takes for these maps."""
    S = maps.shape[0]
    slot_bytes = maps[0].nbytes
    assert gap % 4 == 0
    pitch = (slot_bytes + 3) // 4 * 4 + gap
    buf = np.full((S, pitch), sentinel, dtype=np.uint8)
    view = buf[:, :slot_bytes].view(maps.dtype).reshape(maps.shape)
    view[...] = maps
    assert view.ctypes.data == buf.ctypes.data and view.strides[0] == pitch
    return view, buf


def expected(L, fw, fh, n_frames, records, hops, stride, maps, fill=0):
    """(maps after the hops, via [n, mh, mw] with VIA_FILL where a record is refused, status [n]) by propagate_map on a copy"""
    want = np.array(maps, copy=True)
    via = np.full((len(hops),) + maps.shape[2:], VIA_FILL, dtype=np.uint8)
    status = np.zeros(len(hops), dtype=np.int64)
    for i, h in enumerate(hops):
        st, v = L.propagate_map(fw, fh, n_frames, records, h, stride, want, fill)
        status[i] = st
        if st == 0:
            via[i] = v
    return want, via, status


def assert_equal(got, want, what=""):
    """got, want = (maps, via, status); via may be None on both sides"""
    for name, g, w in zip(("maps", "via", "status"), got, want):
        if g is None and name == "via":
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "status":
            g, w = g.astype(np.int64), w.astype(np.int64)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            raise AssertionError("%s: %s differs in %d places, first at %s: %s, expected %s" % (what, name, len(at), at[0].tolist(), g[tuple(at[0])], w[tuple(at[0])]))
