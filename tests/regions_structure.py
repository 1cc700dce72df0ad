"""The calls of leon_pipeline_resample_regions that tests/test_regions_structure.py (the facts, CPU), tests/test_pipeline_regions_abi.py
(leon_pipeline_regions_check accepts them) and tests/test_pipeline_regions_gpu.py (k_regions) share: per stream of
resample_structure.STREAMS one out size and a list of boxes, chosen for what one launch of k_regions then holds side by side -- every
region with tables and tap counts of its own.  What each call is here for is proved from resample_structure.tile_facts, the kernel's
own expressions; nothing here touches a device.  A helper, not a test module."""
import resample_structure as R
from resample_structure import BICUBIC, TRIANGLE

FILTERS = (TRIANGLE, BICUBIC)


class Call:
    """stream: a key of resample_structure.STREAMS; size: (out_h, out_w) of every region; boxes: (x, y, w, h) in frame pixels;
    refused: a box the library refuses (ratio above 16), or None"""
    def __init__(self, stream, size, boxes, refused=None):
        self.stream, self.size, self.boxes, self.refused = stream, size, boxes, refused

    @property
    def frame(self):
        return R.frame_wh(self.stream)

    def tiles(self, box, filter):
        return R.tile_facts(self.frame, box, self.size, filter)

    def regions(self, n_frames, boxes=None):
        """[(frame index, x, y, w, h)]: the boxes dealt over every frame of a window of n_frames frames in an order that is not the
        frames' own (a stride of 4, which shares no factor with the 9 frames of the streams), the first frame taken twice: n_frames + 1
        regions, every box at least once"""
        boxes = self.boxes if boxes is None else boxes
        assert n_frames % 2 == 1 and n_frames + 1 >= len(boxes)
        order = [(4 * i + 2) % n_frames for i in range(n_frames)]
        assert sorted(order) == list(range(n_frames)) and order != sorted(order)
        order.append(order[0])
        return [(f,) + tuple(boxes[i % len(boxes)]) for i, f in enumerate(order)]

    def __repr__(self):
        return self.stream


CALLS = {
    # ratio 16 across (592 -> 37), identity, an enlargement of about 2; boxes on all four frame edges; the fill row of the odd height
    "608x57": Call("608x57", (13, 37), [(0, 0, 592, 57), (5, 3, 37, 13), (301, 20, 19, 7), (571, 0, 37, 57), (16, 0, 592, 52)], refused=(1, 44, 600, 13)),
    # the four corners, odd origins, one pixel enlarged, one tile per region
    "96x64": Call("96x64", (8, 32), [(0, 0, 96, 64), (0, 0, 33, 9), (63, 55, 33, 9), (0, 47, 17, 17), (79, 0, 17, 17), (31, 17, 32, 8), (40, 24, 16, 4), (95, 63, 1, 1)]),
    # the unfused road: a frame width that is no multiple of 8, an odd height
    "100x57": Call("100x57", (16, 24), [(0, 0, 100, 57), (3, 41, 49, 16), (75, 1, 25, 56), (50, 28, 24, 16), (0, 0, 12, 8)]),
}


def placement(size, element_bytes):
    """(region_bytes, the default pitch) of include/leon_pipeline.h: 3 * out_height * out_width * element bytes, rounded up to 256"""
    n = 3 * size[0] * size[1] * element_bytes
    return n, (n + 255) // 256 * 256
