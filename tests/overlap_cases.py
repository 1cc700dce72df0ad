"""The cases of the suppress and match tests (leon_pipeline_suppress_regions, leon_pipeline_match_regions), shared by the CPU and the
GPU files, each with what it asserts about ITSELF through the definitions in Python integers (leon_ctypes.suppress_boxes,
match_boxes), so that no case can pass empty: a chain really keeps its third row, a random set really keeps and suppresses rows, a
second-best case really falls to the second best.  The expected arrays of a case are computed once and shared (expected_suppress,
expected_match): the sentinel FILL stands wherever the definition writes nothing."""
import functools

import numpy as np

FILL = -77
IOU, IOMIN = 0, 1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
THREADS = 256                       # leon_overlap.h's kOverlapThreads


def row(x, y, w, h, frame=0, r0=0, r1=0, r2=0):
    return [frame, x, y, w, h, r0, r1, r2]


def terms(measure, a, b):
    """(inter, den) of two (x, y, w, h) boxes, written out once more for the cases' own assertions"""
    iw = max(min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]), 0)
    ih = max(min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]), 0)
    inter = iw * ih
    return inter, (min(a[2] * a[3], b[2] * b[3]) if measure == IOMIN else a[2] * a[3] + b[2] * b[3] - inter)


# the single pairs at the edges: (name, frame, a, b, measure, the largest threshold the pair reaches or 0 for none)
PAIRS = [
    ("3x1 shifted by 1", (64, 64), (0, 0, 3, 1), (1, 0, 3, 1), IOU, 32768),
    ("4x4 touching", (64, 64), (0, 0, 4, 4), (4, 0, 4, 4), IOU, 0),
    ("4x4 touching, iomin", (64, 64), (0, 0, 4, 4), (4, 0, 4, 4), IOMIN, 0),
    ("8x8 inside 64x64, iomin", (64, 64), (16, 16, 8, 8), (0, 0, 64, 64), IOMIN, 65536),
    ("8x8 inside 64x64, iou", (64, 64), (16, 16, 8, 8), (0, 0, 64, 64), IOU, 1024),
    ("identical", (352, 240), (17, 31, 40, 23), (17, 31, 40, 23), IOU, 65536),
    ("identical, iomin", (352, 240), (17, 31, 40, 23), (17, 31, 40, 23), IOMIN, 65536),
    ("1x1 on itself", (352, 240), (351, 239, 1, 1), (351, 239, 1, 1), IOU, 65536),
    ("1x1 beside 1x1", (352, 240), (350, 239, 1, 1), (351, 239, 1, 1), IOU, 0),
    ("4096x4096 on itself", (4096, 4096), (0, 0, 4096, 4096), (0, 0, 4096, 4096), IOU, 65536),
    ("4096x4096 on 4095x4096", (4096, 4096), (0, 0, 4096, 4096), (1, 0, 4095, 4096), IOU, 65520),
    ("4096x4096 on 4095x4096, iomin", (4096, 4096), (0, 0, 4096, 4096), (1, 0, 4095, 4096), IOMIN, 65536),
]


def pair_thresholds(reach):
    """t - 1, t and t + 1 around the largest threshold reached, inside 1 .. 65536; for a pair that reaches none: 1 and 2"""
    return [t for t in ((reach - 1, reach, reach + 1) if reach else (1, 2)) if 1 <= t <= 65536]


def check_pairs():
    for name, _, a, b, measure, reach in PAIRS:
        inter, den = terms(measure, a, b)
        assert (inter * 65536 // den if inter else 0) == reach or (reach == 65536 and inter == den), name
        for t in pair_thresholds(reach):
            assert (inter * 65536 >= t * den) == (reach != 0 and t <= reach), (name, t)


def random_rows(n, k, fw, fh, lo, hi, seed, frames=1):
    g = np.random.default_rng(seed)
    w, h = g.integers(lo, hi + 1, size=(n, k)), g.integers(lo, hi + 1, size=(n, k))
    x, y = (g.random((n, k)) * (fw - w + 1)).astype(np.int64), (g.random((n, k)) * (fh - h + 1)).astype(np.int64)
    r = np.zeros((n, k, 8), dtype=np.int32)
    r[..., 0], r[..., 1], r[..., 2], r[..., 3], r[..., 4] = g.integers(0, frames, size=(n, k)), x, y, w, h
    return r


def refused_rows(fw, fh, n_frames):
    """every status word a row can get, each with the first fault that decides it: (row, status)"""
    return [(row(0, 0, 8, 8, r0=1), 1), (row(0, 0, 8, 8, r1=-1), 1), (row(0, 0, 8, 8, r2=7), 1), (row(0, 0, 0, 0, frame=-1, r0=5), 1),      # RESERVED before FRAME and BOX
            (row(0, 0, 8, 8, frame=-1), 2), (row(0, 0, 8, 8, frame=n_frames), 2), (row(0, 0, 0, 0, frame=I32_MAX), 2),                      # FRAME before BOX
            (row(0, 0, 0, 8), 3), (row(0, 0, 8, 0), 3), (row(-1, 0, 8, 8), 3), (row(0, -1, 8, 8), 3), (row(fw - 7, 0, 8, 8), 3), (row(0, fh - 7, 8, 8), 3),
            (row(0, 0, I32_MAX, 8), 3), (row(I32_MAX, 0, 1, 1), 3), (row(0, 0, -5, -5), 3),
            (row(0, 0, 0, 0), 3)]                                                                                                           # propose's filler


class Suppress:
    def __init__(self, name, frame, rows, scores=None, stride=1, threshold=32768, measure=IOU, n_frames=4, by=None, kept=None):
        self.name, (self.fw, self.fh), self.n_frames = name, frame, n_frames
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        if self.rows.ndim == 2:
            self.rows = self.rows[None]
        self.scores = None if scores is None else np.ascontiguousarray(scores, dtype=np.int32).reshape(-1)
        self.stride, self.threshold, self.measure = stride, threshold, measure
        self.by, self.kept = by, kept          # what the case states: by of set 0 written out, (least kept, least suppressed) per set

    def kw(self):
        return dict(scores=self.scores, score_stride=self.stride, threshold_q16=self.threshold, measure=self.measure)

    def set_scores(self, s):
        k = self.rows.shape[1]
        return None if self.scores is None else [int(self.scores[(s * k + i) * self.stride]) for i in range(k)]


class Match:
    def __init__(self, name, frame, a, b, threshold=32768, measure=IOU, n_frames=4, match_a=None, overlap=None, least=None):
        self.name, (self.fw, self.fh), self.n_frames = name, frame, n_frames
        self.a, self.b = (np.ascontiguousarray(v, dtype=np.int32) for v in (a, b))
        if self.a.ndim == 2:
            self.a, self.b = self.a[None], self.b[None]
        self.threshold, self.measure = threshold, measure
        self.match_a, self.overlap, self.least = match_a, overlap, least          # set 0 written out; the least pairs of every set

    def kw(self):
        return dict(threshold_q16=self.threshold, measure=self.measure)


@functools.lru_cache(maxsize=None)
def suppress_cases():
    cases = []
    for name, frame, a, b, measure, reach in PAIRS:
        for t in pair_thresholds(reach):
            cases.append(Suppress("pair %s at %d" % (name, t), frame, [row(*a), row(*b)], [1, 0], threshold=t, measure=measure, by=[-1, 0 if reach and t <= reach else -1]))
    # the third row is kept because its only suppressor was itself suppressed: what "suppress if any better row overlaps" gets wrong
    cases.append(Suppress("chain", (64, 64), [row(0, 0, 10, 10), row(4, 0, 10, 10), row(8, 0, 10, 10)], [3, 2, 1], threshold=int(0.4 * 65536), by=[-1, 0, -1]))
    cases.append(Suppress("chain, scores reversed", (64, 64), [row(0, 0, 10, 10), row(4, 0, 10, 10), row(8, 0, 10, 10)], [1, 2, 3], threshold=int(0.4 * 65536), by=[-1, 2, -1]))
    dup = [row(5, 5, 20, 20)] * 4 + [row(40, 5, 20, 20)] * 3
    cases.append(Suppress("ties: all scores equal", (64, 64), dup, [9] * 7, by=[-1, 0, 0, 0, -1, 4, 4]))
    cases.append(Suppress("ties: no scores", (64, 64), dup, None, by=[-1, 0, 0, 0, -1, 4, 4]))
    cases.append(Suppress("ties: no scores, stride 8", (64, 64), dup, None, stride=8, by=[-1, 0, 0, 0, -1, 4, 4]))
    cases.append(Suppress("scores INT32_MIN and INT32_MAX", (64, 64), dup, [I32_MIN, 0, I32_MAX, -1, I32_MIN, I32_MAX, I32_MIN + 1], by=[2, 2, -1, 2, 5, -1, 5]))
    info = np.array([[3, 100], [9, 101], [5, 102], [9, 103], [1, 104], [2, 105], [8, 106]], dtype=np.int32)          # {cells, first}: the cells are the score
    cases.append(Suppress("score_stride 2 over info", (64, 64), dup, info, stride=2, by=[1, -1, 1, 1, 6, 6, -1]))
    for k in (1, 2, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1):
        r = random_rows(1, k, 1920, 1080, 16, 160, seed=k)
        cases.append(Suppress("K %d" % k, (1920, 1080), r, np.random.default_rng(k).integers(-50, 50, size=k), threshold=16384, measure=IOMIN,
                              kept=(1, 1 if k >= 63 else 0)))
    for n in (1, 3, 5):
        bad = refused_rows(352, 240, 4)
        r = random_rows(n, 24, 352, 240, 16, 96, seed=100 + n, frames=4)
        for s in range(n):
            for q, (b, _) in enumerate(bad):
                if (q + s) % 2 == 0 or s == n - 1:
                    r[s, (7 * q + s) % 24] = b
        if n > 1:
            r[1] = [bad[q % len(bad)][0] for q in range(24)]          # a set without one accepted row
        cases.append(Suppress("n %d with refused rows" % n, (352, 240), r, np.random.default_rng(n).integers(0, 5, size=n * 24), threshold=13107, measure=IOU))
    for k, frame, lo, hi in ((64, (352, 240), 16, 96), (1024, (1920, 1080), 16, 160)):
        for measure, t in ((IOU, 32768), (IOMIN, 49152)):
            frame_name = "%dx%d" % frame
            r = random_rows(1, k, frame[0], frame[1], lo, hi, seed=7 * k + measure)
            cases.append(Suppress("random %d in %s, measure %d" % (k, frame_name, measure), frame, r, np.random.default_rng(k + measure).integers(0, 1000, size=k),
                                  threshold=t, measure=measure, kept=(1, 1)))
    return cases


def grid_rows(k, fw, fh, seed, jitter):
    """k boxes of 20 x 20 on the cells of a 32-pixel grid, every cell at most once, in a seeded order, each moved by up to `jitter`"""
    g = np.random.default_rng(seed)
    cols, rows_ = fw // 32, fh // 32
    assert cols * rows_ >= k
    cells = np.arange(cols * rows_)
    r = np.zeros((1, k, 8), dtype=np.int32)
    r[0, :, 1] = 32 * (cells[:k] % cols) + g.integers(0, jitter + 1, size=k)
    r[0, :, 2] = 32 * (cells[:k] // cols) + g.integers(0, jitter + 1, size=k)
    r[0, :, 3:5] = 20
    return r


@functools.lru_cache(maxsize=None)
def match_cases():
    cases = []
    for name, frame, a, b, measure, reach in PAIRS:
        inter, den = terms(measure, a, b)
        for t in pair_thresholds(reach):
            hit = reach != 0 and t <= reach
            cases.append(Match("pair %s at %d" % (name, t), frame, [row(*a)], [row(*b)], threshold=t, measure=measure, match_a=[0 if hit else -1],
                               overlap=[inter * 65536 // den if hit else 0]))
    for ka, kb in ((5, 9), (9, 5), (1, 40), (40, 1)):
        cases.append(Match("Ka %d, Kb %d" % (ka, kb), (352, 240), random_rows(1, ka, 352, 240, 40, 120, seed=ka), random_rows(1, kb, 352, 240, 40, 120, seed=50 + kb),
                           threshold=6554, least=1))
    one, two = row(10, 10, 30, 30), row(12, 10, 30, 30)
    cases.append(Match("duplicates on both sides", (64, 64), [two, one, one, two, one], [one, one, two, one], threshold=32768, match_a=[2, 0, 1, -1, 3],
                       overlap=[65536, 65536, 65536, 0, 65536]))
    # A1's best partner is B0, which the better pair (A0, B0) takes: A1 falls to B1; A2 reaches nothing
    cases.append(Match("second best and unmatched", (64, 64), [row(0, 0, 10, 10), row(2, 0, 10, 10), row(40, 40, 10, 10)], [row(0, 0, 10, 10), row(6, 0, 10, 10), row(20, 40, 10, 10)],
                       threshold=int(0.3 * 65536), match_a=[0, 1, -1], overlap=[65536, 6 * 65536 // 14, 0]))
    same = np.tile(np.array(row(100, 100, 50, 40), dtype=np.int32), (1, 256, 1))
    cases.append(Match("256 x 256 identical", (352, 240), same, same, threshold=65536, match_a=list(range(256)), overlap=[65536] * 256))
    for k in (THREADS - 1, THREADS, THREADS + 1, 1024):
        a, b = grid_rows(k, 1920, 1080, seed=k, jitter=6), grid_rows(k, 1920, 1080, seed=k + 1, jitter=6)
        b[0] = b[0][np.random.default_rng(k).permutation(k)]
        cases.append(Match("sparse %d x %d" % (k, k), (1920, 1080), a, b, threshold=13107, measure=IOU, least=k // 2))
    for n in (1, 3, 5):
        bad = refused_rows(352, 240, 4)
        a, b = random_rows(n, 20, 352, 240, 40, 120, seed=200 + n, frames=4), random_rows(n, 31, 352, 240, 40, 120, seed=300 + n, frames=4)
        for s in range(n):
            for q, (r, _) in enumerate(bad):
                if (q + s) % 2 == 0:
                    a[s, (3 * q + s) % 20] = r
                else:
                    b[s, (5 * q + s) % 31] = r
        if n > 1:
            a[1] = [bad[q % len(bad)][0] for q in range(20)]          # a pair whose set of a has no accepted row
        cases.append(Match("n %d with refused rows" % n, (352, 240), a, b, threshold=6554, measure=IOMIN))
    for measure, t in ((IOU, 13107), (IOMIN, 32768)):
        cases.append(Match("random 64 x 64, measure %d" % measure, (352, 240), random_rows(1, 64, 352, 240, 16, 96, seed=11), random_rows(1, 64, 352, 240, 16, 96, seed=12),
                           threshold=t, measure=measure, least=8))
    return cases


def filled(values, shape):
    """a definition's list (None: not written) as an int32 array with FILL where nothing is written"""
    return np.array([FILL if v is None else v for v in values], dtype=np.int32).reshape(shape)


@functools.lru_cache(maxsize=None)
def expected_suppress(L, index):
    """(out [n, K, 8], order [n, K], by [n, K], count [n], status [n, K]) of case `index` by the definition, and the case's own assertions"""
    c = suppress_cases()[index]
    n, k = c.rows.shape[:2]
    outs = []
    for s in range(n):
        out, order, by, count, status = L.suppress_boxes(c.fw, c.fh, c.n_frames, c.rows[s].tolist(), c.set_scores(s), c.threshold, c.measure)
        accepted = sum(1 for v in status if v == 0)
        assert count == sum(1 for v in by if v == -1) and count <= accepted and (count > 0) == (accepted > 0), c.name
        if s == 0 and c.by is not None:
            assert by == c.by, (c.name, by)
        if c.kept is not None:
            assert count >= c.kept[0] and accepted - count >= c.kept[1], (c.name, count, accepted)
        outs.append((filled(sum(out, []), (k, 8)), filled(order, k), filled(by, k), count, filled(status, k)))
    got = tuple(np.stack([o[i] for o in outs]).astype(np.int32) for i in range(5))
    for g in got:
        g.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_match(L, index):
    """(match_a [n, Ka], match_b [n, Kb], overlap [n, Ka], count [n], status_a, status_b) of case `index` by the definition"""
    c = match_cases()[index]
    n, ka, kb = c.a.shape[0], c.a.shape[1], c.b.shape[1]
    outs = []
    for s in range(n):
        ma, mb, ov, count, sa, sb = L.match_boxes(c.fw, c.fh, c.n_frames, c.a[s].tolist(), c.b[s].tolist(), c.threshold, c.measure)
        assert count == sum(1 for v in ma if v is not None and v >= 0) == sum(1 for v in mb if v is not None and v >= 0), c.name
        assert all(mb[j] == i for i, j in enumerate(ma) if j is not None and j >= 0), c.name
        if s == 0 and c.match_a is not None:
            assert ma == c.match_a and ov == c.overlap, (c.name, ma, ov)
        if c.least is not None:
            assert count >= c.least, (c.name, count)
        outs.append((filled(ma, ka), filled(mb, kb), filled(ov, ka), count, filled(sa, ka), filled(sb, kb)))
    got = tuple(np.stack([o[i] for o in outs]).astype(np.int32) for i in range(6))
    for g in got:
        g.setflags(write=False)
    return got


def assert_equal(got, want, names, what):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, "%s: %s has shape %s, not %s" % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError("%s: %s differs in %d words, first at %s: %d, the definition has %d" % (what, name, int((g != w).sum()), at.tolist(), g[tuple(at)], w[tuple(at)]))


SUPPRESS_NAMES = ("out", "order", "by", "count", "status")
MATCH_NAMES = ("match_a", "match_b", "overlap", "count", "status_a", "status_b")
