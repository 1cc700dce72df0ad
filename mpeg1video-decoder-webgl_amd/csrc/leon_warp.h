// leon_warp.h -- one record of a warp call judged, and the integers every sample of it stands on (the definition of
// include/leon_pipeline.h, leon_pipeline_warp_regions), for the host (warp_regions_check, warp_region_status: leon_pipeline_impl.h)
// and the device (k_warp: leon_kernels.h): ONE text, as leon_resize_row.h is for the axis-aligned calls.  Integers only.
#ifndef LEON_WARP_H
#define LEON_WARP_H
#include <stdint.h>
#include "leon_resize_row.h"

namespace leon {

// the two status words a warp record adds to kRegion* (LEON_REGION_SCALE, LEON_REGION_OFFSET)
enum { kRegionScale = 7, kRegionOffset = 8 };

static constexpr int kWarpMaxLog2 = 2;                        // S = 1 << g <= 4
static constexpr int32_t kWarpMaxOffset = 1 << 29;            // |tx|, |ty|, Q16: 8192 pixels

struct WarpRecord {                      // = leon_pipeline_warp_region
    int32_t frame;
    int32_t m[6];                        // a00, a01, tx, a10, a11, ty in Q16
    int32_t reserved;
};

// g of the definition: the larger squared column norm of the matrix against (2^(16 + g) + 1)^2; -1: above the last threshold
LEON_HD inline int32_t warp_supersample(const int32_t* m)
{
    const int64_t a00 = m[0], a01 = m[1], a10 = m[3], a11 = m[4];
    const int64_t c0 = a00 * a00 + a10 * a10, c1 = a01 * a01 + a11 * a11;          // each <= 2^63: unsigned below
    const uint64_t s2 = (uint64_t)(c0 > c1 ? c0 : c1);
    for (int32_t g = 0; g <= kWarpMaxLog2; g++) {
        const uint64_t lim = ((uint64_t)1 << (16 + g)) + 1;
        if (s2 <= lim * lim) return g;
    }
    return -1;
}

// 0 exactly when leon_pipeline_warp_regions_check accepts the record alone; otherwise the first failing check in its order: the
// reserved word, the frame index, the scale, the offsets.  *g: the record's supersampling (valid with status 0).
LEON_HD inline int32_t warp_record_status(const WarpRecord& r, int32_t n_frames, int32_t* g)
{
    *g = 0;
    if (r.reserved) return kRegionReserved;
    if (r.frame < 0 || r.frame >= n_frames) return kRegionFrame;
    const int32_t gg = warp_supersample(r.m);
    if (gg < 0) return kRegionScale;
    // (INT32_MIN has no negative: compare on both sides)
    if (r.m[2] > kWarpMaxOffset || r.m[2] < -kWarpMaxOffset || r.m[5] > kWarpMaxOffset || r.m[5] < -kWarpMaxOffset) return kRegionOffset;
    *g = gg;
    return kRegionOk;
}

// The numerator of a sample position on one axis: (a, b, t) = (a00, a01, tx) or (a10, a11, ty); sub-sample (i, j) of output pixel
// (ox, oy); S = 1 << g.  Inside 2^36 for a judged record (|a|, |b| <= 2^18 + 1, coordinates below 2^12, |t| <= 2^29).
LEON_HD inline int64_t warp_numerator(int32_t a, int32_t b, int32_t t, int32_t g, int32_t ox, int32_t oy, int32_t i, int32_t j)
{
    const int64_t S2 = (int64_t)2 << g;
    return (int64_t)a * (S2 * ox + 2 * i + 1) + (int64_t)b * (S2 * oy + 2 * j + 1) + S2 * ((int64_t)t - 32768);
}
// ... and its position in 1/256 pixel: the pixel is q >> 8, the bilinear fraction q & 255 (arithmetic shifts)
LEON_HD inline int32_t warp_q(int64_t N, int32_t g)
{
    return (int32_t)(((N >> (g + 1)) + 128) >> 8);
}

// ---- how k_warp cuts a 32 x 8 tile into pieces whose source footprint fits its stage ---------------------------------------------
// A piece is pw x ph output pixels; the levels halve the tile in turn.  Its footprint is the bounding box of its four corner samples
// and their bilinear neighbours, aligned to 8 columns and even rows, staged at a row pitch of width + 1 dwords (odd: a rotation by
// 90 degrees walks down a column, and an even pitch would put a wave's 32 lanes on one or two banks).
static constexpr int kWarpStagePx = 8192;                     // dwords of the stage
// Of the five levels only 0 and 1 are reachable: with column norms of at most 2^18 + 1 the largest level-1 bound of any record the
// judgement lets through is (80 + 1) * 74 = 5994 dwords, so levels 2 to 4 have never run on a device and k_warp's row loop takes one
// trip.  tests/test_warp_sweep_structure.py (test_no_legal_record_takes_a_level_above_1) pins that number: raising kWarpMaxLog2 or
// shrinking the stage makes it fail before untested pieces start to run.
static constexpr int kWarpLevels = 5;
LEON_HD inline int32_t warp_piece_w(int32_t level) { return level < 1 ? 32 : level < 3 ? 16 : 8; }          // 32 16 16 8 8
LEON_HD inline int32_t warp_piece_h(int32_t level) { return level < 2 ? 8 : level < 4 ? 4 : 2; }            //  8  8  4 4 2
// An upper bound of a piece's aligned footprint on one axis from the matrix alone: the distance between the first and the last
// sample's numerators is at most |a| * (2S * (pw - 1) + 2S - 2) + |b| * (2S * (ph - 1) + 2S - 2); so many whole pixels apart, two
// more for the two floors' fractions and the bilinear neighbour, one to count, and `align` - 1 lost on each side.
LEON_HD inline int32_t warp_span_bound(int32_t a, int32_t b, int32_t g, int32_t pw, int32_t ph, int32_t align)
{
    const int64_t S2 = (int64_t)2 << g;
    const int64_t aa = a < 0 ? -(int64_t)a : a, bb = b < 0 ? -(int64_t)b : b;
    const int64_t d = aa * (S2 * pw - 2) + bb * (S2 * ph - 2);
    const int64_t px = (d >> (g + 17)) + 3;
    return (int32_t)((px + 2 * (align - 1)) & ~(int64_t)(align - 1));
}
LEON_HD inline bool warp_level_fits(const int32_t* m, int32_t g, int32_t level)
{
    const int32_t pw = warp_piece_w(level), ph = warp_piece_h(level);
    const int32_t sw = warp_span_bound(m[0], m[1], g, pw, ph, 8), sh = warp_span_bound(m[3], m[4], g, pw, ph, 2);
    return (int64_t)(sw + 1) * sh <= kWarpStagePx;
}
// the first level whose bound fits (the last one always does: every |a| <= 2^18 + 1 gives 48 + 1 dwords by 42 rows at most)
LEON_HD inline int32_t warp_level(const int32_t* m, int32_t g)
{
    int32_t level = 0;
    while (level < kWarpLevels - 1 && !warp_level_fits(m, g, level)) level++;
    return level;
}

}  // namespace leon
#endif
