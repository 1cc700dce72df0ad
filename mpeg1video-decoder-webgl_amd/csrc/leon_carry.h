// leon_carry.h -- one hop of a box along the stream's motion vectors (the definition of include/leon_pipeline.h,
// leon_pipeline_carry_regions), for the host (carry_record_host: leon_pipeline_impl.h) and the device (k_carry: leon_kernels.h): ONE
// text, as leon_motion.h and leon_warp.h are for their calls.  Integers only: the judgement of a record, the pick of the motion record
// that votes and its sense, a macroblock's weight and vote, and the finish.
#ifndef LEON_CARRY_H
#define LEON_CARRY_H
#include <stdint.h>
#include "leon_resize_row.h"
#include "leon_motion.h"

namespace leon {

// the status word a carry record adds to kRegion* (LEON_REGION_NO_REFERENCE)
enum { kRegionNoReference = 9 };

struct CarryRecord {                     // = leon_pipeline_carry_region
    int32_t frame;
    int32_t x, y, width, height;
    int32_t target;
    int32_t reserved[2];
};

// a frame of the window as the device finds it: its record's index in the motion ring and the window frames its vectors point into
struct CarryFrame {
    uint32_t ring;
    int32_t fwd, bwd;                    // -1: none among the window's frames
    uint32_t reserved;
};

// all int64: 2^16 macroblocks x weight 2^8 x |int16| 2^15 x two directions = 2^40
struct CarrySums {
    int64_t A, I, SH, SV;
};

// the checks that need no reference, in regions_check's order: the reserved words, both frame indices, the box
LEON_HD inline int32_t carry_record_status(const CarryRecord& r, int32_t fw, int32_t fh, int32_t n_frames)
{
    if (r.reserved[0] | r.reserved[1]) return kRegionReserved;
    if (r.frame < 0 || r.frame >= n_frames || r.target < 0 || r.target >= n_frames) return kRegionFrame;
    if (r.width < 1 || r.height < 1 || r.x < 0 || r.y < 0 || r.x > fw || r.y > fh || r.width > fw - r.x || r.height > fh - r.y) return kRegionBox;
    return kRegionOk;
}

// Which record votes, and in which sense: S = frame, T = target; fwd_t / bwd_t and fwd_s / bwd_s what those two frames point into.
// *m the frame whose record votes, *sense -1 (from the reference to the picture that predicts from it) or +1, *d the direction bits
// that vote; S == T: no vote at all (*d = 0).  Returns kRegionOk or kRegionNoReference.
LEON_HD inline int32_t carry_pick(int32_t s, int32_t t, int32_t fwd_t, int32_t bwd_t, int32_t fwd_s, int32_t bwd_s, int32_t* m, int32_t* sense, int32_t* d)
{
    *m = s; *sense = 1; *d = 0;
    if (s == t) return kRegionOk;
    const int32_t dt = (fwd_t == s ? kMotionFwd : 0) | (bwd_t == s ? kMotionBwd : 0);
    if (dt) { *m = t; *sense = -1; *d = dt; return kRegionOk; }
    const int32_t ds = (fwd_s == t ? kMotionFwd : 0) | (bwd_s == t ? kMotionBwd : 0);
    if (ds) { *d = ds; return kRegionOk; }
    return kRegionNoReference;
}

// the pixel area macroblock (i, j) shares with the box: 1 .. 256 inside the covered rectangle
LEON_HD inline int32_t carry_weight(int32_t x, int32_t y, int32_t w, int32_t h, int32_t i, int32_t j)
{
    const int32_t x0 = x > 16 * i ? x : 16 * i, x1 = x + w < 16 * i + 16 ? x + w : 16 * i + 16;
    const int32_t y0 = y > 16 * j ? y : 16 * j, y1 = y + h < 16 * j + 16 ? y + h : 16 * j + 16;
    return (x1 - x0) * (y1 - y0);
}

// one macroblock of M's record added to the sums: fwd and bwd the dwords (fwd_h, fwd_v) and (bwd_h, bwd_v), h in the low half
LEON_HD inline void carry_vote(int32_t d, uint32_t info, uint32_t fwd, uint32_t bwd, int32_t a, CarrySums* s)
{
    if (d & info & kMotionFwd) {
        s->A += a;
        s->SH += (int64_t)a * (int16_t)(uint16_t)fwd;
        s->SV += (int64_t)a * (int16_t)(uint16_t)(fwd >> 16);
    }
    if (d & info & kMotionBwd) {
        s->A += a;
        s->SH += (int64_t)a * (int16_t)(uint16_t)bwd;
        s->SV += (int64_t)a * (int16_t)(uint16_t)(bwd >> 16);
    }
    if (info & kMotionIntra) s->I += a;
}

// floor((sense * S + A) / (2 * A)): half-pel to pixels, to nearest, ties up; A > 0
LEON_HD inline int32_t carry_round(int32_t sense, int64_t S, int64_t A)
{
    const int64_t num = (sense < 0 ? -S : S) + A, den = 2 * A;
    int64_t q = num / den;
    if (num % den < 0) q--;
    return (int32_t)q;
}

// the moved box (out: frame = target, the box, three words of 0) and the votes {A, I, dh, dv}
LEON_HD inline void carry_finish(const CarryRecord& r, int32_t fw, int32_t fh, int32_t sense, const CarrySums& s, int32_t* out, int32_t* votes)
{
    const int32_t dh = s.A ? carry_round(sense, s.SH, s.A) : 0, dv = s.A ? carry_round(sense, s.SV, s.A) : 0;
    const int32_t nx = r.x + dh, ny = r.y + dv;            // |dh|, |dv| <= 2^14 and the box is inside a frame of at most 4096
    out[0] = r.target;
    out[1] = nx < 0 ? 0 : nx > fw - r.width ? fw - r.width : nx;
    out[2] = ny < 0 ? 0 : ny > fh - r.height ? fh - r.height : ny;
    out[3] = r.width;
    out[4] = r.height;
    out[5] = 0; out[6] = 0; out[7] = 0;
    votes[0] = (int32_t)s.A; votes[1] = (int32_t)s.I; votes[2] = dh; votes[3] = dv;
}

}  // namespace leon
#endif
