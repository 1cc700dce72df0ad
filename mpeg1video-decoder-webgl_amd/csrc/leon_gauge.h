// leon_gauge.h -- the statistics of a frame's motion and activity records under one box (the definition of include/leon_pipeline.h,
// leon_pipeline_gauge_regions), for the host (gauge_record_host: leon_pipeline_impl.h) and the device (k_gauge: leon_kernels.h): ONE
// text, as leon_carry.h is for its calls.  Integers only: the judgement of a record, one macroblock added to the sums, the finish.  The
// cover and the weight are the carry family's (carry_weight); the cells are leon_activity.h's, the entries leon_motion.h's.
#ifndef LEON_GAUGE_H
#define LEON_GAUGE_H
#include <stdint.h>
#include "leon_carry.h"
#include "leon_activity.h"

namespace leon {

enum { kGaugeMotion = 1, kGaugeActivity = 2 };          // the bits of `sources`
enum { kGaugeWords = 16 };                               // int64 words of a record's statistics

struct GaugeRecord {                     // = leon_pipeline_region
    int32_t frame;
    int32_t x, y, width, height;
    int32_t reserved[3];
};

// all int64: 2^16 macroblocks x weight 2^8 = 2^24, x a value of at most 65535 (32768 for a vector's magnitude): below 2^41.
// w[7] is a maximum, every other word a sum.
struct GaugeSums {
    int64_t w[kGaugeWords];
};

// regions_check's order: the reserved words, the frame index, the box -- the last two in carry_record_status's own words, the record
// read as a hop onto its own frame
LEON_HD inline int32_t gauge_record_status(const GaugeRecord& r, int32_t fw, int32_t fh, int32_t n_frames)
{
    if (r.reserved[0]) return kRegionReserved;
    return carry_record_status(CarryRecord{r.frame, r.x, r.y, r.width, r.height, r.frame, {r.reserved[1], r.reserved[2]}}, fw, fh, n_frames);
}

// one macroblock of weight a added to the sums: lo and hi the dwords of its activity cell (leon_activity.h), info and fwd / bwd its
// motion entry (leon_motion.h); what belongs to a source the call does not ask for is not looked at
LEON_HD inline void gauge_cell(int32_t sources, int32_t a, uint32_t lo, uint32_t hi, uint32_t info, uint32_t fwd, uint32_t bwd, GaugeSums* s)
{
    const int64_t A = a;
    s->w[0] += A;
    if (sources & kGaugeActivity) {
        const uint32_t blocks = (hi >> 16) & 255u, ac_mag = lo >> 16;
        s->w[1] += blocks != 0u ? A : 0;
        s->w[2] += A * (int64_t)(lo & 0xffffu);
        s->w[3] += A * (int64_t)ac_mag;
        s->w[4] += A * (int64_t)(hi & 0xffffu);
        s->w[5] += A * (int64_t)(hi >> 24);
        s->w[6] += A * (int64_t)activity_popcount6(blocks);
        s->w[7] = (int64_t)ac_mag > s->w[7] ? (int64_t)ac_mag : s->w[7];
    }
    if (sources & kGaugeMotion) {
        s->w[8] += (info & 1u) ? A : 0;
        s->w[9] += (info & 2u) ? A : 0;
        s->w[10] += (info & 4u) ? A : 0;
        s->w[11] += (fwd | bwd) != 0u ? A : 0;
        s->w[12] += A * (int64_t)motion_abs16(fwd);
        s->w[13] += A * (int64_t)motion_abs16(fwd >> 16);
        s->w[14] += A * (int64_t)motion_abs16(bwd);
        s->w[15] += A * (int64_t)motion_abs16(bwd >> 16);
    }
}

// the 16 words of a record: the words of a source the call did not ask for are written as 0
LEON_HD inline void gauge_finish(int32_t sources, const GaugeSums& s, int64_t* out)
{
    out[0] = s.w[0];
    for (int k = 1; k < 8; k++) out[k] = (sources & kGaugeActivity) ? s.w[k] : 0;
    for (int k = 8; k < kGaugeWords; k++) out[k] = (sources & kGaugeMotion) ? s.w[k] : 0;
}

}  // namespace leon
#endif
