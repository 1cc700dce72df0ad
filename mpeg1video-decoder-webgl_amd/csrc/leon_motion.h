// leon_motion.h -- one macroblock of a frame's motion record and the record's layout (the definition of include/leon_pipeline.h,
// LEON_PIPELINE_OUTPUT_MOTION), for the host (leon_pipeline_motion_record, leon_pipeline_motion_layout: leon_pipeline_impl.h) and
// the device (k_motion: leon_kernels.h): ONE text, as leon_warp.h and leon_resize_row.h are for their calls.  Integers only.
// A vector pair travels as the dword the maps hold it in, h in the low half and v in the high half (little endian on both sides).
#ifndef LEON_MOTION_H
#define LEON_MOTION_H
#include <stdint.h>
#include "leon_resize_row.h"

namespace leon {

enum { kMotionFwd = 1, kMotionBwd = 2, kMotionIntra = 4 };      // the bits of `info`
static constexpr int32_t kMotionMaxMb = 256;                   // macroblocks an axis: 4096 samples

// where the parts of a record lie: mv int16[mbs][4] at 0, info uint8[mbs], summary uint32[8]; every part starts on a 256-byte boundary
struct MotionLayout {
    uint32_t mbs, info_offset, summary_offset, record_bytes, record_pitch;
};
LEON_HD inline uint32_t motion_pad256(uint32_t v) { return (v + 255u) & ~255u; }
LEON_HD inline MotionLayout motion_layout(uint32_t mbw, uint32_t mbh)
{
    MotionLayout L;
    L.mbs = mbw * mbh;
    L.info_offset = motion_pad256(8u * L.mbs);
    L.summary_offset = L.info_offset + motion_pad256(L.mbs);
    L.record_bytes = L.summary_offset + 32u;
    L.record_pitch = motion_pad256(L.record_bytes);
    return L;
}

// Macroblock k of a picture of `type` (LEON_PIC_I / _P / _B = 1 / 2 / 3): repadd = repadd[k], dir = mb_dir[k], fwd and bwd = the dwords
// (mv_fwd[2k], mv_fwd[2k + 1]) and (mv_bwd[2k], mv_bwd[2k + 1]) -- whatever stands there where the picture has no such map, it is not
// used.  Returns info; *o_fwd and *o_bwd are the record's (fwd_h, fwd_v) and (bwd_h, bwd_v).  The stream-carried part of the maps: an
// unused direction's entry (the parser's predictor) reads as zero, the intra map (stale at skipped macroblocks) is not asked.
LEON_HD inline uint32_t motion_mb(int32_t type, uint32_t repadd, uint32_t dir, uint32_t fwd, uint32_t bwd, uint32_t* o_fwd, uint32_t* o_bwd)
{
    const bool intra = type == 1 || repadd >= 128u;
    const uint32_t d = intra ? 0u : (type == 2 ? (uint32_t)kMotionFwd : (dir & 3u));
    *o_fwd = (d & kMotionFwd) ? fwd : 0u;
    *o_bwd = (d & kMotionBwd) ? bwd : 0u;
    return intra ? (uint32_t)kMotionIntra : d;
}

LEON_HD inline uint32_t motion_abs16(uint32_t half)            // |int16| of the low 16 bits, 0 .. 32768
{
    const int32_t v = (int32_t)(int16_t)(uint16_t)half;
    return (uint32_t)(v < 0 ? -v : v);
}

// one macroblock of the RECORD added to the eight summary words
LEON_HD inline void motion_count(uint32_t info, uint32_t fwd, uint32_t bwd, uint32_t* s)
{
    s[0] += info & 1u;
    s[1] += (info >> 1) & 1u;
    s[2] += (info >> 2) & 1u;
    s[3] += (fwd | bwd) != 0u ? 1u : 0u;
    s[4] += motion_abs16(fwd);
    s[5] += motion_abs16(fwd >> 16);
    s[6] += motion_abs16(bwd);
    s[7] += motion_abs16(bwd >> 16);
}

}  // namespace leon
#endif
