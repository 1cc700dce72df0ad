// leon_activity.h -- one entry and one macroblock of a frame's activity record and the record's layout (the definition of
// include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_ACTIVITY), for the host (leon_pipeline_activity_record, leon_pipeline_activity_layout:
// leon_pipeline_impl.h) and the device (k_activity, k_activity_summary: leon_kernels.h): ONE text, as leon_motion.h is for its calls.
// Integers only.  The group lists are include/leon_vlc.h's; only the groups of Y, Cb and Cr are read.
#ifndef LEON_ACTIVITY_H
#define LEON_ACTIVITY_H
#include <stdint.h>
#include "leon_resize_row.h"

namespace leon {

static constexpr int32_t kActivityMaxMb = 256;                  // macroblocks an axis, as kMotionMaxMb
static constexpr uint32_t kActivitySat = 65535u;                // where the three sums of a cell stop

// where the parts of a record lie: cell [mbs] of 8 bytes at 0, summary uint32[8]; both start on a 256-byte boundary
struct ActivityLayout {
    uint32_t mbs, summary_offset, record_bytes, record_pitch;
};
LEON_HD inline uint32_t activity_pad256(uint32_t v) { return (v + 255u) & ~255u; }
LEON_HD inline ActivityLayout activity_layout(uint32_t mbw, uint32_t mbh)
{
    ActivityLayout L;
    L.mbs = mbw * mbh;
    L.summary_offset = activity_pad256(8u * L.mbs);
    L.record_bytes = L.summary_offset + 32u;
    L.record_pitch = activity_pad256(L.record_bytes);
    return L;
}

// the groups of a picture (include/leon_vlc.h) and the tasks k_activity cuts it into: the 8 macroblocks under one chroma group of one
// macroblock row
struct ActivityGeom {
    uint32_t mbw, mbh, groups_y, groups_c, n_y, n_c, tasks, reserved;
};
LEON_HD inline ActivityGeom activity_geom(uint32_t mbw, uint32_t mbh)
{
    ActivityGeom G;
    G.mbw = mbw; G.mbh = mbh;
    G.groups_y = (mbw + 3u) / 4u;
    G.groups_c = (mbw + 7u) / 8u;
    G.n_y = 2u * mbh * G.groups_y;
    G.n_c = mbh * G.groups_c;
    G.tasks = mbh * G.groups_c;
    G.reserved = 0u;
    return G;
}

// the entries of group `gid` in a list of `cap` entries: [*begin, *end), both offsets clamped to the capacity before anything is
// addressed with them and an end in front of its begin read as an empty group -- whatever grp_off holds, no entry outside the list
LEON_HD inline void activity_span(uint32_t off0, uint32_t off1, uint32_t cap, uint32_t* begin, uint32_t* end)
{
    const uint32_t b = off0 < cap ? off0 : cap, e = off1 < cap ? off1 : cap;
    *begin = b;
    *end = e < b ? b : e;
}

// |level| of an entry, 0 .. 32768; 0: the entry counts nothing
LEON_HD inline uint32_t activity_abs(uint32_t e)
{
    const int32_t v = (int32_t)(int16_t)(uint16_t)(e & 0xffffu);
    return (uint32_t)(v < 0 ? -v : v);
}
LEON_HD inline uint32_t activity_b(uint32_t e) { return (e >> 20) & 7u; }                          // block in group
LEON_HD inline bool activity_is_dc(uint32_t e) { return ((e >> 23) & 7u) == 0u && ((e >> 17) & 7u) == 0u; }   // row 0, column 0

// Block b of group g in block row R of a plane (0 Y, 1 Cb, 2 Cr): the macroblock column it belongs to (which may lie at or behind
// mbw: it counts nothing then), its macroblock row and which of the macroblock's six blocks it is
LEON_HD inline void activity_place(uint32_t plane, uint32_t R, uint32_t g, uint32_t b, uint32_t* mx, uint32_t* my, uint32_t* j)
{
    if (plane == 0u) {
        *mx = 4u * g + (b >> 1);
        *my = R >> 1;
        *j = 2u * (R & 1u) + (b & 1u);
    } else {
        *mx = 8u * g + b;
        *my = R;
        *j = 3u + plane;
    }
}

LEON_HD inline uint32_t activity_sat(uint64_t v) { return v < (uint64_t)kActivitySat ? (uint32_t)v : kActivitySat; }

// A macroblock's cell from its exact sums, its block bits and qscale_map[k], as the two dwords it is stored as (little endian):
// lo = ac_count | ac_mag << 16, hi = dc_mag | blocks << 16 | qscale << 24; a macroblock that codes nothing shows no qscale
LEON_HD inline void activity_cell(uint64_t ac_count, uint64_t ac_mag, uint64_t dc_mag, uint32_t blocks, uint32_t qscale, uint32_t* lo, uint32_t* hi)
{
    *lo = activity_sat(ac_count) | (activity_sat(ac_mag) << 16);
    *hi = activity_sat(dc_mag) | ((blocks & 63u) << 16) | ((blocks & 63u) ? (qscale & 255u) << 24 : 0u);
}

LEON_HD inline uint32_t activity_popcount6(uint32_t v)
{
    v &= 63u;
    v = (v & 0x15u) + ((v >> 1) & 0x15u);
    return (v & 3u) + ((v >> 2) & 3u) + ((v >> 4) & 3u);
}

// one cell of the RECORD added to the eight summary words ([4] is a maximum)
LEON_HD inline void activity_count(uint32_t lo, uint32_t hi, uint32_t* s)
{
    const uint32_t blocks = (hi >> 16) & 255u, ac_mag = lo >> 16;
    s[0] += blocks != 0u ? 1u : 0u;
    s[1] += lo & 0xffffu;
    s[2] += ac_mag;
    s[3] += hi & 0xffffu;
    s[4] = ac_mag > s[4] ? ac_mag : s[4];
    s[5] += hi >> 24;
    s[6] += activity_popcount6(blocks);
}

}  // namespace leon
#endif
