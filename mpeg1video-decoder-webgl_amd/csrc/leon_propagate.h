// leon_propagate.h -- one hop of a dense map along the stream's motion vectors (the definition of include/leon_pipeline.h,
// leon_pipeline_propagate_maps), for the host (propagate_record_host: leon_pipeline_impl.h) and the device (k_propagate:
// leon_kernels.h): ONE text, as leon_carry.h, leon_motion.h and leon_warp.h are for their calls.  Integers only, and no arithmetic on
// a map's elements at all: the judgement of a record, a cell's macroblock, pick, displacement and clamp, and the walk of one work unit.
#ifndef LEON_PROPAGATE_H
#define LEON_PROPAGATE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "leon_resize_row.h"
#include "leon_motion.h"

namespace leon {

// the status word a propagate record adds to kRegion* (LEON_REGION_SLOT)
enum { kRegionSlot = 10 };
enum { kPropagateFill = 0, kPropagateFwd = 1, kPropagateBwd = 2 };      // the bytes of `via`
static constexpr int32_t kPropagateMaxPlanes = 4096, kPropagateMaxSlots = 65535, kPropagateGroup = 4;

struct PropagateHop {                    // = leon_pipeline_propagate_hop
    int32_t target;
    int32_t dst_slot, fwd_slot, bwd_slot;
    int32_t reserved[4];
};

// what a call's maps look like; made by propagate_geometry alone
struct PropagateGeom {
    int32_t mw, mh;                      // cells of a map
    int32_t mbw;                         // macroblocks a row of the coded picture
    int32_t ls;                          // log2 of the stride
    int32_t e;                           // bytes an element
    int32_t planes, group;               // planes of a map, planes a work unit's lane loops over (blockIdx.y counts groups)
    int32_t fast;                        // 1: a unit is one destination dword, 0: a unit is one cell
    uint32_t units_row, units;           // work units a map row, a plane
    size_t plane_bytes;                  // mh * mw * e
};

LEON_HD inline int32_t propagate_log2(int32_t s) { return s == 1 ? 0 : s == 2 ? 1 : s == 4 ? 2 : s == 8 ? 3 : s == 16 ? 4 : -1; }

// false: a stride, element size or plane count outside the definition
LEON_HD inline bool propagate_geometry(int32_t fw, int32_t fh, int32_t mbw, int32_t s, int32_t planes, int32_t e, PropagateGeom* g)
{
    const int32_t ls = propagate_log2(s);
    if (ls < 0 || (e != 1 && e != 2 && e != 4) || planes < 1 || planes > kPropagateMaxPlanes || fw < 1 || fh < 1) return false;
    g->mw = (fw + s - 1) >> ls;
    g->mh = (fh + s - 1) >> ls;
    g->mbw = mbw;
    g->ls = ls;
    g->e = e;
    g->planes = planes;
    g->group = planes < kPropagateGroup ? planes : kPropagateGroup;
    // the fast path: a row is whole dwords, and so is a macroblock's run of cells: a destination dword never straddles a macroblock
    g->fast = ((g->mw * e) % 4 == 0 && ((16 >> ls) * e) % 4 == 0) ? 1 : 0;
    g->units_row = g->fast ? (uint32_t)(g->mw * e) / 4u : (uint32_t)g->mw;
    g->units = g->units_row * (uint32_t)g->mh;
    g->plane_bytes = (size_t)g->mh * (size_t)g->mw * (size_t)e;
    return true;
}

// the judgement of a record, in this order: the reserved words, the target, the slots
LEON_HD inline int32_t propagate_hop_status(const PropagateHop& h, int32_t n_frames, int32_t n_slots)
{
    if (h.reserved[0] | h.reserved[1] | h.reserved[2] | h.reserved[3]) return kRegionReserved;
    if (h.target < 0 || h.target >= n_frames) return kRegionFrame;
    if (h.dst_slot < 0 || h.dst_slot >= n_slots || h.fwd_slot < -1 || h.fwd_slot >= n_slots || h.bwd_slot < -1 || h.bwd_slot >= n_slots) return kRegionSlot;
    if (h.dst_slot == h.fwd_slot || h.dst_slot == h.bwd_slot) return kRegionSlot;
    return kRegionOk;
}

// the macroblock of T's record under cell (cx, cy)
LEON_HD inline uint32_t propagate_mb(const PropagateGeom& g, uint32_t cx, uint32_t cy)
{
    return (((cy << g.ls) >> 4) * (uint32_t)g.mbw) + ((cx << g.ls) >> 4);
}

// half-pel luma units to cells: floor((v + s) / (2 s)), to nearest, ties up, floor also below zero (the shift is arithmetic)
LEON_HD inline int32_t propagate_cells(uint32_t half, int32_t ls)
{
    return ((int32_t)(int16_t)(uint16_t)half + (1 << ls)) >> (1 + ls);
}

// the pick: forward where the macroblock has it and the map is supplied, else backward likewise, else fill.  fwd and bwd the record's
// dwords (fwd_h, fwd_v) and (bwd_h, bwd_v), h in the low half.  Returns via; *slot, *dx, *dy are set where via != 0.
LEON_HD inline int32_t propagate_pick(const PropagateHop& h, int32_t ls, uint32_t info, uint32_t fwd, uint32_t bwd, int32_t* slot, int32_t* dx, int32_t* dy)
{
    uint32_t v;
    int32_t via;
    if ((info & kMotionFwd) && h.fwd_slot >= 0) { via = kPropagateFwd; v = fwd; *slot = h.fwd_slot; }
    else if ((info & kMotionBwd) && h.bwd_slot >= 0) { via = kPropagateBwd; v = bwd; *slot = h.bwd_slot; }
    else { *slot = 0; *dx = 0; *dy = 0; return kPropagateFill; }
    *dx = propagate_cells(v, ls);
    *dy = propagate_cells(v >> 16, ls);
    return via;
}

LEON_HD inline int32_t propagate_clamp(int32_t v, int32_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// aligned loads and stores of the opaque bytes (the callers see to the alignment: 4-byte aligned maps, a pitch that is a multiple of 4)
LEON_HD inline uint32_t propagate_load32(const uint8_t* p)
{
    uint32_t v;
    memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
}
LEON_HD inline void propagate_store32(uint8_t* p, uint32_t v) { memcpy(__builtin_assume_aligned(p, 4), &v, 4); }
LEON_HD inline uint32_t propagate_load(const uint8_t* p, int32_t e)
{
    if (e == 4) return propagate_load32(p);
    if (e == 2) {
        uint16_t v;
        memcpy(&v, __builtin_assume_aligned(p, 2), 2);
        return v;
    }
    return *p;
}
LEON_HD inline void propagate_store(uint8_t* p, uint32_t v, int32_t e)
{
    if (e == 4) propagate_store32(p, v);
    else if (e == 2) {
        const uint16_t w = (uint16_t)v;
        memcpy(__builtin_assume_aligned(p, 2), &w, 2);
    } else *p = (uint8_t)v;
}
// bytes sh .. sh + 3 of the eight bytes {lo, hi}; sh 0 .. 3
LEON_HD inline uint32_t propagate_funnel(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return sh ? (lo >> (8u * sh)) | (hi << (32u - 8u * sh)) : lo;
#endif
}
// the low e bytes of `fill` in every element of a dword
LEON_HD inline uint32_t propagate_fill32(uint32_t fill, int32_t e)
{
    return e == 4 ? fill : e == 2 ? (fill & 0xffffu) * 0x10001u : (fill & 0xffu) * 0x1010101u;
}

// Work unit u of planes p0 .. p1 - 1 of one hop whose status is kRegionOk.  record: T's motion record (mv at 0, info at info_offset).
// maps: the caller's buffer of maps_bytes bytes, slots at slot_pitch; via: this hop's [mh][mw] bytes, or NULL (no via asked for, or a
// plane group that does not write it).  The macroblock, pick and addresses are worked out once; the loop runs over the planes.
// Every load lies inside the source slot's planes, every store inside the destination slot's.
LEON_HD inline void propagate_unit(const PropagateGeom& g, const uint8_t* record, uint32_t info_offset, uint8_t* maps, size_t maps_bytes, size_t slot_pitch,
                                   const PropagateHop& h, uint32_t fill, uint8_t* via, uint32_t u, int32_t p0, int32_t p1)
{
    const uint32_t cy = u / g.units_row, ux = u - cy * g.units_row;
    const int32_t e = g.e, cells = g.fast ? 4 / e : 1;          // cells a unit
    const uint32_t cx = ux * (uint32_t)cells;
    const uint32_t k = propagate_mb(g, cx, cy);
    int32_t slot, dx, dy;
    const int32_t pick = propagate_pick(h, g.ls, record[info_offset + k], propagate_load32(record + 8u * (size_t)k), propagate_load32(record + 8u * (size_t)k + 4u), &slot,
                                        &dx, &dy);
    const size_t cell = (size_t)cy * (size_t)g.mw + cx;
    if (via) {
        if (cells == 4) propagate_store32(via + cell, (uint32_t)pick * 0x1010101u);
        else if (cells == 2) propagate_store(via + cell, (uint32_t)pick * 0x101u, 2);
        else via[cell] = (uint8_t)pick;
    }
    uint8_t* dst = maps + (size_t)h.dst_slot * slot_pitch + cell * (size_t)e + (size_t)p0 * g.plane_bytes;
    if (pick == kPropagateFill) {
        const uint32_t word = propagate_fill32(fill, e);
        for (int32_t pl = p0; pl < p1; pl++, dst += g.plane_bytes) {
            if (g.fast) propagate_store32(dst, word);
            else propagate_store(dst, word, e);
        }
        return;
    }
    const int32_t sy = propagate_clamp((int32_t)cy + dy, g.mh - 1), sx0 = (int32_t)cx + dx;
    const size_t row = (size_t)slot * slot_pitch + (size_t)p0 * g.plane_bytes + (size_t)sy * (size_t)g.mw * (size_t)e;      // the source row's offset in maps
    if (!g.fast) {
        // four planes' loads ahead of their stores: dst and src are one buffer to the compiler, which would wait for each load in turn
        const uint8_t* src = maps + row + (size_t)propagate_clamp(sx0, g.mw - 1) * (size_t)e;
        for (int32_t q = p0; q < p1; q += kPropagateGroup, dst += kPropagateGroup * g.plane_bytes, src += kPropagateGroup * g.plane_bytes) {
            uint32_t v[kPropagateGroup];
#pragma unroll
            for (int32_t j = 0; j < kPropagateGroup; j++)
                if (q + j < p1) v[j] = propagate_load(src + (size_t)j * g.plane_bytes, e);
#pragma unroll
            for (int32_t j = 0; j < kPropagateGroup; j++)
                if (q + j < p1) propagate_store(dst + (size_t)j * g.plane_bytes, v[j], e);
        }
        return;
    }
    if (sx0 >= 0 && sx0 + cells <= g.mw) {
        // the clamp leaves the unit alone: four source bytes in a run, read as the aligned dwords around them.  A plane is whole dwords,
        // so the first lies inside it; the second is read only when the shift takes bytes of it, and then it lies inside the plane too
        // -- the bound against maps_bytes holds whatever the caller's pitch
        size_t off = row + (size_t)sx0 * (size_t)e;
        const uint32_t sh = (uint32_t)(off & 3u);
        off -= sh;
        for (int32_t q = p0; q < p1; q += kPropagateGroup, dst += kPropagateGroup * g.plane_bytes, off += kPropagateGroup * g.plane_bytes) {
            uint32_t lo[kPropagateGroup], hi[kPropagateGroup];
#pragma unroll
            for (int32_t j = 0; j < kPropagateGroup; j++)
                if (q + j < p1) {
                    const size_t at = off + (size_t)j * g.plane_bytes;
                    lo[j] = propagate_load32(maps + at);
                    hi[j] = (sh && at + 8u <= maps_bytes) ? propagate_load32(maps + at + 4u) : 0u;
                }
#pragma unroll
            for (int32_t j = 0; j < kPropagateGroup; j++)
                if (q + j < p1) propagate_store32(dst + (size_t)j * g.plane_bytes, propagate_funnel(hi[j], lo[j], sh));
        }
        return;
    }
    // a unit that the clamp touches: element by element
    const uint8_t* src = maps + row;
    for (int32_t pl = p0; pl < p1; pl++, dst += g.plane_bytes, src += g.plane_bytes) {
        uint32_t word = 0;
#pragma unroll
        for (int32_t i = 0; i < 4; i++)
            if (i < cells) word |= propagate_load(src + (size_t)propagate_clamp(sx0 + i, g.mw - 1) * (size_t)e, e) << (8 * e * i);
        propagate_store32(dst, word);
    }
}

}  // namespace leon
#endif
