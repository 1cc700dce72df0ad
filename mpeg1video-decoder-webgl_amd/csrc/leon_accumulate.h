// leon_accumulate.h -- one hop of the accumulated motion and residual along a GOP's chain (the definition of include/leon_pipeline.h,
// leon_pipeline_accumulate), for the host (accumulate_record_host: leon_pipeline_impl.h; tests/native/accumulate_check.cpp walks it)
// and the device (k_accumulate: leon_kernels.h): ONE text, as leon_propagate.h is for its calls.  Integers only.  The judgement of a
// hop, the pick, the rounding and the clamp are leon_propagate.h's own functions; what is here is the accumulator's geometry and the
// walk of one work unit: 4 destination elements (8 bytes) of one plane, which never straddle a macroblock (a macroblock row is 16 luma
// or 8 chroma elements and the coded width is a multiple of 16).
#ifndef LEON_ACCUMULATE_H
#define LEON_ACCUMULATE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "leon_propagate.h"
#include "leon_residual.h"

namespace leon {

enum { kAccumulateMotion = 1, kAccumulateResidual = 2 };          // the bits of `parts`
enum { kAccAX = 0, kAccAY = 1, kAccAGE = 2, kAccRY = 3, kAccRCb = 4, kAccRCr = 5, kAccKinds = 6 };          // the planes, in their order in a slot
static constexpr int32_t kAccumulateUnit = 4;          // elements a work unit

// what a call's accumulators look like; made by accumulate_geometry alone
struct AccumulateGeom {
    int32_t cw, ch, mbw, parts;
    int32_t planes;                      // planes asked for: 3 (one part) or 6 (both); blockIdx.y counts them
    uint32_t luma_stride, chroma_stride; // ELEMENTS a row: the residual record's strides
    uint32_t off[kAccKinds];             // a plane's offset in a slot, 0 for an absent one
    uint32_t res_off[kAccKinds];         // a residual plane's offset in T's residual record (kinds RY, RCb, RCr)
    uint32_t units_luma, units_chroma;   // work units a plane
    uint32_t slot_bytes;
};

// false: a coded size that is no multiple of 16 or parts outside 1 .. 3.  With parts = 2 the planes lie as a residual record's do.
LEON_HD inline bool accumulate_geometry(int32_t cw, int32_t ch, int32_t parts, AccumulateGeom* g)
{
    if (cw < 16 || ch < 16 || (cw & 15) || (ch & 15) || parts < 1 || parts > (kAccumulateMotion | kAccumulateResidual)) return false;
    const ResidualLayout R = residual_layout((uint32_t)cw, (uint32_t)ch);
    g->cw = cw; g->ch = ch; g->mbw = cw >> 4; g->parts = parts;
    g->planes = parts == (kAccumulateMotion | kAccumulateResidual) ? 6 : 3;
    g->luma_stride = R.luma_stride; g->chroma_stride = R.chroma_stride;
    const uint32_t luma_bytes = residual_pad(2u * R.luma_stride * (uint32_t)ch, 256u), chroma_bytes = residual_pad(2u * R.chroma_stride * (uint32_t)(ch >> 1), 256u);
    uint32_t at = 0;
    for (int32_t k = 0; k < kAccKinds; k++) {
        const bool present = (parts & (k < kAccRY ? kAccumulateMotion : kAccumulateResidual)) != 0;
        g->off[k] = present ? at : 0u;
        if (present) at += k < kAccRCb ? luma_bytes : chroma_bytes;
        g->res_off[k] = k == kAccRCb ? R.cb_offset : k == kAccRCr ? R.cr_offset : 0u;
    }
    // the last plane takes its rows alone: no pad behind it
    g->slot_bytes = at - ((parts & kAccumulateResidual) ? chroma_bytes - 2u * R.chroma_stride * (uint32_t)(ch >> 1) : luma_bytes - 2u * R.luma_stride * (uint32_t)ch);
    g->units_luma = (uint32_t)(cw / kAccumulateUnit) * (uint32_t)ch;
    g->units_chroma = (uint32_t)((cw >> 1) / kAccumulateUnit) * (uint32_t)(ch >> 1);
    return true;
}

// the kind of the q-th plane asked for, and its work units
LEON_HD inline int32_t accumulate_kind(const AccumulateGeom& g, int32_t q) { return (g.parts & kAccumulateMotion) ? q : q + kAccRY; }
LEON_HD inline uint32_t accumulate_units(const AccumulateGeom& g, int32_t q) { return accumulate_kind(g, q) >= kAccRCb ? g.units_chroma : g.units_luma; }

LEON_HD inline int32_t accumulate_sat16(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
// two saturating 16-bit adds in a dword
LEON_HD inline uint32_t accumulate_add2(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short accumulate_v2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(__builtin_bit_cast(accumulate_v2, a), __builtin_bit_cast(accumulate_v2, b)));
#else
    const int32_t lo = accumulate_sat16((int32_t)(int16_t)(uint16_t)a + (int32_t)(int16_t)(uint16_t)b);
    const int32_t hi = accumulate_sat16((int32_t)(int16_t)(uint16_t)(a >> 16) + (int32_t)(int16_t)(uint16_t)(b >> 16));
    return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
#endif
}
LEON_HD inline uint32_t accumulate_both(int32_t v) { return ((uint32_t)v & 0xffffu) * 0x10001u; }

struct AccumulateWords { uint32_t w[2]; };
// 8 bytes at a 4-byte aligned address (a slot's pitch is a multiple of 4), and at an 8-byte aligned one (a residual record's unit)
LEON_HD inline void accumulate_store(uint8_t* p, AccumulateWords v) { memcpy(__builtin_assume_aligned(p, 4), &v, 8); }
LEON_HD inline AccumulateWords accumulate_load8(const uint8_t* p)
{
    AccumulateWords v;
    memcpy(&v, __builtin_assume_aligned(p, 8), 8);
    return v;
}

// Work unit u of the q-th plane asked for, of one hop whose status is kRegionOk.  motion: T's motion record (mv at 0, info at
// info_offset); residual: T's residual record (read for the kinds RY, RCb, RCr alone; may be null otherwise); slots: the caller's buffer
// of slots_bytes bytes, accumulators at slot_pitch; via: this hop's [mbh][mbw] bytes, or NULL (no via asked for, or a plane that does
// not write it: the callers hand it to plane 0, which is a luma plane whatever the parts).
// Every load lies inside the source slot's plane, every store inside the destination slot's.
LEON_HD inline void accumulate_unit(const AccumulateGeom& g, const uint8_t* motion, uint32_t info_offset, const uint8_t* residual, uint8_t* slots, size_t slots_bytes,
                                    size_t slot_pitch, const PropagateHop& h, uint8_t* via, int32_t q, uint32_t u)
{
    const int32_t kind = accumulate_kind(g, q), ls = kind >= kAccRCb ? 1 : 0;          // log2 of the stride: luma 1, chroma 2 luma pixels an element
    const int32_t w = g.cw >> ls, hgt = g.ch >> ls;
    const uint32_t stride = ls ? g.chroma_stride : g.luma_stride, units_row = (uint32_t)w / (uint32_t)kAccumulateUnit;
    const uint32_t y = u / units_row, x = (u - y * units_row) * (uint32_t)kAccumulateUnit;
    const uint32_t k = (y >> (4 - ls)) * (uint32_t)g.mbw + (x >> (4 - ls));
    int32_t slot, dx, dy;
    const int32_t pick = propagate_pick(h, ls, motion[info_offset + k], propagate_load32(motion + 8u * (size_t)k), propagate_load32(motion + 8u * (size_t)k + 4u), &slot, &dx, &dy);
    if (via && !((x | y) & 15u)) via[k] = (uint8_t)pick;
    const size_t at = (size_t)g.off[kind] + ((size_t)y * stride + x) * 2u;
    uint8_t* dst = slots + (size_t)h.dst_slot * slot_pitch + at;
    if (pick == kPropagateFill) {          // a restart: the sample is its own origin
        accumulate_store(dst, AccumulateWords{{0u, 0u}});
        return;
    }
    const int32_t sy = propagate_clamp((int32_t)y + dy, hgt - 1), sx0 = (int32_t)x + dx;
    const size_t row = (size_t)slot * slot_pitch + (size_t)g.off[kind] + (size_t)sy * stride * 2u;          // the source row's offset in slots
    AccumulateWords own;          // what the hop itself adds: the displacement behind the clamp, one hop, T's residual
    if (kind >= kAccRY) own = accumulate_load8(residual + g.res_off[kind] + ((size_t)y * stride + x) * 2u);
    else own.w[0] = own.w[1] = accumulate_both(kind == kAccAX ? dx : kind == kAccAY ? sy - (int32_t)y : 1);
    if (sx0 >= 0 && sx0 + kAccumulateUnit <= w) {
        // the clamp leaves the unit alone: eight source bytes in a run at a 2-byte aligned address, read as the aligned dwords around
        // them.  A plane is whole dwords, so the first two lie inside it; the third is read only when the shift takes bytes of it, and
        // then it lies inside the plane too -- the bound against slots_bytes holds whatever the caller's pitch
        size_t off = row + (size_t)sx0 * 2u;
        const uint32_t sh = (uint32_t)(off & 3u);
        off -= sh;
        const uint32_t lo = propagate_load32(slots + off), mid = propagate_load32(slots + off + 4u);
        const uint32_t hi = (sh && off + 12u <= slots_bytes) ? propagate_load32(slots + off + 8u) : 0u;
        accumulate_store(dst, AccumulateWords{{accumulate_add2(propagate_funnel(mid, lo, sh), own.w[0]), accumulate_add2(propagate_funnel(hi, mid, sh), own.w[1])}});
        return;
    }
    // a unit that the clamp touches: element by element; AX's own term differs from element to element
    AccumulateWords out{{0u, 0u}};
#pragma unroll
    for (int32_t i = 0; i < kAccumulateUnit; i++) {
        const int32_t sx = propagate_clamp(sx0 + i, w - 1);
        const int32_t s = (int32_t)(int16_t)(uint16_t)propagate_load(slots + row + (size_t)sx * 2u, 2);
        const int32_t add = kind == kAccAX ? sx - ((int32_t)x + i) : (int32_t)(int16_t)(uint16_t)(own.w[i >> 1] >> (16 * (i & 1)));
        out.w[i >> 1] |= ((uint32_t)accumulate_sat16(s + add) & 0xffffu) << (16 * (i & 1));
    }
    accumulate_store(dst, out);
}

}  // namespace leon
#endif
