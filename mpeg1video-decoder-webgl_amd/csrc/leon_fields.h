// leon_fields.h -- boxes of int16 fields (motion vectors, residual planes, accumulators) resampled into a model's tensors (the
// definition of include/leon_pipeline.h, leon_pipeline_field_tensors), for the host (field_tensor_record_host: leon_pipeline_impl.h;
// tests/native/fields_check.cpp walks it) and the device (k_fields: leon_kernels.h): ONE text, as leon_accumulate.h is for its calls.
// What is here: the judgement of a channel, the address of a field's value under a frame pixel, the two passes of one output sample
// in exact 64-bit integers, the element conversion (two binary32 operations, then fp16 / bf16 rounding in integers), the plain loop
// over one sample (the CPU definition) and the kernel's walk of one output tile as barrier-separated steps over a tile's shared
// memory, which the device runs with its lanes and a stand-alone program replays lane by lane.  The tables are the pixel road's
// (leon_resize_row.h; k_box_tables builds them on the device, resize_axis_build on the host): nothing here builds one.
#ifndef LEON_FIELDS_H
#define LEON_FIELDS_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "leon_resize_row.h"

namespace leon {

enum { kFieldSourceBuffer = 0, kFieldSourceMotion = 1, kFieldSourceResidual = 2 };          // = LEON_FIELD_SOURCE_*
enum { kFieldF16 = 1, kFieldBF16 = 2, kFieldF32 = 3 };                                      // = LEON_TENSOR_F16 / _BF16 / _F32
static constexpr int32_t kFieldMaxChannels = 8, kFieldMaxShift = 4, kFieldMaxElemStride = 4;
static constexpr int kFieldWeightShift = 22;
// the kernel's tile: 32 x 8 output samples, a lane each in the vertical pass; h rows as the pixel road's triangle kernels size them
// (<= 7 * 16 + 33 + 2 = 147 rows under 8 output rows at a ratio of 16)
static constexpr int kFieldTileX = 32, kFieldTileY = 8, kFieldLanes = 256, kFieldHRows = 160, kFieldMaxTaps = kResizeMaxTapsTriangle;
static constexpr int kFieldStoreBytes = 16;                                   // the widest store: a 16-byte line of the tensor
static constexpr int kFieldPackStride = kFieldTileX * 4 + kFieldStoreBytes;   // a tile row of the widest element, and its place in its line

struct FieldChannel {                    // = leon_pipeline_field_channel
    uint32_t offset_bytes;
    int32_t row_stride, elem_stride, shift;
    float scale, bias;
    int32_t reserved[2];
};                                       // 32 bytes

LEON_HD inline int32_t field_elem_bytes(int32_t dtype) { return dtype == kFieldF32 ? 4 : 2; }

LEON_HD inline uint32_t field_bits(float v)
{
    uint32_t x;
    memcpy(&x, &v, 4);
    return x;
}
LEON_HD inline bool field_finite(float v) { return (field_bits(v) & 0x7f800000u) != 0x7f800000u; }

// binary32 -> binary16, round to nearest even, in integers (the same bits wherever it runs)
LEON_HD inline uint32_t field_f16_bits(float v)
{
    const uint32_t x = field_bits(v), sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (a >= 0x477ff000u) return sign | 0x7c00u;                      // 65520 and above round to infinity
    if (a < 0x38800000u) {                                            // below 2^-14: a subnormal, or zero
        if (a < 0x33000000u) return sign;                             // below 2^-25
        const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126u - (a >> 23);          // sh: 14 .. 24
        uint32_t q = m >> sh;
        const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
        if (rem > half || (rem == half && (q & 1u))) q++;
        return sign | q;
    }
    uint32_t h = (a - 0x38000000u) >> 13;
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;
    return sign | h;
}
// binary32 -> bfloat16, round to nearest even, in integers
LEON_HD inline uint32_t field_bf16_bits(float v)
{
    const uint32_t x = field_bits(v);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (x >> 16) | 0x40u;
    return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
}
// u = fl32(fl32((float)r * scale) + bias): two separately rounded operations
LEON_HD inline float field_value(int32_t r, float scale, float bias)
{
#pragma clang fp contract(off)
    const float m = (float)r * scale;
    return m + bias;
}
// the element's bits: 16 for fp16 / bf16, 32 for fp32
LEON_HD inline uint32_t field_elem(float u, int32_t dtype) { return dtype == kFieldF16 ? field_f16_bits(u) : dtype == kFieldBF16 ? field_bf16_bits(u) : field_bits(u); }

// ---- the judgement of a channel: 0, or the first thing wrong with it ------------------------------------------------------------------
enum { kFieldOk = 0, kFieldBadReserved, kFieldBadShift, kFieldBadElemStride, kFieldBadRowStride, kFieldBadOffset, kFieldBadScale, kFieldBadRange, kFieldBadExtent };
// bytes from the item's start to the end of the channel's last element over a frame of fw x fh
LEON_HD inline uint64_t field_channel_end(const FieldChannel& c, int32_t fw, int32_t fh)
{
    return (uint64_t)c.offset_bytes + 2u * ((uint64_t)((fh - 1) >> c.shift) * (uint64_t)c.row_stride + (uint64_t)((fw - 1) >> c.shift) * (uint64_t)c.elem_stride) + 2u;
}
// limit: the item's bytes (item_pitch_bytes, or the record's)
LEON_HD inline int32_t field_channel_judge(const FieldChannel& c, int32_t fw, int32_t fh, int32_t dtype, uint64_t limit)
{
#pragma clang fp contract(off)
    if (c.reserved[0] | c.reserved[1]) return kFieldBadReserved;
    if (c.shift < 0 || c.shift > kFieldMaxShift) return kFieldBadShift;
    if (c.elem_stride < 1 || c.elem_stride > kFieldMaxElemStride) return kFieldBadElemStride;
    if (c.row_stride < 0) return kFieldBadRowStride;
    if (c.offset_bytes & 1u) return kFieldBadOffset;
    if (!field_finite(c.scale) || !field_finite(c.bias)) return kFieldBadScale;
    // every stored element is finite: |u| <= fl32(fl32(32768 |scale|) + |bias|), and rounding to the element type is monotone
    const float most = field_value(32768, c.scale < 0.0f ? -c.scale : c.scale, c.bias < 0.0f ? -c.bias : c.bias);
    if (!field_finite(most)) return kFieldBadRange;
    if (dtype == kFieldF16 && (field_f16_bits(most) & 0x7c00u) == 0x7c00u) return kFieldBadRange;
    if (dtype == kFieldBF16 && (field_bf16_bits(most) & 0x7f80u) == 0x7f80u) return kFieldBadRange;
    if (field_channel_end(c, fw, fh) > limit) return kFieldBadExtent;
    return kFieldOk;
}

// ---- a field's value under frame pixel (x, y): nearest-neighbour replication of its cell ------------------------------------------
LEON_HD inline int32_t field_at(const uint8_t* item, const FieldChannel& c, int32_t x, int32_t y)
{
    const size_t at = (size_t)c.offset_bytes + 2u * ((size_t)(y >> c.shift) * (size_t)c.row_stride + (size_t)(x >> c.shift) * (size_t)c.elem_stride);
    uint16_t v;
    memcpy(&v, __builtin_assume_aligned(item + at, 2), 2);
    return (int32_t)(int16_t)v;
}
LEON_HD inline int32_t field_sat16(int64_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : (int32_t)v; }
// the horizontal pass of one sample: row y of the frame, taps first .. first + n - 1 (inside the frame: the tables say so)
LEON_HD inline int32_t field_h(const uint8_t* item, const FieldChannel& c, int32_t y, int32_t first, int32_t n, const int32_t* w)
{
    int64_t acc = (int64_t)1 << (kFieldWeightShift - 1);
    for (int32_t k = 0; k < n; k++) acc += (int64_t)w[k] * (int64_t)field_at(item, c, first + k, y);
    return field_sat16(acc >> kFieldWeightShift);
}

// a region's tables as k_box_tables and plan_resize lay them out
struct FieldTables {
    const int32_t *fx, *nx, *wx, *fy, *ny, *wy;
    int32_t taps_x, taps_y;              // row lengths of wx and wy
};
// The plain loop: output sample (ox, oy) of one channel, both passes
LEON_HD inline int32_t field_sample(const uint8_t* item, const FieldChannel& c, const FieldTables& T, int32_t ox, int32_t oy)
{
    int64_t acc = (int64_t)1 << (kFieldWeightShift - 1);
    const int32_t* wy = T.wy + (size_t)oy * (size_t)T.taps_y;
    for (int32_t k = 0; k < T.ny[oy]; k++)
        acc += (int64_t)wy[k] * (int64_t)field_h(item, c, T.fy[oy] + k, T.fx[ox], T.nx[ox], T.wx + (size_t)ox * (size_t)T.taps_x);
    return field_sat16(acc >> kFieldWeightShift);
}
// ... and the element it becomes, stored at its place of a dense CHW tensor of `channels` x oh x ow
LEON_HD inline void field_store_elem(uint8_t* at, uint32_t bits, int32_t eb)
{
    if (eb == 4) memcpy(__builtin_assume_aligned(at, 4), &bits, 4);
    else {
        const uint16_t v = (uint16_t)bits;
        memcpy(__builtin_assume_aligned(at, 2), &v, 2);
    }
}

// ---- the kernel's walk of one tile: steps between barriers, `tid` = 0 .. kFieldLanes - 1 --------------------------------------------
// What a workgroup holds in LDS (16992 bytes).  wx rows are kFieldMaxTaps = 33 words apart: the lanes of the horizontal pass read
// different rows at the same tap, 33 words apart is a bank apart.
struct FieldTile {
    int32_t wx[kFieldTileX * kFieldMaxTaps], wy[kFieldTileY * kFieldMaxTaps];
    int32_t fx[kFieldTileX], nx[kFieldTileX], fy[kFieldTileY], ny[kFieldTileY];
    int16_t h[kFieldHRows * kFieldTileX];                              // the horizontal pass's results: row rr of the tile's rows, column o
    alignas(16) uint8_t pack[kFieldTileY * kFieldPackStride];          // the tile's elements in memory order, each row at its offset in its 16-byte line
};
struct FieldTileAt {
    int32_t ox0, oy0, nox, noy;          // the tile's origin and extent in the output
};
LEON_HD inline FieldTileAt field_tile_at(int32_t ow, int32_t oh, int32_t bx, int32_t by)
{
    FieldTileAt a;
    a.ox0 = bx * kFieldTileX; a.oy0 = by * kFieldTileY;
    a.nox = ow - a.ox0 < kFieldTileX ? ow - a.ox0 : kFieldTileX;
    a.noy = oh - a.oy0 < kFieldTileY ? oh - a.oy0 : kFieldTileY;
    return a;
}
// step 1: the tile's rows of the tables into LDS (counts are at most 33: k_box_tables refuses the region otherwise)
LEON_HD inline void field_step_tables(FieldTile& t, const FieldTables& T, const FieldTileAt& a, int32_t tid)
{
    if (tid < a.nox) { t.fx[tid] = T.fx[a.ox0 + tid]; t.nx[tid] = T.nx[a.ox0 + tid]; }
    else if (tid >= kFieldTileX && tid - kFieldTileX < a.noy) { t.fy[tid - kFieldTileX] = T.fy[a.oy0 + tid - kFieldTileX]; t.ny[tid - kFieldTileX] = T.ny[a.oy0 + tid - kFieldTileX]; }
    const int32_t tx = T.taps_x < kFieldMaxTaps ? T.taps_x : kFieldMaxTaps, ty = T.taps_y < kFieldMaxTaps ? T.taps_y : kFieldMaxTaps;
    for (int32_t i = tid; i < a.nox * tx; i += kFieldLanes) {
        const int32_t o = i / tx, k = i - o * tx;
        t.wx[o * kFieldMaxTaps + k] = T.wx[(size_t)(a.ox0 + o) * (size_t)T.taps_x + k];
    }
    for (int32_t i = tid; i < a.noy * ty; i += kFieldLanes) {
        const int32_t o = i / ty, k = i - o * ty;
        t.wy[o * kFieldMaxTaps + k] = T.wy[(size_t)(a.oy0 + o) * (size_t)T.taps_y + k];
    }
}
// (behind the barrier, every lane the same) the frame rows the tile's vertical taps need: ry0 .. ry0 + rows - 1
LEON_HD inline void field_tile_rows(const FieldTile& t, const FieldTileAt& a, int32_t* ry0, int32_t* rows)
{
    int32_t lo = t.fy[0], hi = t.fy[0] + t.ny[0];
    for (int32_t s = 1; s < a.noy; s++) {
        lo = t.fy[s] < lo ? t.fy[s] : lo;
        hi = t.fy[s] + t.ny[s] > hi ? t.fy[s] + t.ny[s] : hi;
    }
    *ry0 = lo;
    *rows = hi - lo < kFieldHRows ? hi - lo : kFieldHRows;          // (never more: the tile's constants say why)
}
// step 2, per channel: the horizontal pass of those rows into h; lane = (column o = tid & 31, rows tid >> 5, 8 apart)
LEON_HD inline void field_step_h(FieldTile& t, const uint8_t* item, const FieldChannel& c, const FieldTileAt& a, int32_t ry0, int32_t rows, int32_t tid)
{
    const int32_t o = tid & (kFieldTileX - 1);
    if (o >= a.nox) return;
    const int32_t first = t.fx[o], n = t.nx[o] < kFieldMaxTaps ? t.nx[o] : kFieldMaxTaps;
    for (int32_t rr = tid / kFieldTileX; rr < rows; rr += kFieldLanes / kFieldTileX)
        t.h[rr * kFieldTileX + o] = (int16_t)field_h(item, c, ry0 + rr, first, n, t.wx + o * kFieldMaxTaps);
}
// byte offset in the region's tensor of the tile's row `sub` of channel q
LEON_HD inline size_t field_row_start(int32_t ow, int32_t oh, const FieldTileAt& a, int32_t q, int32_t sub, int32_t eb)
{
    return (((size_t)q * (size_t)oh + (size_t)(a.oy0 + sub)) * (size_t)ow + (size_t)a.ox0) * (size_t)eb;
}
// step 3: the vertical pass from h, a lane per output sample (o = tid & 31, sub = tid >> 5), the element into the packed tile
LEON_HD inline void field_step_v(FieldTile& t, const FieldChannel& c, const FieldTileAt& a, int32_t ow, int32_t oh, int32_t q, int32_t dtype, int32_t ry0, int32_t rows, int32_t tid)
{
    const int32_t o = tid & (kFieldTileX - 1), sub = tid / kFieldTileX;
    if (o >= a.nox || sub >= a.noy) return;
    const int32_t eb = field_elem_bytes(dtype);
    int64_t acc = (int64_t)1 << (kFieldWeightShift - 1);
    const int32_t r0 = t.fy[sub] - ry0;
    for (int32_t k = 0; k < t.ny[sub] && r0 + k < rows; k++) acc += (int64_t)t.wy[sub * kFieldMaxTaps + k] * (int64_t)t.h[(r0 + k) * kFieldTileX + o];
    const uint32_t bits = field_elem(field_value(field_sat16(acc >> kFieldWeightShift), c.scale, c.bias), dtype);
    const size_t g0 = field_row_start(ow, oh, a, q, sub, eb);
    field_store_elem(t.pack + sub * kFieldPackStride + (g0 & (size_t)(kFieldStoreBytes - 1)) + (size_t)(o * eb), bits, eb);
}
// step 4: the packed rows out, a lane per (row = tid >> 4, 16-byte line of the tensor = tid & 15): a line that lies inside the row whole
// in one 16-byte store -- `out`, the region's tensor, is 16-byte aligned --; a line at an end of the row element by element, for the
// tile beside this one (or the row above or below) owns its other bytes
struct FieldLine { uint32_t w[4]; };
LEON_HD inline void field_step_store(const FieldTile& t, uint8_t* out, const FieldTileAt& a, int32_t ow, int32_t oh, int32_t q, int32_t dtype, int32_t tid)
{
    const int32_t eb = field_elem_bytes(dtype), row = tid >> 4, line = tid & 15;
    if (row >= a.noy || line > (kFieldTileX * eb + kFieldStoreBytes - 1) / kFieldStoreBytes) return;
    const size_t g0 = field_row_start(ow, oh, a, q, row, eb), g1 = g0 + (size_t)(a.nox * eb);
    const size_t a0 = (g0 & ~(size_t)(kFieldStoreBytes - 1)) + (size_t)(kFieldStoreBytes * line);
    const uint8_t* from = t.pack + row * kFieldPackStride + kFieldStoreBytes * line;
    if (a0 >= g0 && a0 + kFieldStoreBytes <= g1) {
        FieldLine v;
        memcpy(&v, __builtin_assume_aligned(from, 16), 16);
        memcpy(__builtin_assume_aligned(out + a0, 16), &v, 16);
    } else if (a0 + kFieldStoreBytes > g0 && a0 < g1) {
        for (int32_t e = 0; e < kFieldStoreBytes; e += eb)
            if (a0 + (size_t)e >= g0 && a0 + (size_t)e < g1) {
                uint32_t bits = 0;
                memcpy(&bits, from + e, (size_t)eb);
                field_store_elem(out + a0 + e, bits, eb);
            }
    }
}

}  // namespace leon
#endif
