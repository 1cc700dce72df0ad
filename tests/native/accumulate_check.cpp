// accumulate_check.cpp -- csrc/leon_accumulate.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_accumulate_walk_native.py): the walk k_accumulate's lanes take over the work units of every plane asked for -- the funnelled
// path and the element path -- over heap buffers of EXACTLY slots_bytes, against the plain loop over elements, for parts 1, 2 and 3 at
// 16 x 16, 64 x 48 and 128 x 32.  The sources include the last slot of the buffer with vectors into its bottom-right corner: a dword
// read past the buffer's end is an error here, not on a device.  The records lie on the heap too, at exactly their sizes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_accumulate.h"

using namespace leon;

static int failed = 0;
static long runs = 0;

static void check(bool ok, const char* what, int a, int b, int c, int d)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
}

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
// floor(a / b), b > 0
static int floor_div(int a, int b) { return a / b - ((a % b) < 0 ? 1 : 0); }

// the definition, element by element, from the header's text: planes in the order AX AY AGE RY RCb RCr
static void by_elements(int cw, int ch, int parts, const uint32_t off[6], uint32_t luma_stride, uint32_t chroma_stride, const uint8_t* rec, uint32_t info_offset,
                        const uint8_t* res, uint32_t cb_offset, uint32_t cr_offset, uint8_t* slots, size_t pitch, const PropagateHop& h, uint8_t* via)
{
    const int mbw = cw / 16;
    for (int kind = 0; kind < 6; kind++) {
        if (!(parts & (kind < 3 ? 1 : 2))) continue;
        const int step = kind >= 4 ? 2 : 1, w = cw / step, hh = ch / step;
        const uint32_t stride = kind >= 4 ? chroma_stride : luma_stride;
        const uint32_t res_off = kind == 4 ? cb_offset : kind == 5 ? cr_offset : 0;
        for (int y = 0; y < hh; y++)
            for (int x = 0; x < w; x++) {
                const size_t k = (size_t)((y * step) >> 4) * mbw + ((x * step) >> 4);
                int16_t v[4];
                std::memcpy(v, rec + 8 * k, 8);
                const int info = rec[info_offset + k];
                int pick = 0, slot = -1, vh = 0, vv = 0;
                if ((info & 1) && h.fwd_slot >= 0) { pick = 1; slot = h.fwd_slot; vh = v[0]; vv = v[1]; }
                else if ((info & 2) && h.bwd_slot >= 0) { pick = 2; slot = h.bwd_slot; vh = v[2]; vv = v[3]; }
                via[k] = (uint8_t)pick;
                int16_t out = 0;
                if (pick) {
                    int sx = x + floor_div(vh + step, 2 * step), sy = y + floor_div(vv + step, 2 * step);
                    sx = sx < 0 ? 0 : sx > w - 1 ? w - 1 : sx;
                    sy = sy < 0 ? 0 : sy > hh - 1 ? hh - 1 : sy;
                    int16_t s, r = 0;
                    std::memcpy(&s, slots + (size_t)slot * pitch + off[kind] + ((size_t)sy * stride + sx) * 2, 2);
                    if (kind >= 3) std::memcpy(&r, res + res_off + ((size_t)y * stride + x) * 2, 2);
                    const int own = kind == 0 ? sx - x : kind == 1 ? sy - y : kind == 2 ? 1 : r;
                    out = (int16_t)sat16(s + own);
                }
                std::memcpy(slots + (size_t)h.dst_slot * pitch + off[kind] + ((size_t)y * stride + x) * 2, &out, 2);
            }
    }
}

// the grid of k_accumulate: a plane a row of blocks of 256 lanes sized for a luma plane, each lane one unit
static void by_units(const AccumulateGeom& g, const uint8_t* rec, uint32_t info_offset, const uint8_t* res, uint8_t* slots, size_t slots_bytes, size_t pitch,
                     const PropagateHop& h, uint8_t* via)
{
    const uint32_t blocks = (g.units_luma + 255u) / 256u;
    for (int q = 0; q < g.planes; q++)
        for (uint32_t bx = 0; bx < blocks; bx++)
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t u = bx * 256u + t;
                if (u >= accumulate_units(g, q)) continue;
                accumulate_unit(g, rec, info_offset, res, slots, slots_bytes, pitch, h, q == 0 ? via : nullptr, q, u);
            }
}

static void one(int cw, int ch, int parts, int gap, int kind, uint32_t seed)
{
    const int mbw = cw / 16, mbh = ch / 16, n_slots = 3;
    AccumulateGeom g;
    check(accumulate_geometry(cw, ch, parts, &g), "geometry", cw, ch, parts, 0);
    const MotionLayout L = motion_layout((uint32_t)mbw, (uint32_t)mbh);
    const ResidualLayout R = residual_layout((uint32_t)cw, (uint32_t)ch);
    check(parts != 2 || (g.off[3] == 0 && g.off[4] == R.cb_offset && g.off[5] == R.cr_offset && g.slot_bytes == R.record_bytes), "parts 2 lies as a residual record", cw, ch, 0, 0);
    // the records on the heap, exactly record_bytes each
    uint8_t* rec = static_cast<uint8_t*>(std::malloc(L.record_bytes));
    std::memset(rec, 0, L.record_bytes);
    for (uint32_t k = 0; k < L.mbs; k++) {
        int16_t v[4];
        for (int c = 0; c < 4; c++) {
            const uint32_t r = lcg(&seed);
            v[c] = kind == 0   ? (int16_t)((int)(r >> 8) % 129 - 64)          // leaves at every edge of these pictures
                   : kind == 1 ? (int16_t)32767                             // into the bottom-right corner
                   : kind == 2 ? (int16_t)-32768                            // into the top-left corner
                   : kind == 3 ? (int16_t)((c & 1) ? 2 * (ch - 1) : 2 * (cw - 4) - (int)(k & 3))          // the last units of the last rows, every alignment
                               : (int16_t)((int)(r >> 8) % 7 - 3);          // the ties
        }
        std::memcpy(rec + 8 * k, v, 8);
        rec[L.info_offset + k] = kind == 0 ? (uint8_t)(k % 5 == 4 ? 4 : 1 + (lcg(&seed) >> 9) % 3) : (uint8_t)(1 + k % 3);
    }
    uint8_t* res = static_cast<uint8_t*>(std::aligned_alloc(8, R.record_bytes));
    for (size_t i = 0; i < R.record_bytes; i += 2) {
        const int16_t r = (int16_t)((int)(lcg(&seed) >> 8) % 2001 - 1000);
        std::memcpy(res + i, &r, 2);
    }
    const size_t pitch = (size_t)g.slot_bytes + (size_t)gap, slots_bytes = (size_t)n_slots * pitch;
    // two buffers of EXACTLY slots_bytes: the sources include the last slot.  Random bits: the whole int16 range, so both saturations happen
    uint8_t* a = static_cast<uint8_t*>(std::malloc(slots_bytes));
    uint8_t* b = static_cast<uint8_t*>(std::malloc(slots_bytes));
    for (size_t i = 0; i < slots_bytes; i++) a[i] = (uint8_t)(lcg(&seed) >> 13);
    std::memcpy(b, a, slots_bytes);
    const size_t n_mbs = (size_t)mbw * mbh;
    std::vector<uint8_t> va(n_mbs), vb(n_mbs);
    const PropagateHop hops[4] = {{0, 0, 2, 1, {0, 0, 0, 0}}, {0, 1, 2, -1, {0, 0, 0, 0}}, {0, 0, -1, 2, {0, 0, 0, 0}}, {0, 1, -1, -1, {0, 0, 0, 0}}};
    for (const PropagateHop& h : hops) {
        check(propagate_hop_status(h, 1, n_slots) == kRegionOk, "status", cw, ch, parts, kind);
        std::memset(va.data(), 0xEE, n_mbs);
        std::memset(vb.data(), 0xEE, n_mbs);
        by_elements(cw, ch, parts, g.off, g.luma_stride, g.chroma_stride, rec, L.info_offset, res, R.cb_offset, R.cr_offset, a, pitch, h, va.data());
        by_units(g, rec, L.info_offset, (parts & 2) ? res : nullptr, b, slots_bytes, pitch, h, vb.data());
        check(std::memcmp(a, b, slots_bytes) == 0, "slots", cw, ch, parts, kind);
        check(va == vb, "via", cw, ch, parts, kind);
        runs++;
    }
    std::free(rec); std::free(res); std::free(a); std::free(b);
}

int main()
{
    const int sizes[3][2] = {{16, 16}, {64, 48}, {128, 32}};
    uint32_t seed = 4242;
    for (const auto& f : sizes)
        for (int parts = 1; parts <= 3; parts++)
            for (int gap : {0, 4, 256})
                for (int kind = 0; kind < 5; kind++) one(f[0], f[1], parts, gap, kind, seed += 31);
    // what the geometry refuses
    {
        AccumulateGeom g;
        check(!accumulate_geometry(60, 48, 1, &g) && !accumulate_geometry(64, 40, 1, &g) && !accumulate_geometry(0, 16, 1, &g), "a size that is no multiple of 16", 0, 0, 0, 0);
        check(!accumulate_geometry(64, 48, 0, &g) && !accumulate_geometry(64, 48, 4, &g), "parts outside 1 .. 3", 0, 0, 0, 0);
    }
    // the packed add against the scalar one, around both ends
    for (int x : {-32768, -32767, -1, 0, 1, 32766, 32767})
        for (int y : {-32768, -5000, -1, 0, 1, 5000, 32767}) {
            const uint32_t r = accumulate_add2(((uint32_t)x & 0xffffu) | ((uint32_t)y << 16), ((uint32_t)y & 0xffffu) | ((uint32_t)x << 16));
            check((int16_t)(uint16_t)r == sat16(x + y) && (int16_t)(uint16_t)(r >> 16) == sat16(x + y), "add2", x, y, 0, 0);
        }
    std::printf("%ld walks\n", runs);
    std::printf("accumulate_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
