// propagate_check.cpp -- csrc/leon_propagate.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_propagate_walk_native.py): the walk k_propagate's lanes take over the work units of a map -- both paths, every plane
// group -- over heap buffers of EXACTLY maps_bytes, against the plain loop over cells, for every stride and element size at 64 x 48
// and 61 x 45.  The sources include the last slot of the buffer with vectors into its bottom-right corner: a dword read past the
// buffer's end is an error here, not on a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_propagate.h"

using namespace leon;

static int failed = 0;
static long runs = 0;

static void check(bool ok, const char* what, int a, int b, int c, int d)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
}

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

// the definition, cell by cell, byte by byte
static void by_cells(const PropagateGeom& g, const uint8_t* rec, uint32_t info_offset, uint8_t* maps, size_t pitch, const PropagateHop& h, uint32_t fill, uint8_t* via)
{
    const int s = 1 << g.ls;
    for (int cy = 0; cy < g.mh; cy++)
        for (int cx = 0; cx < g.mw; cx++) {
            const size_t k = (size_t)((cy * s) >> 4) * g.mbw + ((cx * s) >> 4);
            int16_t v[4];
            std::memcpy(v, rec + 8 * k, 8);
            const int info = rec[info_offset + k];
            int pick = 0, slot = -1, vh = 0, vv = 0;
            if ((info & 1) && h.fwd_slot >= 0) { pick = 1; slot = h.fwd_slot; vh = v[0]; vv = v[1]; }
            else if ((info & 2) && h.bwd_slot >= 0) { pick = 2; slot = h.bwd_slot; vh = v[2]; vv = v[3]; }
            via[(size_t)cy * g.mw + cx] = (uint8_t)pick;
            // floor((v + s) / (2 s)) with a division that floors
            int dx = (vh + s) / (2 * s), dy = (vv + s) / (2 * s);
            if ((vh + s) % (2 * s) < 0) dx--;
            if ((vv + s) % (2 * s) < 0) dy--;
            int sx = cx + dx, sy = cy + dy;
            sx = sx < 0 ? 0 : sx > g.mw - 1 ? g.mw - 1 : sx;
            sy = sy < 0 ? 0 : sy > g.mh - 1 ? g.mh - 1 : sy;
            for (int pl = 0; pl < g.planes; pl++) {
                uint8_t* d = maps + (size_t)h.dst_slot * pitch + pl * g.plane_bytes + ((size_t)cy * g.mw + cx) * g.e;
                if (!pick) std::memcpy(d, &fill, g.e);          // (little endian: the low e bytes)
                else std::memcpy(d, maps + (size_t)slot * pitch + pl * g.plane_bytes + ((size_t)sy * g.mw + sx) * g.e, g.e);
            }
        }
}

// the grid of k_propagate: plane groups by blocks of 256 lanes, each lane one unit
static void by_units(const PropagateGeom& g, const uint8_t* rec, uint32_t info_offset, uint8_t* maps, size_t maps_bytes, size_t pitch, const PropagateHop& h, uint32_t fill, uint8_t* via)
{
    const uint32_t blocks = (g.units + 255u) / 256u;
    for (int y = 0; y * g.group < g.planes; y++)
        for (uint32_t bx = 0; bx < blocks; bx++)
            for (uint32_t t = 0; t < 256u; t++) {
                const uint32_t u = bx * 256u + t;
                if (u >= g.units) continue;
                const int p0 = y * g.group, p1 = p0 + g.group < g.planes ? p0 + g.group : g.planes;
                propagate_unit(g, rec, info_offset, maps, maps_bytes, pitch, h, fill, y == 0 ? via : nullptr, u, p0, p1);
            }
}

static void one(int fw, int fh, int s, int e, int planes, int gap, int kind, uint32_t seed)
{
    const int mbw = (fw + 15) / 16, mbh = (fh + 15) / 16, n_slots = 3;
    PropagateGeom g;
    check(propagate_geometry(fw, fh, mbw, s, planes, e, &g), "geometry", fw, s, e, planes);
    const MotionLayout L = motion_layout((uint32_t)mbw, (uint32_t)mbh);
    // a record on the heap, exactly record_bytes
    uint8_t* rec = static_cast<uint8_t*>(std::malloc(L.record_bytes));
    std::memset(rec, 0, L.record_bytes);
    for (uint32_t k = 0; k < L.mbs; k++) {
        int16_t v[4];
        for (int c = 0; c < 4; c++) {
            const uint32_t r = lcg(&seed);
            v[c] = kind == 0   ? (int16_t)((int)(r >> 8) % (32 * s + 1) - 16 * s)
                   : kind == 1 ? (int16_t)32767          // into the bottom-right corner
                   : kind == 2 ? (int16_t)-32768         // into the top-left corner
                               : (int16_t)((c & 1) ? 2 * s * 2 : 2 * s * 3 + 1);
        }
        std::memcpy(rec + 8 * k, v, 8);
        rec[L.info_offset + k] = kind == 0 ? (uint8_t)(k % 5 == 4 ? 4 : 1 + (lcg(&seed) >> 9) % 3) : (uint8_t)(1 + k % 3);
    }
    const size_t slot_bytes = (size_t)planes * g.plane_bytes, pitch = (slot_bytes + 3) / 4 * 4 + (size_t)gap;
    size_t maps_bytes = (size_t)n_slots * pitch;
    // two buffers of EXACTLY maps_bytes: the sources include the last slot
    uint8_t* a = static_cast<uint8_t*>(std::malloc(maps_bytes));
    uint8_t* b = static_cast<uint8_t*>(std::malloc(maps_bytes));
    for (size_t i = 0; i < maps_bytes; i++) a[i] = (uint8_t)(lcg(&seed) >> 13);
    std::memcpy(b, a, maps_bytes);
    const size_t n_cells = (size_t)g.mh * g.mw;
    uint8_t* va = static_cast<uint8_t*>(std::malloc(n_cells));
    uint8_t* vb = static_cast<uint8_t*>(std::malloc(n_cells));
    const PropagateHop hops[4] = {{0, 0, 2, 1, {0, 0, 0, 0}}, {0, 1, 2, -1, {0, 0, 0, 0}}, {0, 0, -1, 2, {0, 0, 0, 0}}, {0, 1, -1, -1, {0, 0, 0, 0}}};
    for (int fast = g.fast; fast >= 0; fast--) {          // the fast path where the geometry allows it, and the cell path always
        PropagateGeom q = g;
        if (!fast && g.fast) { q.fast = 0; q.units_row = (uint32_t)q.mw; q.units = q.units_row * (uint32_t)q.mh; }
        for (const PropagateHop& h : hops) {
            check(propagate_hop_status(h, 1, n_slots) == kRegionOk, "status", s, e, planes, kind);
            std::memset(va, 0xEE, n_cells);
            std::memset(vb, 0xEE, n_cells);
            by_cells(q, rec, L.info_offset, a, pitch, h, 0xC3B2A190u, va);
            by_units(q, rec, L.info_offset, b, maps_bytes, pitch, h, 0xC3B2A190u, vb);
            check(std::memcmp(a, b, maps_bytes) == 0, fast ? "maps, fast path" : "maps, cell path", fw, s, e, planes * 10 + kind);
            check(std::memcmp(va, vb, n_cells) == 0, fast ? "via, fast path" : "via, cell path", fw, s, e, planes * 10 + kind);
            runs++;
        }
    }
    std::free(rec); std::free(a); std::free(b); std::free(va); std::free(vb);
}

int main()
{
    const int frames[2][2] = {{64, 48}, {61, 45}};
    uint32_t seed = 777;
    for (const auto& f : frames)
        for (int s = 1; s <= 16; s *= 2)
            for (int e = 1; e <= 4; e *= 2)
                for (int planes : {1, 3, 4, 5, 9})
                    for (int kind = 0; kind < 4; kind++) one(f[0], f[1], s, e, planes, planes == 3 ? 8 : 0, kind, seed += 31);
    // the judgement
    {
        const PropagateHop ok{0, 0, 1, -1, {0, 0, 0, 0}};
        check(propagate_hop_status(ok, 1, 2) == kRegionOk, "ok", 0, 0, 0, 0);
        PropagateHop h = ok; h.reserved[3] = 1; h.target = 5; h.dst_slot = 9;
        check(propagate_hop_status(h, 1, 2) == kRegionReserved, "reserved first", 0, 0, 0, 0);
        h = ok; h.target = 1; h.dst_slot = 9;
        check(propagate_hop_status(h, 1, 2) == kRegionFrame, "frame before slot", 0, 0, 0, 0);
        h = ok; h.dst_slot = 2;
        check(propagate_hop_status(h, 1, 2) == kRegionSlot, "dst outside", 0, 0, 0, 0);
        h = ok; h.fwd_slot = -2;
        check(propagate_hop_status(h, 1, 2) == kRegionSlot, "source below -1", 0, 0, 0, 0);
        h = ok; h.bwd_slot = 0;
        check(propagate_hop_status(h, 1, 2) == kRegionSlot, "dst among the sources", 0, 0, 0, 0);
    }
    // the rounding: floor((v + s) / (2 s)) for every int16 and every stride
    for (int ls = 0; ls <= 4; ls++)
        for (int v = -32768; v <= 32767; v++) {
            const int s = 1 << ls, d = propagate_cells((uint32_t)(uint16_t)(int16_t)v, ls);
            check(2 * s * d <= v + s && v + s < 2 * s * (d + 1), "floor", ls, v, d, 0);
        }
    std::printf("%ld walks\n", runs);
    std::printf("propagate_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
