// activity_check.cpp -- csrc/leon_activity.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_activity_walk_native.py): the walk k_activity takes over a picture's group lists -- a task per chroma group and
// macroblock row, its six lists in the kernel's order, 64 lanes striding over each list's entries, lane l adding into word l & 7 of
// the task's bins, lanes 0 .. 7 adding a macroblock's words up and storing its cell -- and k_activity_summary's walk over the cells,
// 256 lanes and their partial words, against the plain loop over the groups in their own order.  Every list and map is allocated at
// exactly its padded size (pad256(4 (n_groups + 1)), pad256(4 n + 4), pad256(mbs)) and the record at exactly its pitch, so a read that
// left a list or a store that left the record is a heap overflow the sanitizer reports; the padding holds 0xFF, which would count as
// level -1 if a clamp let it.  The capacity handed to the walk is exactly grp_off[last].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_activity.h"

using namespace leon;

static int failed = 0;
static const uint32_t kLanes = 64, kSpread = 8;
static const uint8_t kSentinel = 0xA5;

static void check(bool ok, const char* what, uint32_t mbw, uint32_t mbh)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at %u x %u macroblocks\n", what, mbw, mbh);
}

struct Lists {
    uint32_t* grp_off;      // malloc'ed at exactly the padded sizes
    uint32_t* entries;
    uint8_t* qscale;
    uint32_t cap;
};

// the kernels' walk, task by task and lane by lane
static void by_tasks(const Lists& D, uint8_t* rec, const ActivityGeom& G, const ActivityLayout& L)
{
    for (uint32_t task = 0; task < G.tasks; task++) {
        const uint32_t my = task / G.groups_c, c = task - my * G.groups_c;
        std::vector<uint64_t> bins(3 * 8 * kSpread, 0);
        uint64_t seen_s = 0;
        for (uint32_t lane = 0; lane < kLanes; lane++) {
            uint64_t seen = 0;
            for (uint32_t part = 0; part < 6u; part++) {
                const uint32_t plane = part < 4u ? 0u : part - 3u;
                const uint32_t R = plane == 0u ? 2u * my + (part >> 1) : my, g = plane == 0u ? 2u * c + (part & 1u) : c;
                if (plane == 0u && g >= G.groups_y) continue;
                const uint32_t gid = plane == 0u ? R * G.groups_y + g : G.n_y + (plane - 1u) * G.n_c + R * G.groups_c + g;
                uint32_t begin, end;
                activity_span(D.grp_off[gid], D.grp_off[gid + 1u], D.cap, &begin, &end);
                for (uint32_t i = begin + lane; i < end; i += 64u) {
                    const uint32_t e = D.entries[i], a = activity_abs(e);
                    uint32_t mx, mmy, j;
                    activity_place(plane, R, g, activity_b(e), &mx, &mmy, &j);
                    if (a == 0u || mx >= G.mbw) continue;
                    if (mmy != my || mx < 8u * c || mx >= 8u * c + 8u) { check(false, "an entry outside its task", G.mbw, G.mbh); continue; }
                    const uint32_t m = (mx - 8u * c) & 7u, at = m * kSpread + (lane & 7u);
                    if (activity_is_dc(e)) {
                        bins[2u * 8u * kSpread + at] += a;
                    } else {
                        bins[at] += 1;
                        bins[8u * kSpread + at] += a;
                    }
                    seen |= 1ull << (6u * m + j);
                }
            }
            seen_s |= seen;
        }
        for (uint32_t lane = 0; lane < 8u; lane++) {
            const uint32_t mx = 8u * c + lane;
            if (mx >= G.mbw) continue;
            uint64_t sum[3] = {0, 0, 0};
            for (int f = 0; f < 3; f++)
                for (uint32_t r = 0; r < kSpread; r++) sum[f] += bins[((size_t)f * 8u + lane) * kSpread + r];
            const uint32_t k = my * G.mbw + mx;
            uint32_t cell[2];
            activity_cell(sum[0], sum[1], sum[2], (uint32_t)(seen_s >> (6u * lane)) & 63u, D.qscale[k], &cell[0], &cell[1]);
            std::memcpy(rec + 8u * (size_t)k, cell, 8);
        }
    }
    // k_activity_summary: 256 lanes over the cells, their partial words added up (a maximum in [4])
    std::vector<uint32_t> part(8 * 256, 0u);
    for (uint32_t lane = 0; lane < 256u; lane++)
        for (uint32_t k = lane; k < L.mbs; k += 256u) {
            uint32_t cell[2];
            std::memcpy(cell, rec + 8u * (size_t)k, 8);
            activity_count(cell[0], cell[1], &part[8 * lane]);
        }
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t lane = 0; lane < 256u; lane++)
        for (int i = 0; i < 7; i++) s[i] = i == 4 ? (part[8 * lane + i] > s[i] ? part[8 * lane + i] : s[i]) : s[i] + part[8 * lane + i];
    std::memcpy(rec + L.summary_offset, s, 32);
}

// the definition: one group after the other in the lists' own order, exact sums per macroblock
static void plain(const Lists& D, uint8_t* rec, const ActivityGeom& G, const ActivityLayout& L)
{
    std::vector<uint64_t> sums(3 * (size_t)L.mbs, 0);
    std::vector<uint8_t> blocks(L.mbs, 0);
    for (uint32_t plane = 0; plane < 3u; plane++) {
        const uint32_t rows = plane == 0u ? 2u * G.mbh : G.mbh, groups = plane == 0u ? G.groups_y : G.groups_c;
        const uint32_t first = plane == 0u ? 0u : G.n_y + (plane - 1u) * G.n_c;
        for (uint32_t R = 0; R < rows; R++)
            for (uint32_t g = 0; g < groups; g++) {
                const uint32_t gid = first + R * groups + g;
                for (uint32_t i = D.grp_off[gid]; i < D.grp_off[gid + 1]; i++) {
                    const uint32_t e = D.entries[i];
                    const int32_t level = (int16_t)(uint16_t)(e & 0xffffu);
                    const uint32_t a = (uint32_t)(level < 0 ? -level : level), b = (e >> 20) & 7u;
                    const bool dc = ((e >> 23) & 7u) == 0u && ((e >> 17) & 7u) == 0u;
                    const uint32_t mx = plane == 0u ? 4u * g + (b >> 1) : 8u * g + b, my = plane == 0u ? R >> 1 : R;
                    const uint32_t j = plane == 0u ? 2u * (R & 1u) + (b & 1u) : 3u + plane;
                    if (level == 0 || mx >= G.mbw) continue;
                    const size_t k = (size_t)my * G.mbw + mx;
                    if (dc) sums[2 * (size_t)L.mbs + k] += a;
                    else { sums[k] += 1; sums[(size_t)L.mbs + k] += a; }
                    blocks[k] |= (uint8_t)(1u << j);
                }
            }
    }
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (size_t k = 0; k < L.mbs; k++) {
        const uint64_t v[3] = {sums[k], sums[L.mbs + k], sums[2 * (size_t)L.mbs + k]};
        uint16_t h[3];
        for (int f = 0; f < 3; f++) h[f] = (uint16_t)(v[f] > 65535u ? 65535u : v[f]);
        const uint8_t q = blocks[k] ? D.qscale[k] : (uint8_t)0;
        std::memcpy(rec + 8 * k, h, 6);
        rec[8 * k + 6] = blocks[k];
        rec[8 * k + 7] = q;
        s[0] += blocks[k] != 0;
        s[1] += h[0]; s[2] += h[1]; s[3] += h[2];
        s[4] = h[1] > s[4] ? h[1] : s[4];
        s[5] += q;
        s[6] += (uint32_t)__builtin_popcount(blocks[k]);
    }
    std::memcpy(rec + L.summary_offset, s, 32);
}

static uint32_t g_seed = 2463534242u;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
    return g_seed;
}

static void* padded(size_t padded_bytes)
{
    void* p = std::malloc(padded_bytes);
    if (!p) std::abort();
    std::memset(p, 0xFF, padded_bytes);
    return p;
}

// huge: one group of 140000 entries of -32768 (a sum past 2^32 before it saturates); else sizes from the list below
static void one(uint32_t mbw, uint32_t mbh, bool huge)
{
    static const uint32_t sizes[7] = {0, 1, 63, 64, 65, 129, 512};
    static const int32_t levels[6] = {0, 1, -1, 255, -255, -32768};
    const ActivityGeom G = activity_geom(mbw, mbh);
    const ActivityLayout L = activity_layout(mbw, mbh);
    const uint32_t n_groups = G.n_y + 2u * G.n_c;
    check(G.tasks == mbh * G.groups_c && L.summary_offset >= 8u * L.mbs && L.record_pitch >= L.record_bytes && L.record_bytes == L.summary_offset + 32u, "layout", mbw, mbh);
    std::vector<uint32_t> off(n_groups + 1, 0u);
    for (uint32_t g = 0; g < n_groups; g++) off[g + 1] = off[g] + (huge ? (g == 0 ? 140000u : 0u) : sizes[rnd() % 7u]);
    const uint32_t n = off[n_groups];
    Lists D;
    D.cap = n;
    D.grp_off = static_cast<uint32_t*>(padded(activity_pad256(4u * (n_groups + 1u))));
    D.entries = static_cast<uint32_t*>(padded(activity_pad256(4u * n + 4u)));
    D.qscale = static_cast<uint8_t*>(padded(activity_pad256(L.mbs)));
    std::memcpy(D.grp_off, off.data(), 4 * (size_t)(n_groups + 1));
    for (uint32_t i = 0; i < n; i++) {
        const int32_t level = huge ? -32768 : ((rnd() & 1u) ? levels[rnd() % 6u] : (int32_t)(rnd() % 4095u) - 2047);
        uint32_t r = rnd() & 7u, c = rnd() & 7u;
        if (rnd() % 6u == 0u) r = c = 0u;
        if (huge) { r = 1u; c = 0u; }
        const uint32_t b = huge ? 0u : rnd() & 7u, junk = (i & 3u) == 3u ? rnd() & 63u : 0u;
        D.entries[i] = ((uint32_t)level & 0xffffu) | ((r * 128u + b * 16u + c * 2u) << 16) | (junk << 26);
    }
    for (uint32_t k = 0; k < L.mbs; k++) D.qscale[k] = (uint8_t)(1u + rnd() % 31u);
    uint8_t* a = static_cast<uint8_t*>(std::malloc(L.record_pitch));
    uint8_t* b = static_cast<uint8_t*>(std::malloc(L.record_pitch));
    if (!a || !b) std::abort();
    std::memset(a, kSentinel, L.record_pitch);
    std::memset(b, kSentinel, L.record_pitch);
    by_tasks(D, a, G, L);
    plain(D, b, G, L);
    check(std::memcmp(a, b, 8 * (size_t)L.mbs) == 0, "cells", mbw, mbh);
    check(std::memcmp(a + L.summary_offset, b + L.summary_offset, 32) == 0, "summary", mbw, mbh);
    bool kept = true;
    for (size_t i = 8 * (size_t)L.mbs; i < L.summary_offset; i++) kept = kept && a[i] == kSentinel;
    for (size_t i = L.record_bytes; i < L.record_pitch; i++) kept = kept && a[i] == kSentinel;
    check(kept, "the bytes between and behind the parts", mbw, mbh);
    if (huge) {
        uint32_t s[8];
        std::memcpy(s, a + L.summary_offset, 32);
        check(s[0] == 1u && s[1] == 65535u && s[2] == 65535u && s[3] == 0u && s[4] == 65535u && s[6] == 1u && s[7] == 0u, "saturation past 2^32", mbw, mbh);
    }
    std::free(a); std::free(b);
    std::free(D.grp_off); std::free(D.entries); std::free(D.qscale);
}

int main()
{
    static const uint32_t widths[8] = {1, 4, 5, 8, 9, 12, 13, 37}, heights[3] = {1, 2, 3};
    for (uint32_t w : widths)
        for (uint32_t h : heights)
            for (int round = 0; round < 3; round++) one(w, h, false);
    for (uint32_t w = 1; w <= 40; w++) one(w, 1u + w % 4u, false);
    one(120, 68, false);
    one(256, 256, false);
    one(1, 1, true);
    one(9, 2, true);
    check(activity_abs(0x8000u) == 32768u && activity_abs(0xffffu) == 1u && activity_abs(0x12340000u) == 0u, "activity_abs", 0, 0);
    check(activity_sat(65534u) == 65534u && activity_sat(65535u) == 65535u && activity_sat(1ull << 40) == 65535u, "activity_sat", 0, 0);
    uint32_t lo, hi;
    activity_cell(1, 2, 3, 0u, 17u, &lo, &hi);
    check(lo == (1u | 2u << 16) && hi == 3u, "a macroblock without blocks shows no qscale", 0, 0);
    std::printf("activity_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
