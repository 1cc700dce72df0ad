// residual_check.cpp -- csrc/leon_residual.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_residual_walk_native.py): every task of k_residual's decomposition, both halves and all 64 lanes, for the sizes whose groups
// differ -- one task per plane (16x16), two block-row pairs (48x32), groups exactly full (128x16), a third luma and a second chroma group
// with one valid block (144x32), ten luma groups with two valid blocks in the last (592x32) and the largest picture (4096x4096).  A lane
// that stores adds 1 to each of its 16 bytes of a record allocated at exactly record_bytes, so a store outside the record is a heap
// overflow the sanitizer reports; afterwards every specified element must have been stored exactly once and every pad column and gap
// between planes never.  The tasks' group ids must be a permutation of 0 .. n_y + 2 n_c - 1, each task's second id the one that shares
// its macroblocks.
#include <cstdio>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_residual.h"

using namespace leon;

static int failed = 0;

static void check(bool ok, const char* what, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at (%u, %u, %u, %u)\n", what, a, b, c, d);
}

static void walk(uint32_t cw, uint32_t ch)
{
    const ResidualLayout L = residual_layout(cw, ch);
    const ResidualGeom G = residual_geom(cw / 16, ch / 16);
    check(L.cb_offset % 256 == 0 && L.cr_offset % 256 == 0 && L.record_pitch % 256 == 0 && L.record_pitch >= L.record_bytes, "alignment", cw, ch, L.cb_offset, L.cr_offset);
    check(L.luma_stride % 64 == 0 && L.chroma_stride % 64 == 0 && L.luma_stride >= cw && L.chroma_stride >= cw / 2, "strides", cw, ch, L.luma_stride, L.chroma_stride);
    check(G.tasks == G.mbh * (G.groups_y + G.groups_c), "task count", cw, ch, G.tasks, 0);
    std::vector<uint8_t> stored(L.record_bytes, 0);          // exactly record_bytes
    std::vector<uint8_t> gid_seen(G.n_y + 2 * G.n_c, 0);
    for (uint32_t t = 0; t < G.tasks; t++) {
        const ResidualTask T = residual_task(G, t);
        check(T.chroma == (t >= G.tasks_y ? 1u : 0u) && T.Rt < G.mbh && T.g < (T.chroma ? G.groups_c : G.groups_y), "task", cw, ch, t, T.g);
        // the second half shares the first one's macroblocks: luma the block row below, chroma the Cr group of the same place
        check(T.gid[1] == T.gid[0] + (T.chroma ? G.n_c : G.groups_y), "second group id", cw, ch, t, T.gid[1]);
        for (uint32_t h = 0; h < 2; h++) {
            check(T.gid[h] < gid_seen.size(), "group id range", cw, ch, t, T.gid[h]);
            if (T.gid[h] < gid_seen.size()) gid_seen[T.gid[h]]++;
            for (uint32_t lane = 0; lane < 64; lane++) {
                uint32_t off = 0;
                const bool stores = residual_store(L, T, h, lane, &off);
                const uint32_t block = 8 * T.g + (lane & 7);
                check(stores == (block < residual_block_width(L, T.chroma)), "who stores", cw, ch, t, lane);
                check(off % 16 == 0, "16-byte alignment", cw, ch, t, lane);
                // the 8 lanes of a row: 128 contiguous bytes
                uint32_t off0 = 0;
                residual_store(L, T, h, lane & ~7u, &off0);
                check(off == off0 + 16 * (lane & 7) && off0 % 128 == 0, "a row of 8 lanes is one 128-byte line", cw, ch, t, lane);
                if (stores)
                    for (uint32_t i = 0; i < 16; i++) stored[(size_t)off + i]++;          // (outside the record: the sanitizer stops here)
            }
        }
    }
    for (size_t g = 0; g < gid_seen.size(); g++) check(gid_seen[g] == 1, "every group read by exactly one task half", cw, ch, (uint32_t)g, gid_seen[g]);
    // every byte of the record: a specified element stored once, everything else never
    std::vector<uint8_t> want(L.record_bytes, 0);
    for (uint32_t plane = 0; plane < 3; plane++) {
        const uint32_t W = plane ? cw / 2 : cw, H = plane ? ch / 2 : ch, stride = plane ? L.chroma_stride : L.luma_stride;
        const size_t base = plane == 0 ? 0 : (plane == 1 ? L.cb_offset : L.cr_offset);
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < 2 * W; x++) want[base + 2 * (size_t)y * stride + x] = 1;
    }
    size_t bad = 0, first = 0;
    for (size_t i = 0; i < want.size(); i++)
        if (stored[i] != want[i] && !bad++) first = i;
    check(bad == 0, "bytes stored other than once where specified and never elsewhere (count, first)", cw, ch, (uint32_t)bad, (uint32_t)first);
}

int main()
{
    const uint32_t sizes[][2] = {{16, 16}, {48, 32}, {128, 16}, {144, 32}, {592, 32}, {4096, 4096}, {1920, 1088}, {16, 4096}, {4096, 16}};
    for (const auto& s : sizes) walk(s[0], s[1]);
    std::printf("residual_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
