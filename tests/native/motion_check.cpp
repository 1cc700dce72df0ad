// motion_check.cpp -- csrc/leon_motion.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_motion_walk_native.py): the walk k_motion's workgroup takes over a picture's macroblocks -- 256 lanes, lane l at
// k0 = 4 l, 4 l + 1024, ..., a dword of repadd and of mb_dir and 16 bytes of each vector map in, 32 bytes of vectors and a dword of
// info out, the summary counted where k0 + i < mbs, 256 partial sums added up -- against the plain loop over motion_mb and
// motion_count, for mbs = 1 .. 2100 and 65536 and the three picture types.  Every map is allocated at exactly its padded size
// (pad256(mbs), pad256(4 mbs)) and the record at exactly its pitch, so a read of the last lane that left a map's padding, or a tail
// store that left the record, is a heap overflow the sanitizer reports; the padding holds 0xFF, which counts if the guard lets it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_motion.h"

using namespace leon;

static int failed = 0;
static const uint32_t kLanes = 256;
static const uint8_t kSentinel = 0xA5;

static void check(bool ok, const char* what, uint32_t mbs, int type)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at mbs %u, type %d\n", what, mbs, type);
}

struct Maps {
    uint8_t *repadd, *mb_dir, *mv_fwd, *mv_bwd;      // malloc'ed at exactly the padded sizes
};

// the kernel's walk, lane by lane
static void by_lanes(int32_t type, const Maps& m, uint8_t* rec, const MotionLayout& G)
{
    std::vector<uint32_t> part(8 * kLanes, 0u);
    const uint32_t mbs = G.mbs;
    for (uint32_t lane = 0; lane < kLanes; lane++) {
        uint32_t* s = &part[8 * lane];
        for (uint32_t k0 = 4u * lane; k0 < mbs; k0 += 4u * kLanes) {
            uint32_t ra = 0u, di = 0u, fi[4] = {0u, 0u, 0u, 0u}, bi[4] = {0u, 0u, 0u, 0u};
            if (type != 1) {
                std::memcpy(&ra, m.repadd + k0, 4);
                std::memcpy(fi, m.mv_fwd + 4 * (size_t)k0, 16);
            }
            if (type == 3) {
                std::memcpy(&di, m.mb_dir + k0, 4);
                std::memcpy(bi, m.mv_bwd + 4 * (size_t)k0, 16);
            }
            uint32_t of[4], ob[4], info4 = 0u;
            for (int i = 0; i < 4; i++) {
                const uint32_t info = motion_mb(type, (ra >> (8 * i)) & 255u, (di >> (8 * i)) & 255u, fi[i], bi[i], &of[i], &ob[i]);
                info4 |= info << (8 * i);
                if (k0 + (uint32_t)i < mbs) motion_count(info, of[i], ob[i], s);
            }
            const uint32_t mv[8] = {of[0], ob[0], of[1], ob[1], of[2], ob[2], of[3], ob[3]};
            std::memcpy(rec + (size_t)k0 * 8u, mv, 32);
            std::memcpy(rec + G.info_offset + k0, &info4, 4);
        }
    }
    uint32_t sum[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t lane = 0; lane < kLanes; lane++)
        for (int i = 0; i < 8; i++) sum[i] += part[8 * lane + i];
    std::memcpy(rec + G.summary_offset, sum, 32);
}

// the definition: one macroblock after the other
static void plain(int32_t type, const Maps& m, uint8_t* rec, const MotionLayout& G)
{
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < G.mbs; k++) {
        uint32_t f = 0u, b = 0u, of, ob;
        if (type != 1) std::memcpy(&f, m.mv_fwd + 4 * (size_t)k, 4);
        if (type == 3) std::memcpy(&b, m.mv_bwd + 4 * (size_t)k, 4);
        const uint32_t info = motion_mb(type, type != 1 ? m.repadd[k] : 0u, type == 3 ? m.mb_dir[k] : 0u, f, b, &of, &ob);
        motion_count(info, of, ob, s);
        std::memcpy(rec + 8 * (size_t)k, &of, 4);
        std::memcpy(rec + 8 * (size_t)k + 4, &ob, 4);
        rec[G.info_offset + k] = (uint8_t)info;
    }
    std::memcpy(rec + G.summary_offset, s, 32);
}

static uint32_t g_seed = 2463534242u;
static uint32_t rnd()
{
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
    return g_seed;
}

static uint8_t* padded(size_t bytes, size_t padded_bytes, bool extreme)
{
    static const uint8_t repadd_values[5] = {0, 1, 127, 128, 255};
    uint8_t* p = static_cast<uint8_t*>(std::malloc(padded_bytes));
    if (!p) std::abort();
    std::memset(p, 0xFF, padded_bytes);
    for (size_t i = 0; i < bytes; i++) p[i] = extreme ? repadd_values[rnd() % 5u] : (uint8_t)rnd();
    return p;
}

static void one(uint32_t mbw, uint32_t mbh)
{
    const MotionLayout G = motion_layout(mbw, mbh);
    const uint32_t mbs = G.mbs;
    const size_t mpad = motion_pad256(mbs), vpad = motion_pad256(4u * mbs), c4 = (mbs + 3u) & ~3u;
    check(G.info_offset >= 8 * c4 && G.summary_offset >= G.info_offset + c4 && G.record_pitch >= G.record_bytes && mpad >= c4 && vpad >= 4 * c4, "layout", mbs, 0);
    Maps m{padded(mbs, mpad, true), padded(mbs, mpad, false), padded(4 * (size_t)mbs, vpad, false), padded(4 * (size_t)mbs, vpad, false)};
    uint8_t* a = static_cast<uint8_t*>(std::malloc(G.record_pitch));
    uint8_t* b = static_cast<uint8_t*>(std::malloc(G.record_pitch));
    if (!a || !b) std::abort();
    for (int type = 1; type <= 3; type++) {
        std::memset(a, kSentinel, G.record_pitch);
        std::memset(b, kSentinel, G.record_pitch);
        by_lanes(type, m, a, G);
        plain(type, m, b, G);
        check(std::memcmp(a, b, 8 * (size_t)mbs) == 0, "vectors", mbs, type);
        check(std::memcmp(a + G.info_offset, b + G.info_offset, mbs) == 0, "info", mbs, type);
        check(std::memcmp(a + G.summary_offset, b + G.summary_offset, 32) == 0, "summary", mbs, type);
        bool kept = true;
        for (size_t i = 8 * c4; i < G.info_offset; i++) kept = kept && a[i] == kSentinel;
        for (size_t i = G.info_offset + c4; i < G.summary_offset; i++) kept = kept && a[i] == kSentinel;
        for (size_t i = G.record_bytes; i < G.record_pitch; i++) kept = kept && a[i] == kSentinel;
        check(kept, "the bytes behind the last group of four", mbs, type);
    }
    std::free(a); std::free(b);
    std::free(m.repadd); std::free(m.mb_dir); std::free(m.mv_fwd); std::free(m.mv_bwd);
}

int main()
{
    for (uint32_t mbs = 1; mbs <= 2100; mbs++) {
        uint32_t h = 1;
        while (mbs / h > 256u || mbs % h) h++;          // a factoring inside 256 x 256 where there is one
        if (mbs / h <= 256u && h <= 256u) one(mbs / h, h);
        else one(mbs, 1);                               // a prime above 256: no picture, but the walk and the layout ask for mbs alone
    }
    one(256, 256);
    // the bound: both directions everywhere, every word -2048, 65536 macroblocks: 2^27 in every sum, 256 lanes of 2^19 each
    {
        const MotionLayout G = motion_layout(256, 256);
        std::vector<uint8_t> repadd(motion_pad256(G.mbs), 0), dir(motion_pad256(G.mbs), 3), rec(G.record_pitch, kSentinel);
        std::vector<uint16_t> v(motion_pad256(4 * G.mbs) / 2, (uint16_t)-2048);
        Maps m{repadd.data(), dir.data(), reinterpret_cast<uint8_t*>(v.data()), reinterpret_cast<uint8_t*>(v.data())};
        by_lanes(3, m, rec.data(), G);
        uint32_t s[8];
        std::memcpy(s, rec.data() + G.summary_offset, 32);
        check(s[0] == 65536u && s[1] == 65536u && s[2] == 0u && s[3] == 65536u && s[4] == 1u << 27 && s[5] == 1u << 27 && s[6] == 1u << 27 && s[7] == 1u << 27, "2^27", G.mbs, 3);
        check(motion_abs16(0x8000u) == 32768u && motion_abs16(0xF800u) == 2048u && motion_abs16(0x7FFFu) == 32767u, "motion_abs16", 0, 0);
    }
    std::printf("motion_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
