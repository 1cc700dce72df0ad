// gauge_check.cpp -- csrc/leon_gauge.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_gauge_walk_native.py): the walk k_gauge's wave takes over the macroblocks a box covers -- 64 lanes, lane l at k = l,
// l + 64, ..., k -> (k / cols, k % cols), 64 partial sums added up and the maximum taken across them -- against the plain double loop
// over the same rectangle, for every box of a small grid and each set of sources, and for the whole frame of the largest grid with
// every value at its extreme, where a word reaches 2^24 * 65535.  Every record is allocated at exactly record_bytes, so a load past a
// record's specified bytes is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_gauge.h"

using namespace leon;

static int failed = 0;

static void check(bool ok, const char* what, int a, int b, int c, int d)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
}

struct Records {
    std::vector<uint8_t> motion, activity;          // exactly record_bytes each
    MotionLayout ml;
    ActivityLayout al;
    int mbw;
};

static Records make(int mbw, int mbh)
{
    Records r;
    r.ml = motion_layout((uint32_t)mbw, (uint32_t)mbh);
    r.al = activity_layout((uint32_t)mbw, (uint32_t)mbh);
    r.motion.assign(r.ml.record_bytes, 0);
    r.activity.assign(r.al.record_bytes, 0);
    r.mbw = mbw;
    return r;
}

static void put(Records& r, size_t mb, uint32_t lo, uint32_t hi, uint32_t info, uint32_t fwd, uint32_t bwd)
{
    std::memcpy(&r.activity[8 * mb], &lo, 4);
    std::memcpy(&r.activity[8 * mb + 4], &hi, 4);
    std::memcpy(&r.motion[8 * mb], &fwd, 4);
    std::memcpy(&r.motion[8 * mb + 4], &bwd, 4);
    r.motion[r.ml.info_offset + mb] = (uint8_t)info;
}

// one macroblock as the kernel loads it: 8 bytes of the cell, 8 bytes of mv, one byte of info, whichever the sources ask for
static void load_and_add(const Records& r, int sources, int x, int y, int w, int h, int mi, int mj, GaugeSums* s)
{
    const size_t mb = (size_t)mj * (size_t)r.mbw + (size_t)mi;
    uint32_t lo = 0, hi = 0, fwd = 0, bwd = 0, info = 0;
    if (sources & kGaugeActivity) {
        std::memcpy(&lo, &r.activity[8 * mb], 4);
        std::memcpy(&hi, &r.activity[8 * mb + 4], 4);
    }
    if (sources & kGaugeMotion) {
        std::memcpy(&fwd, &r.motion[8 * mb], 4);
        std::memcpy(&bwd, &r.motion[8 * mb + 4], 4);
        info = r.motion[r.ml.info_offset + mb];
    }
    gauge_cell(sources, carry_weight(x, y, w, h, mi, mj), lo, hi, info, fwd, bwd, s);
}

static void by_rows(const Records& r, int sources, int x, int y, int w, int h, int64_t* out)
{
    GaugeSums s{};
    for (int j = y >> 4; j <= (y + h - 1) >> 4; j++)
        for (int i = x >> 4; i <= (x + w - 1) >> 4; i++) load_and_add(r, sources, x, y, w, h, i, j, &s);
    gauge_finish(sources, s, out);
}

static void by_lanes(const Records& r, int sources, int x, int y, int w, int h, int64_t* out)
{
    static GaugeSums lane[64];
    std::memset(lane, 0, sizeof(lane));
    const int32_t i0 = x >> 4, j0 = y >> 4;
    const uint32_t cols = (uint32_t)(((x + w - 1) >> 4) - i0 + 1), rows = (uint32_t)(((y + h - 1) >> 4) - j0 + 1);
    for (uint32_t l = 0; l < 64; l++)
        for (uint32_t k = l; k < cols * rows; k += 64u) {
            const uint32_t jj = k / cols, ii = k - jj * cols;
            load_and_add(r, sources, x, y, w, h, i0 + (int32_t)ii, j0 + (int32_t)jj, &lane[l]);
        }
    // what crosses the wave: the sums of the sources asked for, the maximum as 32 bits
    GaugeSums s{};
    for (const GaugeSums& p : lane) {
        s.w[0] += p.w[0];
        if (sources & kGaugeActivity) {
            for (int k = 1; k < 7; k++) s.w[k] += p.w[k];
            s.w[7] = (int64_t)((uint32_t)p.w[7] > (uint32_t)s.w[7] ? (uint32_t)p.w[7] : (uint32_t)s.w[7]);
        }
        if (sources & kGaugeMotion)
            for (int k = 8; k < kGaugeWords; k++) s.w[k] += p.w[k];
    }
    gauge_finish(sources, s, out);
}

int main()
{
    // every box of a 40 x 36 frame in a 3 x 3 grid (step 3 and 5 on the vertical axis), each set of sources
    {
        const int mbw = 3, mbh = 3, fw = 40, fh = 36;
        Records r = make(mbw, mbh);
        uint32_t seed = 12345;
        for (int k = 0; k < mbw * mbh; k++) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t blocks = k % 4 == 1 ? 0u : (seed >> 9) & 63u, info = k % 4 == 3 ? 4u : 1u + k % 3;
            uint32_t lo, hi;
            activity_cell(k == 2 ? 70000u : seed & 0x3ffu, k == 2 ? 70000u : (seed >> 10) & 0xffffu, k == 4 ? 65535u : (seed >> 3) & 0xfffu, blocks, 1u + (seed >> 27), &lo, &hi);
            if (!blocks) lo = hi = 0u;
            put(r, (size_t)k, lo, hi, info, (info & 1u) ? seed : 0u, (info & 2u) ? seed * 2654435761u : 0u);
        }
        long boxes = 0;
        for (int x = 0; x < fw; x++)
            for (int y = 0; y < fh; y += 3)
                for (int w = 1; w <= fw - x; w++)
                    for (int h = 1; h <= fh - y; h += 5) {
                        const GaugeRecord rec{0, x, y, w, h, {0, 0, 0}};
                        check(gauge_record_status(rec, fw, fh, 1) == kRegionOk, "status", x, y, w, h);
                        for (int sources = 1; sources <= 3; sources++) {
                            int64_t a[kGaugeWords], b[kGaugeWords];
                            by_rows(r, sources, x, y, w, h, a);
                            by_lanes(r, sources, x, y, w, h, b);
                            check(std::memcmp(a, b, sizeof(a)) == 0, "lanes", x, y, w, h);
                            check(a[0] == (int64_t)w * h, "word 0 is the box's area", x, y, w, h);
                            bool zero = true;
                            for (int k = 1; k < 8; k++) zero = zero && ((sources & kGaugeActivity) || a[k] == 0);
                            for (int k = 8; k < kGaugeWords; k++) zero = zero && ((sources & kGaugeMotion) || a[k] == 0);
                            check(zero, "a source that was not asked for reads 0", x, y, w, h);
                            check(a[1] <= a[0] && a[8] + a[10] <= 2 * a[0] && a[11] <= a[0] && a[7] <= 65535, "bounds", x, y, w, h);
                        }
                        boxes++;
                    }
        std::printf("%ld boxes\n", boxes);
    }
    // the statuses and their order
    {
        const int fw = 40, fh = 36;
        check(gauge_record_status(GaugeRecord{9, 0, 0, 0, 0, {1, 0, 0}}, fw, fh, 2) == kRegionReserved, "reserved 0", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{9, 0, 0, 0, 0, {0, 1, 0}}, fw, fh, 2) == kRegionReserved, "reserved 1", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{9, 0, 0, 0, 0, {0, 0, -1}}, fw, fh, 2) == kRegionReserved, "reserved 2", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{2, 0, 0, 0, 0, {0, 0, 0}}, fw, fh, 2) == kRegionFrame, "frame", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{-1, 0, 0, 1, 1, {0, 0, 0}}, fw, fh, 2) == kRegionFrame, "frame below 0", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{1, 0, 0, 0, 1, {0, 0, 0}}, fw, fh, 2) == kRegionBox, "empty", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{1, 39, 35, 2, 1, {0, 0, 0}}, fw, fh, 2) == kRegionBox, "leaves the frame", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{1, 2147483647, 0, 2147483647, 1, {0, 0, 0}}, fw, fh, 2) == kRegionBox, "no overflow", 0, 0, 0, 0);
        check(gauge_record_status(GaugeRecord{1, 39, 35, 1, 1, {0, 0, 0}}, fw, fh, 2) == kRegionOk, "the last pixel", 0, 0, 0, 0);
    }
    // the largest picture, every value at its extreme: 2^24 * 65535 and 2^24 * 32768, below 2^41
    {
        const int mb = 256, f = 4096;
        Records r = make(mb, mb);
        for (size_t k = 0; k < (size_t)mb * mb; k++) put(r, k, 0xffffffffu, 0x1f3fffffu, 3u, 0x80008000u, 0x80008000u);
        int64_t a[kGaugeWords], b[kGaugeWords];
        by_rows(r, 3, 0, 0, f, f, a);
        by_lanes(r, 3, 0, 0, f, f, b);
        const int64_t area = (int64_t)1 << 24;
        check(std::memcmp(a, b, sizeof(a)) == 0, "2^40 by lanes", 0, 0, f, f);
        check(a[0] == area && a[1] == area && a[2] == area * 65535 && a[3] == area * 65535 && a[4] == area * 65535 && a[5] == area * 31 && a[6] == area * 6 && a[7] == 65535,
              "2^40, activity", 0, 0, f, f);
        check(a[8] == area && a[9] == area && a[10] == 0 && a[11] == area && a[12] == area * 32768 && a[15] == area * 32768, "2^40, motion", 0, 0, f, f);
        for (int k = 0; k < kGaugeWords; k++) check(a[k] < ((int64_t)1 << 41), "below 2^41", k, 0, 0, 0);
    }
    std::printf("gauge_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
