// propose_check.cpp -- csrc/leon_propose.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_propose_walk_native.py).  Three texts give the rows of a request and must agree word for word:
//   * the library's host text (propose_request_host: the hot predicate, a flood fill with a stack, the box, the filler);
//   * a brute-force fill written here that shares nothing with it: labels spread to neighbours until nothing changes;
//   * k_propose's steps taken one thread after the other over an LDS image allocated at exactly propose_lds().bytes -- the masks by
//     64-cell ballots, propose_run_start, union by smallest index on 16-bit labels, the counts in the roots' slots, the rows and the
//     packed extents -- so that an index past any part of the image is a heap overflow the sanitizer reports.
// Every mask of the 3 x 3 and the 4 x 4 grid (512 and 65536 masks), both connectivities, from records allocated at exactly
// record_bytes; then frames smaller than their grid, K and min_cells around the counts, and the largest grid.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_propose.h"

using namespace leon;

static int failed = 0;

static void check(bool ok, const char* what, int a, int b, int c, int d)
{
    if (ok) return;
    if (failed++ < 10) std::printf("FAILED %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
}

struct Records {
    uint8_t *motion, *activity;          // malloc'ed at exactly record_bytes each
    MotionLayout ml;
    ActivityLayout al;
};
static Records make(int mbw, int mbh)
{
    Records r;
    r.ml = motion_layout((uint32_t)mbw, (uint32_t)mbh);
    r.al = activity_layout((uint32_t)mbw, (uint32_t)mbh);
    r.motion = static_cast<uint8_t*>(std::calloc(r.ml.record_bytes, 1));
    r.activity = static_cast<uint8_t*>(std::calloc(r.al.record_bytes, 1));
    return r;
}
static void drop(Records& r) { std::free(r.motion); std::free(r.activity); }
static void put(Records& r, size_t mb, uint32_t ac_mag, uint32_t info, uint32_t fwd, uint32_t bwd)
{
    const uint32_t lo = (ac_mag << 16) | 0x1234u, hi = 0x1f3f0777u;
    std::memcpy(r.activity + 8 * mb, &lo, 4);
    std::memcpy(r.activity + 8 * mb + 4, &hi, 4);
    std::memcpy(r.motion + 8 * mb, &fwd, 4);
    std::memcpy(r.motion + 8 * mb + 4, &bwd, 4);
    r.motion[r.ml.info_offset + mb] = (uint8_t)info;
}

struct Rows {
    std::vector<int32_t> regions, info;
    int32_t count;
    bool operator==(const Rows& o) const { return regions == o.regions && info == o.info && count == o.count; }
};

static bool hot_of(const Records& r, const ProposeConfig& c, int fw, int fh, int mbw, int k)
{
    uint32_t lo = 0, f = 0, b = 0, nf = 0;
    if (c.sources & kProposeActivity) std::memcpy(&lo, r.activity + 8 * (size_t)k, 4);
    if (c.sources & kProposeMotion) {
        std::memcpy(&f, r.motion + 8 * (size_t)k, 4);
        std::memcpy(&b, r.motion + 8 * (size_t)k + 4, 4);
        nf = r.motion[r.ml.info_offset + (size_t)k];
    }
    return propose_hot(c, fw, fh, k % mbw, k / mbw, lo, nf, f, b);
}

static Rows by_library(const Records& r, const ProposeConfig& c, int fw, int fh, int mbw, int mbh, int frame)
{
    Rows o{std::vector<int32_t>((size_t)c.max_boxes * 8, -9), std::vector<int32_t>((size_t)c.max_boxes * 2, -9), -9};
    propose_request_host(c, fw, fh, mbw, mbh, (c.sources & kProposeMotion) ? r.motion : nullptr, (c.sources & kProposeActivity) ? r.activity : nullptr, frame, o.regions.data(),
                         o.info.data(), &o.count);
    return o;
}

// labels spread until nothing changes; then the components in the order of their label, which is their smallest cell
static Rows by_brute_force(const Records& r, const ProposeConfig& c, int fw, int fh, int mbw, int mbh, int frame)
{
    const int mbs = mbw * mbh;
    std::vector<int> lab((size_t)mbs, -1);
    for (int k = 0; k < mbs; k++)
        if (hot_of(r, c, fw, fh, mbw, k)) lab[(size_t)k] = k;
    for (bool changed = true; changed;) {
        changed = false;
        for (int k = 0; k < mbs; k++) {
            if (lab[(size_t)k] < 0) continue;
            for (int dj = -1; dj <= 1; dj++)
                for (int di = -1; di <= 1; di++) {
                    const int i = k % mbw + di, j = k / mbw + dj;
                    if (i < 0 || i >= mbw || j < 0 || j >= mbh || (c.connectivity != 8 && di * dj != 0)) continue;
                    const int q = lab[(size_t)(j * mbw + i)];
                    if (q >= 0 && q < lab[(size_t)k]) { lab[(size_t)k] = q; changed = true; }
                }
        }
    }
    Rows o{std::vector<int32_t>((size_t)c.max_boxes * 8, 0), std::vector<int32_t>((size_t)c.max_boxes * 2, 0), 0};
    for (int k = 0; k < c.max_boxes; k++) { o.regions[8 * (size_t)k] = frame; o.info[2 * (size_t)k + 1] = -1; }
    for (int first = 0; first < mbs; first++) {
        if (lab[(size_t)first] != first) continue;
        int cells = 0, i0 = mbw, i1 = -1, j0 = mbh, j1 = -1;
        for (int k = 0; k < mbs; k++)
            if (lab[(size_t)k] == first) {
                cells++;
                i0 = std::min(i0, k % mbw); i1 = std::max(i1, k % mbw); j0 = std::min(j0, k / mbw); j1 = std::max(j1, k / mbw);
            }
        if (cells < c.min_cells) continue;
        if (o.count < c.max_boxes) {
            int32_t* b = &o.regions[8 * (size_t)o.count];
            b[1] = 16 * i0; b[2] = 16 * j0;
            b[3] = std::min(16 * (i1 + 1), fw) - b[1];
            b[4] = std::min(16 * (j1 + 1), fh) - b[2];
            o.info[2 * (size_t)o.count] = cells; o.info[2 * (size_t)o.count + 1] = first;
        }
        o.count++;
    }
    return o;
}

// ---- k_propose's steps, one thread after the other: the same functions of leon_propose.h on the same indices
static uint32_t get(const uint32_t* lab, uint32_t c) { return (lab[c >> 1] >> ((c & 1u) << 4)) & 0xffffu; }
static void set(uint32_t* lab, uint32_t c, uint32_t v) { lab[c >> 1] = (lab[c >> 1] & ~(0xffffu << ((c & 1u) << 4))) | ((v & 0xffffu) << ((c & 1u) << 4)); }
static uint32_t find(const uint32_t* lab, uint32_t c)
{
    for (uint32_t l = get(lab, c); l != c; l = get(lab, c)) c = l;
    return c;
}
static void unite(uint32_t* lab, uint32_t a, uint32_t b)
{
    a = find(lab, a); b = find(lab, b);
    if (a == b) return;
    if (a < b) std::swap(a, b);
    set(lab, a, b);
}
static void ballot(uint32_t* mask, uint32_t base, const std::vector<bool>& lanes)
{
    uint64_t b = 0;
    for (int l = 0; l < 64; l++) b |= (uint64_t)lanes[(size_t)l] << l;
    mask[base >> 5] = (uint32_t)b;
    mask[(base >> 5) + 1u] = (uint32_t)(b >> 32);
}
static Rows by_kernel_steps(const Records& r, const ProposeConfig& c, int fw, int fh, int mbw_, int mbh, int frame)
{
    const uint32_t mbw = (uint32_t)mbw_, mbs = mbw * (uint32_t)mbh, K = (uint32_t)c.max_boxes, T = kProposeThreads;
    const ProposeLds L = propose_lds(mbs, K);
    uint32_t* const lds = static_cast<uint32_t*>(std::malloc(L.bytes));          // not initialised, as LDS is not
    std::memset(lds, 0xa5, L.bytes);
    uint32_t *lab = lds, *hot = lds + L.hot, *root = lds + L.root, *rows = lds + L.rows, *scan = lds + L.scan;
    const uint32_t padded = 32u * L.mask_words;
    std::vector<bool> lanes(64);
    for (uint32_t base = 0; base < padded; base += 64) {                                                           // 1
        for (uint32_t l = 0; l < 64; l++) lanes[l] = base + l < mbs && hot_of(r, c, fw, fh, mbw_, (int)(base + l));
        ballot(hot, base, lanes);
    }
    for (uint32_t k = 0; k < mbs; k++)                                                                             // 2
        if (propose_bit(hot, k)) set(lab, k, propose_run_start(hot, k, k - k % mbw));
    for (uint32_t k = mbw; k < mbs; k++) {                                                                         // 3
        if (!propose_bit(hot, k)) continue;
        const uint32_t i = k % mbw, up = k - mbw;
        const bool left = i > 0u && propose_bit(hot, k - 1u);
        if (propose_bit(hot, up)) {
            if (!(left && propose_bit(hot, up - 1u))) unite(lab, k, up);
        } else if (c.connectivity == 8) {
            if (i > 0u && !left && propose_bit(hot, up - 1u)) unite(lab, k, up - 1u);
            if (i + 1u < mbw && !propose_bit(hot, k + 1u) && propose_bit(hot, up + 1u)) unite(lab, k, up + 1u);
        }
    }
    for (uint32_t k = 0; k < mbs; k++)                                                                             // 4
        if (propose_bit(hot, k)) set(lab, k, find(lab, k));
    for (uint32_t base = 0; base < padded; base += 64) {                                                           // 5
        for (uint32_t l = 0; l < 64; l++) lanes[l] = base + l < mbs && propose_bit(hot, base + l) && get(lab, base + l) == base + l;
        ballot(root, base, lanes);
        for (uint32_t l = 0; l < 64; l++)
            if (lanes[l]) set(lab, base + l, 0u);
    }
    for (uint32_t k = 0; k < mbs; k++)                                                                             // 6
        if (propose_bit(hot, k) && !propose_bit(root, k)) {
            const uint32_t at = get(lab, k);
            lab[at >> 1] += 1u << ((at & 1u) << 4);
        }
    const uint32_t per = (L.mask_words + T - 1u) / T, least = (uint32_t)c.min_cells;                                // 7
    std::vector<uint32_t> sum(T, 0u);
    for (uint32_t t = 0; t < T; t++)
        for (uint32_t w = std::min(t * per, L.mask_words); w < std::min(std::min(t * per, L.mask_words) + per, L.mask_words); w++)
            for (uint32_t m = root[w]; m; m &= m - 1u) sum[t] += get(lab, (w << 5) + (uint32_t)__builtin_ctz(m)) + 1u >= least ? 1u : 0u;
    for (uint32_t wv = 0; wv < T / 64u; wv++) {
        scan[wv] = 0u;
        for (uint32_t l = 0; l < 64; l++) scan[wv] += sum[64u * wv + l];
    }
    uint32_t total = 0u;                                                                                           // 8
    for (uint32_t wv = 0; wv < T / 64u; wv++) total += scan[wv];
    uint32_t run = 0u;
    for (uint32_t t = 0; t < T; t++)
        for (uint32_t w = std::min(t * per, L.mask_words); w < std::min(std::min(t * per, L.mask_words) + per, L.mask_words); w++)
            for (uint32_t m = root[w]; m; m &= m - 1u) {
                const uint32_t at = (w << 5) + (uint32_t)__builtin_ctz(m), less = get(lab, at);
                uint32_t row = 0xffffu;
                if (less + 1u >= least) {
                    if (run < K) {
                        row = run;
                        rows[2u * row] = at | (less << 16);
                        rows[2u * row + 1u] = propose_extent(at % mbw, at / mbw);
                    }
                    run++;
                }
                set(lab, at, row);
            }
    check(run == total, "the scan's total", (int)run, (int)total, 0, 0);
    for (uint32_t k = 0; k < mbs; k++)                                                                             // 9
        if (propose_bit(hot, k) && !propose_bit(root, k)) {
            const uint32_t row = get(lab, get(lab, k));
            if (row != 0xffffu) rows[2u * row + 1u] = propose_extent_join(rows[2u * row + 1u], propose_extent(k % mbw, k / mbw));
        }
    Rows o{std::vector<int32_t>((size_t)K * 8, -9), std::vector<int32_t>((size_t)K * 2, -9), (int32_t)total};        // 10
    for (uint32_t k = 0; k < K; k++) {
        if (k < std::min(total, K)) {
            const uint32_t a = rows[2u * k], e = rows[2u * k + 1u], first = a & 0xffffu;
            propose_box(frame, fw, fh, (int32_t)(255u - (e & 255u)), (int32_t)((e >> 8) & 255u), (int32_t)(first / mbw), (int32_t)((e >> 16) & 255u), &o.regions[8 * (size_t)k]);
            o.info[2 * (size_t)k] = (int32_t)(a >> 16) + 1;
            o.info[2 * (size_t)k + 1] = (int32_t)first;
        } else {
            propose_filler(frame, &o.regions[8 * (size_t)k], &o.info[2 * (size_t)k]);
        }
    }
    std::free(lds);
    return o;
}

static void all_three(const Records& r, const ProposeConfig& c, int fw, int fh, int mbw, int mbh, const char* what, int a, bool brute = true)
{
    const Rows lib = by_library(r, c, fw, fh, mbw, mbh, 3), steps = by_kernel_steps(r, c, fw, fh, mbw, mbh, 3);
    check(lib == steps, what, a, c.connectivity, lib.count, steps.count);
    if (brute) check(lib == by_brute_force(r, c, fw, fh, mbw, mbh, 3), "the library against the brute-force fill", a, c.connectivity, lib.count, c.min_cells);
}

int main()
{
    // every mask of 3 x 3 and 4 x 4, both connectivities: bit k of the mask's number is raster cell k, hot by the activity record at
    // exactly the threshold (a cold cell one below it), K = 5 so that the fullest masks overflow it
    for (int side = 3; side <= 4; side++) {
        Records r = make(side, side);
        long masks = 0;
        for (uint32_t m = 0; m < (1u << (side * side)); m++, masks++) {
            for (int k = 0; k < side * side; k++) put(r, (size_t)k, (m >> k) & 1u ? 300u : 299u, 1u, 0u, 0u);
            for (int conn = 4; conn <= 8; conn += 4) {
                const ProposeConfig c{kProposeActivity, 0, 0, 300, conn, 1, 5, 0};
                all_three(r, c, 16 * side, 16 * side, side, side, "every mask: the library against the kernel's steps", (int)m);
            }
        }
        std::printf("%ld masks of %d x %d\n", masks, side, side);
        drop(r);
    }
    // the motion source: a word of -32768 at threshold 32768, the intra flag, both sources; frames smaller than their grids (61 x 45
    // and 33 x 17 in 4 x 3: a column and a row wholly outside); K and min_cells around the counts
    {
        const int mbw = 4, mbh = 3;
        Records r = make(mbw, mbh);
        uint32_t seed = 99;
        for (int round = 0; round < 200; round++) {
            for (int k = 0; k < mbw * mbh; k++) {
                seed = seed * 1664525u + 1013904223u;
                const uint32_t kind = (seed >> 28) & 7u;
                put(r, (size_t)k, (seed >> 8) & 1u ? 65535u : 7u, kind == 0 ? 4u : 1u, kind == 1 ? 0x00008000u : kind == 2 ? 0x7fff0000u : 3u, kind == 3 ? 0x80000001u : 0u);
            }
            for (int conn = 4; conn <= 8; conn += 4)
                for (int K = 1; K <= 7; K += 2)
                    for (int least = 1; least <= 4; least++) {
                        all_three(r, ProposeConfig{kProposeMotion, 0, 32768, 0, conn, least, K, 0}, 61, 45, mbw, mbh, "motion at 32768", round);
                        all_three(r, ProposeConfig{kProposeMotion, kProposeIntra, 32767, 0, conn, least, K, 0}, 33, 17, mbw, mbh, "motion and intra", round);
                        all_three(r, ProposeConfig{kProposeMotion | kProposeActivity, kProposeIntra, 4, 65535, conn, least, K, 0}, 64, 48, mbw, mbh, "both sources", round);
                    }
        }
        const ProposeConfig c{kProposeMotion | kProposeActivity, 0, 1, 1, 8, 1, 4, 0};
        const Rows o = by_library(r, c, 33, 17, mbw, mbh, 3);          // everything hot: one component of the 3 x 2 cells inside the frame
        check(o.count == 1 && o.info[0] == 6 && o.regions[3] == 33 && o.regions[4] == 17 && o.regions[8 + 3] == 0 && o.info[3] == -1, "33 x 17 in 4 x 3", o.count, o.info[0], 0, 0);
        drop(r);
    }
    // a grid whose rows do not end on a word of the masks (22 wide), seeded masks at several densities; and 120 x 68
    for (int shape = 0; shape < 2; shape++) {
        const int mbw = shape ? 120 : 22, mbh = shape ? 68 : 15;
        Records r = make(mbw, mbh);
        uint32_t seed = 7;
        for (int round = 0; round < (shape ? 6 : 60); round++) {
            for (int k = 0; k < mbw * mbh; k++) {
                seed = seed * 1664525u + 1013904223u;
                put(r, (size_t)k, (seed >> 16) % 10u < (uint32_t)(1 + round % 9) ? 300u : 0u, 1u, 0u, 0u);
            }
            for (int conn = 4; conn <= 8; conn += 4)
                all_three(r, ProposeConfig{kProposeActivity, 0, 0, 300, conn, 1 + round % 3, 16, 0}, 16 * mbw - 5, 16 * mbh - 9, mbw, mbh, "seeded masks", round, !shape);
        }
        drop(r);
    }
    // the largest grid: everything hot (one component of 65536 cells, which 16 bits hold as 65535 + 1), a checkerboard (32768
    // components under 4, K = 1024), every other row (128 components of 256)
    {
        const int mb = 256;
        Records r = make(mb, mb);
        for (int pattern = 0; pattern < 3; pattern++) {
            for (int k = 0; k < mb * mb; k++) {
                const bool on = pattern == 0 || (pattern == 1 ? (k % mb + k / mb) % 2 == 0 : (k / mb) % 2 == 0);
                put(r, (size_t)k, 0u, 1u, on ? 0x80008000u : 0u, 0u);
            }
            for (int conn = 4; conn <= 8; conn += 4) {
                const ProposeConfig c{kProposeMotion, 0, 32768, 0, conn, 1, 1024, 0};
                all_three(r, c, 4096, 4096, mb, mb, "the largest grid", pattern, false);
                const Rows o = by_library(r, c, 4096, 4096, mb, mb, 3);
                const int want = pattern == 0 ? 1 : pattern == 1 ? (conn == 4 ? 32768 : 1) : 128;
                check(o.count == want, "the largest grid's count", pattern, conn, o.count, want);
                if (pattern == 0) check(o.info[0] == 65536 && o.info[1] == 0 && o.regions[3] == 4096 && o.regions[4] == 4096, "65536 cells", o.info[0], 0, 0, 0);
            }
        }
        const ProposeConfig big{kProposeMotion, 0, 32768, 0, 4, 65536, 2, 0};          // (the rows pattern: no component has 65536 cells)
        check(by_kernel_steps(r, big, 4096, 4096, mb, mb, 3).count == 0, "min_cells 65536", 0, 0, 0, 0);
        drop(r);
    }
    // the request's judgement
    check(propose_request_status(0, 1) == kRegionOk && propose_request_status(1, 1) == kRegionFrame && propose_request_status(-1, 5) == kRegionFrame &&
          propose_request_status(2147483647, 2147483647) == kRegionFrame && propose_request_status(0, 0) == kRegionFrame, "status", 0, 0, 0, 0);
    static_assert(propose_lds(65536, 1024).bytes == 155680, "the LDS the header states");
    std::printf("propose_check: %d failed\n", failed);
    return failed ? 1 : 0;
}
