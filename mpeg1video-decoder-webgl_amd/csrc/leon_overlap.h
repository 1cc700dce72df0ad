// leon_overlap.h -- boxes compared with each other by overlap: greedy suppression inside a set and greedy one-to-one matching of two
// sets (the definitions of include/leon_pipeline.h, leon_pipeline_suppress_regions and leon_pipeline_match_regions), for the host
// (suppress_set_host, match_set_host at the end of this file) and the device (k_suppress, k_match, in this file as well): ONE text for
// the judgement of a row (the gauge family's), the overlap of two boxes, the threshold and the exact comparison of two overlaps.
// Integers only, everything the definitions form in int64.  The kernels are written as STEPS: each step is a function of (tid,
// threads) that a thread of the workgroup runs between two barriers over the workgroup's LDS; the kernels below call them with a
// barrier between each two, and a stand-alone program can take the same steps one thread after another over an LDS image of exactly
// suppress_lds / match_lds bytes.  The host texts share none of the steps: a stable sort and a walk.
#ifndef LEON_OVERLAP_H
#define LEON_OVERLAP_H
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "leon_gauge.h"

namespace leon {

enum { kOverlapIou = 0, kOverlapIomin = 1 };             // cfg.measure
enum { kOverlapMaxRows = 1024, kOverlapMaxThreshold = 65536, kOverlapMaxStride = 8, kOverlapMaxFrame = 4096 };
enum { kOverlapThreads = 256 };                          // both kernels' workgroup: 4 waves
enum { kMatchFree = -1, kMatchRefused = -2, kMatchUnsought = -3 };     // what a row's match / best word holds in LDS besides a partner

struct OverlapConfig {                   // = leon_pipeline_overlap_config
    int32_t measure, threshold, reserved[2];
};
struct OverlapBox {                      // a row's box in LDS
    int32_t x, y, w, h;
};
struct OverlapTerms {                    // inter <= 2^24, den <= 2^25
    int64_t inter, den;
};
// what a launch hands its kernel
struct OverlapCall {
    int32_t measure, threshold;
    int32_t fw, fh, n_frames;
    int32_t n, ka, kb;                   // sets; rows of a set (suppress: ka alone)
    int32_t score_stride, reserved;
};

// a row as k_gauge judges it: the reserved words, the frame, the box
LEON_HD inline int32_t overlap_row_status(const int32_t* r, int32_t fw, int32_t fh, int32_t n_frames)
{
    return gauge_record_status(GaugeRecord{r[0], r[1], r[2], r[3], r[4], {r[5], r[6], r[7]}}, fw, fh, n_frames);
}

LEON_HD inline OverlapTerms overlap_terms(int32_t measure, const OverlapBox& a, const OverlapBox& b)
{
    const int32_t x0 = a.x > b.x ? a.x : b.x, x1 = a.x + a.w < b.x + b.w ? a.x + a.w : b.x + b.w;
    const int32_t y0 = a.y > b.y ? a.y : b.y, y1 = a.y + a.h < b.y + b.h ? a.y + a.h : b.y + b.h;
    const int32_t iw = x1 - x0 > 0 ? x1 - x0 : 0, ih = y1 - y0 > 0 ? y1 - y0 : 0;
    const int64_t inter = (int64_t)iw * ih, aa = (int64_t)a.w * a.h, bb = (int64_t)b.w * b.h;
    return OverlapTerms{inter, measure == kOverlapIomin ? (aa < bb ? aa : bb) : aa + bb - inter};
}
// do the two boxes share a pixel at all: where they do not, inter is 0 and the pair reaches no threshold (which is 1 at the least) --
// four compares that spare the walks the 64-bit terms of most pairs
LEON_HD inline bool overlap_meets(const OverlapBox& a, const OverlapBox& b) { return a.x < b.x + b.w && b.x < a.x + a.w && a.y < b.y + b.h && b.y < a.y + a.h; }
LEON_HD inline bool overlap_reaches(int32_t threshold, const OverlapTerms& t) { return t.inter * 65536 >= (int64_t)threshold * t.den; }
// is a's overlap larger than b's: inter_a / den_a > inter_b / den_b, exactly (products below 2^50)
LEON_HD inline bool overlap_above(const OverlapTerms& a, const OverlapTerms& b) { return a.inter * b.den > b.inter * a.den; }
LEON_HD inline int32_t overlap_q16(const OverlapTerms& t) { return (int32_t)((uint64_t)(t.inter * 65536) / (uint64_t)t.den); }

// the key rows are sorted by, ascending: the score descending, then the row index ascending; below every key a refused row or the
// padding holds (all ones)
LEON_HD inline uint64_t suppress_key(int32_t score, uint32_t row) { return ((uint64_t)~((uint32_t)score ^ 0x80000000u) << 32) | row; }
#define LEON_SUPPRESS_NO_KEY (~(uint64_t)0)

// ---- what k_suppress keeps in LDS for one set of K rows: [boxes | keys | by | order], every part a whole number of dwords.  boxes: 16
// bytes a row; keys: 8 bytes for each of `sorted` slots, K rounded up to a power of two (the sort is bitonic); by: a dword a RANK (-1:
// kept so far, else the row that cleared it); order: a dword a kept row, its input index.  24 K + 8 sorted bytes: 32768 at K = 1024.
struct SuppressLds {
    uint32_t sorted;                     // key slots
    uint32_t keys, by, order;            // dword offsets of the parts behind the boxes (which start at 0)
    uint32_t bytes;
};
LEON_HD constexpr SuppressLds suppress_lds(uint32_t K)
{
    SuppressLds L{};
    L.sorted = 1u;
    while (L.sorted < K) L.sorted <<= 1;
    L.keys = 4u * K;
    L.by = L.keys + 2u * L.sorted;
    L.order = L.by + K;
    L.bytes = 4u * (L.order + K);
    return L;
}
// ---- ... and k_match for a pair of sets of Ka and Kb rows: [boxes A | boxes B | match A | match B | best A | best B | pairs].  match:
// the partner taken, kMatchFree or kMatchRefused; best: the best free partner found, kMatchFree for none (for good: the free rows only
// get fewer) or kMatchUnsought; pairs: one dword.  24 (Ka + Kb) + 4 bytes: 49156 at 1024 and 1024.
struct MatchLds {
    uint32_t box_b, match_a, match_b, best_a, best_b, pairs;       // dword offsets behind the boxes of A (which start at 0)
    uint32_t bytes;
};
LEON_HD constexpr MatchLds match_lds(uint32_t Ka, uint32_t Kb)
{
    MatchLds L{};
    L.box_b = 4u * Ka;
    L.match_a = L.box_b + 4u * Kb;
    L.match_b = L.match_a + Ka;
    L.best_a = L.match_b + Kb;
    L.best_b = L.best_a + Ka;
    L.pairs = L.best_b + Kb;
    L.bytes = 4u * (L.pairs + 1u);
    return L;
}

// ---- the steps of k_suppress.  rows, scores, status: the set's own (scores and status may be null) ---------------------------------
// 1  a thread a key slot: the row judged, its status out, its box and key into LDS; a refused row and the padding get no key
LEON_HD inline void suppress_step_load(uint32_t* lds, const SuppressLds& L, const OverlapCall& c, uint32_t tid, uint32_t threads, const int32_t* rows, const int32_t* scores,
                                       int32_t* status)
{
    const uint32_t K = (uint32_t)c.ka;
    OverlapBox* const box = reinterpret_cast<OverlapBox*>(lds);
    uint64_t* const keys = reinterpret_cast<uint64_t*>(lds + L.keys);
    int32_t* const by = reinterpret_cast<int32_t*>(lds + L.by);
    for (uint32_t i = tid; i < L.sorted; i += threads) {
        uint64_t key = LEON_SUPPRESS_NO_KEY;
        if (i < K) {
            const int32_t* r = rows + 8u * (size_t)i;
            const int32_t st = overlap_row_status(r, c.fw, c.fh, c.n_frames);
            if (status) status[i] = st;
            if (st == kRegionOk) {
                box[i] = OverlapBox{r[1], r[2], r[3], r[4]};
                key = suppress_key(scores ? scores[(size_t)i * (uint32_t)c.score_stride] : 0, i);
            }
            by[i] = -1;
        }
        keys[i] = key;
    }
}
// 2  one compare-and-exchange pass of the bitonic sort: block k, distance j; a thread a pair
LEON_HD inline void suppress_step_sort(uint32_t* lds, const SuppressLds& L, uint32_t k, uint32_t j, uint32_t tid, uint32_t threads)
{
    uint64_t* const keys = reinterpret_cast<uint64_t*>(lds + L.keys);
    for (uint32_t p = tid; p < L.sorted / 2u; p += threads) {
        const uint32_t lo = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), hi = lo | j;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0u)) { keys[lo] = b; keys[hi] = a; }
    }
}
// the accepted rows: the keys in front of the first slot without one (the same answer in every thread)
LEON_HD inline uint32_t suppress_accepted(const uint32_t* lds, const SuppressLds& L)
{
    const uint64_t* const keys = reinterpret_cast<const uint64_t*>(lds + L.keys);
    uint32_t lo = 0, hi = L.sorted;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] == LEON_SUPPRESS_NO_KEY) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
// 3  rank r of the walk, behind a barrier: is it still kept (the same answer in every thread)?  Then it is kept for good -- thread 0
//    notes it as kept row `kept` -- and clears every later rank that is kept so far and reaches the threshold with it.  A thread owns
//    the ranks tid, tid + threads, ..: by[t] is written by its owner alone and read by all only as by[r] behind the next barrier.
LEON_HD inline bool suppress_step_walk(uint32_t* lds, const SuppressLds& L, const OverlapCall& c, uint32_t r, uint32_t m, uint32_t kept, uint32_t tid, uint32_t threads)
{
    const OverlapBox* const box = reinterpret_cast<const OverlapBox*>(lds);
    const uint64_t* const keys = reinterpret_cast<const uint64_t*>(lds + L.keys);
    int32_t* const by = reinterpret_cast<int32_t*>(lds + L.by);
    if (by[r] != -1) return false;
    const uint32_t row = (uint32_t)keys[r];
    const OverlapBox a = box[row];
    if (tid == 0) lds[L.order + kept] = row;
    for (uint32_t t = (r + 1u) + (tid + threads - (r + 1u) % threads) % threads; t < m; t += threads)
        if (by[t] == -1) {
            const OverlapBox b = box[(uint32_t)keys[t]];
            if (overlap_meets(a, b) && overlap_reaches(c.threshold, overlap_terms(c.measure, a, b))) by[t] = (int32_t)row;
        }
    return true;
}
// 4  the outputs of the set: by for the m accepted rows, every row of out (may be null) and order (may be null), the count
LEON_HD inline void suppress_step_store(const uint32_t* lds, const SuppressLds& L, const OverlapCall& c, uint32_t m, uint32_t kept, uint32_t tid, uint32_t threads,
                                        const int32_t* rows, int32_t* out, int32_t* order, int32_t* by_out, int32_t* count)
{
    const uint32_t K = (uint32_t)c.ka;
    const OverlapBox* const box = reinterpret_cast<const OverlapBox*>(lds);
    const uint64_t* const keys = reinterpret_cast<const uint64_t*>(lds + L.keys);
    for (uint32_t r = tid; r < m; r += threads) by_out[(uint32_t)keys[r]] = (int32_t)lds[L.by + r];
    for (uint32_t k = tid; k < K; k += threads) {
        const bool used = k < kept;
        const uint32_t row = used ? lds[L.order + k] : 0u;
        if (out) {
            int32_t* const o = out + 8u * (size_t)k;
            const OverlapBox b = used ? box[row] : OverlapBox{0, 0, 0, 0};
            o[0] = used ? rows[8u * (size_t)row] : 0;
            o[1] = b.x; o[2] = b.y; o[3] = b.w; o[4] = b.h;
            o[5] = 0; o[6] = 0; o[7] = 0;
        }
        if (order) order[k] = used ? (int32_t)row : -1;
    }
    if (tid == 0) *count = (int32_t)kept;
}

// ---- the steps of k_match.  a, b: the pair's sets; status_a, status_b may be null ----------------------------------------------------
// 1  a thread a row of either set: judged, its status out, its box into LDS, free and unsought -- or refused
LEON_HD inline void match_step_load(uint32_t* lds, const MatchLds& L, const OverlapCall& c, uint32_t tid, uint32_t threads, const int32_t* a, const int32_t* b,
                                    int32_t* status_a, int32_t* status_b)
{
    for (int side = 0; side < 2; side++) {
        const uint32_t K = (uint32_t)(side ? c.kb : c.ka);
        const int32_t* const rows = side ? b : a;
        int32_t* const status = side ? status_b : status_a;
        OverlapBox* const box = reinterpret_cast<OverlapBox*>(lds + (side ? L.box_b : 0u));
        int32_t* const match = reinterpret_cast<int32_t*>(lds + (side ? L.match_b : L.match_a));
        int32_t* const best = reinterpret_cast<int32_t*>(lds + (side ? L.best_b : L.best_a));
        for (uint32_t i = tid; i < K; i += threads) {
            const int32_t* r = rows + 8u * (size_t)i;
            const int32_t st = overlap_row_status(r, c.fw, c.fh, c.n_frames);
            if (status) status[i] = st;
            if (st == kRegionOk) box[i] = OverlapBox{r[1], r[2], r[3], r[4]};
            match[i] = st == kRegionOk ? kMatchFree : kMatchRefused;
            best[i] = kMatchUnsought;
        }
    }
    if (tid == 0) lds[L.pairs] = 0u;
}
// 2  every free row of either set whose best partner is unsought or was taken looks for its best free partner in the other set: the
//    largest overlap that reaches the threshold, the smallest index among equals (the rows are walked upwards and only a LARGER overlap
//    replaces).  The match words are only read here, the best words written by their rows' owners alone.
LEON_HD inline void match_step_seek(uint32_t* lds, const MatchLds& L, const OverlapCall& c, uint32_t tid, uint32_t threads)
{
    for (int side = 0; side < 2; side++) {
        const uint32_t K = (uint32_t)(side ? c.kb : c.ka), Ko = (uint32_t)(side ? c.ka : c.kb);
        const OverlapBox* const box = reinterpret_cast<const OverlapBox*>(lds + (side ? L.box_b : 0u));
        const OverlapBox* const other = reinterpret_cast<const OverlapBox*>(lds + (side ? 0u : L.box_b));
        const int32_t* const match = reinterpret_cast<const int32_t*>(lds + (side ? L.match_b : L.match_a));
        const int32_t* const taken = reinterpret_cast<const int32_t*>(lds + (side ? L.match_a : L.match_b));
        int32_t* const best = reinterpret_cast<int32_t*>(lds + (side ? L.best_b : L.best_a));
        for (uint32_t i = tid; i < K; i += threads) {
            if (match[i] != kMatchFree) continue;
            const int32_t had = best[i];
            if (had == kMatchFree || (had >= 0 && taken[had] == kMatchFree)) continue;
            const OverlapBox mine = box[i];
            int32_t found = kMatchFree;
            OverlapTerms ft{0, 1};
            for (uint32_t j = 0; j < Ko; j++) {
                if (taken[j] != kMatchFree) continue;
                const OverlapBox its = other[j];
                if (!overlap_meets(mine, its)) continue;
                const OverlapTerms t = side ? overlap_terms(c.measure, its, mine) : overlap_terms(c.measure, mine, its);
                if (!overlap_reaches(c.threshold, t)) continue;
                if (found < 0 || overlap_above(t, ft)) { found = (int32_t)j; ft = t; }
            }
            best[i] = found;
        }
    }
}
// 3  a free row of A and its best partner that names it back are a pair: taken, the overlap out, the pairs this thread took added to
//    the pair's count in LDS.  Behind the next barrier match_pairs() tells every thread whether the round took one: where none did
//    there is no candidate left among the free rows (the largest one is always mutual).  Only a pair's own two match words are
//    written, and no thread reads another's here.
LEON_HD inline void match_step_take(uint32_t* lds, const MatchLds& L, const OverlapCall& c, uint32_t tid, uint32_t threads, int32_t* overlap)
{
    const OverlapBox* const box_a = reinterpret_cast<const OverlapBox*>(lds);
    const OverlapBox* const box_b = reinterpret_cast<const OverlapBox*>(lds + L.box_b);
    int32_t* const match_a = reinterpret_cast<int32_t*>(lds + L.match_a);
    int32_t* const match_b = reinterpret_cast<int32_t*>(lds + L.match_b);
    const int32_t* const best_a = reinterpret_cast<const int32_t*>(lds + L.best_a);
    const int32_t* const best_b = reinterpret_cast<const int32_t*>(lds + L.best_b);
    uint32_t took = 0;
    for (uint32_t i = tid; i < (uint32_t)c.ka; i += threads) {
        if (match_a[i] != kMatchFree) continue;
        const int32_t j = best_a[i];
        if (j < 0 || best_b[j] != (int32_t)i) continue;
        match_a[i] = j;
        match_b[j] = (int32_t)i;
        overlap[i] = overlap_q16(overlap_terms(c.measure, box_a[i], box_b[j]));
        took++;
    }
    if (took) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(lds + L.pairs, took);
#else
        lds[L.pairs] += took;
#endif
    }
}
LEON_HD inline uint32_t match_pairs(const uint32_t* lds, const MatchLds& L) { return lds[L.pairs]; }
// 4  the outputs of the pair: the match words of the rows that are not refused, 0 as the overlap of a row left free, the count
LEON_HD inline void match_step_store(const uint32_t* lds, const MatchLds& L, const OverlapCall& c, uint32_t tid, uint32_t threads, int32_t* match_a, int32_t* match_b,
                                     int32_t* overlap, int32_t* count)
{
    for (uint32_t i = tid; i < (uint32_t)c.ka; i += threads) {
        const int32_t m = (int32_t)lds[L.match_a + i];
        if (m == kMatchRefused) continue;
        match_a[i] = m;
        if (m == kMatchFree) overlap[i] = 0;
    }
    for (uint32_t j = tid; j < (uint32_t)c.kb; j += threads) {
        const int32_t m = (int32_t)lds[L.match_b + j];
        if (m != kMatchRefused) match_b[j] = m;
    }
    if (tid == 0) *count = (int32_t)lds[L.pairs];
}

#if defined(__HIPCC__)
// ---- the kernels: a workgroup a set (a pair of sets), the steps above with a barrier between each two.  Every LDS index is below
// suppress_lds(ka) / match_lds(ka, kb), which the launch passes as dynamic LDS; every global index is below the set's own K rows.
__global__ __launch_bounds__(kOverlapThreads) void k_suppress(const int32_t* __restrict__ rows, const int32_t* __restrict__ scores, int32_t* __restrict__ out,
                                                              int32_t* __restrict__ order, int32_t* __restrict__ by, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ status, OverlapCall c)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_suppress[];
    const uint32_t tid = threadIdx.x, K = (uint32_t)c.ka;
    const size_t set = blockIdx.x, first = set * K;
    const SuppressLds L = suppress_lds(K);
    const int32_t* const my_rows = rows + first * 8u;
    suppress_step_load(s_suppress, L, c, tid, kOverlapThreads, my_rows, scores ? scores + first * (uint32_t)c.score_stride : nullptr, status ? status + first : nullptr);
    __syncthreads();
    for (uint32_t k = 2u; k <= L.sorted; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            suppress_step_sort(s_suppress, L, k, j, tid, kOverlapThreads);
            __syncthreads();
        }
    const uint32_t m = suppress_accepted(s_suppress, L);
    uint32_t kept = 0;
    for (uint32_t r = 0; r < m; r++) {
        if (r) __syncthreads();
        kept += suppress_step_walk(s_suppress, L, c, r, m, kept, tid, kOverlapThreads) ? 1u : 0u;
    }
    __syncthreads();
    suppress_step_store(s_suppress, L, c, m, kept, tid, kOverlapThreads, my_rows, out ? out + first * 8u : nullptr, order ? order + first : nullptr, by + first, count + set);
}

__global__ __launch_bounds__(kOverlapThreads) void k_match(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int32_t* __restrict__ match_a,
                                                           int32_t* __restrict__ match_b, int32_t* __restrict__ overlap, int32_t* __restrict__ count,
                                                           int32_t* __restrict__ status_a, int32_t* __restrict__ status_b, OverlapCall c)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_match[];
    const uint32_t tid = threadIdx.x;
    const size_t set = blockIdx.x, first_a = set * (uint32_t)c.ka, first_b = set * (uint32_t)c.kb;
    const MatchLds L = match_lds((uint32_t)c.ka, (uint32_t)c.kb);
    match_step_load(s_match, L, c, tid, kOverlapThreads, a + first_a * 8u, b + first_b * 8u, status_a ? status_a + first_a : nullptr, status_b ? status_b + first_b : nullptr);
    __syncthreads();
    // (a thread reads the count behind the second barrier of a round and the next addition to it lies behind the first of the next)
    for (uint32_t pairs = 0;;) {
        match_step_seek(s_match, L, c, tid, kOverlapThreads);
        __syncthreads();
        match_step_take(s_match, L, c, tid, kOverlapThreads, overlap + first_a);
        __syncthreads();
        const uint32_t now = match_pairs(s_match, L);
        if (now == pairs) break;
        pairs = now;
    }
    match_step_store(s_match, L, c, tid, kOverlapThreads, match_a + first_a, match_b + first_b, overlap + first_a, count + set);
}
#endif

// ---- host only: the definitions for one set (pair), a sort and a walk that use none of the steps above.  Every pointer the set's own;
// out, order, status (status_a, status_b) may be null.
inline void suppress_set_host(const OverlapCall& c, const int32_t* rows, const int32_t* scores, int32_t* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    const int32_t K = c.ka;
    std::vector<int32_t> walk;
    for (int32_t i = 0; i < K; i++) {
        const int32_t st = overlap_row_status(rows + 8 * (size_t)i, c.fw, c.fh, c.n_frames);
        if (status) status[i] = st;
        if (st == kRegionOk) walk.push_back(i);
    }
    auto score = [&](int32_t i) { return scores ? scores[(size_t)i * (size_t)c.score_stride] : 0; };
    std::stable_sort(walk.begin(), walk.end(), [&](int32_t p, int32_t q) { return score(p) > score(q); });
    auto box = [&](int32_t i) { const int32_t* r = rows + 8 * (size_t)i; return OverlapBox{r[1], r[2], r[3], r[4]}; };
    std::vector<int32_t> kept;
    for (int32_t i : walk) {
        by[i] = -1;
        for (int32_t k : kept)
            if (overlap_reaches(c.threshold, overlap_terms(c.measure, box(k), box(i)))) { by[i] = k; break; }
        if (by[i] == -1) kept.push_back(i);
    }
    for (int32_t k = 0; k < K; k++) {
        const bool used = (size_t)k < kept.size();
        if (out) {
            int32_t* o = out + 8 * (size_t)k;
            for (int u = 0; u < 8; u++) o[u] = used && u < 5 ? rows[8 * (size_t)kept[(size_t)k] + (size_t)u] : 0;
        }
        if (order) order[k] = used ? kept[(size_t)k] : -1;
    }
    *count = (int32_t)kept.size();
}

inline void match_set_host(const OverlapCall& c, const int32_t* a, const int32_t* b, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count, int32_t* status_a,
                           int32_t* status_b)
{
    struct Pair { int32_t i, j; OverlapTerms t; };
    std::vector<int32_t> ok_a, ok_b;
    for (int32_t i = 0; i < c.ka; i++) {
        const int32_t st = overlap_row_status(a + 8 * (size_t)i, c.fw, c.fh, c.n_frames);
        if (status_a) status_a[i] = st;
        if (st == kRegionOk) { ok_a.push_back(i); match_a[i] = -1; overlap[i] = 0; }
    }
    for (int32_t j = 0; j < c.kb; j++) {
        const int32_t st = overlap_row_status(b + 8 * (size_t)j, c.fw, c.fh, c.n_frames);
        if (status_b) status_b[j] = st;
        if (st == kRegionOk) { ok_b.push_back(j); match_b[j] = -1; }
    }
    std::vector<Pair> pairs;
    for (int32_t i : ok_a)
        for (int32_t j : ok_b) {
            const int32_t* p = a + 8 * (size_t)i;
            const int32_t* q = b + 8 * (size_t)j;
            const OverlapTerms t = overlap_terms(c.measure, OverlapBox{p[1], p[2], p[3], p[4]}, OverlapBox{q[1], q[2], q[3], q[4]});
            if (overlap_reaches(c.threshold, t)) pairs.push_back(Pair{i, j, t});
        }
    std::sort(pairs.begin(), pairs.end(), [](const Pair& p, const Pair& q) {
        if (overlap_above(p.t, q.t)) return true;
        if (overlap_above(q.t, p.t)) return false;
        return p.i != q.i ? p.i < q.i : p.j < q.j;
    });
    int32_t taken = 0;
    for (const Pair& p : pairs) {
        if (match_a[p.i] != -1 || match_b[p.j] != -1) continue;
        match_a[p.i] = p.j;
        match_b[p.j] = p.i;
        overlap[p.i] = overlap_q16(p.t);
        taken++;
    }
    *count = taken;
}

}  // namespace leon
#endif
