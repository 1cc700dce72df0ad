// leon_propose.h -- boxes of what moves or changes, from a frame's motion and activity records (the definition of
// include/leon_pipeline.h, leon_pipeline_propose_regions), for the host (propose_record_host: leon_pipeline_impl.h) and the device
// (k_propose: leon_kernels.h): ONE text, as leon_gauge.h is for its calls.  Integers only: the hot predicate from a record's dwords,
// the judgement of a request, the box of a cell extent, the filler row, and the layout of the kernel's LDS with the bit arithmetic it
// labels rows with.  The two searches for the components share none of it: the kernel's (union by smallest index, leon_kernels.h)
// and the host's (a flood fill, propose_request_host at the end of this file, host only, so that a stand-alone program can check it).
#ifndef LEON_PROPOSE_H
#define LEON_PROPOSE_H
#include <stdint.h>
#include <cstring>
#include <vector>
#include "leon_carry.h"
#include "leon_activity.h"

namespace leon {

enum { kProposeMotion = 1, kProposeActivity = 2 };      // the bits of `sources`
enum { kProposeIntra = 1 };                              // the bits of `flags`
enum { kProposeMaxBoxes = 1024, kProposeMaxCells = 65536 };
enum { kProposeThreads = 512 };                           // k_propose's workgroup: 8 waves

struct ProposeConfig {                   // = leon_pipeline_propose_config
    int32_t sources, flags, mv_min, ac_min, connectivity, min_cells, max_boxes, reserved;
};

// a request is a frame of the window; nothing else is judged
LEON_HD inline int32_t propose_request_status(int32_t frame, int32_t n_frames) { return frame < 0 || frame >= n_frames ? kRegionFrame : kRegionOk; }

// Is macroblock (i, j) hot: lo the first dword of its activity cell (leon_activity.h: ac_mag in the high half), info and fwd / bwd its
// motion entry (leon_motion.h); what belongs to a source the config does not ask for is not looked at.  A cell wholly outside the
// frame is never hot, whatever its records hold.
LEON_HD inline bool propose_hot(const ProposeConfig& c, int32_t fw, int32_t fh, int32_t i, int32_t j, uint32_t lo, uint32_t info, uint32_t fwd, uint32_t bwd)
{
    if (16 * i >= fw || 16 * j >= fh) return false;
    bool hot = false;
    if (c.sources & kProposeMotion) {
        const uint32_t a = motion_abs16(fwd), b = motion_abs16(fwd >> 16), d = motion_abs16(bwd), e = motion_abs16(bwd >> 16);
        const uint32_t ab = a > b ? a : b, de = d > e ? d : e;
        hot = (ab > de ? ab : de) >= (uint32_t)c.mv_min || ((c.flags & kProposeIntra) && (info & (uint32_t)kMotionIntra));
    }
    if (c.sources & kProposeActivity) hot = hot || (lo >> 16) >= (uint32_t)c.ac_min;
    return hot;
}

// the row of a component whose cells span columns i0 .. i1 and rows j0 .. j1: {frame, x, y, w, h, 0, 0, 0}, clipped to the frame
LEON_HD inline void propose_box(int32_t frame, int32_t fw, int32_t fh, int32_t i0, int32_t i1, int32_t j0, int32_t j1, int32_t* out)
{
    const int32_t x = 16 * i0, y = 16 * j0, xe = 16 * (i1 + 1) < fw ? 16 * (i1 + 1) : fw, ye = 16 * (j1 + 1) < fh ? 16 * (j1 + 1) : fh;
    out[0] = frame; out[1] = x; out[2] = y; out[3] = xe - x; out[4] = ye - y;
    out[5] = 0; out[6] = 0; out[7] = 0;
}
// a row behind `count`: a box regions_check refuses (LEON_REGION_BOX), and its info {cells 0, first -1}
LEON_HD inline void propose_filler(int32_t frame, int32_t* out, int32_t* info)
{
    out[0] = frame;
    for (int k = 1; k < 8; k++) out[k] = 0;
    info[0] = 0; info[1] = -1;
}

// ---- what k_propose keeps in LDS for one request: [labels | hot mask | root mask | rows | scan], every part a whole number of dwords.
// labels: 16 bits a cell (a cell index; in a root's own slot, later, its cell count less one and then its row), two to a dword;
// the masks: one bit a cell in raster order, padded to the 64 cells a wave writes at a time; rows: two dwords for each of the K rows
// ({first | (cells - 1) << 16}, {255 - i0 | i1 << 8 | j1 << 16}); scan: a dword for each of the workgroup's 8 waves.
// At 256 x 256 and K = 1024: 131072 + 8192 + 8192 + 8192 + 32 = 155680 bytes of a CU's 163840.
struct ProposeLds {
    uint32_t mask_words;                 // dwords of one mask
    uint32_t hot, root, rows, scan;      // dword offsets of the parts behind the labels (which start at 0)
    uint32_t bytes;
};
LEON_HD constexpr ProposeLds propose_lds(uint32_t mbs, uint32_t max_boxes)
{
    ProposeLds L{};
    L.mask_words = 2u * ((mbs + 63u) / 64u);
    L.hot = 32u * ((mbs + 63u) / 64u);           // labels for the padded cells: 64 cells = 32 dwords
    L.root = L.hot + L.mask_words;
    L.rows = L.root + L.mask_words;
    L.scan = L.rows + 2u * max_boxes;
    L.bytes = 4u * (L.scan + (uint32_t)kProposeThreads / 64u);
    return L;
}

LEON_HD inline bool propose_bit(const uint32_t* mask, uint32_t c) { return (mask[c >> 5] >> (c & 31u)) & 1u; }

// The first cell of the run of hot cells that ends at hot cell c, inside c's row (row0 = the row's first cell): the cell behind the
// nearest cold cell in front of c in raster order, or row0.  The row's cells are consecutive bits of the mask wherever its words start.
LEON_HD inline uint32_t propose_run_start(const uint32_t* mask, uint32_t c, uint32_t row0)
{
    uint32_t w = c >> 5;
    uint32_t cold = ~mask[w] & ((1u << (c & 31u)) - 1u);
    while (cold == 0u && (w << 5) > row0) cold = ~mask[--w];
    if (cold == 0u) return row0;
    const uint32_t s = (w << 5) + 32u - (uint32_t)__builtin_clz(cold);
    return s > row0 ? s : row0;
}

// a component's extent packed so that every field only grows: 255 - i0, i1, j1 (j0 is its first cell's row)
LEON_HD inline uint32_t propose_extent(uint32_t i, uint32_t j) { return (255u - i) | (i << 8) | (j << 16); }
LEON_HD inline uint32_t propose_extent_join(uint32_t a, uint32_t b)
{
    const uint32_t f0 = (a & 0xffu) > (b & 0xffu) ? (a & 0xffu) : (b & 0xffu);
    const uint32_t f1 = (a & 0xff00u) > (b & 0xff00u) ? (a & 0xff00u) : (b & 0xff00u);
    const uint32_t f2 = (a & 0xff0000u) > (b & 0xff0000u) ? (a & 0xff0000u) : (b & 0xff0000u);
    return f0 | f1 | f2;
}

// ---- host only: the definition for one accepted request, from the frame's records in host memory (a record the sources do not ask
// for may be null): the hot cells, a flood fill from each component's first cell in raster order (a stack of cells, each hot cell
// entered once), the rows and the filler.  regions: K x 8 words, info: K x 2 words or null.  It uses nothing of the kernel's search.
inline void propose_request_host(const ProposeConfig& c, int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, const uint8_t* mrec, const uint8_t* arec, int32_t frame,
                                 int32_t* regions, int32_t* info, int32_t* count)
{
    const MotionLayout L = motion_layout((uint32_t)mbw, (uint32_t)mbh);
    const int32_t mbs = mbw * mbh, K = c.max_boxes;
    std::vector<uint8_t> hot((size_t)mbs);                // 1: hot and not yet in a component
    for (int32_t k = 0; k < mbs; k++) {
        uint32_t lo = 0, f = 0, b = 0, nf = 0;
        if (c.sources & kProposeActivity) std::memcpy(&lo, arec + 8 * (size_t)k, 4);
        if (c.sources & kProposeMotion) {
            std::memcpy(&f, mrec + 8 * (size_t)k, 4);
            std::memcpy(&b, mrec + 8 * (size_t)k + 4, 4);
            nf = mrec[L.info_offset + (size_t)k];
        }
        hot[(size_t)k] = propose_hot(c, fw, fh, k % mbw, k / mbw, lo, nf, f, b) ? 1 : 0;
    }
    int32_t found = 0;
    std::vector<int32_t> stack;
    for (int32_t first = 0; first < mbs; first++) {       // raster order: a component is met at its smallest cell
        if (!hot[(size_t)first]) continue;
        int32_t cells = 0, i0 = mbw, i1 = -1, j1 = -1;
        hot[(size_t)first] = 0;
        stack.assign(1, first);
        while (!stack.empty()) {
            const int32_t k = stack.back(), i = k % mbw, j = k / mbw;
            stack.pop_back();
            cells++;
            i0 = i < i0 ? i : i0; i1 = i > i1 ? i : i1; j1 = j > j1 ? j : j1;
            for (int32_t dj = -1; dj <= 1; dj++)
                for (int32_t di = -1; di <= 1; di++) {
                    if ((!di && !dj) || (di && dj && c.connectivity != 8)) continue;
                    const int32_t ni = i + di, nj = j + dj;
                    if (ni < 0 || ni >= mbw || nj < 0 || nj >= mbh || !hot[(size_t)nj * (size_t)mbw + (size_t)ni]) continue;
                    hot[(size_t)nj * (size_t)mbw + (size_t)ni] = 0;
                    stack.push_back(nj * mbw + ni);
                }
        }
        if (cells < c.min_cells) continue;
        if (found < K) {
            propose_box(frame, fw, fh, i0, i1, first / mbw, j1, regions + 8 * (size_t)found);
            if (info) { info[2 * found] = cells; info[2 * found + 1] = first; }
        }
        found++;
    }
    for (int32_t k = found; k < K; k++) {
        int32_t nf[2];
        propose_filler(frame, regions + 8 * (size_t)k, nf);
        if (info) { info[2 * k] = nf[0]; info[2 * k + 1] = nf[1]; }
    }
    *count = found;
}

}  // namespace leon
#endif
