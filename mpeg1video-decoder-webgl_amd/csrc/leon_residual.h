// leon_residual.h -- the layout of a frame's residual record (the definition of include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_RESIDUAL),
// the tasks k_residual cuts a picture into and where each lane of a task stores, for the host (leon_pipeline_residual_layout:
// leon_pipeline_impl.h; tests/native/residual_check.cpp walks it) and the device (k_residual: leon_kernels.h): ONE text, as
// leon_activity.h is for its calls.  Integers only.  The arithmetic of the record's values is not here: it is the reconstruction
// kernels' column and row pass (leon_kernels.h), whose definition on the CPU is the oracle.
#ifndef LEON_RESIDUAL_H
#define LEON_RESIDUAL_H
#include <stdint.h>
#include "leon_resize_row.h"

namespace leon {

// where the planes of a record lie: [Y: ch rows | Cb: ch / 2 rows | Cr: ch / 2 rows] of int16, rows luma_stride / chroma_stride ELEMENTS
// apart (the plane's width rounded up to 64: a group's row of 8 blocks is one 128-byte line), every plane on a 256-byte boundary
struct ResidualLayout {
    uint32_t cw, ch, luma_stride, chroma_stride, cb_offset, cr_offset, record_bytes, record_pitch;
};
LEON_HD inline uint32_t residual_pad(uint32_t v, uint32_t to) { return (v + to - 1u) & ~(to - 1u); }
LEON_HD inline ResidualLayout residual_layout(uint32_t cw, uint32_t ch)
{
    ResidualLayout L;
    L.cw = cw; L.ch = ch;
    L.luma_stride = residual_pad(cw, 64u);
    L.chroma_stride = residual_pad(cw >> 1, 64u);
    L.cb_offset = residual_pad(2u * L.luma_stride * ch, 256u);
    L.cr_offset = L.cb_offset + residual_pad(2u * L.chroma_stride * (ch >> 1), 256u);
    L.record_bytes = L.cr_offset + 2u * L.chroma_stride * (ch >> 1);
    L.record_pitch = residual_pad(L.record_bytes, 256u);
    return L;
}

// the groups of a picture (include/leon_vlc.h) and the tasks of k_residual, the reconstruction kernels' decomposition: a task is two
// block groups that share their macroblocks -- luma: block rows 2 Rt and 2 Rt + 1 of group g; chroma: the Cb and the Cr group g of
// block row Rt.  Luma tasks first (Rt-major), then the chroma tasks.
struct ResidualGeom {
    uint32_t mbw, mbh, groups_y, groups_c, n_y, n_c, tasks_y, tasks;
};
LEON_HD inline ResidualGeom residual_geom(uint32_t mbw, uint32_t mbh)
{
    ResidualGeom G;
    G.mbw = mbw; G.mbh = mbh;
    G.groups_y = (mbw + 3u) / 4u;
    G.groups_c = (mbw + 7u) / 8u;
    G.n_y = 2u * mbh * G.groups_y;
    G.n_c = mbh * G.groups_c;
    G.tasks_y = mbh * G.groups_y;
    G.tasks = G.tasks_y + mbh * G.groups_c;
    return G;
}

struct ResidualTask {
    uint32_t chroma, Rt, g;
    uint32_t gid[2];             // the group ids of its two halves: what grp_off is indexed with
};
LEON_HD inline ResidualTask residual_task(const ResidualGeom& G, uint32_t t)
{
    ResidualTask T;
    T.chroma = t >= G.tasks_y ? 1u : 0u;
    if (T.chroma) {
        t -= G.tasks_y;
        T.Rt = t / G.groups_c;
        T.g = t - T.Rt * G.groups_c;
        T.gid[0] = G.n_y + T.Rt * G.groups_c + T.g;
        T.gid[1] = T.gid[0] + G.n_c;
    } else {
        T.Rt = t / G.groups_y;
        T.g = t - T.Rt * G.groups_y;
        T.gid[0] = 2u * T.Rt * G.groups_y + T.g;
        T.gid[1] = T.gid[0] + G.groups_y;
    }
    return T;
}

// blocks a row of the task's plane
LEON_HD inline uint32_t residual_block_width(const ResidualLayout& L, uint32_t chroma) { return (chroma ? L.cw >> 1 : L.cw) >> 3; }

// Lane (n = lane >> 3, b = lane & 7) of half `half` holds the 8 elements of row n of block b of the half's group: *off is the byte
// offset in the record at which it stores them (16 bytes; the 8 lanes of a row: 128 contiguous bytes); false: the block lies at or
// behind the plane's block width and the lane stores nothing
LEON_HD inline bool residual_store(const ResidualLayout& L, const ResidualTask& T, uint32_t half, uint32_t lane, uint32_t* off)
{
    const uint32_t n = lane >> 3, b = lane & 7u;
    const uint32_t row = 8u * (T.chroma ? T.Rt : 2u * T.Rt + half) + n;
    const uint32_t stride = T.chroma ? L.chroma_stride : L.luma_stride;
    const uint32_t plane = T.chroma ? (half ? L.cr_offset : L.cb_offset) : 0u;
    *off = plane + 2u * (row * stride + 64u * T.g + 8u * b);
    return 8u * T.g + b < residual_block_width(L, T.chroma);
}

}  // namespace leon
#endif
