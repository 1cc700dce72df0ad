// leon_resize_row.h -- one output sample's row of a resize table (the definition of include/leon_pipeline.h, leon_pipeline_tensor_resize),
// for the host (resize_axis_build, leon_pipeline_impl.h) and the device (k_box_tables, leon_kernels.h): ONE text, so that a table built
// on the GPU is the table the host builds, word for word.
// Everything here is IEEE binary64 evaluated as written: `/` is the correctly rounded division on both sides, nothing is contracted
// into an fma (the library is compiled with -ffp-contract=off on both halves; the pragmas hold it for other builds), no fast-math
// flag, no reciprocal in place of `/ fscale` or `/ sum`.  The double -> int32 conversions only see values inside the type: the box
// lies inside a frame of at most 4096 samples an axis, so |center| < 2^13 and with support <= 32 every window bound is far inside
// int32, and a weight is a share of its row's sum times 2^22 (resize_axis_build refuses |W| >= 2^23) -- out of range the conversion
// differs between x86 (0x80000000) and the GPU (saturating); in range both truncate toward zero.
#ifndef LEON_RESIZE_ROW_H
#define LEON_RESIZE_ROW_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEON_HD __host__ __device__
#else
#define LEON_HD
#endif

namespace leon {

static constexpr int kResizeMaxTapsTriangle = 33;            // = LEON_RESIZE_MAX_TAPS: 2 * 16 + 1
static constexpr int kResizeMaxTapsCubic = 65;               // = LEON_RESIZE_MAX_TAPS_BICUBIC: 4 * 16 + 1
static constexpr int kResizeMaxRatio = 16;

LEON_HD inline double resize_filter_triangle(double x)
{
    const double t = 1.0 - __builtin_fabs(x);
    return t > 0.0 ? t : 0.0;
}
LEON_HD inline double resize_filter_bicubic(double x)          // Keys' cubic, a = -0.5
{
#pragma clang fp contract(off)
    const double a = -0.5;
    x = __builtin_fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// What every row of one axis shares.  The arguments are inside resize_axis_build's limits (the box non-empty and inside the axis,
// crop_size <= 16 * out_size): the caller has judged them.
struct ResizeAxis {
    double start, scale, fscale, support;
    int32_t in_size;
    bool cubic;
};
LEON_HD inline ResizeAxis resize_axis(int32_t in_size, int32_t crop_start, int32_t crop_size, int32_t out_size, bool cubic)
{
#pragma clang fp contract(off)
    ResizeAxis a;
    a.scale = (double)crop_size / (double)out_size;
    a.fscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = (cubic ? 2.0 : 1.0) * a.fscale;
    a.start = (double)crop_start;
    a.in_size = in_size;
    a.cubic = cubic;
    return a;
}

// The window of output sample o: taps lo .. lo + n - 1 (n < 1: the caller refuses)
struct ResizeWindow {
    double center;
    int32_t lo, n;
};
LEON_HD inline ResizeWindow resize_row_window(const ResizeAxis& a, int32_t o)
{
#pragma clang fp contract(off)
    ResizeWindow w;
    w.center = a.start + ((double)o + 0.5) * a.scale;
    int32_t lo = (int32_t)(w.center - a.support + 0.5), hi = (int32_t)(w.center + a.support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > a.in_size) hi = a.in_size;
    w.lo = lo;
    w.n = hi - lo;
    return w;
}
// the filter's value at tap k of the window
LEON_HD inline double resize_row_tap(const ResizeAxis& a, const ResizeWindow& w, int32_t k)
{
#pragma clang fp contract(off)
    const double x = ((double)(w.lo + k) - w.center + 0.5) / a.fscale;
    return a.cubic ? resize_filter_bicubic(x) : resize_filter_triangle(x);
}
// their sum, in index order (a row evaluated twice -- once for this, once for the weights -- sees the same values: it is deterministic)
LEON_HD inline double resize_row_sum(const ResizeAxis& a, const ResizeWindow& w)
{
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int32_t k = 0; k < w.n; k++) sum += resize_row_tap(a, w, k);
    return sum;
}
// the table's word of a tap: its share of the row in 22 fractional bits, rounded half away from zero
LEON_HD inline int32_t resize_row_weight(double tap, double sum)
{
#pragma clang fp contract(off)
    const double v = (tap / sum) * 4194304.0;
    return v < 0.0 ? (int32_t)(-0.5 + v) : (int32_t)(0.5 + v);
}

// ---- one region of a call whose boxes lie in device memory, judged (LEON_REGION_* of include/leon_pipeline.h) -------------------
// 0 exactly when leon_pipeline_regions_check accepts the region alone; otherwise the first failing check in regions_check's order: the
// reserved words, the frame index, then per axis -- x before y, as resize_axis_build is called -- the box, the ratio, the rows' tap
// counts.  (resize_axis_build's two further refusals, a row without weight and a weight outside 24 bits, cannot happen with these
// filters inside these limits: the sample nearest to a row's centre lies in the box and weighs at least half the filter's peak.)
enum { kRegionOk = 0, kRegionReserved = 1, kRegionFrame = 2, kRegionBox = 3, kRegionRatioX = 4, kRegionRatioY = 5, kRegionTaps = 6 };

// the box and the ratio of one axis: 0, kRegionBox or `ratio_code`
LEON_HD inline int32_t region_axis_status(int32_t in_size, int32_t start, int32_t size, int32_t out_size, int32_t ratio_code)
{
    if (in_size < 1 || size < 1 || start < 0 || start > in_size || size > in_size - start) return kRegionBox;
    if ((int64_t)size > (int64_t)kResizeMaxRatio * (int64_t)out_size) return ratio_code;
    return kRegionOk;
}
// a row's tap count as resize_axis_build judges it
LEON_HD inline bool resize_row_count_ok(int32_t n, bool cubic) { return n >= 1 && n <= (cubic ? kResizeMaxTapsCubic : kResizeMaxTapsTriangle); }

// ---- the letterbox integers (leon_pipeline_letterbox of include/leon_pipeline.h) --------------------------------------------------
// A source of sw x sh scaled to fit cw x ch with its aspect ratio kept, and centred: 64-bit integers only.  One text for the host
// (leon_pipeline_letterbox, the fit of leon_pipeline_resample_regions_fit) and the device (k_fit_tables), so that a region's image
// rectangle is the same four words wherever it is worked out.  All four sizes are >= 1: the caller has judged them.
struct FitRect {
    int32_t ow, oh, x, y;
};
LEON_HD inline FitRect letterbox_rect(int32_t src_w, int32_t src_h, int32_t canvas_w, int32_t canvas_h)
{
    const int64_t sw = src_w, sh = src_h, cw = canvas_w, ch = canvas_h;
    int64_t ow, oh;
    if (cw * sh <= ch * sw) {
        ow = cw;
        oh = (2 * sh * cw + sw) / (2 * sw);
        if (oh < 1) oh = 1;
    } else {
        oh = ch;
        ow = (2 * sw * ch + sh) / (2 * sh);
        if (ow < 1) ow = 1;
    }
    return FitRect{(int32_t)ow, (int32_t)oh, (int32_t)((cw - ow) / 2), (int32_t)((ch - oh) / 2)};
}
// The image rectangle of one region of a letterboxed call (leon_pipeline_regions_fit): the letterbox of the box in the canvas, at
// (0, 0) with the top-left anchor.  A box without a size has no letterbox: it gets the canvas itself, and region_axis_status then
// names the box (kRegionBox) on the axis that has none, in regions_check's order.
LEON_HD inline FitRect region_fit_rect(int32_t box_w, int32_t box_h, int32_t canvas_w, int32_t canvas_h, bool top_left)
{
    if (box_w < 1 || box_h < 1) return FitRect{canvas_w, canvas_h, 0, 0};
    FitRect r = letterbox_rect(box_w, box_h, canvas_w, canvas_h);
    if (top_left) r.x = r.y = 0;
    return r;
}

}  // namespace leon
#endif
