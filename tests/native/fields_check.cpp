// fields_check.cpp -- csrc/leon_fields.h as a stand-alone program (built with the address and undefined-behaviour sanitizers by
// tests/test_fields_walk_native.py): the walk k_fields' lanes take over every tile of the output -- the tables into the tile, the
// horizontal pass, the vertical pass into the packed tile, the 16-byte lines and the elements at a row's ends out -- against the plain
// loop over samples (field_sample), over heap buffers of EXACTLY source_bytes whose last item's channels end at the buffer's last
// byte, and tensors of exactly their bytes: a load past the source or a store past the tensor is an error here, not on a device.
// The tables are built here from leon_resize_row.h's row functions, as k_box_tables lays them out.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../mpeg1video-decoder-webgl_amd/csrc/leon_fields.h"

using namespace leon;

static int failed = 0;
static long runs = 0, samples = 0;

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

struct Axis {
    std::vector<int32_t> first, count, w;
    int32_t taps;
};
static Axis axis_tables(int32_t in_size, int32_t start, int32_t size, int32_t out, bool odd)
{
    Axis a;
    const ResizeAxis A = resize_axis(in_size, start, size, out, false);
    int32_t most = 0;
    for (int32_t o = 0; o < out; o++) most = resize_row_window(A, o).n > most ? resize_row_window(A, o).n : most;
    a.taps = odd ? most | 1 : most;
    a.first.resize(out); a.count.resize(out); a.w.assign((size_t)out * a.taps, 0);
    for (int32_t o = 0; o < out; o++) {
        const ResizeWindow R = resize_row_window(A, o);
        const double sum = resize_row_sum(A, R);
        a.first[o] = R.lo; a.count[o] = R.n;
        for (int32_t k = 0; k < R.n; k++) a.w[(size_t)o * a.taps + k] = resize_row_weight(resize_row_tap(A, R, k), sum);
    }
    return a;
}

struct Case {
    int32_t fw, fh, x, y, w, h, ow, oh, dtype, channels;
    FieldChannel ch[kFieldMaxChannels];
    int32_t n_items, item;
    size_t item_pitch;
    int fill;          // 0: random values, 1: all -32768, 2: all 32767
};

static void run(const Case& c)
{
    runs++;
    // the source: exactly n_items * item_pitch bytes on the heap
    const size_t source_bytes = (size_t)c.n_items * c.item_pitch;
    uint8_t* src = static_cast<uint8_t*>(std::malloc(source_bytes));
    uint32_t seed = 12345u + (uint32_t)runs;
    for (size_t i = 0; i + 1 < source_bytes; i += 2) {
        const int16_t v = c.fill == 1 ? (int16_t)-32768 : c.fill == 2 ? (int16_t)32767 : (int16_t)(lcg(&seed) >> 16);
        std::memcpy(src + i, &v, 2);
    }
    for (int32_t q = 0; q < c.channels; q++)
        if (field_channel_judge(c.ch[q], c.fw, c.fh, c.dtype, c.item_pitch) != kFieldOk) {
            if (failed++ < 10) std::printf("FAILED case %ld: channel %d is refused\n", runs, q);
            std::free(src);
            return;
        }
    const Axis X = axis_tables(c.fw, c.x, c.w, c.ow, true), Y = axis_tables(c.fh, c.y, c.h, c.oh, false);
    const FieldTables T{X.first.data(), X.count.data(), X.w.data(), Y.first.data(), Y.count.data(), Y.w.data(), X.taps, Y.taps};
    const int32_t eb = field_elem_bytes(c.dtype);
    const size_t bytes = (size_t)c.channels * c.oh * c.ow * eb;
    uint8_t* want = static_cast<uint8_t*>(std::aligned_alloc(16, (bytes + 15) & ~(size_t)15));
    uint8_t* got = static_cast<uint8_t*>(std::aligned_alloc(16, (bytes + 15) & ~(size_t)15));
    // (aligned_alloc wants a multiple of the alignment: the walk is checked against the tensor's own end below)
    std::memset(want, 0xA5, (bytes + 15) & ~(size_t)15);
    std::memset(got, 0xA5, (bytes + 15) & ~(size_t)15);
    const uint8_t* item = src + (size_t)c.item * c.item_pitch;
    for (int32_t q = 0; q < c.channels; q++)
        for (int32_t oy = 0; oy < c.oh; oy++)
            for (int32_t ox = 0; ox < c.ow; ox++) {
                field_store_elem(want + (((size_t)q * c.oh + oy) * c.ow + ox) * eb, field_elem(field_value(field_sample(item, c.ch[q], T, ox, oy), c.ch[q].scale, c.ch[q].bias), c.dtype), eb);
                samples++;
            }
    // the kernel's walk: every tile, its steps in order, every lane of a step before the next step (the barriers)
    FieldTile* t = new FieldTile;
    for (int32_t by = 0; by * kFieldTileY < c.oh; by++)
        for (int32_t bx = 0; bx * kFieldTileX < c.ow; bx++) {
            std::memset(static_cast<void*>(t), 0x5A, sizeof(FieldTile));
            const FieldTileAt a = field_tile_at(c.ow, c.oh, bx, by);
            for (int32_t tid = 0; tid < kFieldLanes; tid++) field_step_tables(*t, T, a, tid);
            int32_t ry0, rows;
            field_tile_rows(*t, a, &ry0, &rows);
            if (rows > kFieldHRows - 1 || ry0 < 0 || ry0 + rows > c.fh) {
                if (failed++ < 10) std::printf("FAILED case %ld: tile (%d, %d) needs rows %d .. %d of %d\n", runs, bx, by, ry0, ry0 + rows, c.fh);
                continue;
            }
            for (int32_t q = 0; q < c.channels; q++) {
                for (int32_t tid = 0; tid < kFieldLanes; tid++) field_step_h(*t, item, c.ch[q], a, ry0, rows, tid);
                for (int32_t tid = 0; tid < kFieldLanes; tid++) field_step_v(*t, c.ch[q], a, c.ow, c.oh, q, c.dtype, ry0, rows, tid);
                for (int32_t tid = 0; tid < kFieldLanes; tid++) field_step_store(*t, got, a, c.ow, c.oh, q, c.dtype, tid);
            }
        }
    delete t;
    if (std::memcmp(want, got, (bytes + 15) & ~(size_t)15) != 0) {
        size_t at = 0;
        while (want[at] == got[at]) at++;
        if (failed++ < 10)
            std::printf("FAILED case %ld (%dx%d box %d,%d,%d,%d -> %dx%d dtype %d C %d): byte %zu of %zu is %02x, not %02x\n", runs, c.fw, c.fh, c.x, c.y, c.w, c.h, c.ow, c.oh,
                        c.dtype, c.channels, at, bytes, got[at], want[at]);
    }
    std::free(want);
    std::free(got);
    std::free(src);
}

static FieldChannel channel(uint32_t off, int32_t rs, int32_t es, int32_t shift, float scale, float bias) { return FieldChannel{off, rs, es, shift, scale, bias, {0, 0}}; }

// the channels of a case: shifts 0, 1 and 4 in turn, the shift-4 ones interleaved 4 apart as a motion record's; the item's pitch is the
// end of the channel that ends last, so in the last item that channel ends at the buffer's last byte
static void with_channels(Case c, int32_t channels)
{
    c.channels = channels;
    uint64_t end = 0;
    uint32_t at = 0;
    for (int32_t q = 0; q < channels; q++) {
        const int32_t shift = q % 3 == 0 ? 0 : q % 3 == 1 ? 1 : 4;
        const int32_t cells = ((c.fw - 1) >> shift) + 1;
        const int32_t es = shift == 4 ? 4 : 1, rs = cells * es + (q & 1);
        c.ch[q] = channel(at + (shift == 4 ? 2u * (uint32_t)(q & 3) : 0u), rs, es, shift, 1.0f / (float)(1 + q), (float)q - 1.5f);
        const uint64_t e = field_channel_end(c.ch[q], c.fw, c.fh);
        end = e > end ? e : end;
        at = (uint32_t)((e + 6u) & ~(uint64_t)1);
    }
    c.item_pitch = (size_t)end;
    c.n_items = 3; c.item = 2;
    run(c);
}

int main()
{
    const int32_t frames[][2] = {{16, 16}, {50, 38}, {128, 32}, {127, 33}};
    const int32_t outs[][2] = {{1, 1}, {7, 5}, {31, 7}, {32, 8}, {33, 9}, {9, 3}, {5, 17}, {65, 2}};
    for (const auto& f : frames) {
        const int32_t fw = f[0], fh = f[1];
        for (const auto& o : outs)
            for (int32_t dtype = kFieldF16; dtype <= kFieldF32; dtype++) {
                const int32_t boxes[][4] = {{0, 0, fw, fh}, {0, 0, 3, 3}, {fw - 3, fh - 3, 3, 3}, {fw / 2, 0, fw - fw / 2, fh / 2}, {0, fh / 2, fw / 3 + 1, fh - fh / 2},
                                            {1, 1, fw - 2, fh - 2}};
                for (const auto& b : boxes) {
                    if (b[2] > 16 * o[0] || b[3] > 16 * o[1] || b[2] < 1 || b[3] < 1) continue;
                    Case c{};
                    c.fw = fw; c.fh = fh; c.x = b[0]; c.y = b[1]; c.w = b[2]; c.h = b[3]; c.ow = o[0]; c.oh = o[1]; c.dtype = dtype;
                    for (int32_t channels : {1, 3, 8}) {
                        c.fill = 0;
                        with_channels(c, channels);
                    }
                    c.fill = 1;
                    with_channels(c, 3);
                    c.fill = 2;
                    with_channels(c, 3);
                }
            }
    }
    // a ratio of exactly 16 on both axes: the most rows a tile's vertical taps need
    for (int32_t dtype = kFieldF16; dtype <= kFieldF32; dtype++) {
        Case c{};
        c.fw = 160; c.fh = 144; c.x = 0; c.y = 0; c.w = 160; c.h = 144; c.ow = 10; c.oh = 9; c.dtype = dtype;
        with_channels(c, 3);
    }
    // the rounding of the element types, value by value, against the compiler's own conversions where it has the type
    uint32_t seed = 7u;
    for (int i = 0; i < 2000000; i++) {
        const uint32_t x = i < 1000000 ? lcg(&seed) : (0x33000000u + (uint32_t)(i - 1000000) * 977u) | (i & 1 ? 0x80000000u : 0u);
        float v;
        std::memcpy(&v, &x, 4);
        if (!field_finite(v)) continue;
#if defined(__FLT16_MANT_DIG__)
        const _Float16 h = (_Float16)v;
        uint16_t hb;
        std::memcpy(&hb, &h, 2);
        if (field_f16_bits(v) != hb && failed++ < 10) std::printf("FAILED fp16 of %08x: %04x, not %04x\n", x, field_f16_bits(v), hb);
#endif
        // bf16: the two neighbours, the nearer one, the even one on a tie
        const uint32_t lo = x & 0xffff0000u, hi = lo + 0x10000u, rem = x & 0xffffu;
        const uint32_t want = rem > 0x8000u ? hi : rem < 0x8000u ? lo : (lo & 0x10000u) ? hi : lo;
        if (field_bf16_bits(v) != (want >> 16) && failed++ < 10) std::printf("FAILED bf16 of %08x: %04x, not %04x\n", x, field_bf16_bits(v), want >> 16);
    }
    std::printf("fields_check: %ld cases, %ld samples, %d failed\n", runs, samples, failed);
    return failed ? 1 : 0;
}
