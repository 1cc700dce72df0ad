// leon_kernels.h -- CDNA4 (gfx950) device code of the macroblock-reconstruction path.
//
// Three kernels, all HBM-bound integer/byte work (no MFMA: there is no dense
// contraction in this path):
//   k_recon      dequant + 8x8 IDCT (two passes with the reference's x0.4 int16
//                hand-off) + forward/backward/bidirectional half-pel motion
//                compensation + residual add + clamp, fused, for a BATCH of
//                mutually independent pictures.            (K1a+K1b+K2+K2-B)
//   k_rgba_*     YCbCr 4:2:0 -> RGBA8, fp64 "CPU twin" or fp32 "GL" flavour. (K3)
//   k_copy16     streaming 16 B/lane copy = the measured HBM roofline.
//
// What the arithmetic follows in /root/reference:
//   dequant + column pass   decoders/shaders/mpeg1video.js:19-24 (COL_INT_3, COL_INT_5)
//   row pass + MC + clamp   decoders/shaders/mpeg1video.js:24-29 (ROWSCOM_INT4, INTER_INT1)
//   predictor arithmetic    decoders/jsv.js:895-1129 (copyMacroblock), texel-granular
//                           CLAMP_TO_EDGE of jsv.js:216-217
//   colour conversion       player/easybits.player.js:2674-2785, player/parts/end.js:77-156
//
// Work decomposition of k_recon: one 64-lane wave = one task = TWO "block groups" that share
// their macroblocks (luma: the upper and lower 64x8 halves of four macroblocks; chroma: the Cb
// and the Cr group of one block row); a group = 8 horizontally adjacent 8x8 blocks.  Waves never
// talk to each other (no __syncthreads); each owns a private LDS strip.  One kernel instance
// per picture type and boundary format (k_recon<type, sparse>).
//   prologue every load that does not depend on the macroblock maps is requested first (first
//            coefficient rows or entry runs, matrix columns), then the maps and vectors; when
//            those arrive, the reference rows of BOTH halves (one aligned 12-byte row per lane)
//   stage 1  lane (r,b): coefficient row r of block b -> LDS tile [r][b][c]
//            (sparse boundary: the tile is cleared and the group's entries are scattered into it)
//   stage 2  lane (c = lane>>3, b = lane&7): column c of block b: 8 LDS reads, branch-free dequant
//            of the rows that are live anywhere in the wave (scalar liveness masks; zeros stay
//            zero like the shader's `if (X == 0.) continue`), butterfly, floor(v*0.4f), int16
//            hand-off wrap on a rare path, trunc(5w/2), written transposed to LDS as int32
//   stage 3  lane (n = lane>>3, b = lane&7): row n of block b: two 16-byte LDS reads, butterfly
//   stage 4  same lanes: the 8 lanes of a group hold 64 contiguous samples of ONE picture row, so
//            reference fetches and stores coalesce; lower reference row from lane+8; 8 predicted
//            samples via v_alignbyte + v_lerp_u8, residual add, v_ashr_pk_u8_i32, one 8-byte store
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "leon_resize_row.h"
#include "leon_warp.h"
#include "leon_motion.h"
#include "leon_activity.h"
#include "leon_residual.h"
#include "leon_carry.h"
#include "leon_propagate.h"
#include "leon_accumulate.h"
#include "leon_fields.h"
#include "leon_gauge.h"
#include "leon_propose.h"
#include "leon_overlap.h"


namespace leon {

struct PicDesc {                 // one per picture of a batch, device resident
    const int16_t* coef[4];      // T1: Y, Cb, Cr raw levels (+ A of a yuva stream)
    const uint8_t* qscale;       // T2
    const uint8_t* intra;        // T3
    const uint8_t* repadd;       // T4
    const uint8_t* mb_dir;       // B only
    const int16_t* mv_fwd;       // T5
    const int16_t* mv_bwd;       // B only
    uint8_t*       out;          // slot base: [Y | Cb | Cr]
    const uint8_t* ref_fwd;
    const uint8_t* ref_bwd;
    int32_t        type;         // 1 I, 2 P, 3 B
    uint32_t       n_entries;    // sparse boundary: entries[] length
    const uint32_t* grp_off;     // sparse boundary (include/leon_vlc.h): prefix offsets per 64x8 group
    const uint32_t* entries;     // (tile byte offset << 16) | level
    uint8_t*       rgba;         // fused display conversion: frame_w x frame_h RGBA8 destination (else null)
    int32_t        no_planes;    // with rgba: the slot's planes are not written (picture is never a reference)
    int32_t        pad_;
    const struct QTables* qt;    // the quantiser matrices of the picture's SEQUENCE (the reference reloads them at every sequence
                                 // header, decoders/jsv.js:540-558): one of the decoder's matrix sets
};

struct Geom {
    int32_t cw, ch;              // coded luma size
    int32_t mbw, mbh;
    int32_t gY, gC;              // block groups per block row (luma, chroma)
    int32_t tasksY, tasksC;      // gY*mbh luma tasks (two block rows each), gC*mbh chroma tasks (Cb + Cr)
    int32_t tasks_per_pic;       // tasksY + tasksC
    int32_t wg_per_pic;          // ceil(tasks_per_pic / 4): a workgroup never straddles pictures
    int32_t n_pics;
    int32_t n_wg;                // grid size
    uint32_t inv_wg_per_pic;     // ceil(2^32 / wg_per_pic)
    uint32_t inv_gY, inv_gC;     // ceil(2^32 / gY), ceil(2^32 / gC)
    int32_t fw, fh;              // display crop (fused display conversion)
    int32_t alpha;               // yuva: a fourth, luma-sized plane behind Cr; its tasks follow the chroma tasks
};

struct QTables {                 // T6, per sequence: 256 bytes = what a wave stages in its LDS strip (stage_tables)
    uint8_t qmT[2][8][8];        // [0 intra | 1 non-intra][column c][row i] = Q[i][c]
    uint8_t pmT[8][8];           // premultiplier, [column c][row i]
    uint8_t pad[64];             // (in LDS these 64 bytes carry a display task's vectors: kOffCarry)
};
struct Tables {                  // per decoder
    QTables q;                   // matrix set 0: leon_set_quant_matrices
    int32_t rgba_lut[1280];      // fused display conversion: fixed-point terms of YCbCrToRGBA (leon_rgba_lut.h)
};

// Output of a display task (k_recon_display_out): RGBA (what k_recon_display writes), the cropped YCbCr 4:2:0 planes of the frame
// (include/leon_pipeline.h: rows padded to 64 bytes, planes on 256-byte boundaries), or both.  Pictures with planes output find
// their frame's planes in FrameOut::frames[picture of the launch]: PicDesc keeps its 152 bytes, so the code of the RGBA kernels,
// which index it, stays as it is.
// What a launch writes besides the slot planes, from the host's launch classes down to the kernels' OUT: nothing (kOutSlots: k_recon),
// RGBA (k_recon_display), the frame's planes, both (k_recon_display_out).
static constexpr int kOutSlots = -1, kOutRgba = 0, kOutYcbcr = 1, kOutBoth = 2;
struct FrameOut {
    uint8_t* const* frames;      // per picture of the launch: its frame's planes record [Y | Cb | Cr (| A)]
    uint32_t luma_stride, chroma_stride;   // bytes per row: the plane width rounded up to 64
    uint32_t cb_off, cr_off, a_off;        // byte offsets of the planes in the record (multiples of 256)
    int32_t chroma_height;       // (frame_height + 1) / 2; Y and A have frame_height rows (Geom::fh)
};

static constexpr int kWavesPerWG = 4;
// Launch block sizes and the kernels' __launch_bounds__ come from the same constants: a launch with
// more threads than the bound fails at launch time ("unspecified launch failure" from
// hipGetLastError -- what a 512-thread block-size sweep of the RGBA kernels ran into in round 1).
static constexpr int kReconMaxThreads = 384;
static constexpr int kRgbaBlock = 256;
// A wave's LDS strip.  The tile holds BOTH block groups of a task, [half][row][block][column] int16, and is
// worked on in place: coefficients -> (column pass) the int16 hand-off values w -> (row pass reads them).
static constexpr int kLdsHalf = 1024;            // 8 rows x 128 B of int16: one block group
static constexpr int kLdsTile = 2 * kLdsHalf;
static constexpr int kLdsQtab = 256;             // a QTables: both matrices and the premultiplier (192 B) + 64 spare
static constexpr int kLdsSlots = 128;            // column pass: the ids of the live columns, one byte each
static constexpr int kOffQtab = kLdsTile;
static constexpr int kOffCarry = kOffQtab + 192;  // display kernels: the 64 bytes of the table strip no table uses hold the task's 8 + 8 vectors
static constexpr int kOffSlots = kLdsTile + kLdsQtab;
static constexpr int kLdsPerWave = kOffSlots + kLdsSlots;
// fused display conversion: the Y rows of a half change lanes through a 512-byte park (it shares its place with the
// column ids, which are dead by then), and the Cb and Cr samples of the task's 8 macroblocks (8 rows x 64 bytes
// each) wait in a stash for the luma parts of the same task
static constexpr int kLdsYpark = 512;
static constexpr int kOffYpark = kOffSlots;
static constexpr int kOffStash = kOffYpark + kLdsYpark;
static constexpr int kLdsStash = 2 * 512;
static constexpr int kLdsPerWaveDisplay = kOffStash + kLdsStash;      // 3840: 4 waves + the tables = 20 KB, 8 workgroups per CU
static constexpr int kLdsLut = 1280 * 4;         // display kernels: Tables::rgba_lut, one copy per workgroup, in front of the waves' strips
static constexpr int kLutShift = 21;             // = LEON_RGBA_LUT_SHIFT (static_assert in leon_hip.cpp)
static constexpr int kLdsPerWaveDisplayAlpha = kLdsPerWaveDisplay + 1024;   // yuva: + the parked A samples of a luma part
// dense P / B display tasks (round 4): the two luma parts of a task share ONE liveness scan and ONE column pass -- the right part's
// tile lies behind the wave's strip
// The wave's strip, two layouts:
//   0 (all kernels but the next): [tile 2048 | tables 192 + carried vectors 64 | column ids / Y park 512 | stash 1024 (| A park)]
//   1 (dense P display -- and dense B until it went to the three-tile layout 2 below --, two tiles): [tile L 2048 | carried vectors 64 | column ids 256 | stash 1024 | tile R 2048] = 5440 bytes:
//     4 waves + the conversion tables = 26.25 KB, SIX workgroups per CU (with layout 0 plus a second tile: 28 KB, five -- and the B
//     kernel loses 7 % at five).  What went: the wave's LDS copy of the quantiser tables (the column pass reads its two 8-byte columns
//     from the picture's QTables in memory: 256 bytes that every wave of the launch reads, L1 hits), and the Y park, which now lies in
//     the tile half whose row pass has just read it out.
template <int LAYOUT> struct Lay;
template <> struct Lay<0> { static constexpr int carry = kOffQtab + 192, slots = kOffSlots, stash = kOffStash; static constexpr bool tables_in_lds = true, park_in_tile = false; };
template <> struct Lay<1> { static constexpr int carry = kLdsTile, slots = kLdsTile + 64, stash = kLdsTile + 64 + 256, tile_r = kLdsTile + 64 + 256 + kLdsStash;
                            static constexpr bool tables_in_lds = false, park_in_tile = true; };
static constexpr int kLdsPerWaveDisplayPair = Lay<1>::tile_r + kLdsTile;      // 5440
static constexpr int kOffTileR = Lay<1>::tile_r;
// the luma parts of a display task do not run a front each: dense P and B pictures without alpha (P: the two share recon_luma_pair's on
// layout 1; B: front3_task below)
constexpr bool pair_task(int type, bool sparse, bool alpha) { return !sparse && !alpha && type != 1; }
// dense B display tasks run ONE front for all three parts (layout 2, display_task_front3) instead of the chroma part's and the luma
// pair's.  P stays as it is: the same task measured 1 % SLOWER there (0.473-0.483 against 0.469-0.478 ms per launch, one box,
// alternating, at six and at five workgroups per CU) -- its waves wait for memory, not for issue slots (0.70 of the time a vector
// instruction in flight, B 0.92), and the second barrier costs it more than 100 of 1451 instructions bring.
constexpr bool front3_task(int type, bool sparse, bool alpha) { return pair_task(type, sparse, alpha) && type == 3; }
// a display wave's strip in bytes: what the kernels step by and what the host launches with
constexpr int display_strip_bytes(int type, bool sparse, bool alpha) { return alpha ? kLdsPerWaveDisplayAlpha : (pair_task(type, sparse, alpha) ? kLdsPerWaveDisplayPair : kLdsPerWaveDisplay); }
// dense B display tasks (front3_task) with ONE front for the chroma part and both luma parts (recon_task, FRONT3): three tiles at once.  The
// workgroup's LDS is one static array in blocks, every address a compile-time constant plus a multiple of the wave's number:
//   [tiles L, R 4096 x4 | C first KB x4 | column ids 384 x4 | C second KB x4 | carried vectors 64 x4] = 26368 bytes, SIX workgroups per CU.
// The chroma tile lies in two pieces (Cb rows in the first KB, Cr rows kSfCHalf behind them).  The chroma samples park in the first KB
// (Cb | Cr, 512 bytes each: what `stash` was), each half behind its row pass.  Once every wave's chroma part is through (barrier 1 of
// display_task_front3) the ids and the second KBs are dead, and the conversion tables (kLdsLut) take their place: the Y table over the last
// KB of the ids block, the 4 KB of chroma tables over the four second KBs, contiguous behind it.
static constexpr int kSfIdsPerWave = 3 * 128;
static constexpr int kSfC0 = kWavesPerWG * 2 * kLdsTile;                 // 16384
static constexpr int kSfIds = kSfC0 + kWavesPerWG * kLdsHalf;            // 20480
static constexpr int kSfC1 = kSfIds + kWavesPerWG * kSfIdsPerWave;       // 22016
static constexpr int kSfCarry = kSfC1 + kWavesPerWG * kLdsHalf;          // 26112
static constexpr int kSfBytes = kSfCarry + kWavesPerWG * 64;             // 26368
static constexpr int kSfCHalf = kSfC1 - kSfC0;                           // from a wave's Cb rows to its Cr rows
static constexpr int kSfLut = kSfCarry - kLdsLut;                        // 20992
static_assert(kSfLut >= kSfIds && kSfLut + 1024 == kSfC1 && kSfC1 % 16 == 0, "the tables overlay the ids and the second KBs exactly");
static_assert(6 * kSfBytes <= 160 * 1024, "six workgroups per CU");
template <> struct Lay<2> { static constexpr bool tables_in_lds = false, park_in_tile = true; };
// cache policy bits of the frames' stores (1 sc0, 2 nt, 16 sc1).  nt: the GPU never reads a frame again, and written through the
// caches like everything else it pushes the reference planes out -- round 4, one box, alternating: 5.944 -> 5.818 ms per step (I -5 %,
// P -3.6 %, mixed B -1.2 %); sc0 / sc1: nothing.  (Round 2 measured nt on ALL stores: -4 %, the planes are read again.)
static constexpr int kAuxFrameStore = 2;

// ---- small helpers -----------------------------------------------------------

// Pointers read out of a PicDesc are generic; telling the compiler they are global
// turns flat_load/flat_store into global_load/global_store with an SGPR base.
#define LEON_GLOBAL __attribute__((address_space(1)))
typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v3u __attribute__((ext_vector_type(3)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ const LEON_GLOBAL T* gptr(const T* p) { return (const LEON_GLOBAL T*)p; }
template <typename T>
__device__ __forceinline__ LEON_GLOBAL T* gptr_mut(T* p) { return (LEON_GLOBAL T*)p; }

// a*K + c with a 24-bit multiplier, one full-rate VALU op.  (hipcc turns __mul24 by
// a constant into the quarter-rate v_mul_lo_u32 once it has proven the operand small.)
__device__ __forceinline__ int mad24k(int a, int k, int c)
{
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(k), "v"(c));
    return d;
}

// {sat_u8(a >> SH), sat_u8(b >> SH), sat_u8(c >> SH), sat_u8(d >> SH)}: two v_ashr_pk_u8_i32 (gfx950), the second one
// into the high half of the same register (op_sel[3]; each leaves the other half alone).  Through asm: hipcc's own
// pattern match of med3(ashr)|shl onto this instruction (ROCm 7.2) forgets that it leaves half of the destination
// alone, and the builtin does not know the half-selecting form.
template <int SH>
__device__ __forceinline__ uint32_t sat_pk4(int a, int b, int c, int d)
{
    uint32_t r;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "n"(SH));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(r) : "v"(c), "v"(d), "n"(SH));
    return r;
}

// buffer resource over [p, p + 2 GiB): wave-uniform base in SGPRs, 32-bit byte offsets per lane
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7fffffff, 0x00020000);
}
// Lanes that must not touch memory carry this bit in their 32-bit buffer offset: it is past
// num_records of every resource above, so the load returns 0 and the store is dropped by the
// bounds check -- no exec-mask branch around the instruction, and the number of outstanding
// memory operations stays a compile-time constant (precise s_waitcnt counts instead of 0).
constexpr uint32_t kOobBit = 0x80000000u;
// Cache policy of data that is read exactly once (coefficient rows, entry lists): the `nt` bit.
// The reference rows are re-read by neighbouring groups and must keep their place in L1/L2;
// measured +3 % on the bench workload (sc0 / sc1 on the same loads: nothing; nt on the stores: -4 %).
constexpr int kAuxStreamOnce = 2;
// The dense boundary's coefficient rows go from memory straight into the wave's LDS tile (gfx950:
// buffer_load_dwordx4 ... lds; lane i's 16 bytes land at tile + 16 i, the layout stage 1 reads) -- no registers
// in between (four VGPRs held across half a task cost the B path a wave of occupancy) and no ds_write.  The
// compiler does not order LDS reads behind such a load; the waits are explicit (wait_vmem_all) and sit where
// everything outstanding has long arrived: in front of the reference fetches of a task and in front of the
// stores of a half.  Lanes that must not load (kOobBit) get zeros.
__device__ __forceinline__ void coef_rows_to_lds(const void* plane, char* tile, uint32_t voff, uint32_t soff)
{
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(plane);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)tile, 16, (int)voff, (int)soff, 0, kAuxStreamOnce);
}
// every vector memory operation of this wave has completed (loads, LDS-direct loads, stores)
__device__ __forceinline__ void wait_vmem_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void wait_lds_all() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// what the wave's lanes wrote to LDS before is what every lane of the wave reads behind (waves never talk to each other)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a 64-bit field that a geometry struct carries as two dwords (the struct keeps 4-byte alignment)
__host__ __device__ constexpr size_t join64(uint32_t lo, uint32_t hi) { return ((size_t)hi << 32) | lo; }

// lanes whose value is non-zero, as a scalar mask: ONE v_cmp (the ballot builtin on a
// 16-bit-derived compare costs three vector instructions with this compiler)
__device__ __forceinline__ uint64_t lanes_nonzero(int v)
{
    uint64_t m;
    asm("v_cmp_ne_u32_e64 %0, 0, %1" : "=s"(m) : "v"(v));
    return m;
}

// typed load at base + 32-bit byte offset: global_load with an SGPR base and a VGPR offset
template <typename T>
__device__ __forceinline__ T ldg(const LEON_GLOBAL void* base, uint32_t off)
{
    return *(const LEON_GLOBAL T*)((const LEON_GLOBAL char*)base + off);
}

// sign(v) in {-1, 0, 1}
__device__ __forceinline__ int sign3(int v)
{
    int d;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(d) : "v"(v));
    return d;
}
// opaque 24-bit multiply (keeps hipcc from re-deriving 24-bit operand tricks around it)
__device__ __forceinline__ int mul24_asm(int a, int b)
{
    int d;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// GLSL int '/' 256 (truncation toward zero)
__device__ __forceinline__ int div256(int t)
{
    return (int)(__umul24((unsigned)t >> 31, 255u) + (unsigned)t) >> 8;
}

__device__ __forceinline__ int med3i(int v, int lo, int hi) { return min(max(v, lo), hi); }

// n / d by multiply-high with inv = ceil(2^32/d) (0 encodes d == 1); exact for n*d < 2^32
__device__ __forceinline__ int div_inv(int n, uint32_t inv) { return inv ? (int)__umulhi((uint32_t)n, inv) : n; }

// mpeg1video.js:23 / :26 (same text in both passes)
__device__ __forceinline__ void butterfly8(const int (&X)[8], int (&o)[8])
{
    int b1 = X[4];
    int b3 = X[2] + X[6];
    int b4 = X[5] - X[3];
    int tmp1 = X[1] + X[7];
    int tmp2 = X[3] + X[5];
    int b6 = X[1] - X[7];
    int b7 = tmp1 + tmp2;
    int m0 = X[0];
    const int c128 = 128;
    int x4 = div256(mad24k(b6, 473, mad24k(b4, -196, c128))) - b7;
    int x0 = x4 - div256(mad24k(tmp1 - tmp2, 362, c128));
    int x1 = m0 - b1;
    int x2 = div256(mad24k(X[2] - X[6], 362, c128)) - b3;
    int x3 = m0 + b1;
    int y3 = x1 + x2;
    int y4 = x3 + b3;
    int y5 = x1 - x2;
    int y6 = x3 - b3;
    int y7 = -x0 - div256(mad24k(b4, 473, mad24k(b6, 196, c128)));
    o[0] = b7 + y4;
    o[1] = x4 + y3;
    o[2] = y5 - x0;
    o[3] = y6 - y7;
    o[4] = y6 + y7;
    o[5] = x0 + y5;
    o[6] = y3 - x4;
    o[7] = y4 - b7;
}

// The same butterfly with X[2..7] == 0 / X[4..7] == 0 substituted (every dropped term is an exact
// zero: 0*k + 128 divides to 0).  Chosen wave-uniformly when the higher inputs of all 64 lanes
// are zero, which is the common case for quantised video.
__device__ __forceinline__ void butterfly8_lo2(int X0, int X1, int (&o)[8])
{
    const int c128 = 128;
    int x4 = div256(mad24k(X1, 473, c128)) - X1;
    int x0 = x4 - div256(mad24k(X1, 362, c128));
    int y7 = -x0 - div256(mad24k(X1, 196, c128));
    o[0] = X1 + X0;
    o[1] = x4 + X0;
    o[2] = X0 - x0;
    o[3] = X0 - y7;
    o[4] = X0 + y7;
    o[5] = x0 + X0;
    o[6] = X0 - x4;
    o[7] = X0 - X1;
}
__device__ __forceinline__ void butterfly8_lo4(int X0, int X1, int X2, int X3, int (&o)[8])
{
    const int c128 = 128;
    int b7 = X1 + X3;
    int x4 = div256(mad24k(X1, 473, mad24k(X3, 196, c128))) - b7;
    int x0 = x4 - div256(mad24k(X1 - X3, 362, c128));
    int x2 = div256(mad24k(X2, 362, c128)) - X2;
    int y3 = X0 + x2;
    int y4 = X0 + X2;
    int y5 = X0 - x2;
    int y6 = X0 - X2;
    int y7 = -x0 - div256(mad24k(X3, -473, mad24k(X1, 196, c128)));
    o[0] = b7 + y4;
    o[1] = x4 + y3;
    o[2] = y5 - x0;
    o[3] = y6 - y7;
    o[4] = y6 + y7;
    o[5] = x0 + y5;
    o[6] = y3 - x4;
    o[7] = y4 - b7;
}
// dispatch on the number of leading inputs that can be non-zero (wave-uniform)
__device__ __forceinline__ void butterfly8_n(const int (&X)[8], int n_live, int (&o)[8])
{
    if (n_live <= 2) butterfly8_lo2(X[0], X[1], o);
    else if (n_live <= 4) butterfly8_lo4(X[0], X[1], X[2], X[3], o);
    else butterfly8(X, o);
}

// ---- column pass with the last butterfly stage and the hand-off scaling in packed fp32 -----------
// The eight outputs are four (sum, difference) pairs of the same two integers.  Converted to fp32
// (exact: |.| < 2^24 for every input the dequantiser can produce -- DC <= 32767*256, AC <= 2048*62,
// gains < 2 -- so the sums are exact too) they take one v_pk_add_f32 per pair, and the hand-off
// scale by _y = 0.4 one v_pk_mul_f32 per pair: 8 vector instructions less per group than integer
// adds, eight conversions and eight multiplies.
typedef float v2f __attribute__((ext_vector_type(2)));

struct ColOut { v2f p07, p16, p52, p43; };     // (o0,o7) (o1,o6) (o5,o2) (o4,o3)

__device__ __forceinline__ ColOut col_final(int y4, int b7, int y3, int x4, int y5, int x0, int y6, int y7)
{
    const float fy4 = (float)y4, fb7 = (float)b7, fy3 = (float)y3, fx4 = (float)x4;
    const float fy5 = (float)y5, fx0 = (float)x0, fy6 = (float)y6, fy7 = (float)y7;
    ColOut o;
    o.p07 = v2f{fy4, fy4} + v2f{fb7, -fb7};
    o.p16 = v2f{fy3, fy3} + v2f{fx4, -fx4};
    o.p52 = v2f{fy5, fy5} + v2f{fx0, -fx0};
    o.p43 = v2f{fy6, fy6} + v2f{fy7, -fy7};
    return o;
}

__device__ __forceinline__ ColOut butterfly8_col(const int (&X)[8], int n_live)
{
    const int c128 = 128;
    if (n_live <= 2) {
        const int X0 = X[0], X1 = X[1];
        int x4 = div256(mad24k(X1, 473, c128)) - X1;
        int x0 = x4 - div256(mad24k(X1, 362, c128));
        int y7 = -x0 - div256(mad24k(X1, 196, c128));
        return col_final(X0, X1, X0, x4, X0, x0, X0, y7);
    } else if (n_live <= 4) {
        const int X0 = X[0], X1 = X[1], X2 = X[2], X3 = X[3];
        int b7 = X1 + X3;
        int x4 = div256(mad24k(X1, 473, mad24k(X3, 196, c128))) - b7;
        int x0 = x4 - div256(mad24k(X1 - X3, 362, c128));
        int x2 = div256(mad24k(X2, 362, c128)) - X2;
        int y7 = -x0 - div256(mad24k(X3, -473, mad24k(X1, 196, c128)));
        return col_final(X0 + X2, b7, X0 + x2, x4, X0 - x2, x0, X0 - X2, y7);
    } else {
        int b1 = X[4];
        int b3 = X[2] + X[6];
        int b4 = X[5] - X[3];
        int tmp1 = X[1] + X[7];
        int tmp2 = X[3] + X[5];
        int b6 = X[1] - X[7];
        int b7 = tmp1 + tmp2;
        int m0 = X[0];
        int x4 = div256(mad24k(b6, 473, mad24k(b4, -196, c128))) - b7;
        int x0 = x4 - div256(mad24k(tmp1 - tmp2, 362, c128));
        int x1 = m0 - b1;
        int x2 = div256(mad24k(X[2] - X[6], 362, c128)) - b3;
        int x3 = m0 + b1;
        int y7 = -x0 - div256(mad24k(b4, 473, mad24k(b6, 196, c128)));
        return col_final(x3 + b3, b7, x1 + x2, x4, x1 - x2, x0, x3 - b3, y7);
    }
}

// COL_INT_3 (decoders/shaders/mpeg1video.js:21-22) for one coefficient, branch-free.  qO =
// quantiser_scale * matrix entry, pm = premultiplier, nim = -1 for a non-intra block, 0 for an intra
// block.  X*2 (+ sign(X) for non-intra), * qO, floor(./16), even values step toward zero and 0
// becomes +1 (the shader's oddification), clamp to [-2048, 2047], * pm.  A zero coefficient must
// stay zero (the shader's `continue`):
// sign(X) & 1 replaces the constant 1 of the oddification, so X == 0 gives 0*q -> 0 - 0 -> | 0 -> 0
// and every X != 0 gets exactly the reference's arithmetic.
__device__ __forceinline__ int dequant_any(int X, int qO, int pm, int nim, int lo2048, int hi2047)
{
    const int sg = sign3(X);
    int x2 = (X << 1) + (sg & nim);
    int t = mul24_asm(x2, qO);
    int f = t >> 4;
    int z;
    asm("v_med3_i32 %0, %1, 0, 1" : "=v"(z) : "v"(f));   // inline constants: no registers for 0 and 1
    f = (f - z) | (sg & 1);
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(f) : "v"(f), "s"(lo2048), "v"(hi2047));   // one scalar operand is free
    return __mul24(f, pm);
}

// (int)floorf(x) in one instruction
__device__ __forceinline__ int cvt_floor(float x)
{
    int d;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(d) : "v"(x));
    return d;
}

// _B()/_E() int16 hand-off incl. UNORM8 saturation of the high byte (mpeg1video.js:18)
__device__ __forceinline__ int handoff16(int w)
{
    int r = (int)(short)w;                            // |w| < 65536: w mod 2^16
    if (w >= 65536) r = (w & 255) - 256;              // hi byte saturates at 255
    if (w < -65536) r = w & 255;                      // hi byte saturates at 0
    return r;
}

// ---- motion-compensated prediction of 8 horizontally adjacent samples ------

// exact (a+b+c+d+2)>>2 on 4 packed bytes in three v_lerp_u8 (per byte (p + q + (r & 1)) >> 1: the third operand is a
// per-byte rounding bit) and one xor.  With sa = a+b = 2x+rx, sc = c+d = 2y+ry:
//   (sa + sc + 2) >> 2 = (x + y + 1 + (rx & ry)) >> 1,   and   (a + b + ry) >> 1 = x + (rx & ry)   (ry = LSB of c ^ d)
// so X = lerp(a, b, c ^ d), y = lerp(c, d, 0), result = lerp(X, y, 1).  (Round 1 had three rounded-up averages and a
// five-instruction fix-up: twice the instructions.)
__device__ __forceinline__ uint32_t avg4_u8x4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t X = __builtin_amdgcn_lerp(a, b, c ^ d);
    const uint32_t y = __builtin_amdgcn_lerp(c, d, 0u);
    return __builtin_amdgcn_lerp(X, y, 0x01010101u);
}

// reference texel addressing: sample x lives in RGBA texel x>>2, component x&3; the
// TEXEL index clamps to the edge (jsv.js:216-217 + _p() mpeg1video.js:24)
__device__ __forceinline__ uint32_t ref_px_clamped(const LEON_GLOBAL uint8_t* ref, uint32_t row_off, int W, int x)
{
    int t = min(max(x >> 2, 0), (W >> 2) - 1);
    return ldg<uint8_t>(ref, row_off + (uint32_t)(4 * t + (x & 3)));
}

typedef v3u U3 __attribute__((aligned(4)));    // 12 bytes that are only dword aligned

// raw reference bytes of one predictor: two rows of 12 bytes starting at the aligned
// address below the window, plus the byte shift of the window inside them
struct RefRows {
    uint32_t l0, l1, l2;        // row y+ay
    uint32_t m0, m1, m2;        // row y+ay+oddv
    uint32_t s;                 // window starts at byte s (0..3)
    uint32_t oh;                // horizontal half-pel flag
};

// 9 samples px..px+8 of one row, for vectors that leave the picture (rare, divergent)
__device__ __forceinline__ void gather9_slow(const LEON_GLOBAL uint8_t* ref, uint32_t row_off, int W, int px,
                                             uint32_t& a0, uint32_t& a1, uint32_t& a2)
{
    uint32_t lo = 0, hi = 0;
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        lo |= ref_px_clamped(ref, row_off, W, px + k) << (8 * k);
        hi |= ref_px_clamped(ref, row_off, W, px + 4 + k) << (8 * k);
    }
    a0 = lo;
    a1 = hi;
    a2 = ref_px_clamped(ref, row_off, W, px + 8);
}

// Issue the loads of one predictor: rows y+ay and y+ay+ov, window columns px..px+8.
// px / oh / ov / in_pic come from the task prologue (shared by both halves).
// The lanes (n, b) and (n+1, b) belong to the same block, hence to the same vector: the lower
// row of lane n IS the upper row of lane n+1.  Only the upper row is fetched by every lane;
// the ninth row of a block is fetched by its n == 7 lanes alone (all other lanes carry the
// out-of-range offset, which costs no cache access), and finish_rows() moves the rest
// between lanes.  That halves the L1 accesses of the reference fetch.
__device__ __forceinline__ int clamp_med3(int v, int hi)      // min(max(v, 0), hi) in one instruction
{
    int d;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(d) : "v"(v), "s"(hi));
    return d;
}

// `use` = this lane's macroblock predicts from this reference at all (B pictures: direction map);
// a lane that does not carries the out-of-range offset: no cache access, zeros come back, and
// recon_task() replaces the unused predictor by the other one.
// (The offset of a lane that must not fetch is kOobBit itself, by a select: ADDING the bit to the offset -- tried in round 4
// to save the select -- is wrong for a lane whose unused vector is garbage: its window column is then anything, and the
// sum wraps back into the 2 GiB the resource covers: a real load far outside the allocation.)
__device__ __forceinline__ RefRows fetch_rows(const LEON_GLOBAL uint8_t* ref, int W, int H, int y,
                                              int px, int ay, int oh, int ov, bool in_pic, bool last_row, bool use)
{
    const int yy = y + ay;
    const uint32_t r0 = (uint32_t)__mul24(clamp_med3(yy, H - 1), W);
    // the row below: one line further unless the clamp holds both rows on the same edge line
    const uint32_t r1 = r0 + ((uint32_t)yy < (uint32_t)(H - 1) ? (uint32_t)W : 0u);
    RefRows R;
    R.oh = (uint32_t)oh;
    R.m0 = R.m1 = R.m2 = 0;
    if (in_pic) {
        R.s = (uint32_t)px & 3u;
        uint32_t xo = (uint32_t)px & ~3u;
        // buffer loads: wave-uniform descriptor in SGPRs + 32-bit offset, no 64-bit address math
        const __amdgpu_buffer_rsrc_t rs = buf_rsrc((const void*)ref);
        const v3u a = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(use ? r0 + xo : kOobBit), 0, 0);
        const v3u c = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)(use && last_row && ov ? r1 + xo : kOobBit), 0, 0);
        R.l0 = a.x; R.l1 = a.y; R.l2 = a.z;
        R.m0 = c.x; R.m1 = c.y; R.m2 = c.z;
    } else {                                         // vector leaves the picture (rare)
        R.s = 0;
        gather9_slow(ref, r0, W, px, R.l0, R.l1, R.l2);
        if (last_row && ov) gather9_slow(ref, r1, W, px, R.m0, R.m1, R.m2);
    }
    return R;
}

// second half of fetch_rows: the lower row comes from the lane 8 above (same block, next sample
// row) -- or from the lane itself when the vector has no vertical half-pel part
// `below` (luma, upper half): the half underneath belongs to the same macroblocks, its first row IS the ninth row of this one -- same
// vector, same clamped row address (fetch_rows: r1 of row y equals r0 of row y + 1 at every edge) -- so the upper half fetches no ninth
// row of its own: its last lanes take it from the lower half's first lanes ((lane + 8) & 63 is that lane).
__device__ __forceinline__ void finish_rows(RefRows& R, int ov, bool last_row, int lane, const RefRows* below = nullptr)
{
    const int src = (ov ? ((lane + 8) & 63) : lane) << 2;
    const uint32_t n0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)R.l0);
    const uint32_t n1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)R.l1);
    const uint32_t n2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)R.l2);
    if (below) {
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)below->l0);
        const uint32_t b1 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)below->l1);
        const uint32_t b2 = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)below->l2);
        const bool wrap = last_row && ov;
        R.m0 = wrap ? b0 : n0; R.m1 = wrap ? b1 : n1; R.m2 = wrap ? b2 : n2;
        return;
    }
    if (!(last_row && ov)) { R.m0 = n0; R.m1 = n1; R.m2 = n2; }
}

// (a+b+c+d+2)>>2 / (a+b+1)>>1 / a, selected by the half-pel flags through operand
// duplication: a==b when !oh (shift 0), rows equal when !ov (same row fetched twice)
__device__ __forceinline__ v2u predict8(const RefRows& R)
{
    uint32_t a0 = __builtin_amdgcn_alignbyte(R.l1, R.l0, R.s);
    uint32_t a1 = __builtin_amdgcn_alignbyte(R.l2, R.l1, R.s);
    uint32_t a2 = __builtin_amdgcn_alignbyte(0u, R.l2, R.s);
    uint32_t c0 = __builtin_amdgcn_alignbyte(R.m1, R.m0, R.s);
    uint32_t c1 = __builtin_amdgcn_alignbyte(R.m2, R.m1, R.s);
    uint32_t c2 = __builtin_amdgcn_alignbyte(0u, R.m2, R.s);
    uint32_t b0 = __builtin_amdgcn_alignbyte(a1, a0, R.oh);
    uint32_t b1 = __builtin_amdgcn_alignbyte(a2, a1, R.oh);
    uint32_t d0 = __builtin_amdgcn_alignbyte(c1, c0, R.oh);
    uint32_t d1 = __builtin_amdgcn_alignbyte(c2, c1, R.oh);
    v2u p;
    p.x = avg4_u8x4(a0, b0, c0, d0);
    p.y = avg4_u8x4(a1, b1, c1, d1);
    return p;
}

// byte M of `pred` moved to bits 8..15 (so that it adds as pred*256), one v_perm_b32
template <int M>
__device__ __forceinline__ uint32_t pred_x256(uint32_t pred)
{
    // selector bytes: 0x0c = constant 0x00; 0..3 pick bytes of the second operand.  The selector
    // rides in a scalar register (a VOP3 instruction may read one): the builtin makes the compiler
    // re-materialise it in a vector register in front of every group of uses.
    uint32_t d;
    asm("v_perm_b32 %0, 0, %1, %2" : "=v"(d) : "v"(pred), "s"(0x0c0c000cu | ((uint32_t)M << 8)));
    return d;
}

// ---- one task = two block groups that share their macroblocks ------------------------
//   luma  : the upper and lower 64x8 halves of four macroblocks (block rows 2*Rt, 2*Rt+1)
//   chroma: the Cb and the Cr group at block row Rt
// Everything that depends only on the macroblock -- maps, vectors and their half-pel
// decomposition, quantiser tables, the in-picture test -- is computed once per task.

// Fused display conversion (DISPLAY): the picture leaves the kernel as RGBA8 as well -- the CPU twin of
// the reference's conversion, bit for bit what k_rgba_twin4 below computes in fp64 (here from exact fixed-point
// tables, see rgba_px) -- so the planes of a picture nobody predicts from (B pictures: 8 of 12 in IBBP) are never written and never
// read back, and the others are not read back.  A task then covers 8 macroblocks completely: first the
// chroma part (CHROMA = true: the Cb and Cr groups, whose samples are parked in an LDS stash), then the
// two luma parts (CHROMA = false, 4 macroblocks each), whose lanes hold 8 horizontally adjacent Y samples
// and find their 4 Cb and 4 Cr samples in the stash.
struct Display {
    char* stash;                 // LDS: [Cb | Cr][8 rows][64 bytes]
    int side;                    // luma parts: 0 / 1 = left / right four macroblocks of the chroma group
    char* apark;                 // yuva: the A samples of the four macroblocks, [half][8 rows][64 bytes]
    const char* lut;             // LDS copy of Tables::rgba_lut (the workgroup's)
    uint8_t* planes;             // OUT != kOutRgba: the picture's frame planes (FrameOut), else null
    const struct FrameOut* fo;
};
// AMODE of recon_task in a yuva display task: the A part runs before the Y part of the same four macroblocks
// and parks its samples (kAlphaPark); the Y part's conversion takes its alpha bytes from there (kAlphaTake); kAlphaNone otherwise.
static constexpr int kAlphaNone = 0, kAlphaPark = 1, kAlphaTake = 2;

// byte i of a packed dword, times 2^sh: one v_lshlrev_b32_sdwa (table addresses from packed samples)
template <int I>
__device__ __forceinline__ uint32_t byte_shl(uint32_t v, uint32_t sh)
{
    uint32_t d;
    if constexpr (I == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(d) : "v"(sh), "v"(v));
    else if constexpr (I == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(d) : "v"(sh), "v"(v));
    else if constexpr (I == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(d) : "v"(sh), "v"(v));
    else asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(d) : "v"(sh), "v"(v));
    return d;
}

// The reference's YCbCrToRGBA (player/easybits.player.js:2692-2782) on fixed-point tables: every term of
//   R = store(r(Cr) + ys(Y)), G = store((g1(Cr) - g2(Cb)) + ys(Y)), B = store(b(Cb) + ys(Y))
// (store = Uint8ClampedArray: clamp, round half to even) comes out of an LDS table with 21 fractional bits,
// the sum is shifted, clamped and packed by v_ashr_pk_u8_i32 -- and equals the fp64 arithmetic for all 2^24
// inputs (tools/make_rgba_lut.py explains why and checks it; tests/test_rgba_lut.py, and the exhaustive GPU
// test in tests/test_fused_display_gpu.py).  7 vector instructions per pixel instead of 20 in fp64.
struct ChromaTerms { int r, g, b; };
template <int I>
__device__ __forceinline__ ChromaTerms chroma_terms(const char* lut, uint32_t cb2, uint32_t cr2, uint32_t three)
{
    const v2u rc = *reinterpret_cast<const v2u*>(lut + 1024 + byte_shl<I>(cr2, three));     // {r, g1}[Cr]
    const v2u bc = *reinterpret_cast<const v2u*>(lut + 3072 + byte_shl<I>(cb2, three));     // {b, -g2}[Cb]
    return ChromaTerms{(int)rc.x, (int)(rc.y + bc.y), (int)bc.x};
}
template <int I>
__device__ __forceinline__ uint32_t rgba_px(const char* lut, uint32_t y4, const ChromaTerms& c, int a_fixed, uint32_t two)
{
    const int ys = *reinterpret_cast<const int*>(lut + byte_shl<I>(y4, two));
    // {sat_u8(a >> 21), sat_u8(b >> 21)} go to the low half of the destination, and -- op_sel[3] -- of the second
    // instruction to the high half, the other half left alone: R G B A packed by the two shifts themselves (no byte
    // permute behind them).  Through asm: the builtin knows neither the half-selecting form nor that the other half stays.
    uint32_t px;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "=v"(px) : "v"(ys + c.r), "v"(ys + c.g), "n"(kLutShift));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(px) : "v"(ys + c.b), "v"(a_fixed), "n"(kLutShift));
    return px;
}
// 4 horizontally adjacent pixels of one row: Y samples y4, the two chroma pairs' terms, A samples a4
template <bool ALPHA>
__device__ __forceinline__ v4u rgba_row4(const char* lut, uint32_t y4, const ChromaTerms& c0, const ChromaTerms& c1, uint32_t a4,
                                         uint32_t two, uint32_t k21)
{
    const int opaque = 255 << kLutShift;
    int a[4] = {opaque, opaque, opaque, opaque};
    if constexpr (ALPHA) {
        a[0] = (int)byte_shl<0>(a4, k21); a[1] = (int)byte_shl<1>(a4, k21);
        a[2] = (int)byte_shl<2>(a4, k21); a[3] = (int)byte_shl<3>(a4, k21);
    }
    return v4u{rgba_px<0>(lut, y4, c0, a[0], two), rgba_px<1>(lut, y4, c0, a[1], two),
               rgba_px<2>(lut, y4, c1, a[2], two), rgba_px<3>(lut, y4, c1, a[3], two)};
}

// ---- stage 5 (fused display conversion): RGBA of one half (64 x 8 samples) of a luma part ---------------
// A lane of recon_task holds samples 8b .. 8b+7 of row n; converted as they lie, a store instruction would
// write 16-byte pieces 32 bytes apart (half-filled lines) and the two rows that share a chroma row would
// sit in different lanes.  So the rows went through LDS (`ypark`: [8 rows][64 bytes], written at the end of
// the half and ordered by the fences there) and lane (n, b) converts the pixel quad j = 2b + (n & 1) of the
// row pair p = n >> 1: pixels 4j .. 4j+3 of rows 2p and 2p+1, whose chroma terms it looks up once; a store
// instruction writes 256 contiguous bytes of each of four rows = full 128-byte lines.
template <int AMODE>
__device__ __forceinline__ void display_half(const PicDesc& pd, const Geom& G, const Display& dsp, const char* ypark,
                                             int half, int Rt, int g, int hi3, int lo3)
{
    const int pr = hi3 >> 1, jq = 2 * lo3 + (hi3 & 1);
    const int xa = 64 * g + 4 * jq;                            // first pixel of the lane's quad
    const __amdgpu_buffer_rsrc_t rrs = buf_rsrc(pd.rgba);
    uint32_t two = 2u, three = 3u, k21 = (uint32_t)kLutShift;  // SDWA shift counts live in registers
    asm("" : "+v"(two), "+v"(three));
    if constexpr (AMODE == kAlphaTake) asm("" : "+v"(k21));
    const int yrow = 8 * (2 * Rt + half) + 2 * pr;
    // chroma: row y>>1 = stash row 4*half + p; the quad's two chroma samples are bytes 32*side + 2j, + 1
    const char* yp = ypark + pr * 128 + jq * 4;
    const char* sp = dsp.stash + (4 * half + pr) * 64 + 32 * dsp.side + 2 * jq;
    const uint32_t ya = *reinterpret_cast<const uint32_t*>(yp), yb = *reinterpret_cast<const uint32_t*>(yp + 64);
    const uint32_t cb2 = *reinterpret_cast<const uint16_t*>(sp), cr2 = *reinterpret_cast<const uint16_t*>(sp + 512);
    uint32_t aa = 0u, ab = 0u;                             // yuva: the pixels' A samples, parked by the A part
    if constexpr (AMODE == kAlphaTake) {
        const char* ap = dsp.apark + half * 512 + pr * 128 + jq * 4;
        aa = *reinterpret_cast<const uint32_t*>(ap);
        ab = *reinterpret_cast<const uint32_t*>(ap + 64);
    }
    const ChromaTerms c0 = chroma_terms<0>(dsp.lut, cb2, cr2, three), c1 = chroma_terms<1>(dsp.lut, cb2, cr2, three);
    // the frame is the top-left crop of the coded picture; its width is a multiple of 8 (host check)
    const uint32_t row_off = __umul24((uint32_t)yrow, (uint32_t)G.fw) + (uint32_t)xa;     // both < 4096
    const bool in_a = yrow < G.fh && xa < G.fw, in_b = yrow + 1 < G.fh && xa < G.fw;
    const v4u pa = rgba_row4<AMODE == kAlphaTake>(dsp.lut, ya, c0, c1, aa, two, k21);
    __builtin_amdgcn_raw_buffer_store_b128(pa, rrs, (int)((row_off * 4u) | (in_a ? 0u : kOobBit)), 0, kAuxFrameStore);
    const v4u pb = rgba_row4<AMODE == kAlphaTake>(dsp.lut, yb, c0, c1, ab, two, k21);
    __builtin_amdgcn_raw_buffer_store_b128(pb, rrs, (int)(((row_off + (uint32_t)G.fw) * 4u) | (in_b ? 0u : kOobBit)), 0, kAuxFrameStore);
}

// ---- stage 2 as functions: the liveness scan of a tile and the column pass over a list of live columns ------------------------
// A column id: tile << 7 | half << 6 | c << 3 | b.  scan_tile: lane (c = hi3, b = lo3) looks at its own column of each half of
// `tile`; the live lanes queue up behind the n_before ids that are in the list already.  Returns the new length.
__device__ __forceinline__ uint32_t scan_tile(const char* tile, char* ids, int lane, uint32_t tag, uint32_t n_before, uint64_t (&live)[2], int half_step = kLdsHalf)
{
    const int hi3 = lane >> 3, lo3 = lane & 7;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const char* cp = tile + h * half_step + lo3 * 16 + hi3 * 2;
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) o |= *reinterpret_cast<const uint16_t*>(cp + i * 128);
        live[h] = lanes_nonzero((int)o);
        const uint32_t pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(live[h] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)live[h], n_before));
        if (o != 0u) *reinterpret_cast<uint8_t*>(ids + pos) = (uint8_t)(tag + (uint32_t)lane + 64u * h);
        n_before += (uint32_t)__builtin_popcountll(live[h]);
    }
    return n_before;
}

// The column pass (COL_INT_3 / COL_INT_5, decoders/shaders/mpeg1video.js:19-24) over the n_cols live columns listed in `ids`:
// lane k takes the k-th; the results replace the coefficients in place.  PAIR: ids may name the second tile (tile0 + tile_step),
// whose blocks' quantiser scale and intra flag sit in qia1 (lane b: block b's) as the first tile's in qia0.
// TLDS: the tables are the wave's LDS copy at `qtab`; else they are in `qreg`: the picture's QTables, 256 bytes, dword i in lane i
// -- a lane fetches the two dwords of its column's matrix row and of its premultiplier row with four ds_bpermute.  (Until the end of
// round 4 the two-tile layout, which has no room for the tables in LDS, read them from memory inside this loop: two loads and an
// `s_waitcnt vmcnt(0)` per round -- and loads return in order: the chroma part's wait for its tables was a wait for the REFERENCE
// rows it had requested just before, whose flight the column pass was meant to cover.)
// Three tiles (FRONT3 tasks): the list holds the chroma tile's columns first (n_c of them), then the left luma tile's (up to n_cl),
// then the right one's; ids carry no tile bits -- a column's tile follows from its place in the list.
struct ThreeTiles {
    uint32_t c_off;              // from tile0 to the chroma tile's first KB (its second: + kSfCHalf); tile0 / tile0 + tile_step are the luma tiles
    uint32_t n_c, n_cl;
    uint32_t flags;              // MbCarry::flags of the chroma part: lane m holds macroblock m of the task
};
template <bool PAIR, bool TLDS = true, bool THREE = false>
__device__ __forceinline__ void column_pass(char* tile0, uint32_t tile_step, const char* ids, const char* qtab, uint32_t n_cols, int qia0, int qia1, int lane,
                                            uint32_t qreg = 0u, const ThreeTiles& t3 = ThreeTiles())
{
    // the clamp bounds live in registers (v_med3 takes no literals on gfx950, and the compiler would
    // otherwise re-materialise them in front of every use): one scalar, one vector -- a VOP3
    // instruction may read one scalar register
    int lo2048 = -2048, hi2047 = 2047;
    asm("" : "+s"(lo2048), "+v"(hi2047));
#pragma unroll 1
    for (uint32_t base = 0; base < n_cols; base += 64u) {             // wave-uniform: once, twice for busy I pictures
        const uint32_t k = base + (uint32_t)lane;
        const bool act = k < n_cols;
        uint32_t id = *reinterpret_cast<const uint8_t*>(ids + k);
        id = act ? id : 0u;                               // idle lanes redo column 0 and write nothing
        char* colp = tile0 + ((id & 0x47u) << 4) + ((id >> 2) & 14u);
        if constexpr (PAIR) colp += (id >> 7) * tile_step;
        int bq;
        if constexpr (THREE) {
            const bool in_c = k < t3.n_c, in_r = k >= t3.n_cl;
            // (the half bit of a chroma id steps kSfCHalf, not kLdsHalf)
            uint32_t off = in_c ? t3.c_off + (id & 64u) * (uint32_t)((kSfCHalf - kLdsHalf) / 64) : (in_r ? tile_step : 0u);
            off += ((id & 0x47u) << 4) + ((id >> 2) & 14u);
            // idle lanes redo the column of lane 0 (the first of the round: always live) and write nothing
            colp = tile0 + (act ? off : (uint32_t)__builtin_amdgcn_readfirstlane((int)off));
            // chroma block b: macroblock b; luma block b: macroblock b >> 1 of its side
            const uint32_t b = id & 7u, m = in_c ? b : (b >> 1) + (in_r ? 4u : 0u);
            bq = __builtin_amdgcn_ds_bpermute((int)(m << 2), (int)t3.flags) & 0x11f;
        }
        int X[8];
#pragma unroll
        for (int i = 0; i < 8; i++) X[i] = *reinterpret_cast<const short*>(colp + i * 128);
        if constexpr (!THREE) bq = __builtin_amdgcn_ds_bpermute((int)((id & 7u) << 2), qia0);      // lane b holds block b's macroblock
        if constexpr (PAIR) {
            const int bq1 = __builtin_amdgcn_ds_bpermute((int)((id & 7u) << 2), qia1);
            bq = (id & 128u) ? bq1 : bq;
        }
        const bool bia = bq >= 256;
        const uint32_t qv = (uint32_t)bq & 31u;
        v2u msel, pm8;                                                               // column c of the tables
        if constexpr (TLDS) {
            const char* const qt = qtab + (id & 56u);
            msel = *reinterpret_cast<const v2u*>(qt + (bia ? 0 : 64));
            pm8 = *reinterpret_cast<const v2u*>(qt + 128);
        } else {
            const int qo = (int)((id & 56u) + (bia ? 0u : 64u)), po = (int)((id & 56u) + 128u);      // byte offsets = 4 x the lane that holds the dword
            msel.x = (uint32_t)__builtin_amdgcn_ds_bpermute(qo, (int)qreg);
            msel.y = (uint32_t)__builtin_amdgcn_ds_bpermute(qo + 4, (int)qreg);
            pm8.x = (uint32_t)__builtin_amdgcn_ds_bpermute(po, (int)qreg);
            pm8.y = (uint32_t)__builtin_amdgcn_ds_bpermute(po + 4, (int)qreg);
        }
        int nim = bia ? 0 : -1;
        asm("" : "+v"(nim));                              // keep it a mask (v_and), not a select
        const bool dc_lane = bia && (id & 56u) == 0u;
        uint64_t nz[8];
#pragma unroll
        for (int i = 0; i < 8; i++) nz[i] = lanes_nonzero(X[i]);
        const int dc = X[0];
        int rows_live = 1;                                // wave-uniform: 1 + highest row with a non-zero
#pragma unroll
        for (int i = 0; i < 8; i++) {
            // a row whose coefficients are zero in every column of the pass costs its compare and a scalar
            // branch; in a live row every lane runs the branch-free form (zeros stay zero)
            if (nz[i] != 0) {
                rows_live = i + 1;
                int P = (int)(((i < 4 ? pm8.x : pm8.y) >> (8 * (i & 3))) & 255u);
                const int qO = (int)__umul24(qv, ((i < 4 ? msel.x : msel.y) >> (8 * (i & 3))) & 255u);   // quantiser_scale * Q[i][c] < 2^13
                X[i] = dequant_any(X[i], qO, P, nim, lo2048, hi2047);
            }
        }
        if (dc_lane) X[0] = dc * 256;                     // COL_4 / COL_INT_31
        const ColOut co = butterfly8_col(X, rows_live);
        // floor( float(v) * _y ): the int16 the reference hands from pass 1 to pass 2
        const v2f k04 = {0.4f, 0.4f};
        const v2f s07 = co.p07 * k04, s16 = co.p16 * k04, s52 = co.p52 * k04, s43 = co.p43 * k04;
        // floor and conversion in one instruction (v_cvt_flr_i32_f32)
        int wi[8] = {cvt_floor(s07.x), cvt_floor(s16.x), cvt_floor(s52.y), cvt_floor(s43.y),
                     cvt_floor(s43.x), cvt_floor(s52.x), cvt_floor(s16.y), cvt_floor(s07.y)};
        // |s| < 32768 for all eight: every floor(s) is an int16 as it stands
        const float mx = fmaxf(fmaxf(fmaxf(fabsf(s07.x), fabsf(s16.x)), fmaxf(fabsf(s52.y), fabsf(s43.y))),
                               fmaxf(fmaxf(fabsf(s43.x), fabsf(s52.x)), fmaxf(fabsf(s16.y), fabsf(s07.y))));
        if (mx >= 32768.0f) {                             // outside any real stream: int16 wrap / saturation
#pragma unroll
            for (int n = 0; n < 8; n++) wi[n] = handoff16(wi[n]);
        }
        if (act) {
#pragma unroll
            for (int n = 0; n < 8; n++) *reinterpret_cast<short*>(colp + n * 128) = (short)wi[n];
        }
    }
}

// CARRY (display tasks): the eight macroblocks of a task are looked up in the maps ONCE, by its chroma part (1: lane
// (., m) loads macroblock m's quantiser scale, flags and vectors as always and leaves them in `carry`); the luma and
// alpha parts (2) take theirs from the lane of their macroblock by ds_bpermute -- no loads, no second wait for memory
// in front of their reference fetches.  0: a task on its own loads what it needs.
struct MbCarry { uint32_t flags; };       // q | intra << 8 | repadd >= 128 << 9 | direction << 10 (the vectors: LDS, kOffCarry)
static constexpr int kCarryNone = 0, kCarryLeave = 1, kCarryTake = 2;

// What a recon_task instantiation is: a variant type with these constants.  BACK (dense display tasks whose two luma parts share
// their front, recon_luma_pair): the part's coefficients are in TaskArgs::tile and have been through the column pass already;
// TaskArgs::live says which of its columns were live.
template <int TYPE_, bool SPARSE_> struct PlainLuma {               // a task of k_recon, on its own: luma, or the A plane of a yuva picture (TaskArgs{true})
    static constexpr int TYPE = TYPE_, AMODE = kAlphaNone, CARRY = kCarryNone, LAYOUT = 0, OUT = kOutRgba; static constexpr bool SPARSE = SPARSE_, CHROMA = false, DISPLAY = false, BACK = false, FRONT3 = false;
};
template <int TYPE, bool SPARSE> struct PlainChroma : PlainLuma<TYPE, SPARSE> { static constexpr bool CHROMA = true; };
// the parts of a display task (display_task), in the order they run
template <int TYPE, bool SPARSE, int LAYOUT_, int OUT_> struct DisplayChroma : PlainChroma<TYPE, SPARSE> {         // looks the task's macroblocks up and leaves them to the others
    static constexpr int CARRY = kCarryLeave, LAYOUT = LAYOUT_, OUT = OUT_; static constexpr bool DISPLAY = true;
};
template <int TYPE, bool SPARSE, int OUT_> struct DisplayLuma : PlainLuma<TYPE, SPARSE> {             // four macroblocks' Y, converted right away
    static constexpr int CARRY = kCarryTake, OUT = OUT_; static constexpr bool DISPLAY = true;
};
template <int TYPE, bool SPARSE, int OUT> struct YuvaAPart : DisplayLuma<TYPE, SPARSE, OUT> { static constexpr int AMODE = kAlphaPark; };
template <int TYPE, bool SPARSE, int OUT> struct YuvaYPart : DisplayLuma<TYPE, SPARSE, OUT> { static constexpr int AMODE = kAlphaTake; };
template <int TYPE, int OUT, int LAYOUT_ = 1> struct PairBackHalf : DisplayLuma<TYPE, false, OUT> { static constexpr int LAYOUT = LAYOUT_; static constexpr bool BACK = true; };
// FRONT3 (front3_task: dense B display tasks, layout 2): the chroma part requests the coefficient rows of the task's three tiles, scans them into
// one list of live columns and runs ONE column pass over it; the luma parts are back halves (TaskArgs::live_lr: their live columns)
template <int TYPE> struct Front3Chroma : DisplayChroma<TYPE, false, 2, kOutRgba> { static constexpr bool FRONT3 = true; };

struct TaskArgs {                // what only a few callers of recon_task set
    // a luma-shaped task of k_recon reconstructs the A plane of a yuva picture (wave-uniform; a display task's A part is one by
    // its variant) -- the same code path as luma with its own coefficient plane, the plane behind Cr in every slot, and the alpha
    // groups of the sparse lists
    bool alpha = false;
    char* tile = nullptr;        // BACK: the part's tile
    uint64_t live[2] = {0, 0};   // BACK: its live columns, per half
    uint32_t qreg = 0u;          // layout 1: the quantiser tables, dword i in lane i (column_pass)
    // layout 2: the wave's places in the workgroup's array besides its luma tiles (`lds`: left, + kLdsTile: right)
    char* carry = nullptr;       // the task's vectors, 64 bytes
    char* ids = nullptr;         // FRONT3: the column ids, kSfIdsPerWave bytes
    bool has_right = false;      // FRONT3: the task has a right luma part
    uint64_t (*live_lr)[2] = nullptr;      // FRONT3: the live columns of the left and the right luma tile come back here
    bool lut_barrier = false;    // BACK: the task's first conversion is this part's -- the workgroup's barrier in front of the tables stands here
};

// stage 2: column pass over the LIVE columns of both halves
// A column (half, block, c) without a coefficient gives eight zeros, and zeros are what it holds already.
// Quantised video leaves few columns alive (one in ten in P and B pictures, a third in I pictures), so
// the lanes first find the live ones -- lane (c = hi3, b = lo3) looks at its own column of each half --
// and the wave then runs the pass on them alone, usually in one go for both halves instead of one go
// per half with most lanes computing zeros.  The results replace the coefficients in place.
template <int LAYOUT>
__device__ __forceinline__ void column_front(const PicDesc& pd, char* lds, char* tile, int lane, int qia, uint32_t qreg, uint64_t (&live)[2])
{
    const uint32_t n_cols = scan_tile(tile, lds + Lay<LAYOUT>::slots, lane, 0u, 0u, live);
    wave_sync();
    column_pass<false, Lay<LAYOUT>::tables_in_lds>(tile, 0u, lds + Lay<LAYOUT>::slots, Lay<LAYOUT>::tables_in_lds ? lds + kOffQtab : reinterpret_cast<const char*>(pd.qt),
                                                   n_cols, qia, qia, lane, qreg);
    wave_sync();
}

template <typename V>
__device__ __forceinline__ void recon_task(const PicDesc& pd, const Geom& G, int Rt, int g, char* lds, int lane, Display dsp, MbCarry& carry, const TaskArgs& args = TaskArgs())
{
    constexpr int TYPE = V::TYPE, AMODE = V::AMODE, CARRY = V::CARRY, LAYOUT = V::LAYOUT, OUT = V::OUT;
    constexpr bool CHROMA = V::CHROMA, SPARSE = V::SPARSE, DISPLAY = V::DISPLAY, BACK = V::BACK;
    constexpr bool FRONT3 = V::FRONT3;
    static_assert(!BACK || (LAYOUT != 0 && CARRY == kCarryTake), "a back half runs on the two- and three-tile layouts behind the chroma part");
    static_assert(FRONT3 == (LAYOUT == 2 && CHROMA), "the chroma part of the three-tile layout runs the front");
    const bool alpha = AMODE == kAlphaPark || args.alpha;
    // FRONT3: the chroma tile's first KB (args.tile), its second kSfCHalf behind it
    char* const tile = BACK || FRONT3 ? args.tile : lds;
    constexpr int tile_half = FRONT3 ? kSfCHalf : kLdsHalf;
    char* const carryp = LAYOUT == 2 ? args.carry : lds + Lay<LAYOUT == 2 ? 1 : LAYOUT>::carry;
    const int W = CHROMA ? G.cw >> 1 : G.cw;
    const int H = CHROMA ? G.ch >> 1 : G.ch;
    const int bw = W >> 3;
    const uint32_t ysz = (uint32_t)G.cw * (uint32_t)G.ch;
    const uint32_t a_off = !CHROMA && alpha ? ysz + (ysz >> 1) : 0u;       // byte offset of the A plane in a slot
    const int hi3 = lane >> 3, lo3 = lane & 7;

    // ---- shared prologue ----------------------------------------------------------------
    const int Qld = g * 8 + lo3;                      // stage-1 role: lane (r = hi3, b = lo3)
    const bool ld_ok = Qld < bw;
    // afterwards: lane (n = hi3, b = lo3) in the row pass and behind it: the 8 lanes of an aligned
    // group hold the 8 blocks of ONE sample row, so the reference fetches and the stores of a group are
    // contiguous along a picture row and the texture addresser merges them into 64-byte accesses (with
    // rows across adjacent lanes every lane was its own L1 access, and the vector L1 -- one access per
    // clock -- was the limiter)
    const int b = lo3;
    const int Qb = g * 8 + b;
    const bool valid = Qb < bw;
    const int Qs = valid ? Qb : bw - 1;
    // everything that does not depend on the macroblock maps is requested first: the coefficient rows of
    // BOTH halves (dense boundary: straight into the tile) or the first entries of both runs (sparse)
    const int R0 = CHROMA ? Rt : 2 * Rt;
    const uint32_t coef_voff = (2u * ((uint32_t)__mul24(8 * R0 + hi3, W) + (uint32_t)(8 * Qld))) | (ld_ok ? 0u : kOobBit);
    const uint32_t half_step = CHROMA ? 0u : 8u * (uint32_t)W;   // luma: next block row; chroma: next plane
    // sparse boundary: the two groups of the task are two runs of entries[]; the first 64
    // entries of each are requested here (one dword per lane), longer runs loop in stage 1
    uint32_t ent_first[2] = {0u, 0u}, ent_start[2] = {0u, 0u}, ent_count[2] = {0u, 0u};
    // a resource of exactly n_entries dwords: indices past the list read 0, whatever grp_off says
    const __amdgpu_buffer_rsrc_t ent_rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(SPARSE ? pd.entries : nullptr), 0, SPARSE ? (int)(pd.n_entries * 4u) : 0, 0x00020000);
    if constexpr (SPARSE) {
        const uint32_t nY = 2u * (uint32_t)G.tasksY, nC = (uint32_t)G.tasksC;
        const uint32_t gid0 = CHROMA ? nY + (uint32_t)(Rt * G.gC + g) : (uint32_t)(2 * Rt * G.gY + g) + (alpha ? nY + 2u * nC : 0u);
        const uint32_t gid1 = CHROMA ? gid0 + nC : gid0 + (uint32_t)G.gY;
        const LEON_GLOBAL uint32_t* go = gptr(pd.grp_off);    // wave-uniform index; global, not flat: a flat load counts on the LDS counter too
        const uint32_t gid[2] = {gid0, gid1};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t s0 = go[gid[h]], e0 = go[gid[h] + 1];
            ent_start[h] = s0;
            ent_count[h] = e0 > s0 ? min(e0 - s0, 512u) : 0u;      // a group holds at most 8*64 coefficients
            ent_first[h] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                ent_rs, (int)(((s0 + (uint32_t)lane) * 4u) | ((uint32_t)lane < ent_count[h] ? 0u : kOobBit)), 0, kAuxStreamOnce);
        }
    } else if constexpr (!BACK) {
        // the previous task of this wave may still be reading the tile
        wait_lds_all();
        __builtin_amdgcn_wave_barrier();
        if constexpr (FRONT3) {
            coef_rows_to_lds(pd.coef[1], tile, coef_voff, 0u);
            coef_rows_to_lds(pd.coef[2], tile + kSfCHalf, coef_voff, 0u);
            // the luma parts' rows: lane (r = hi3, b = lo3) as above, 16 block columns per chroma group, the lower block row 8 W samples on
            const uint32_t row_off = (uint32_t)__mul24(16 * Rt + hi3, G.cw);
            const int Ql = 16 * g + lo3, Qr = Ql + 8;
            const uint32_t vl = (2u * (row_off + (uint32_t)(8 * Ql))) | (Ql < (G.cw >> 3) ? 0u : kOobBit);
            coef_rows_to_lds(pd.coef[0], lds, vl, 0u);
            coef_rows_to_lds(pd.coef[0], lds + kLdsHalf, vl, 16u * (uint32_t)G.cw);
            if (args.has_right) {
                const uint32_t vr = (2u * (row_off + (uint32_t)(8 * Qr))) | (Qr < (G.cw >> 3) ? 0u : kOobBit);
                coef_rows_to_lds(pd.coef[0], lds + kLdsTile, vr, 0u);
                coef_rows_to_lds(pd.coef[0], lds + kLdsTile + kLdsHalf, vr, 16u * (uint32_t)G.cw);
            }
        } else {
        coef_rows_to_lds(pd.coef[CHROMA ? 1 : (alpha ? 3 : 0)], lds, coef_voff, 0u);
        coef_rows_to_lds(pd.coef[CHROMA ? 2 : (alpha ? 3 : 0)], lds + kLdsHalf, coef_voff, 2u * half_step);
        }
    }
    const uint32_t mb = (uint32_t)(CHROMA ? Rt * G.mbw + Qs : Rt * G.mbw + (Qs >> 1));
    uint32_t mf = 0, mk = 0, flags;
    if constexpr (CARRY == kCarryTake) {
        // this lane's macroblock is number 4 * side + (block >> 1) of the task: its chroma-part lane holds it
        const int src = (4 * dsp.side + (lo3 >> 1)) << 2;
        flags = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)carry.flags);
        // the vectors wait in LDS (the 64 bytes behind the staged tables: kOffCarry) -- carried in registers like the
        // flags, the three words went to scratch memory in the B kernel (12 bytes per lane: +6 % HBM traffic per launch)
        if (TYPE != 1) mf = *reinterpret_cast<const uint32_t*>(carryp + src);
        if (TYPE == 3) mk = *reinterpret_cast<const uint32_t*>(carryp + 32 + src);
    } else {
        flags = (uint32_t)(ldg<uint8_t>(gptr(pd.qscale), mb) & 31) | (ldg<uint8_t>(gptr(pd.intra), mb) != 0 ? 256u : 0u);   // I pictures honour the intra map too (COL_3)
        if (TYPE != 1) {
            flags |= ldg<uint8_t>(gptr(pd.repadd), mb) >= 128 ? 512u : 0u;    // .r > 0.5
            mf = ldg<uint32_t>(gptr(pd.mv_fwd), mb * 4);
        }
        if (TYPE == 3) {
            mk = ldg<uint32_t>(gptr(pd.mv_bwd), mb * 4);
            flags |= (uint32_t)(ldg<uint8_t>(gptr(pd.mb_dir), mb) & 3) << 10;
        }
        if constexpr (CARRY == kCarryLeave) {       // lane i < 8 holds macroblock i of the task (and so does every lane i + 8 k)
            carry.flags = flags;
            if (TYPE != 1) *reinterpret_cast<uint32_t*>(carryp + ((lane & 7) << 2)) = mf;
            if (TYPE == 3) *reinterpret_cast<uint32_t*>(carryp + 32 + ((lane & 7) << 2)) = mk;
        }
    }
    // FRONT3: the quantiser tables, dword i of the 256 bytes in lane i, requested behind the maps and landed with them
    uint32_t qreg = args.qreg;
    if constexpr (FRONT3) qreg = ldg<uint32_t>(gptr(pd.qt), (uint32_t)lane * 4u);
    const int q = (int)(flags & 31u);
    const bool ia = (flags & 256u) != 0u;
    const int x0 = 8 * Qs;
    bool nopred = false;
    // per reference: window column, half-pel flags, vertical offset, base selection
    int pxA = 0, ayA = 0, ohA = 0, ovA = 0, pxB = 0, ayB = 0, ohB = 0, ovB = 0;
    bool inA = true, inB = true, usef = true, useb = true;
    if (TYPE != 1) {
        nopred = (flags & 512u) != 0u;
        if (TYPE == 3) {
            const int dir = (int)(flags >> 10) & 3;
            usef = (dir & 1) != 0;
            useb = (dir & 2) != 0;
            nopred = nopred || dir == 0;
            // predictor A always reads the forward reference, B the backward one (scalar bases,
            // 32-bit offsets); an unused direction fetches nothing (out-of-range offset in
            // fetch_rows; its vector is zeroed so that the in-picture fast path is taken) and is
            // replaced by the other predictor afterwards: (p + p + 1) >> 1 == p
            if (!usef) mf = 0;                                // both components at once
            if (!useb) mk = 0;
        }
        const int fh = (int)(short)(mf & 0xffff), fv = (int)mf >> 16;
        const int bh = (int)(short)(mk & 0xffff), bv = (int)mk >> 16;
        {   // chroma: vector truncated toward zero first (mv_coef 0.5), then floor / parity
            int h = CHROMA ? fh / 2 : fh, v = CHROMA ? fv / 2 : fv;
            pxA = x0 + (h >> 1); ohA = h & 1; ayA = v >> 1; ovA = v & 1;
            inA = (uint32_t)pxA < (uint32_t)(W - 7 - ohA);    // 0 <= px && px + 7 + oh <= W - 1 (W >= 8)
        }
        if (TYPE == 3) {
            int h = CHROMA ? bh / 2 : bh, v = CHROMA ? bv / 2 : bv;
            pxB = x0 + (h >> 1); ohB = h & 1; ayB = v >> 1; ovB = v & 1;
            inB = (uint32_t)pxB < (uint32_t)(W - 7 - ohB);
        }
    }
    // lanes that take nothing from a reference: the direction map says so (B), or the macroblock is
    // not predicted at all (RepAdd / no direction).  They fetch nothing, and never take the slow path.
    const bool useA = usef && !nopred, useB = useb && !nopred;
    inA = inA || !useA;
    inB = inB || !useB;
    // quantiser scale and intra flag of this lane's block, for the lanes of the column pass to fetch (ds_bpermute)
    const int qia = q | (ia ? 256 : 0);

    // per-lane offsets of the task's first half; the second half differs by a scalar
    const uint32_t out_voff = ((uint32_t)__mul24(8 * R0 + hi3, W) + (uint32_t)x0) | (valid ? 0u : kOobBit);
    RefRows rfh[2], rbh[2];
    // B pictures: a wave whose macroblocks all predict from one side only (the leading pictures of
    // a closed GOP, runs of forward- or backward-only macroblocks) neither fetches nor interpolates
    // the other reference.  Wave-uniform, so it costs two scalar tests.
    const bool any_f = TYPE != 3 || __builtin_amdgcn_ballot_w64(useA) != 0;
    const bool any_b = TYPE == 3 && __builtin_amdgcn_ballot_w64(useB) != 0;
    // the coefficient rows (requested before the maps the reference fetches wait for anyway) have landed
    if constexpr (!SPARSE && !BACK) wait_vmem_all();
    if (TYPE != 1) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int Rh = CHROMA ? Rt : 2 * Rt + h;
            const uint32_t po = CHROMA ? (h == 0 ? ysz : ysz + (ysz >> 2)) : a_off;
            // (luma, upper half: no ninth row of its own -- finish_rows takes it from the lower half)
            const bool ninth = hi3 == 7 && (CHROMA || h == 1);
            if (any_f) rfh[h] = fetch_rows(gptr(pd.ref_fwd) + po, W, H, 8 * Rh + hi3, pxA, ayA, ohA, ovA, inA, ninth, useA);
            if (TYPE == 3 && any_b) rbh[h] = fetch_rows(gptr(pd.ref_bwd) + po, W, H, 8 * Rh + hi3, pxB, ayB, ohB, ovB, inB, ninth, useB);
        }
    }

    // B: the wave started at priority 3 (k_recon_display) and drops to 0 now that everything its front waits for is requested -- young
    // waves first: their loads are on the way while the older ones compute.  (One box, ms per mixed B launch: 0.919-0.922 here, 0.936-0.938
    // in front of the wait for the coefficient rows, 0.939-0.944 behind the chroma part, where the two-front task had it.)
    if constexpr (FRONT3 && TYPE == 3) __builtin_amdgcn_s_setprio(0);
    // ---- stage 1: the tile [half][r][b][c] ---------------------------------------------------------
    // dense: the rows are there (LDS-direct loads, waited for above); sparse: clear the tile and scatter both runs
    if constexpr (SPARSE) {
        *reinterpret_cast<v4i*>(lds + lane * 16) = v4i{0, 0, 0, 0};
        *reinterpret_cast<v4i*>(lds + kLdsHalf + lane * 16) = v4i{0, 0, 0, 0};
        wave_sync();
#pragma unroll
        for (int h = 0; h < 2; h++) {
            // scatter the group's entries into the cleared tile; the offset is masked to the tile
            uint32_t e = ent_first[h];
            if (e != 0u) *reinterpret_cast<short*>(lds + h * kLdsHalf + ((e >> 16) & 1022u)) = (short)e;
#pragma unroll 1
            for (uint32_t k = 64u; k < ent_count[h]; k += 64u) {     // wave-uniform, rare
                const uint32_t idx = k + (uint32_t)lane;
                e = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                    ent_rs, (int)(((ent_start[h] + idx) * 4u) | (idx < ent_count[h] ? 0u : kOobBit)), 0, kAuxStreamOnce);
                if (e != 0u) *reinterpret_cast<short*>(lds + h * kLdsHalf + ((e >> 16) & 1022u)) = (short)e;
            }
        }
    }
    wave_sync();

    uint64_t live[2] = {args.live[0], args.live[1]};
    if constexpr (FRONT3) {
        // one list, one pass: the chroma tile's live columns, then the left and the right luma tile's
        ThreeTiles t3{(uint32_t)(tile - lds), 0u, 0u, carry.flags};
        t3.n_c = scan_tile(tile, args.ids, lane, 0u, 0u, live, kSfCHalf);
        t3.n_cl = scan_tile(lds, args.ids, lane, 0u, t3.n_c, args.live_lr[0]);
        uint32_t n_cols = t3.n_cl;
        if (args.has_right) n_cols = scan_tile(lds + kLdsTile, args.ids, lane, 0u, n_cols, args.live_lr[1]);
        wave_sync();
        column_pass<false, false, true>(lds, (uint32_t)kLdsTile, args.ids, nullptr, n_cols, 0, 0, lane, qreg, t3);
        wave_sync();
    } else if constexpr (!BACK) column_front<LAYOUT>(pd, lds, tile, lane, qia, qreg, live);

#pragma unroll
    for (int half = 0; half < 2; half++) {
        const uint32_t plane_off = CHROMA ? (half == 0 ? ysz : ysz + (ysz >> 2)) : a_off;
        RefRows rf = rfh[half], rb = rbh[half];
        int t[8];
        const uint64_t colbits = live[half];
        if (colbits == 0) {
            // no coefficient in any of the 8 blocks: residual 0 = (0 + 128) / 256
#pragma unroll
            for (int m = 0; m < 8; m++) t[m] = 128;
        } else {
            // ---- stage 3: row pass ---------------------------------------------------------
            // lane (n = hi3, b = lo3): row n of block b, eight int16 w; int( w / _y ) == trunc(5w/2) == trunc(w * 2.5f)
            // (exact products, the conversion truncates).  Columns that are dead in every block of the half give
            // zero inputs (wave-uniform): lane (c, b) of the liveness mask -> byte c
            const int cols_live = 8 - (__builtin_clzll(colbits | 1ull) >> 3);
            const v4u wv = *reinterpret_cast<const v4u*>(tile + half * tile_half + hi3 * 128 + lo3 * 16);
            const v2f k25 = {2.5f, 2.5f};
            const v2f a = v2f{(float)(short)(wv.x & 0xffffu), (float)((int)wv.x >> 16)} * k25;
            const int Y0 = (int)a.x + 128, Y1 = (int)a.y;                           // "+128" of (t+128)/256
            if (cols_live <= 2) {
                butterfly8_lo2(Y0, Y1, t);
            } else {
                const v2f bb = v2f{(float)(short)(wv.y & 0xffffu), (float)((int)wv.y >> 16)} * k25;
                if (cols_live <= 4) {
                    butterfly8_lo4(Y0, Y1, (int)bb.x, (int)bb.y, t);
                } else {
                    const v2f cc = v2f{(float)(short)(wv.z & 0xffffu), (float)((int)wv.z >> 16)} * k25;
                    const v2f dd = v2f{(float)(short)(wv.w & 0xffffu), (float)((int)wv.w >> 16)} * k25;
                    const int Y[8] = {Y0, Y1, (int)bb.x, (int)bb.y, (int)cc.x, (int)cc.y, (int)dd.x, (int)dd.y};
                    butterfly8(Y, t);
                }
            }
            // t/256 truncating == arithmetic shift after adding 255 to negative values.  Without a
            // prediction (I pictures) the difference between truncation and floor is invisible:
            // it only exists for negative t, which the final clamp turns into 0 either way.
            if (TYPE != 1) {
#pragma unroll
                for (int m = 0; m < 8; m++) t[m] += (t[m] >> 31) & 255;
            }
        }

        // ---- stage 4: prediction, add, clamp, store ------------------------------------------
        if (TYPE != 1) {
            v2u pred = {0u, 0u};
            if (any_f) {
                finish_rows(rf, ovA, hi3 == 7, lane, !CHROMA && half == 0 ? &rfh[1] : nullptr);
                pred = predict8(rf);
            }
            if (TYPE == 3) {
                v2u pb = {0u, 0u};
                if (any_b) {
                    finish_rows(rb, ovB, hi3 == 7, lane, !CHROMA && half == 0 ? &rbh[1] : nullptr);
                    pb = predict8(rb);
                }
                v2u pf = usef ? pred : pb;
                pb = useb ? pb : pred;
                pred.x = __builtin_amdgcn_lerp(pf.x, pb.x, 0x01010101u);
                pred.y = __builtin_amdgcn_lerp(pf.y, pb.y, 0x01010101u);
            }
            if (nopred) pred = v2u{0u, 0u};
            // clamp(t/256 + pred) == sat_u8((t + pred*256) >> 8)
            t[0] += pred_x256<0>(pred.x);
            t[1] += pred_x256<1>(pred.x);
            t[2] += pred_x256<2>(pred.x);
            t[3] += pred_x256<3>(pred.x);
            t[4] += pred_x256<0>(pred.y);
            t[5] += pred_x256<1>(pred.y);
            t[6] += pred_x256<2>(pred.y);
            t[7] += pred_x256<3>(pred.y);
        }
        v2u o;
        o.x = sat_pk4<8>(t[0], t[1], t[2], t[3]);
        o.y = sat_pk4<8>(t[4], t[5], t[6], t[7]);
        if constexpr (!DISPLAY) {
            __builtin_amdgcn_raw_buffer_store_b64(o, buf_rsrc(pd.out + plane_off), (int)out_voff, (int)(half ? half_step : 0u), 0);
        } else {
            // planes only for pictures that will be predicted from.  A scalar branch (the flag is the picture's): until round 4 the
            // store was issued into a resource without records, which drops it -- after the texture path has processed it; a B task
            // issued six such stores among its 54 memory instructions
            if (!pd.no_planes) __builtin_amdgcn_raw_buffer_store_b64(o, buf_rsrc(pd.out + plane_off), (int)out_voff, (int)(half ? half_step : 0u), 0);
            if constexpr (OUT != kOutRgba) {
                // the frame's cropped plane: the same 8 samples, row y of Y / A (luma: half = the next block row) or of Cb / Cr
                // (chroma: half = the plane).  Every 8-byte chunk of the coded width lies inside the 64-byte row stride, so only
                // rows past the plane height are dropped -- by the offset select, like every other store here.
                const FrameOut& fo = *dsp.fo;
                const int y = CHROMA ? 8 * Rt + hi3 : 8 * (2 * Rt + half) + hi3;
                const bool in = valid && y < (CHROMA ? fo.chroma_height : G.fh);
                const uint32_t po = CHROMA ? (half ? fo.cr_off : fo.cb_off) : (AMODE == kAlphaPark ? fo.a_off : 0u);
                const uint32_t fvoff = (__umul24((uint32_t)y, CHROMA ? fo.chroma_stride : fo.luma_stride) + (uint32_t)x0) | (in ? 0u : kOobBit);
                __builtin_amdgcn_raw_buffer_store_b64(o, buf_rsrc(dsp.planes + po), (int)fvoff, 0, kAuxFrameStore);
            }
            if constexpr (OUT == kOutYcbcr) {
                // no display stage: nothing is parked for a conversion
            } else if constexpr (CHROMA) {
                // park the samples for the luma parts: [plane = half][row hi3][8 bytes of macroblock lo3]
                if constexpr (FRONT3) {      // the stash is the tile's first KB, whose row pass (stage 3) must have read it out
                    wait_lds_all();
                    __builtin_amdgcn_wave_barrier();
                }
                *reinterpret_cast<v2u*>(dsp.stash + half * 512 + hi3 * 64 + lo3 * 8) = o;
            } else if constexpr (AMODE == kAlphaPark) {
                // yuva, A part: the samples wait for the Y part of the same macroblocks
                *reinterpret_cast<v2u*>(dsp.apark + half * 512 + hi3 * 64 + lo3 * 8) = o;
            } else {
                // converted right away (stage 5): the rows change lanes through the park
                if constexpr (Lay<LAYOUT>::park_in_tile) {      // the tile half is read out (stage 3): every lane's read has completed
                    wait_lds_all();
                    __builtin_amdgcn_wave_barrier();
                }
                *reinterpret_cast<v2u*>((Lay<LAYOUT>::park_in_tile ? tile + half * kLdsHalf : lds + kOffYpark) + hi3 * 64 + lo3 * 8) = o;
            }
        }
        if constexpr (DISPLAY && !CHROMA && AMODE != kAlphaPark && OUT != kOutYcbcr) {
            wave_sync();
            if constexpr (LAYOUT == 2) {
                // the conversion tables lie where every wave's column ids and Cr rows were: the chunks this wave requested (behind
                // barrier 1, in front of this part's reference rows) have landed, and then every wave's have
                if (args.lut_barrier && half == 0) {
                    wait_vmem_all();
                    __syncthreads();
                }
            }
            display_half<AMODE>(pd, G, dsp, Lay<LAYOUT>::park_in_tile ? tile + half * kLdsHalf : lds + kOffYpark, half, Rt, g, hi3, lo3);
            // the next half parks its rows in the same place
            wave_sync();
        }
    }
}

// The two luma parts of a dense display task (P and B pictures) with ONE front: the coefficient rows of both parts are requested
// together (two tiles), one liveness scan lists the live columns of all four halves, ONE column pass takes them -- a P or B part
// has about a dozen live columns of 128, and a pass costs ~140 instructions however few of its 64 lanes have a column -- and then each
// part runs its back half (maps from the chroma part, reference fetches, row passes, prediction, stores, conversion) as before.
// I pictures keep a front per part: with ~40 live columns per part the shared pass would run twice anyway.
template <int TYPE, int OUT = kOutRgba>
__device__ __forceinline__ void recon_luma_pair(const PicDesc& pd, const Geom& G, int Rt, int gc, char* lds, int lane, Display dsp, MbCarry& carry, bool has_right,
                                                uint32_t qreg)
{
    const int W = G.cw, hi3 = lane >> 3, lo3 = lane & 7;
    char* const tileR = lds + kOffTileR;
    // the previous part of this wave (the chroma part) may still be reading the tile
    wait_lds_all();
    __builtin_amdgcn_wave_barrier();
    const uint32_t row_off = (uint32_t)__mul24(16 * Rt + hi3, W);
    {
        const int Qld = 16 * gc + lo3;
        const uint32_t voff = (2u * (row_off + (uint32_t)(8 * Qld))) | (Qld < (W >> 3) ? 0u : kOobBit);
        coef_rows_to_lds(pd.coef[0], lds, voff, 0u);
        coef_rows_to_lds(pd.coef[0], lds + kLdsHalf, voff, 16u * (uint32_t)W);
    }
    if (has_right) {
        const int Qld = 16 * gc + 8 + lo3;
        const uint32_t voff = (2u * (row_off + (uint32_t)(8 * Qld))) | (Qld < (W >> 3) ? 0u : kOobBit);
        coef_rows_to_lds(pd.coef[0], tileR, voff, 0u);
        coef_rows_to_lds(pd.coef[0], tileR + kLdsHalf, voff, 16u * (uint32_t)W);
    }
    // quantiser scale | intra << 8 of the macroblock of block b of either part, in lane b (the chroma part's lanes hold the task's
    // eight macroblocks: lane m, macroblock m)
    const int qiaL = __builtin_amdgcn_ds_bpermute((lo3 >> 1) << 2, (int)carry.flags) & 0x11f;
    const int qiaR = __builtin_amdgcn_ds_bpermute((4 + (lo3 >> 1)) << 2, (int)carry.flags) & 0x11f;
    wait_vmem_all();
    wave_sync();
    TaskArgs left{false, lds}, right{false, tileR};
    uint32_t n_cols = scan_tile(lds, lds + Lay<1>::slots, lane, 0u, 0u, left.live);
    if (has_right) n_cols = scan_tile(tileR, lds + Lay<1>::slots, lane, 128u, n_cols, right.live);
    wave_sync();
    column_pass<true, false>(lds, (uint32_t)kOffTileR, lds + Lay<1>::slots, nullptr, n_cols, qiaL, qiaR, lane, qreg);
    wave_sync();
    dsp.side = 0;
    recon_task<PairBackHalf<TYPE, OUT>>(pd, G, Rt, 2 * gc, lds, lane, dsp, carry, left);
    if (has_right) {
        dsp.side = 1;
        recon_task<PairBackHalf<TYPE, OUT>>(pd, G, Rt, 2 * gc + 1, lds, lane, dsp, carry, right);
    }
}

// A wave's copy of the quantiser matrices and the premultiplier (the first 64 dwords of Tables; the column pass
// reads them by the column its lane was handed): one load and one LDS write per lane, once per wave.
// Straight into LDS (lane i's dword at kOffQtab + 4 i), nothing waits here: through a register (round 1-4: load, s_waitcnt vmcnt(0),
// ds_write) the wave made a round trip to memory before it requested its first coefficient row.  The tables are read by the column
// pass, behind the task's wait for its coefficient rows (dense: wait_vmem_all) or first entries (sparse; loads return in order).
__device__ __forceinline__ void stage_tables(const QTables* __restrict__ Tg, char* lds, int lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)Tg, 0, 256, 0x00020000);
    // (the matrices and the premultiplier only: the 64 bytes behind them are the display task's vectors in LDS, kOffCarry, written
    // by the chroma part -- which a load that lands late must not overwrite)
    if (lane < 48) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(lds + kOffQtab), 4, lane * 4, 0, 0, 0);
}

// XCD-aware workgroup remap: hardware deals workgroups round-robin over the 8 XCDs;
// give each XCD one contiguous run of the task space so that vertically adjacent
// block groups (which share reference lines) meet in the same L2.  Bijective for any n.
__device__ __forceinline__ int xcd_remap(int bid, int n)
{
    int q = n >> 3, r = n & 7;
    int x = bid & 7, j = bid >> 3;
    return x * q + min(x, r) + j;
}

// workgroup -> (picture, workgroup inside the picture).  B pictures come in pairs that predict from the same two
// anchors (the host keeps the pictures of a GOP adjacent): the workgroups of two consecutive pictures alternate, so
// both read the same reference lines at about the same time and the second read finds them in the XCD's L2 -- one
// after the other, a reference pair (6 MB at 1080p) is gone from the 4 MB L2 before it is used again.
template <int TYPE>
__device__ __forceinline__ void pic_of_wg(const Geom& G, int wg, int& pic, int& twg)
{
    if (TYPE == 3) {
        const int half = wg >> 1;
        const int pair = div_inv(half, G.inv_wg_per_pic);
        twg = half - pair * G.wg_per_pic;
        pic = 2 * pair + (wg & 1);
    } else {
        pic = div_inv(wg, G.inv_wg_per_pic);
        twg = wg - pic * G.wg_per_pic;
    }
}

template <int TYPE, bool SPARSE>
__device__ __forceinline__ void recon_dispatch(const PicDesc& pd, const Geom& G, int t, char* lds, int lane)
{
    const Display none{nullptr, 0};
    MbCarry own{};
    if (t < G.tasksY) {
        int Rt = div_inv(t, G.inv_gY), g = t - Rt * G.gY;
        recon_task<PlainLuma<TYPE, SPARSE>>(pd, G, Rt, g, lds, lane, none, own);
    } else if (t < G.tasksY + G.tasksC) {
        t -= G.tasksY;
        int Rt = div_inv(t, G.inv_gC), g = t - Rt * G.gC;
        recon_task<PlainChroma<TYPE, SPARSE>>(pd, G, Rt, g, lds, lane, none, own);
    } else {                                   // yuva: the A plane, luma-shaped
        t -= G.tasksY + G.tasksC;
        int Rt = div_inv(t, G.inv_gY), g = t - Rt * G.gY;
        recon_task<PlainLuma<TYPE, SPARSE>>(pd, G, Rt, g, lds, lane, none, own, TaskArgs{true});
    }
}

// One kernel per picture type: the register budget of the I and P paths is not held hostage
// by the two predictors of the B path (VGPRs decide waves per SIMD), and a launch only ever
// contains pictures of one type.
template <int TYPE, bool SPARSE>
__global__ __launch_bounds__(kReconMaxThreads) void k_recon(const PicDesc* __restrict__ descs, Geom G,
                                               const Tables* __restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int wg = xcd_remap(blockIdx.x, G.n_wg);
    int pic, twg;
    pic_of_wg<TYPE>(G, wg, pic, twg);
    const int t = twg * kWavesPerWG + wave;
    if (t >= G.tasks_per_pic || pic >= G.n_pics) return;
    char* lds = smem + wave * kLdsPerWave;
    const PicDesc& pd = descs[pic];
    stage_tables(pd.qt, lds, lane);
    recon_dispatch<TYPE, SPARSE>(pd, G, t, lds, lane);
}

// The same reconstruction with the display conversion fused in (see Display above).  One wave = the 8
// macroblocks of one chroma group, all components: tasks_per_pic = tasksC here (the host sets Geom up
// for that), the chroma part first, then the left and the right luma part.
// The sparse B kernel (what the pipeline runs most) is held to 72 registers = 7 waves per SIMD: it wants 74, the two
// spilled dwords (8 bytes of scratch per lane) cost less than the wave brings: +1..2 % end to end, three pairs on one box.
// one display task of a wave: the chroma part, the workgroup's barrier in front of the first table lookup (`first`: every wave of the
// workgroup comes by here exactly once), the luma parts.  false: the wave has no task (and none behind this one).
// OUT (kOutYcbcr / kOutBoth): the task also stores the frame's planes (FrameOut); kOutYcbcr converts nothing, so it neither waits
// for the conversion tables nor meets the other waves at the barrier.
template <int TYPE, bool SPARSE, bool ALPHA, int OUT = kOutRgba>
__device__ __forceinline__ bool display_task(const PicDesc* __restrict__ descs, const Geom& G, int pic, int t, char* lds, int lane, const char* lut, bool first,
                                             const FrameOut* fo = nullptr)
{
    constexpr bool kPair = pair_task(TYPE, SPARSE, ALPHA);      // recon_luma_pair
    const bool live = t < G.tasks_per_pic && pic < G.n_pics;
    const PicDesc& pd = descs[live ? pic : 0];
    const int Rt = div_inv(t, G.inv_gC), gc = t - Rt * G.gC;
    Display dsp{lds + (kPair ? Lay<1>::stash : Lay<0>::stash), 0, lds + kLdsPerWaveDisplay, lut, nullptr, fo};
    if constexpr (OUT != kOutRgba) dsp.planes = fo->frames[live ? pic : 0];
    if constexpr (!kPair) {
        if (!first) { wait_lds_all(); __builtin_amdgcn_wave_barrier(); }      // the column pass of the task before has read its tables
        stage_tables(pd.qt, lds, lane);
    }
    MbCarry carry{};
    // the two-tile layout has no room for the quantiser tables in LDS: the wave keeps them in ONE register, dword i of the 256 bytes
    // in lane i (column_pass takes what it needs by ds_bpermute); requested first, landed with the macroblock maps
    uint32_t qreg = 0u;
    if constexpr (kPair) qreg = ldg<uint32_t>(gptr(pd.qt), (uint32_t)lane * 4u);
    const TaskArgs tables{false, nullptr, {0, 0}, qreg};
    if (live) recon_task<DisplayChroma<TYPE, SPARSE, kPair ? 1 : 0, OUT>>(pd, G, Rt, gc, lds, lane, dsp, carry, tables);
    if (first) {
        if (!live) wait_vmem_all();      // (a wave with a task has waited for memory behind its chroma part's loads: its chunks of the tables are in)
        if constexpr (OUT != kOutYcbcr) __syncthreads();      // the conversion tables have landed: every wave's chunks
    }
    if (!live) return false;
    // the two luma parts as two calls, not a loop: the loop form keeps 15 more registers live (B path: 93).
    // yuva: the A part of the same four macroblocks first (AMODE 1), then the Y part that displays them (AMODE 2).
    if constexpr (kPair) {
        recon_luma_pair<TYPE, OUT>(pd, G, Rt, gc, lds, lane, dsp, carry, 2 * gc + 1 < G.gY, qreg);
        return true;
    }
    dsp.side = 0;
    if constexpr (ALPHA) {
        recon_task<YuvaAPart<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc, lds, lane, dsp, carry);
        recon_task<YuvaYPart<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc, lds, lane, dsp, carry);
    } else {
        recon_task<DisplayLuma<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc, lds, lane, dsp, carry);
    }
    if (2 * gc + 1 < G.gY) {
        dsp.side = 1;
        if constexpr (ALPHA) {
            recon_task<YuvaAPart<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc + 1, lds, lane, dsp, carry);
            recon_task<YuvaYPart<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc + 1, lds, lane, dsp, carry);
        } else {
            recon_task<DisplayLuma<TYPE, SPARSE, OUT>>(pd, G, Rt, 2 * gc + 1, lds, lane, dsp, carry);
        }
    }
    return true;
}

// A dense B display task with one front (front3_task; layout 2, see kSfBytes): the chroma part runs the front for all three tiles and its own back
// half; barrier 1 -- every wave of the workgroup is through with its column ids and its Cr rows; the wave requests its chunks of the
// conversion tables into their place and goes on with the left luma part, which meets the others at barrier 2 in front of its first
// table lookup (recon_task, lut_barrier); the right part.  A wave without a task takes part in both barriers and loads its chunks.
// The compiler does not order LDS reads behind an LDS-direct load: each wave waits for its own chunks itself (wait_vmem_all in front of
// barrier 2; the left part's reference rows were requested behind them and are needed before that, so the wait finds the chunks landed).
template <int TYPE>
__device__ __forceinline__ void display_task_front3(const PicDesc* __restrict__ descs, const Geom& G, int pic, int t, char* sf, int wave, int lane, const Tables* __restrict__ T)
{
    const bool live = t < G.tasks_per_pic && pic < G.n_pics;
    const PicDesc& pd = descs[live ? pic : 0];
    const int Rt = div_inv(t, G.inv_gC), gc = t - Rt * G.gC;
    char* const lds = sf + wave * (2 * kLdsTile);
    char* const c0 = sf + kSfC0 + wave * kLdsHalf;
    const bool has_right = 2 * gc + 1 < G.gY;
    Display dsp{c0, 0, nullptr, sf + kSfLut, nullptr, nullptr};
    MbCarry carry{};
    uint64_t live_lr[2][2] = {{0, 0}, {0, 0}};
    TaskArgs front{};
    front.tile = c0;
    front.carry = sf + kSfCarry + wave * 64;
    front.ids = sf + kSfIds + wave * kSfIdsPerWave;
    front.has_right = has_right;
    front.live_lr = live_lr;
    if (live) recon_task<Front3Chroma<TYPE>>(pd, G, Rt, gc, lds, lane, dsp, carry, front);
    if (TYPE == 3) __builtin_amdgcn_s_setprio(0);      // (a wave without a task drops here; the others have, in their front)
    wait_lds_all();
    __syncthreads();            // barrier 1
    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc((void*)T->rgba_lut, 0, kLdsLut, 0x00020000);
    for (int c = wave; c < kLdsLut / 1024; c += kWavesPerWG)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(lrs, (__attribute__((address_space(3))) void*)(sf + kSfLut + c * 1024), 16, (int)(lane * 16u), c * 1024, 0, 0);
    if (!live) {
        wait_vmem_all();
        __syncthreads();        // barrier 2
        return;
    }
    TaskArgs part{};
    part.tile = lds;
    part.live[0] = live_lr[0][0]; part.live[1] = live_lr[0][1];
    part.carry = front.carry;
    part.lut_barrier = true;
    dsp.side = 0;
    recon_task<PairBackHalf<TYPE, kOutRgba, 2>>(pd, G, Rt, 2 * gc, lds, lane, dsp, carry, part);
    if (has_right) {
        part.tile = lds + kLdsTile;
        part.live[0] = live_lr[1][0]; part.live[1] = live_lr[1][1];
        part.lut_barrier = false;
        dsp.side = 1;
        recon_task<PairBackHalf<TYPE, kOutRgba, 2>>(pd, G, Rt, 2 * gc + 1, lds, lane, dsp, carry, part);
    }
}

template <int TYPE, bool SPARSE, bool ALPHA = false>
__global__ __launch_bounds__(kReconMaxThreads) __attribute__((amdgpu_waves_per_eu(TYPE == 3 && !ALPHA ? 7 : 4)))
void k_recon_display(const PicDesc* __restrict__ descs, Geom G,
                                                                    const Tables* __restrict__ T)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // B waves start at priority 3 and drop to 0 in their front (recon_task, FRONT3: one box, alternating, ms per mixed B launch of the
    // two-front task: 1.027-1.031 without priorities, 0.992-0.993 with; other picture types: no better or slower).  (The dense, non-alpha kernel only: in the pipeline's sparse
    // launches a raised priority takes issue slots from the parser kernels beside them -- 175-177 k against 181-182 k pictures/s end to end)
    if (TYPE == 3 && !SPARSE && !ALPHA) __builtin_amdgcn_s_setprio(3);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    const int wg = xcd_remap(blockIdx.x, G.n_wg);
    int pic, twg;
    pic_of_wg<TYPE>(G, wg, pic, twg);
    if constexpr (front3_task(TYPE, SPARSE, ALPHA)) {
        // one static array: every LDS address of the task is a compile-time constant plus a multiple of the wave's number
        __shared__ __attribute__((aligned(16))) char sf_s[kSfBytes];
        display_task_front3<TYPE>(descs, G, pic, twg * kWavesPerWG + wave, sf_s, wave, lane0, T);
    } else {
    const int wpw = (int)(blockDim.x >> 6);
    // the conversion tables: 5 KB per workgroup, requested before anything else and needed only after the
    // chroma part -- the barrier in display_task finds them long landed.  Straight into LDS, 1 KB per instruction (lane i's 16
    // bytes at chunk + 16 i), the chunks dealt to the workgroup's waves: nothing waits for them here.  (Until round 4 the
    // tables went through registers: load, s_waitcnt vmcnt(0), ds_write -- a round trip to memory at the head of EVERY
    // workgroup, in front of its first coefficient load; a workgroup of the B kernel lives 24 us.)  A wave's chunks have landed
    // when its next full wait for memory returns: the chroma part's, behind its coefficient loads (dense) or first entries
    // (sparse; loads return in order) -- a wave without a task waits in display_task -- and the barrier there makes every
    // wave's chunks everybody's.
    __shared__ __attribute__((aligned(16))) int32_t lut_s[kLdsLut / 4];      // static: its LDS address is a compile-time constant
    static_assert(kLdsLut % 1024 == 0, "whole chunks");
    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc((void*)T->rgba_lut, 0, kLdsLut, 0x00020000);
    for (int c = wave; c < kLdsLut / 1024; c += wpw)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(lrs, (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(lut_s) + c * 1024), 16,
                                                 (int)(lane0 * 16u), c * 1024, 0, 0);
    char* lds = smem + wave * display_strip_bytes(TYPE, SPARSE, ALPHA);
    // (Round 4 tried a wave running two to five tasks one after the other, so that the frames' stores of a task drain while the wave
    // works on the next: 5.89-5.92 ms per step with two against 5.90-5.95 with one, worse with three and five, and 10-20 registers more
    // for the loop -- not kept.)
    display_task<TYPE, SPARSE, ALPHA>(descs, G, pic, twg * wpw + wave, lds, lane0, reinterpret_cast<const char*>(lut_s), true);
    }
}


// The same launch with the frame's YCbCr planes as output (OUT = kOutYcbcr: planes only, no conversion; kOutBoth: planes and
// RGBA).  I and P pictures still write their slots (motion compensation reads the coded-size planes), B pictures (no_planes) only
// the frame's planes.  The strip layout and the launch geometry are k_recon_display's; kOutYcbcr leaves the strip's stash and park
// unused and loads no conversion tables.  A kernel of its own rather than a parameter of k_recon_display: a fourth argument would
// move the implicit arguments the RGBA kernels read.  Each instantiation keeps at least its RGBA twin's waves per SIMD: the yuva P kernel
// with both outputs wants 104 scalar registers (7 waves) and is held to the twin's 8.
template <int TYPE, bool SPARSE, bool ALPHA, int OUT>
__global__ __launch_bounds__(kReconMaxThreads) __attribute__((amdgpu_waves_per_eu(TYPE == 3 && !ALPHA ? 7 : (TYPE == 2 && ALPHA && OUT == kOutBoth ? 8 : 4))))
void k_recon_display_out(const PicDesc* __restrict__ descs, Geom G, const Tables* __restrict__ T, FrameOut fo)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (TYPE == 3 && !SPARSE && !ALPHA) __builtin_amdgcn_s_setprio(3);      // as k_recon_display
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    const int wg = xcd_remap(blockIdx.x, G.n_wg);
    int pic, twg;
    pic_of_wg<TYPE>(G, wg, pic, twg);
    const int wpw = (int)(blockDim.x >> 6);
    // the conversion tables (kOutBoth only), as k_recon_display loads them
    __shared__ __attribute__((aligned(16))) int32_t lut_s[kLdsLut / 4];
    if constexpr (OUT == kOutBoth) {
        const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc((void*)T->rgba_lut, 0, kLdsLut, 0x00020000);
        for (int c = wave; c < kLdsLut / 1024; c += wpw)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(lrs, (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(lut_s) + c * 1024), 16,
                                                     (int)(lane0 * 16u), c * 1024, 0, 0);
    }
    char* lds = smem + wave * display_strip_bytes(TYPE, SPARSE, ALPHA);
    display_task<TYPE, SPARSE, ALPHA, OUT>(descs, G, pic, twg * wpw + wave, lds, lane0, OUT == kOutBoth ? reinterpret_cast<const char*>(lut_s) : nullptr, true, &fo);
}

// ---- the frames' planes on the unfused road: slot planes -> cropped frame planes (FrameOut layout) ------------------------
// One launch per batch: blockIdx.z = picture (src_slots[z] -> FrameOut::frames[z]), blockIdx.y = plane (Y, Cb, Cr, A), a lane = one
// piece of one row: 16 bytes of Y / A (the slot's luma rows are coded_width apart, a multiple of 16), 8 bytes of Cb / Cr (their rows
// are coded_width / 2 apart, a multiple of 8 only).  A piece never reaches past the coded row nor past the 64-byte destination stride.
struct CropGeom {
    int32_t cw, ch, fw, fh;
    int32_t cwid;                // (fw + 1) / 2
    uint32_t slot_stride_lo, slot_stride_hi;
    int32_t alpha;
};
__global__ __launch_bounds__(kRgbaBlock) void k_planes_crop(const uint8_t* __restrict__ slots, const int32_t* __restrict__ src_slots, FrameOut fo, CropGeom G)
{
    const int plane = blockIdx.y;
    if (plane == 3 && !G.alpha) return;
    const bool luma = plane == 0 || plane == 3;
    const uint32_t piece = luma ? 16u : 8u;
    const uint32_t pw = (uint32_t)(luma ? G.fw : G.cwid), ph = (uint32_t)(luma ? G.fh : fo.chroma_height);
    const uint32_t per_row = (pw + piece - 1) / piece;
    const uint32_t idx = blockIdx.x * (uint32_t)blockDim.x + threadIdx.x;
    if (idx >= per_row * ph) return;
    const uint32_t y = idx / per_row, x = (idx - y * per_row) * piece;
    const uint32_t ysz = (uint32_t)G.cw * (uint32_t)G.ch;
    const uint32_t src_w = luma ? (uint32_t)G.cw : (uint32_t)G.cw >> 1;
    const uint32_t src_plane = plane == 0 ? 0u : plane == 1 ? ysz : plane == 2 ? ysz + (ysz >> 2) : ysz + (ysz >> 1);
    const size_t stride = join64(G.slot_stride_lo, G.slot_stride_hi);
    const uint8_t* src = slots + (size_t)src_slots[blockIdx.z] * stride + src_plane + (size_t)y * src_w + x;
    uint8_t* dst = fo.frames[blockIdx.z] + (plane == 0 ? 0u : plane == 1 ? fo.cb_off : plane == 2 ? fo.cr_off : fo.a_off)
                 + (size_t)y * (luma ? fo.luma_stride : fo.chroma_stride) + x;
    if (luma) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
}

// ---- K3: YCbCr 4:2:0 -> RGBA8 ------------------------------------------------------

struct RgbaGeom {
    int32_t cw, ch, fw, fh;
    int32_t cols, rows;          // fw>>1, fh>>1 quads
    int32_t n;                   // frames in the batch
    int32_t flavour;             // 0 CPU twin (fp64), 1 GL (fp32); bit 8: yuva -- the A byte comes from the slot's fourth plane
    uint32_t slot_stride_lo, slot_stride_hi;   // bytes between slots
    uint32_t inv_cols4;          // ceil(2^32 / (fw/4)): the 4x2 kernel walks a frame linearly
};

// Uint8ClampedArray store: clamp, round half to even (2^52+2^51 trick; |x| < 2^31)
__device__ __forceinline__ uint32_t u8_clamped(double x)
{
    double t = x + 6755399441055744.0;
    int i = __double2loint(t);
    return (uint32_t)med3i(i, 0, 255);
}

// CPU twin, one thread per 2x2 quad, with the reference's flat index progression
// (player/easybits.player.js:2692-2782): identical to a plain crop for even frame
// widths, and reproducing its one-sample-per-row-pair drift for odd ones.
__global__ __launch_bounds__(kRgbaBlock) void k_rgba_twin(const uint8_t* __restrict__ slots, const int32_t* __restrict__ slot_ids,
                                                   uint8_t* __restrict__ rgba, RgbaGeom G)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    const int f = blockIdx.z;
    if (col >= G.cols) return;
    const size_t stride = join64(G.slot_stride_lo, G.slot_stride_hi);
    const uint8_t* Y = slots + (size_t)slot_ids[f] * stride;
    const uint8_t* Cb = Y + (size_t)G.cw * G.ch;
    const uint8_t* Cr = Cb + ((size_t)G.cw * G.ch >> 2);
    uint8_t* dst = rgba + (size_t)f * G.fw * G.fh * 4;
    const int odd = G.fw & 1;
    const int hw = G.cw >> 1;
    const int yi1 = row * (2 * G.cw - odd) + 2 * col;
    const int yi2 = yi1 + G.cw;
    const int ci = row * hw + col;
    const size_t d1 = 4 * ((size_t)row * (2 * G.fw - odd) + 2 * col);
    const size_t d2 = d1 + 4 * (size_t)G.fw;
    const double yuvr = (double)Cr[ci] - 128.0, yuvb = (double)Cb[ci] - 128.0;
    const double r = yuvr * 1.59603;
    const double g = (-0.81297 * yuvr) - (0.39176 * yuvb);
    const double b = yuvb * 2.01723;
    uint32_t px[4];
    const int yidx[4] = {yi1, yi1 + 1, yi2, yi2 + 1};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double ys = ((double)Y[yidx[k]] - 16.0) * 1.16438;
        px[k] = u8_clamped(r + ys) | (u8_clamped(g + ys) << 8) | (u8_clamped(b + ys) << 16) | 0xff000000u;
    }
    *reinterpret_cast<uint32_t*>(dst + d1) = px[0];
    *reinterpret_cast<uint32_t*>(dst + d1 + 4) = px[1];
    *reinterpret_cast<uint32_t*>(dst + d2) = px[2];
    *reinterpret_cast<uint32_t*>(dst + d2 + 4) = px[3];
}

// Fast path of the CPU twin for frame widths that are a multiple of 4 (no index drift): one thread =
// 4 x 2 pixels = two 2x2 quads, same fp64 operations in the same order as k_rgba_twin.  The 64 lanes
// of a wave store 1 KB of contiguous RGBA per row with one 16-byte store each -- 5.8 TB/s; the
// 8 x 2 form (two 16-byte stores per lane and row, lanes 32 bytes apart) reached 5.4.
__global__ __launch_bounds__(kRgbaBlock) void k_rgba_twin4(const uint8_t* __restrict__ slots, const int32_t* __restrict__ slot_ids,
                                                    uint8_t* __restrict__ rgba, RgbaGeom G)
{
    // one thread per (row pair, group of 4 columns), numbered linearly through the frame: a 1920-wide
    // row pair is 7.5 waves, and a row-shaped grid would leave every eighth wave half empty
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t cols4 = (uint32_t)G.fw >> 2;
    if (idx >= cols4 * (uint32_t)G.rows) return;
    const int row = (int)(G.inv_cols4 ? __umulhi(idx, G.inv_cols4) : idx);   // exact: idx * cols4 < 2^32
    const int col4 = (int)(idx - (uint32_t)row * cols4);
    const int f = blockIdx.z;
    const size_t stride = join64(G.slot_stride_lo, G.slot_stride_hi);
    const uint8_t* Y = slots + (size_t)slot_ids[f] * stride;
    const uint8_t* Cb = Y + (size_t)G.cw * G.ch;
    const uint8_t* Cr = Cb + ((size_t)G.cw * G.ch >> 2);
    const int hw = G.cw >> 1;
    const uint32_t y0 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(Y + (size_t)(2 * row) * G.cw + 4 * col4));
    const uint32_t y1 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(Y + (size_t)(2 * row + 1) * G.cw + 4 * col4));
    const uint32_t cb2 = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(Cb + (size_t)row * hw + 2 * col4));
    const uint32_t cr2 = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(Cr + (size_t)row * hw + 2 * col4));
    uint32_t o0[4], o1[4];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double yuvr = (double)((cr2 >> (8 * q)) & 255u) - 128.0, yuvb = (double)((cb2 >> (8 * q)) & 255u) - 128.0;
        const double r = yuvr * 1.59603;
        const double g = (-0.81297 * yuvr) - (0.39176 * yuvb);
        const double b = yuvb * 2.01723;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int px = 2 * q + k;
            const double ya = ((double)((y0 >> (8 * px)) & 255u) - 16.0) * 1.16438;
            const double yb = ((double)((y1 >> (8 * px)) & 255u) - 16.0) * 1.16438;
            o0[px] = u8_clamped(r + ya) | (u8_clamped(g + ya) << 8) | (u8_clamped(b + ya) << 16) | 0xff000000u;
            o1[px] = u8_clamped(r + yb) | (u8_clamped(g + yb) << 8) | (u8_clamped(b + yb) << 16) | 0xff000000u;
        }
    }
    const __amdgpu_buffer_rsrc_t rs = buf_rsrc(rgba + (size_t)f * G.fw * G.fh * 4);
    const uint32_t o = ((uint32_t)(2 * row) * (uint32_t)G.fw + 4u * (uint32_t)col4) * 4u;
    __builtin_amdgcn_raw_buffer_store_b128(v4u{o0[0], o0[1], o0[2], o0[3]}, rs, (int)o, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(v4u{o1[0], o1[1], o1[2], o1[3]}, rs, (int)(o + (uint32_t)G.fw * 4u), 0, 0);
}

// yuva: the A byte of every converted pixel comes from the slot's fourth plane (behind Cr) instead of the
// constant 255 -- a second pass over the frame, launched for alpha decoders only so that the conversion
// kernels above stay as they are.  One thread per pixel quad of a row (frame width is even for alpha).
__global__ __launch_bounds__(kRgbaBlock) void k_rgba_alpha(const uint8_t* __restrict__ slots, const int32_t* __restrict__ slot_ids,
                                                           uint8_t* __restrict__ rgba, RgbaGeom G, int cover_w, int cover_h)
{
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 2;
    const int yy = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= cover_w || yy >= cover_h) return;
    const size_t stride = join64(G.slot_stride_lo, G.slot_stride_hi);
    const size_t ysz = (size_t)G.cw * G.ch;
    const uint8_t* A = slots + (size_t)slot_ids[f] * stride + ysz + (ysz >> 1);
    uint8_t* dst = rgba + ((size_t)f * G.fw * G.fh + (size_t)yy * G.fw + x) * 4;
    dst[3] = A[(size_t)yy * G.cw + x];
    if (x + 1 < cover_w) dst[7] = A[(size_t)yy * G.cw + x + 1];
}

// fills what the quad loop never writes (odd last row / column, drift leftovers) with 255
__global__ __launch_bounds__(kRgbaBlock) void k_fill255(uint32_t* __restrict__ p, size_t n_dwords)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_dwords) p[i] = 0xffffffffu;
}

// GL flavour: every pixel of the frame_w x frame_h crop, fp32, left-to-right, no contraction
__global__ __launch_bounds__(kRgbaBlock) void k_rgba_gl(const uint8_t* __restrict__ slots, const int32_t* __restrict__ slot_ids,
                                                 uint8_t* __restrict__ rgba, RgbaGeom G)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    const int f = blockIdx.z;
    if (x >= G.fw) return;
    const size_t stride = join64(G.slot_stride_lo, G.slot_stride_hi);
    const uint8_t* Y = slots + (size_t)slot_ids[f] * stride;
    const uint8_t* Cb = Y + (size_t)G.cw * G.ch;
    const uint8_t* Cr = Cb + ((size_t)G.cw * G.ch >> 2);
    const int hw = G.cw >> 1;
    const float fy = (float)Y[(size_t)yy * G.cw + x] / 255.0f;
    const float fcb = (float)Cb[(size_t)(yy >> 1) * hw + (x >> 1)] / 255.0f;
    const float fcr = (float)Cr[(size_t)(yy >> 1) * hw + (x >> 1)] / 255.0f;
    const float M[3][4] = {{1.16438f, 0.00000f, 1.59603f, -0.87079f},
                           {1.16438f, -0.39176f, -0.81297f, 0.52959f},
                           {1.16438f, 2.01723f, 0.00000f, -1.08139f}};
    uint32_t o = 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float s = fy * M[c][0];
        s = s + fcb * M[c][1];
        s = s + fcr * M[c][2];
        s = s + M[c][3];
        s = fminf(fmaxf(s, 0.0f), 1.0f);
        o |= (uint32_t)__float2int_rn(s * 255.0f) << (8 * c);
    }
    *reinterpret_cast<uint32_t*>(rgba + ((size_t)f * G.fw * G.fh + (size_t)yy * G.fw + x) * 4) = o;
}

// ---- the frames as tensors (leon_pipeline.h, LEON_PIPELINE_OUTPUT_TENSOR, leon_pipeline_tensor_format) ----------------------------
// frame planes record (FrameOut layout) -> elements R, G, B, dense: [3][fh][fw] (CHW) or [fh][fw][3] (HWC, channels last) of 1-, 2- or
// 4-byte elements.  The colour value comes from the fused display's integer tables (chroma_terms / rgba_px above -- the arithmetic is
// not restated); the element is the colour value itself (1 byte: no table, none in LDS) or table[c][colour value] (3 x 256 elements,
// built by the host: tensor_table_build, in LDS beside the conversion tables -- fp16 and bf16 differ in the table only: the kernels
// are made per element SIZE).  One launch per window, blockIdx.z = frame: frame_ids[z] is the frame's index in both rings.  Threads
// are numbered linearly through the frame (k_rgba_twin4: a row-shaped grid leaves every eighth wave of a 1920-wide row half empty).
// Fast path (fw % 8 == 0): a lane takes 8 pixels x 2 rows -- one 8-byte Y load per row, 4 Cb + 4 Cr bytes for both -- or 4 pixels x
// 2 rows of 4-byte elements (k_rgba_twin4's shape).  The store side is what differs:
//   float CHW: 16 bytes per channel and row, so that a wave stores 64 x 16 B = 1 KB contiguous with ONE instruction.  (fp32 with 8
//     pixels per lane, two 16-byte stores 32 bytes apart, every instruction writing half of each line it touches: 18.5 ms per 1536
//     1080p frames, 2.3 TB/s -- measured, dropped.)
//   uint8 CHW: 8 bytes per channel and row -- one b64 store, a wave writes 512 contiguous bytes per instruction.
//   HWC: a lane's row piece is 24 / 48 / 48 contiguous bytes (1- / 2- / 4-byte elements).  Stored from the lane that made it that is
//     three instructions whose lanes lie 24 or 48 bytes apart, each writing a third of every line it touches (the shape recorded
//     above as measured and dropped for fp32).  So the wave's 64 pieces (1536 B / 3 KB / 3 KB, contiguous in the frame but
//     for the seam where the wave crosses into the next row pair) change lanes through the wave's LDS strip: written at lane * piece,
//     read back at (j * 64 + lane) * third-of-a-piece, j = 0 .. 2 -- so store instruction j writes the thirds 64 j .. 64 j + 63 in
//     order, 64 x 16 B = 1 KB contiguous (64 x 8 B = 512 B for uint8: a third of 24 bytes).  A third never straddles two pieces, so
//     its address is its source lane's row offset (ds_bpermute) plus 0, 1 or 2 thirds.  LDS banks: pieces of 12 dwords written as
//     b128 by groups of 8 lanes land on 32 different banks (12 l mod 32, l = 0 .. 7: 0 12 24 4 16 28 8 20, 4 dwords each), pieces of
//     6 dwords written as b64 by groups of 16 lanes too (6 l mod 32 covers every even bank once); the reads are contiguous.
//     Rows go one after the other through the same strip (both at once would put the 2- and 4-byte kernels over 20 KB).
// Other even widths: a lane takes one 2 x 2 quad, element stores.  The planes are read once and the tensor is never read again here:
// both non-temporal.  An odd frame height leaves the last row at the CPU twin's fill value 255 (its quad loop covers fh >> 1 row
// pairs): table[c][255].  The tensor's buffer resource ends with the frame: the second row of an HWC lane in the fill row pair, and
// anything a wrong offset would reach behind the frame, is dropped by the bounds check.
static constexpr int kLayoutChw = 0, kLayoutHwc = 1;          // = LEON_TENSOR_LAYOUT_*
// what both tensor kernels find a frame's planes and its tensor by
struct RingGeom {
    uint32_t luma_stride, chroma_stride, cb_off, cr_off;      // FrameOut
    uint32_t planes_pitch_lo, planes_pitch_hi, tensor_pitch_lo, tensor_pitch_hi;      // bytes between ring frames
};
struct TensorGeom {
    int32_t fw, fh;
    uint32_t per_row, n_items;           // lanes per row pair (lane_px pixels each), lanes per frame ((fh + 1) / 2 row pairs)
    RingGeom ring;
    int32_t fast;                        // fw % 8 == 0
};
template <int EB> struct ElemOf { typedef uint8_t type; };
template <> struct ElemOf<2> { typedef uint16_t type; };
template <> struct ElemOf<4> { typedef uint32_t type; };
// pixels per lane and row on the fast path
constexpr int lane_px(int eb) { return eb == 4 ? 4 : 8; }
// bytes of a lane's row piece in the HWC layout, and of the wave's exchange strip
constexpr int image_piece_bytes(int eb) { return lane_px(eb) * 3 * eb; }
constexpr int image_strip_bytes(int eb, int layout) { return layout == kLayoutHwc ? 64 * image_piece_bytes(eb) : 0; }

// The conversion tables into LDS as k_recon_display loads them (1 KB chunks straight into LDS); the caller waits (wait_vmem_all) and syncs
__device__ __forceinline__ void display_lut_to_lds(int32_t* lut_s, const Tables* T)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane0 = threadIdx.x & 63;
    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc((void*)T->rgba_lut, 0, kLdsLut, 0x00020000);
    for (int c = wave; c < kLdsLut / 1024; c += kRgbaBlock / 64)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(lrs, (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(lut_s) + c * 1024), 16,
                                                 (int)(lane0 * 16u), c * 1024, 0, 0);
}
// The CPU twin's RGBA dwords (A = 255) of 4 pixels of one row: Y samples y4, two chroma pairs; fill: the twin's fill row, 255
__device__ __forceinline__ void tensor_px4(const char* lut, uint32_t y4, const ChromaTerms& c0, const ChromaTerms& c1, bool fill, uint32_t two, uint32_t (&px)[4])
{
    const int opaque = 255 << kLutShift;
    px[0] = rgba_px<0>(lut, y4, c0, opaque, two); px[1] = rgba_px<1>(lut, y4, c0, opaque, two);
    px[2] = rgba_px<2>(lut, y4, c1, opaque, two); px[3] = rgba_px<3>(lut, y4, c1, opaque, two);
    if (fill) px[0] = px[1] = px[2] = px[3] = 0xffffffffu;
}
// ... of 8 pixels: Y samples y8, the four chroma pairs' terms
__device__ __forceinline__ void tensor_px8(const char* lut, v2u y8, const ChromaTerms (&c)[4], bool fill, uint32_t two, uint32_t (&px)[8])
{
    const int opaque = 255 << kLutShift;
    px[0] = rgba_px<0>(lut, y8.x, c[0], opaque, two); px[1] = rgba_px<1>(lut, y8.x, c[0], opaque, two);
    px[2] = rgba_px<2>(lut, y8.x, c[1], opaque, two); px[3] = rgba_px<3>(lut, y8.x, c[1], opaque, two);
    px[4] = rgba_px<0>(lut, y8.y, c[2], opaque, two); px[5] = rgba_px<1>(lut, y8.y, c[2], opaque, two);
    px[6] = rgba_px<2>(lut, y8.y, c[3], opaque, two); px[7] = rgba_px<3>(lut, y8.y, c[3], opaque, two);
    if (fill) {
#pragma unroll
        for (int k = 0; k < 8; k++) px[k] = 0xffffffffu;
    }
}

template <int EB>
__device__ __forceinline__ uint32_t image_elem(const typename ElemOf<EB>::type* tab, uint32_t px, int ch)
{
    const uint32_t v = (px >> (8 * ch)) & 255u;
    if constexpr (EB == 1) return v;
    else return tab[ch * 256 + v];
}

// One row of a lane, CHW: `off` = its first element in a channel plane; in: false stores nothing
// fp32: 4 pixels -> 16 bytes per channel
__device__ __forceinline__ void tensor_row4_f32(const uint32_t* tab, const uint32_t (&px)[4], __amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t plane_elems, bool in)
{
    const uint32_t oob = in ? 0u : kOobBit;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const v4u e = {image_elem<4>(tab, px[0], ch), image_elem<4>(tab, px[1], ch), image_elem<4>(tab, px[2], ch), image_elem<4>(tab, px[3], ch)};
        __builtin_amdgcn_raw_buffer_store_b128(e, rs, (int)((((uint32_t)ch * plane_elems + off) * 4u) | oob), 0, kAuxFrameStore);
    }
}
// 16-bit elements: 8 pixels -> 16 bytes per channel
__device__ __forceinline__ void tensor_row8(const uint16_t* tab, const uint32_t (&px)[8], __amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t plane_elems, bool in)
{
    const uint32_t oob = in ? 0u : kOobBit;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) e[k] = image_elem<2>(tab, px[k], ch);
        __builtin_amdgcn_raw_buffer_store_b128(v4u{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)}, rs,
                                               (int)((((uint32_t)ch * plane_elems + off) * 2u) | oob), 0, kAuxFrameStore);
    }
}
// uint8: 8 pixels -> 8 bytes per channel (`off` may carry kOobBit)
__device__ __forceinline__ void image_row_chw_u8(const uint32_t (&px)[8], __amdgpu_buffer_rsrc_t rs, uint32_t off, uint32_t plane_bytes)
{
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const int sh = 8 * ch;
        const uint32_t lo = ((px[0] >> sh) & 255u) | (((px[1] >> sh) & 255u) << 8) | (((px[2] >> sh) & 255u) << 16) | (((px[3] >> sh) & 255u) << 24);
        const uint32_t hi = ((px[4] >> sh) & 255u) | (((px[5] >> sh) & 255u) << 8) | (((px[6] >> sh) & 255u) << 16) | (((px[7] >> sh) & 255u) << 24);
        __builtin_amdgcn_raw_buffer_store_b64(v2u{lo, hi}, rs, (int)((uint32_t)ch * plane_bytes + off), 0, kAuxFrameStore);
    }
}

// One row piece of a lane, HWC: NPX pixels -> the wave's strip -> three store instructions of contiguous thirds.  `rowoff`: byte offset
// of this lane's piece in the frame (kOobBit: none); strip: the wave's; lane: 0 .. 63.  All 64 lanes take part.
template <int EB, int NPX>
__device__ __forceinline__ void image_row_hwc(const typename ElemOf<EB>::type* tab, const uint32_t (&px)[NPX], char* strip, int lane,
                                              __amdgpu_buffer_rsrc_t rs, uint32_t rowoff)
{
    constexpr int kPiece = NPX * 3 * EB, kThird = kPiece / 3;
    static_assert(kPiece == image_piece_bytes(EB) && (kThird == 8 || kThird == 16), "a third is one b64 or b128 store");
    uint32_t d[kPiece / 4];
    if constexpr (EB == 1) {
#pragma unroll
        for (int g = 0; g < NPX / 4; g++) {          // 4 pixels: R G B R | G B R G | B R G B
            const uint32_t p0 = px[4 * g] & 0xffffffu, p1 = px[4 * g + 1] & 0xffffffu, p2 = px[4 * g + 2] & 0xffffffu, p3 = px[4 * g + 3] & 0xffffffu;
            d[3 * g] = p0 | (p1 << 24);
            d[3 * g + 1] = (p1 >> 8) | (p2 << 16);
            d[3 * g + 2] = (p2 >> 16) | (p3 << 8);
        }
    } else if constexpr (EB == 2) {
#pragma unroll
        for (int i = 0; i < kPiece / 4; i++)
            d[i] = image_elem<EB>(tab, px[(2 * i) / 3], (2 * i) % 3) | (image_elem<EB>(tab, px[(2 * i + 1) / 3], (2 * i + 1) % 3) << 16);
    } else {
#pragma unroll
        for (int i = 0; i < kPiece / 4; i++) d[i] = image_elem<EB>(tab, px[i / 3], i % 3);
    }
    char* mine = strip + lane * kPiece;
    if constexpr (kThird == 8) {
#pragma unroll
        for (int j = 0; j < 3; j++) *reinterpret_cast<v2u*>(mine + 8 * j) = v2u{d[2 * j], d[2 * j + 1]};
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) *reinterpret_cast<v4u*>(mine + 16 * j) = v4u{d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3]};
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int k = j * 64 + lane;          // the wave's third k: piece k / 3, part k % 3
        const int from = k / 3, part = k - 3 * from;
        const uint32_t at = (uint32_t)__builtin_amdgcn_ds_bpermute(from * 4, (int)rowoff) + (uint32_t)(part * kThird);
        if constexpr (kThird == 8) __builtin_amdgcn_raw_buffer_store_b64(*reinterpret_cast<const v2u*>(strip + k * 8), rs, (int)at, 0, kAuxFrameStore);
        else __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const v4u*>(strip + k * 16), rs, (int)at, 0, kAuxFrameStore);
    }
    wave_sync();          // the strip is free for the next row
}

template <int EB, int LAYOUT>
__global__ __launch_bounds__(kRgbaBlock) void k_tensor(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ tensor_ring, const uint32_t* __restrict__ frame_ids,
                                                       const uint32_t* __restrict__ table, const Tables* __restrict__ T, TensorGeom G)
{
    typedef typename ElemOf<EB>::type Elem;
    constexpr int kNpx = lane_px(EB);
    constexpr int kStrip = image_strip_bytes(EB, LAYOUT);
    __shared__ __attribute__((aligned(16))) int32_t lut_s[kLdsLut / 4];
    __shared__ __attribute__((aligned(16))) Elem tab_s[EB == 1 ? 16 : 3 * 256];
    __shared__ __attribute__((aligned(16))) char strip_s[kStrip ? (kRgbaBlock / 64) * kStrip : 16];
    {   // the conversion tables, the element table through registers
        display_lut_to_lds(lut_s, T);
        if constexpr (EB != 1) {
            constexpr int kDwords = 3 * 256 * EB / 4;
            for (int i = threadIdx.x; i < kDwords; i += kRgbaBlock) reinterpret_cast<uint32_t*>(tab_s)[i] = table[i];
        }
        wait_vmem_all();
        __syncthreads();
    }
    const uint32_t idx_raw = blockIdx.x * (uint32_t)kRgbaBlock + threadIdx.x;
    const bool valid = idx_raw < G.n_items;
    if constexpr (LAYOUT == kLayoutChw) {
        if (!valid) return;          // cheaper for the CHW stores: with it `valid` below is a constant
    }
    const uint32_t idx = valid ? idx_raw : 0u;          // HWC (the exchange needs all 64 lanes of a wave): lanes behind the frame load what lane 0 loads and store nothing
    const char* lut = reinterpret_cast<const char*>(lut_s);
    const uint32_t pair = idx / G.per_row, col = idx - pair * G.per_row;
    const uint32_t fid = frame_ids[blockIdx.z];
    const uint8_t* src = planes_ring + (size_t)fid * join64(G.ring.planes_pitch_lo, G.ring.planes_pitch_hi);
    uint8_t* dst = tensor_ring + (size_t)fid * join64(G.ring.tensor_pitch_lo, G.ring.tensor_pitch_hi);
    const uint32_t r0 = 2u * pair, fw = (uint32_t)G.fw, fh = (uint32_t)G.fh;
    const bool has_r1 = r0 + 1u < fh;                    // false: the last row of an odd height, left at 255 by the twin
    const uint32_t plane_elems = fw * fh;
    uint32_t two = 2u, three = 3u;                       // SDWA shift counts live in registers (display_half)
    asm("" : "+v"(two), "+v"(three));
    const uint8_t* yrow = src + (size_t)r0 * G.ring.luma_stride;
    const uint8_t* cbrow = src + G.ring.cb_off + (size_t)pair * G.ring.chroma_stride;
    const uint8_t* crrow = src + G.ring.cr_off + (size_t)pair * G.ring.chroma_stride;
    if (G.fast) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)(3u * plane_elems * EB), 0x00020000);
        const uint32_t oob = valid ? 0u : kOobBit;
        uint32_t pa[kNpx], pb[kNpx];
        if constexpr (kNpx == 4) {
            const uint32_t y0 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(yrow + 4u * col));
            const uint32_t y1 = has_r1 ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(yrow + G.ring.luma_stride + 4u * col)) : 0u;
            const uint32_t cb2 = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(cbrow + 2u * col));
            const uint32_t cr2 = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(crrow + 2u * col));
            const ChromaTerms c0 = chroma_terms<0>(lut, cb2, cr2, three), c1 = chroma_terms<1>(lut, cb2, cr2, three);
            tensor_px4(lut, y0, c0, c1, !has_r1, two, pa);
            tensor_px4(lut, y1, c0, c1, false, two, pb);
        } else {
            const v2u y0 = __builtin_nontemporal_load(reinterpret_cast<const v2u*>(yrow + 8u * col));
            const v2u y1 = has_r1 ? __builtin_nontemporal_load(reinterpret_cast<const v2u*>(yrow + G.ring.luma_stride + 8u * col)) : v2u{0u, 0u};
            const uint32_t cb4 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(cbrow + 4u * col));
            const uint32_t cr4 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(crrow + 4u * col));
            const ChromaTerms c[4] = {chroma_terms<0>(lut, cb4, cr4, three), chroma_terms<1>(lut, cb4, cr4, three),
                                      chroma_terms<2>(lut, cb4, cr4, three), chroma_terms<3>(lut, cb4, cr4, three)};
            tensor_px8(lut, y0, c, !has_r1, two, pa);
            tensor_px8(lut, y1, c, false, two, pb);
        }
        const uint32_t off = r0 * fw + (uint32_t)kNpx * col;          // the lane's first pixel
        if constexpr (LAYOUT == kLayoutHwc) {
            char* strip = strip_s + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kStrip;
            const int lane = threadIdx.x & 63;
            const uint32_t rowoff = (off * 3u * EB) | oob;
            image_row_hwc<EB, kNpx>(tab_s, pa, strip, lane, rs, rowoff);
            image_row_hwc<EB, kNpx>(tab_s, pb, strip, lane, rs, rowoff + fw * 3u * EB);          // (behind the frame without a second row)
        } else if constexpr (EB == 4) {
            tensor_row4_f32(tab_s, pa, rs, off, plane_elems, valid);
            tensor_row4_f32(tab_s, pb, rs, off + fw, plane_elems, valid && has_r1);
        } else if constexpr (EB == 2) {
            tensor_row8(tab_s, pa, rs, off, plane_elems, valid);
            tensor_row8(tab_s, pb, rs, off + fw, plane_elems, valid && has_r1);
        } else {
            image_row_chw_u8(pa, rs, off | oob, plane_elems);
            image_row_chw_u8(pb, rs, (off + fw) | (valid && has_r1 ? 0u : kOobBit), plane_elems);
        }
    } else if (valid) {
        const uint32_t y0 = *reinterpret_cast<const uint16_t*>(yrow + 2u * col);
        const uint32_t y1 = has_r1 ? *reinterpret_cast<const uint16_t*>(yrow + G.ring.luma_stride + 2u * col) : 0u;
        const ChromaTerms c0 = chroma_terms<0>(lut, (uint32_t)cbrow[col], (uint32_t)crrow[col], three);
        const int opaque = 255 << kLutShift;
        uint32_t px[4] = {rgba_px<0>(lut, y0, c0, opaque, two), rgba_px<1>(lut, y0, c0, opaque, two),
                          rgba_px<0>(lut, y1, c0, opaque, two), rgba_px<1>(lut, y1, c0, opaque, two)};
        if (!has_r1) px[0] = px[1] = 0xffffffffu;
        Elem* out = reinterpret_cast<Elem*>(dst);
        // element strides of a channel, a pixel and a row
        const size_t sc = LAYOUT == kLayoutHwc ? 1 : plane_elems, sx = LAYOUT == kLayoutHwc ? 3 : 1, sy = (size_t)fw * sx;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            Elem* o = out + (size_t)ch * sc + (size_t)r0 * sy + (size_t)(2u * col) * sx;
            __builtin_nontemporal_store((Elem)image_elem<EB>(tab_s, px[0], ch), o);
            __builtin_nontemporal_store((Elem)image_elem<EB>(tab_s, px[1], ch), o + sx);
            if (has_r1) {
                __builtin_nontemporal_store((Elem)image_elem<EB>(tab_s, px[2], ch), o + sy);
                __builtin_nontemporal_store((Elem)image_elem<EB>(tab_s, px[3], ch), o + sy + sx);
            }
        }
    }
}

// ---- the frames as tensors at a model's input size (leon_pipeline.h, leon_pipeline_tensor_resize) -----------------------
// frame planes record -> [3][oh][ow] elements: a crop box of the frame resampled with the host's integer tables (per axis first[o],
// count[o], weights[o][taps], 22 fractional bits: leon_pipeline_resize_weights is the definition), horizontal pass first with an
// 8-bit result, then vertical, then the element table of k_tensor.  One launch per window, blockIdx.z = frame as in k_tensor.
// A workgroup owns kResTileX x kResTileY output pixels.  Their source footprint -- columns first_x[tile's first] (rounded down to
// 8) .. end_x[tile's last], rows first_y .. end_y -- is walked in chunks of whole source rows that fit the staging buffer (a
// footprint that does not fit is split, never refused: ratio 16 stages 6 rows of 544 pixels at a time).  Per chunk: (1) every
// source sample is loaded once (non-temporal: 8 Y bytes per row and 4 Cb + 4 Cr bytes for a row pair per lane, k_tensor's shape)
// and converted once with chroma_terms / rgba_px into RGBX dwords in LDS; (2) the horizontal pass, a lane per (output column, row
// pair), writes packed 8-bit results to the tile's h rows in LDS -- two rows per lane share every weight read.  After the last
// chunk (3) the vertical pass, a lane per output pixel, reads h, looks the three elements up and stores them.  Products are
// v_mad_u32_u24 (triangle: weights <= 2^22, samples < 2^8; the sums stay below 2^31).  Rows at and beyond the frame height are never loaded
// (kOobBit) and never tapped; the last row of an odd height is the CPU twin's fill row, 255.
// The filter (LEON_RESIZE_*) is a traits struct: what the LDS is sized for and the sign of the arithmetic.  Triangle weights are
// never negative; bicubic ones are (down to about -0.074 * 2^22), so its sums are signed -- v_mad_i32_i24, an arithmetic shift and
// a clamp on both sides (v_med3_i32) -- and its support of 2 doubles the taps: k_resample<EB, LAYOUT, F> is instantiated per filter,
// and the triangle kernels are compiled exactly as they were before there was a second one.
static constexpr int kResTileX = 32, kResTileY = 8;          // kResTileX * kResTileY = kRgbaBlock: the vertical pass is one pixel per lane
static constexpr int kResStagePx = 4096;                     // staging dwords: 6 rows of the widest footprint (triangle: 31 * 16 + 33 + 14 <= 544 columns, 578 dwords
                                                             // padded; bicubic: 31 * 16 + 65 + 14 <= 576 columns, 612 dwords padded)
static constexpr int kResWeightShift = 22;
struct ResTriangle {
    static constexpr int kMaxTaps = 33;                      // = LEON_RESIZE_MAX_TAPS: 2 * 16 + 1
    static constexpr int kHRows = 160;                       // h rows of a tile: <= 7 * 16 + 33 + 2 = 147, and one spare for the odd tail
    static constexpr bool kSigned = false;
    typedef uint32_t Acc;
};
struct ResCubic {
    static constexpr int kMaxTaps = 65;                      // = LEON_RESIZE_MAX_TAPS_BICUBIC: 4 * 16 + 1
    static constexpr int kHRows = 192;                       // <= 7 * 16 + 65 + 2 = 179, and the spare row
    static constexpr bool kSigned = true;
    typedef int32_t Acc;
};
struct ResampleGeom {
    int32_t fw, fh, ow, oh;
    int32_t taps_x, taps_y;              // row length of the weight tables
    uint32_t off_cx, off_wx, off_fy, off_cy, off_wy;          // int32 offsets in the table buffer (first_x at 0)
    RingGeom ring;
};
// Where the resampled image lies in its tensor (leon_pipeline_tensor_canvas): only the store addresses of resample_body ask.
// ImageIsTensor: the tensor IS the image (k_resample) -- its overloads below are constants and fields of ResampleGeom, and those
// kernels come out instruction for instruction as before there was a canvas.  CanvasGeom: the image at (x, y) in a width x height tensor (k_letterbox).
struct ImageIsTensor {
};
struct CanvasGeom {
    int32_t cw, ch, x, y;
    uint32_t pad;                        // the pad pixel's 8-bit R, G, B in bits 0, 8, 16
};
__device__ __forceinline__ uint32_t tensor_plane_elems(const ResampleGeom& G, const ImageIsTensor&) { return (uint32_t)G.ow * (uint32_t)G.oh; }
__device__ __forceinline__ uint32_t tensor_plane_elems(const ResampleGeom&, const CanvasGeom& c) { return (uint32_t)c.cw * (uint32_t)c.ch; }
__device__ __forceinline__ int tensor_width(const ResampleGeom& G, const ImageIsTensor&) { return G.ow; }
__device__ __forceinline__ int tensor_width(const ResampleGeom&, const CanvasGeom& c) { return c.cw; }
__device__ __forceinline__ int tensor_left(const ImageIsTensor&) { return 0; }
__device__ __forceinline__ int tensor_left(const CanvasGeom& c) { return c.x; }
__device__ __forceinline__ int tensor_top(const ImageIsTensor&) { return 0; }
__device__ __forceinline__ int tensor_top(const CanvasGeom& c) { return c.y; }
struct LetterboxGeom {
    ResampleGeom image;
    CanvasGeom canvas;
};

// Column c of a staged row lies at dword c + (c >> 4): the horizontal pass's lanes are the tile's output columns and read columns
// about `ratio` apart -- at a ratio of 16 or 8 unpadded rows would put all of them on two or four LDS banks; one pad dword per 16
// turns those strides into 17 and 8.5.
__host__ __device__ constexpr int resample_col(int c) { return c + (c >> 4); }
__device__ __forceinline__ uint32_t resample_px(uint32_t ar, uint32_t ag, uint32_t ab)
{
    return min(ar >> kResWeightShift, 255u) | (min(ag >> kResWeightShift, 255u) << 8) | (min(ab >> kResWeightShift, 255u) << 16);
}
// signed sums: floor (arithmetic shift), then clamped on both sides
__device__ __forceinline__ uint32_t resample_px(int32_t ar, int32_t ag, int32_t ab)
{
    const int32_t r = min(max(ar >> kResWeightShift, 0), 255), g = min(max(ag >> kResWeightShift, 0), 255), b = min(max(ab >> kResWeightShift, 0), 255);
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}
// acc + weight * sample, sample < 2^8: |weight| < 2^23 and the sums inside 32 bits are the table builder's promise (resize_axis_build)
__device__ __forceinline__ uint32_t resample_mad(int32_t w, uint32_t sample, uint32_t acc) { return __umul24((uint32_t)w, sample) + acc; }
__device__ __forceinline__ int32_t resample_mad(int32_t w, uint32_t sample, int32_t acc) { return __mul24(w, (int32_t)sample) + acc; }

// Two store forms.  Float CHW (EB = 2 or 4): one element store per lane and channel.  8-bit elements and the channels-last layout
// (leon_pipeline_tensor_format with leon_pipeline_tensor_resize): the tile leaves through LDS: once the vertical pass has read them the h rows
// are dead, and the tile's elements are packed there in memory order -- HWC: the 8 tile rows, 96 elements each; uint8 CHW: 3 x 8
// channel rows of 32 bytes -- every row at the offset its first byte has in its 16-byte line of the frame (the tensor starts on a
// 256-byte boundary).  A lane then takes one aligned 16-byte line of one row: inside the row it is ONE b128 store, at the row's two
// ends its elements go one by one (a row's start is aligned to nothing: out_width is any number).
// In a canvas (`C`: ImageIsTensor or CanvasGeom) only the store addresses move: the tiles are numbered from the image's origin, a
// tile row still stores the bytes of [g0, g1) and nothing else, its row stride and plane size are the canvas's.
// Where a workgroup's frame and tensor lie (`W`) is asked once, behind the table loads.  RingFrame: frame_ids[blockIdx.z] of the
// pipeline's rings (k_resample, k_letterbox).  RegionFrame: the two addresses k_regions / k_fitted made from the region's descriptor.
struct FramePair {
    const uint8_t* src;
    uint8_t* dst;
};
struct RingFrame {
    const uint8_t* __restrict__ planes_ring;
    uint8_t* __restrict__ tensor_ring;
    const uint32_t* __restrict__ frame_ids;
    __device__ __forceinline__ FramePair locate(const ResampleGeom& G) const
    {
        const uint32_t fid = frame_ids[blockIdx.z];
        return FramePair{planes_ring + (size_t)fid * join64(G.ring.planes_pitch_lo, G.ring.planes_pitch_hi),
                         tensor_ring + (size_t)fid * join64(G.ring.tensor_pitch_lo, G.ring.tensor_pitch_hi)};
    }
};
struct RegionFrame {
    FramePair at;
    __device__ __forceinline__ FramePair locate(const ResampleGeom&) const { return at; }
};
template <int EB, int LAYOUT, class F, class C, class W>
__device__ __forceinline__ void resample_body(const W& where, const uint32_t* __restrict__ table, const Tables* __restrict__ T, const int32_t* __restrict__ rt,
                                              const ResampleGeom& G, const C& place)
{
    typedef typename ElemOf<EB>::type Elem;
    typedef typename F::Acc Acc;
    static_assert(kResTileX * kResTileY == kRgbaBlock && kResTileX == 32, "lane = (tid & 31, tid >> 5)");
    __shared__ __attribute__((aligned(16))) int32_t lut_s[kLdsLut / 4];
    __shared__ __attribute__((aligned(16))) Elem tab_s[EB == 1 ? 16 : 3 * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage_s[kResStagePx];
    __shared__ __attribute__((aligned(16))) uint32_t h_s[F::kHRows * kResTileX];
    __shared__ int32_t wx_s[kResTileX * F::kMaxTaps], wy_s[kResTileY * F::kMaxTaps];
    __shared__ int32_t fx_s[kResTileX], nx_s[kResTileX], fy_s[kResTileY], ny_s[kResTileY];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * kResTileX, oy0 = blockIdx.y * kResTileY;
    const int nox = min(kResTileX, G.ow - ox0), noy = min(kResTileY, G.oh - oy0);
    const int32_t* first_x = rt;
    const int32_t* count_x = rt + G.off_cx;
    const int32_t* first_y = rt + G.off_fy;
    const int32_t* count_y = rt + G.off_cy;
    {   // the conversion tables and the element table as k_tensor loads them, then the tile's slices of the resampling tables
        display_lut_to_lds(lut_s, T);
        if constexpr (EB != 1) {
            constexpr int kDwords = 3 * 256 * EB / 4;
            for (int i = tid; i < kDwords; i += kRgbaBlock) reinterpret_cast<uint32_t*>(tab_s)[i] = table[i];
        }
        const int32_t* wxg = rt + G.off_wx + (size_t)ox0 * G.taps_x;
        for (int i = tid; i < nox * G.taps_x; i += kRgbaBlock) wx_s[i] = wxg[i];
        const int32_t* wyg = rt + G.off_wy + (size_t)oy0 * G.taps_y;
        for (int i = tid; i < noy * G.taps_y; i += kRgbaBlock) wy_s[i] = wyg[i];
        if (tid < nox) { fx_s[tid] = first_x[ox0 + tid]; nx_s[tid] = count_x[ox0 + tid]; }
        if (tid < noy) { fy_s[tid] = first_y[oy0 + tid]; ny_s[tid] = count_y[oy0 + tid]; }
        wait_vmem_all();
        __syncthreads();
    }
    // the tile's source footprint (first and end are monotone in o)
    const int cx0 = first_x[ox0] & ~7;
    const int sw = (first_x[ox0 + nox - 1] + count_x[ox0 + nox - 1] - cx0 + 7) & ~7;      // staged columns: whole 8-pixel groups, inside luma_stride
    const int ry0 = first_y[oy0] & ~1;                                                    // even: a row pair shares its chroma row
    const int ry1 = first_y[oy0 + noy - 1] + count_y[oy0 + noy - 1];                      // <= fh
    const int sw8 = sw >> 3;
    const int swp = resample_col(sw);                                                     // dwords of a staged row
    const int rc = (kResStagePx / swp) & ~1;                                              // rows per chunk
    const int pair_t = tid / sw8, col_t = tid - pair_t * sw8;                             // this lane's first item of a chunk ...
    const int pair_step = kRgbaBlock / sw8, col_step = kRgbaBlock - pair_step * sw8;      // ... and the way to its next

    const char* lut = reinterpret_cast<const char*>(lut_s);
    const FramePair frame = where.locate(G);
    const uint8_t* src = frame.src;
    uint8_t* dst = frame.dst;
    const __amdgpu_buffer_rsrc_t prs = buf_rsrc(src);
    uint32_t two = 2u, three = 3u;                       // SDWA shift counts live in registers (display_half)
    asm("" : "+v"(two), "+v"(three));
    const int o = tid & 31, sub = tid >> 5;

    for (int r = ry0; r < ry1; r += rc) {
        const int rows = min(rc, ry1 - r);
        // (1) rows r .. r + rows - 1 (whole pairs), columns cx0 .. cx0 + sw - 1 -> RGBX in stage_s[row][swp]
        const int n_pairs = (rows + 1) >> 1;
        for (int pair = pair_t, col = col_t; pair < n_pairs;) {
            const int row = r + 2 * pair;
            const bool in0 = row < G.fh, in1 = row + 1 < G.fh;
            const uint32_t yo = (uint32_t)row * G.ring.luma_stride + (uint32_t)(cx0 + 8 * col);
            const uint32_t co = (uint32_t)(row >> 1) * G.ring.chroma_stride + (uint32_t)((cx0 >> 1) + 4 * col);
            const v2u y0 = __builtin_amdgcn_raw_buffer_load_b64(prs, (int)(in0 ? yo : kOobBit), 0, kAuxStreamOnce);
            const v2u y1 = __builtin_amdgcn_raw_buffer_load_b64(prs, (int)(in1 ? yo + G.ring.luma_stride : kOobBit), 0, kAuxStreamOnce);
            const uint32_t cb4 = __builtin_amdgcn_raw_buffer_load_b32(prs, (int)(in0 ? G.ring.cb_off + co : kOobBit), 0, kAuxStreamOnce);
            const uint32_t cr4 = __builtin_amdgcn_raw_buffer_load_b32(prs, (int)(in0 ? G.ring.cr_off + co : kOobBit), 0, kAuxStreamOnce);
            const ChromaTerms c[4] = {chroma_terms<0>(lut, cb4, cr4, three), chroma_terms<1>(lut, cb4, cr4, three),
                                      chroma_terms<2>(lut, cb4, cr4, three), chroma_terms<3>(lut, cb4, cr4, three)};
            uint32_t a[8], b[8];
            tensor_px8(lut, y0, c, !in1, two, a);        // (!in1: the last row of an odd height, left at 255 by the twin)
            tensor_px8(lut, y1, c, false, two, b);
            uint32_t* s0 = stage_s + (2 * pair) * swp + resample_col(8 * col);            // (8 columns of one group of 16: contiguous)
#pragma unroll
            for (int k = 0; k < 8; k++) { s0[k] = a[k]; s0[swp + k] = b[k]; }
            pair += pair_step; col += col_step;
            if (col >= sw8) { col -= sw8; pair++; }
        }
        __syncthreads();
        // (2) horizontal pass: output column o of the tile, staged rows 2 * sub, 2 * sub + 1, then 16 rows on
        if (o < nox) {
            const int n = nx_s[o];
            const int32_t* w = wx_s + o * G.taps_x;
            for (int rr = 2 * sub; rr < rows; rr += 2 * (kRgbaBlock / 32)) {
                const uint32_t* s = stage_s + rr * swp;
                const int c0 = fx_s[o] - cx0;
                Acc ar = (Acc)1 << (kResWeightShift - 1), ag = ar, ab = ar, br = ar, bg = ar, bb = ar;
                for (int k = 0; k < n; k++) {
                    const int at = resample_col(c0 + k);
                    const int32_t wk = w[k];
                    const uint32_t pa = s[at], pb = s[at + swp];
                    ar = resample_mad(wk, pa & 255u, ar); ag = resample_mad(wk, (pa >> 8) & 255u, ag); ab = resample_mad(wk, (pa >> 16) & 255u, ab);
                    br = resample_mad(wk, pb & 255u, br); bg = resample_mad(wk, (pb >> 8) & 255u, bg); bb = resample_mad(wk, (pb >> 16) & 255u, bb);
                }
                uint32_t* hrow = h_s + (r - ry0 + rr) * kResTileX + o;       // (the second row of an odd tail lands in the spare row)
                hrow[0] = resample_px(ar, ag, ab);
                hrow[kResTileX] = resample_px(br, bg, bb);
            }
        }
        __syncthreads();
    }
    // (3) vertical pass: output pixel (ox0 + o, oy0 + sub)
    const bool valid = o < nox && sub < noy;
    Acc ar = (Acc)1 << (kResWeightShift - 1), ag = ar, ab = ar;
    if (valid) {
        const int n = ny_s[sub];
        const int32_t* w = wy_s + sub * G.taps_y;
        const uint32_t* hcol = h_s + (fy_s[sub] - ry0) * kResTileX + o;
        for (int k = 0; k < n; k++) {
            const int32_t wk = w[k];
            const uint32_t pa = hcol[k * kResTileX];
            ar = resample_mad(wk, pa & 255u, ar); ag = resample_mad(wk, (pa >> 8) & 255u, ag); ab = resample_mad(wk, (pa >> 16) & 255u, ab);
        }
    }
    const uint32_t px = resample_px(ar, ag, ab);
    // the tensor's row stride and plane, the tile's origin in the tensor
    const uint32_t plane_elems = tensor_plane_elems(G, place);
    if constexpr (LAYOUT == kLayoutChw && EB != 1) {
        const __amdgpu_buffer_rsrc_t rs = buf_rsrc(dst);
        const uint32_t at = (uint32_t)(oy0 + sub + tensor_top(place)) * (uint32_t)tensor_width(G, place) + (uint32_t)(ox0 + o + tensor_left(place));
        const uint32_t oob = valid ? 0u : kOobBit;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const Elem e = tab_s[ch * 256 + ((px >> (8 * ch)) & 255u)];
            const uint32_t voff = (((uint32_t)ch * plane_elems + at) * (uint32_t)sizeof(Elem)) | oob;
            if constexpr (sizeof(Elem) == 4) __builtin_amdgcn_raw_buffer_store_b32(e, rs, (int)voff, 0, kAuxFrameStore);
            else __builtin_amdgcn_raw_buffer_store_b16(e, rs, (int)voff, 0, kAuxFrameStore);
        }
    } else {
        // rows of the tile in memory order: HWC 8 of 96 elements, uint8 CHW 3 x 8 of 32 bytes; 16 spare bytes for the row's place in its line
        constexpr bool kHwc = LAYOUT == kLayoutHwc;
        constexpr int kRowElems = kHwc ? 3 * kResTileX : kResTileX, kRowStride = kRowElems * EB + 16;
        constexpr int kRows = kHwc ? kResTileY : 3 * kResTileY, kLines = (kRowElems * EB + 15) / 16 + 1;
        constexpr int kLinesP2 = kLines <= 4 ? 4 : 32;          // work items of a row: a power of two of lanes
        static_assert(kRows * kRowStride <= (int)sizeof(h_s) && kLines <= kLinesP2 && kRows * kLinesP2 <= kRgbaBlock, "the packed tile fits the h rows, a lane per line");
        // byte offset in the frame of row `row` of the tile's rows (row = tile row, or channel * 8 + tile row)
        auto row_start = [&](int row) -> uint32_t {
            if constexpr (kHwc) return ((uint32_t)(oy0 + row + tensor_top(place)) * (uint32_t)tensor_width(G, place) + (uint32_t)(ox0 + tensor_left(place))) * 3u * EB;
            else return ((uint32_t)(row >> 3) * plane_elems + (uint32_t)(oy0 + (row & 7) + tensor_top(place)) * (uint32_t)tensor_width(G, place) + (uint32_t)(ox0 + tensor_left(place))) * EB;
        };
        char* pack = reinterpret_cast<char*>(h_s);
        __syncthreads();          // every lane has read its h column
        if (valid) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int row = kHwc ? sub : ch * kResTileY + sub;
                const int at = (int)(row_start(row) & 15u) + (kHwc ? (o * 3 + ch) * EB : o * EB);
                *reinterpret_cast<Elem*>(pack + row * kRowStride + at) = (Elem)image_elem<EB>(tab_s, px, ch);
            }
        }
        __syncthreads();
        const int row = tid / kLinesP2, line = tid & (kLinesP2 - 1);
        if (row < kRows && (kHwc ? row : (row & 7)) < noy) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)(3u * plane_elems * EB), 0x00020000);
            const uint32_t g0 = row_start(row), g1 = g0 + (uint32_t)(nox * (kHwc ? 3 : 1) * EB);      // the row's bytes in the frame
            const uint32_t a0 = (g0 & ~15u) + 16u * (uint32_t)line;                                   // this lane's line
            const char* from = pack + row * kRowStride + 16 * line;
            if (a0 >= g0 && a0 + 16u <= g1) __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const v4u*>(from), rs, (int)a0, 0, kAuxFrameStore);
            else if (a0 + 16u > g0 && a0 < g1) {
                // a line at an end of the row: the tile beside this one (and the row above or below) owns the line's other bytes and
                // writes them itself, so only the elements inside [g0, g1) may be stored -- one by one
                for (int e = 0; e < 16 / EB; e++) {
                    const uint32_t a = a0 + (uint32_t)(e * EB);
                    if (a < g0 || a >= g1) continue;
                    const Elem v = *reinterpret_cast<const Elem*>(from + e * EB);
                    if constexpr (EB == 4) __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)a, 0, kAuxFrameStore);
                    else if constexpr (EB == 2) __builtin_amdgcn_raw_buffer_store_b16(v, rs, (int)a, 0, kAuxFrameStore);
                    else __builtin_amdgcn_raw_buffer_store_b8(v, rs, (int)a, 0, kAuxFrameStore);
                }
            }
        }
    }
}


template <int EB, int LAYOUT, class F>
__global__ __launch_bounds__(kRgbaBlock) void k_resample(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ tensor_ring, const uint32_t* __restrict__ frame_ids,
                                                         const uint32_t* __restrict__ table, const Tables* __restrict__ T, const int32_t* __restrict__ rt,
                                                         ResampleGeom G)
{
    resample_body<EB, LAYOUT, F>(RingFrame{planes_ring, tensor_ring, frame_ids}, table, T, rt, G, ImageIsTensor{});
}

// ---- regions of delivered frames as a tensor batch (leon_pipeline.h, leon_pipeline_resample_regions) ---------------------
// blockIdx.z is the region, blockIdx.x / y the tiles of the out size all regions of a call share.  What k_resample has as launch
// constants a region has of its own -- the source frame, the destination, the tables of its box with their row lengths -- and a
// workgroup reads it from the region's descriptor (one address per workgroup: scalar loads), then runs resample_body.  Each region's
// tables are laid out as plan_resize lays out a pipeline's, `rt_base` int32 words into the call's table buffer.
// One family for both roads: the host writes descriptors whose status is 0, k_box_tables one of kRegion*.
struct RegionDesc {
    uint32_t frame_id;                   // index into the planes ring
    uint32_t rt_base;                    // int32 offset of the region's first_x in the table buffer
    uint32_t off_cx, off_wx, off_fy, off_cy, off_wy;          // as ResampleGeom's, from rt_base
    int32_t taps_x, taps_y;              // row lengths of this region's weight tables (taps_x odd)
    uint32_t dst_lo, dst_hi;             // byte offset of the region's tensor in the caller's buffer: index * pitch
    int32_t status;                      // 0 on the host road; k_box_tables: kRegion* (non-zero: the region's workgroups leave at once)
    int32_t iw, ih, ix, iy;              // k_fitted only: the region's image, iw x ih at (ix, iy) of its tensor (0 where the image is the tensor)
};                                       // 64 bytes
template <int EB, int LAYOUT, class F>
__global__ __launch_bounds__(kRgbaBlock) void k_regions(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ out, const RegionDesc* __restrict__ descs,
                                                        const uint32_t* __restrict__ table, const Tables* __restrict__ T, const int32_t* __restrict__ tabs,
                                                        ResampleGeom G)
{
    const RegionDesc& d = descs[blockIdx.z];
    if (d.status != kRegionOk) return;   // a refused region stores nothing anywhere
    G.taps_x = d.taps_x; G.taps_y = d.taps_y;
    G.off_cx = d.off_cx; G.off_wx = d.off_wx; G.off_fy = d.off_fy; G.off_cy = d.off_cy; G.off_wy = d.off_wy;
    const RegionFrame where{FramePair{planes_ring + (size_t)d.frame_id * join64(G.ring.planes_pitch_lo, G.ring.planes_pitch_hi), out + join64(d.dst_lo, d.dst_hi)}};
    resample_body<EB, LAYOUT, F>(where, table, T, tabs + d.rt_base, G, ImageIsTensor{});
}

// ---- regions whose boxes lie in device memory (leon_pipeline.h, leon_pipeline_resample_regions_device) -------------------
// Behind a detector that ran on the GPU nothing about a box is known on the host.  Per chunk of regions two launches in stream order
// over one scratch: k_box_tables judges each region and writes its descriptor and tables, k_regions<EB, LAYOUT, F> runs behind the
// descriptor's status word.
// k_box_tables: one workgroup per region.  The region's record is one address per workgroup (scalar loads); its status is
// region_axis_status and the rows' tap counts, which the workgroup reduces first (a lane takes every 256th output sample of both
// axes; two LDS words) -- the row length of a table is the largest count of its rows and has to be known before a weight is stored.
// A valid region's tables then lie as plan_resize lays out a pipeline's -- first_x | count_x | Wx | first_y | count_y | Wy, rows of
// taps_x | 1 and taps_y words, zero behind count[o] -- in the region's fixed slot of the scratch (slot_words: the filter's worst case
// for the out size, so no prefix sum and nothing read back).  A lane builds whole rows: the sum in index order first, then the
// weights from the same expressions once more (leon_resize_row.h; no array of doubles per lane).  fp64 throughout, a division per tap
// and another per weight, a row's words stored by one lane: measured, 4096 regions of 224 x 224 (triangle, ratio 1 .. 8) take 0.09 -
// 0.16 ms, a hundredth of the k_regions launch behind it.
struct BoxRecord {                       // = leon_pipeline_region
    int32_t frame, x, y, width, height, reserved[3];
};
struct BoxCall {
    int32_t fw, fh, ow, oh;
    int32_t n_frames, cubic;
    uint32_t slot_words;                 // int32 words of a region's slot in the table buffer
    uint32_t first;                      // the chunk's first region in the call: region i of the launch is written to (first + i) * pitch
    uint32_t pitch_lo, pitch_hi;
};
// this lane's share of an axis's rows: the largest count, INT32_MAX when resize_axis_build refuses one
__device__ __forceinline__ int32_t box_axis_most(const ResizeAxis& A, int32_t out_size)
{
    int32_t most = 0;
    for (int32_t o = (int32_t)threadIdx.x; o < out_size; o += kRgbaBlock) {
        const int32_t n = resize_row_window(A, o).n;
        most = max(most, resize_row_count_ok(n, A.cubic) ? n : INT32_MAX);
    }
    return most;
}
// row o of an axis: first, count and the `row_len` words at `row` (count <= row_len: the caller reduced the counts)
__device__ __forceinline__ void box_axis_row(const ResizeAxis& A, int32_t o, int32_t* __restrict__ first, int32_t* __restrict__ count, int32_t* __restrict__ row,
                                             int32_t row_len)
{
    const ResizeWindow R = resize_row_window(A, o);
    const double sum = resize_row_sum(A, R);
    first[o] = R.lo;
    count[o] = R.n;
    for (int32_t k = 0; k < R.n; k++) row[k] = resize_row_weight(resize_row_tap(A, R, k), sum);
    for (int32_t k = R.n; k < row_len; k++) row[k] = 0;
}
// What the tables of a region are built for (`FIT`).  BoxStretch: the call's out size, every region's (k_box_tables).  BoxLetterbox: the
// region's own image, the letterbox of its box in the call's out size -- the canvas (k_fit_tables); the rectangle goes into the
// descriptor's spare words and, for a region that is valid, to the caller's `rects`.  The slot of a region is sized for the canvas,
// which no image exceeds on either axis.
struct BoxStretch {
    __device__ __forceinline__ FitRect rect(const BoxRecord&, const BoxCall& c) const { return FitRect{c.ow, c.oh, 0, 0}; }
    __device__ __forceinline__ void place(RegionDesc&, const FitRect&, uint32_t) const {}
};
struct BoxLetterbox {
    int32_t* __restrict__ rects;         // n x 4 words (x, y, width, height) from the chunk's first region on, or NULL
    int32_t top_left;
    __device__ __forceinline__ FitRect rect(const BoxRecord& r, const BoxCall& c) const { return region_fit_rect(r.width, r.height, c.ow, c.oh, top_left != 0); }
    __device__ __forceinline__ void place(RegionDesc& d, const FitRect& f, uint32_t i) const
    {
        d.iw = f.ow; d.ih = f.oh; d.ix = f.x; d.iy = f.y;
        if (rects && threadIdx.x < 4) rects[(size_t)i * 4 + threadIdx.x] = threadIdx.x == 0 ? f.x : threadIdx.x == 1 ? f.y : threadIdx.x == 2 ? f.ow : f.oh;
    }
};
template <class FIT>
__device__ __forceinline__ void box_tables_body(const BoxRecord* __restrict__ boxes, const uint32_t* __restrict__ frame_ids, RegionDesc* __restrict__ descs,
                                                int32_t* __restrict__ tabs, int32_t* __restrict__ status_out, const BoxCall& c, const FIT& fit)
{
    __shared__ int32_t most_s[2];
    const uint32_t i = blockIdx.x;
    const BoxRecord r = boxes[i];
    const bool cubic = c.cubic != 0;
    const FitRect image = fit.rect(r, c);
    const int32_t ow = image.ow, oh = image.oh;
    int32_t status = kRegionOk, sx = kRegionOk, sy = kRegionOk;
    if (r.reserved[0] | r.reserved[1] | r.reserved[2]) status = kRegionReserved;
    else if (r.frame < 0 || r.frame >= c.n_frames) status = kRegionFrame;
    else {
        sx = region_axis_status(c.fw, r.x, r.width, ow, kRegionRatioX);
        sy = region_axis_status(c.fh, r.y, r.height, oh, kRegionRatioY);
    }
    // (the axes of a box that is refused are never evaluated: resize_axis stands on region_axis_status)
    const bool do_x = status == kRegionOk && sx == kRegionOk, do_y = status == kRegionOk && sy == kRegionOk;
    ResizeAxis X{}, Y{};
    if (do_x) X = resize_axis(c.fw, r.x, r.width, ow, cubic);
    if (do_y) Y = resize_axis(c.fh, r.y, r.height, oh, cubic);
    if (threadIdx.x < 2) most_s[threadIdx.x] = 0;
    __syncthreads();
    if (do_x) atomicMax(&most_s[0], box_axis_most(X, ow));
    if (do_y) atomicMax(&most_s[1], box_axis_most(Y, oh));
    __syncthreads();
    const int32_t most_x = most_s[0], most_y = most_s[1];
    if (status == kRegionOk)
        status = sx != kRegionOk ? sx : most_x == INT32_MAX ? kRegionTaps : sy != kRegionOk ? sy : most_y == INT32_MAX ? kRegionTaps : kRegionOk;
    RegionDesc d{};
    d.status = status;
    if (status == kRegionOk) {
        d.frame_id = frame_ids[r.frame];
        d.rt_base = i * c.slot_words;
        d.taps_x = most_x | 1; d.taps_y = most_y;
        d.off_cx = (uint32_t)ow;
        d.off_wx = d.off_cx + (uint32_t)ow;
        d.off_fy = d.off_wx + (uint32_t)ow * (uint32_t)d.taps_x;
        d.off_cy = d.off_fy + (uint32_t)oh;
        d.off_wy = d.off_cy + (uint32_t)oh;
        const uint64_t dst = (uint64_t)(c.first + i) * join64(c.pitch_lo, c.pitch_hi);
        d.dst_lo = (uint32_t)(dst & 0xffffffffu); d.dst_hi = (uint32_t)(dst >> 32);
        fit.place(d, image, i);
    }
    if (threadIdx.x == 0) {
        descs[i] = d;
        if (status_out) status_out[i] = status;
    }
    if (status != kRegionOk) return;
    int32_t* __restrict__ t = tabs + (size_t)d.rt_base;
    for (int32_t row = (int32_t)threadIdx.x; row < ow + oh; row += kRgbaBlock) {
        if (row < ow) box_axis_row(X, row, t, t + d.off_cx, t + d.off_wx + (size_t)row * (size_t)d.taps_x, d.taps_x);
        else box_axis_row(Y, row - ow, t + d.off_fy, t + d.off_cy, t + d.off_wy + (size_t)(row - ow) * (size_t)d.taps_y, d.taps_y);
    }
}
__global__ __launch_bounds__(kRgbaBlock) void k_box_tables(const BoxRecord* __restrict__ boxes, const uint32_t* __restrict__ frame_ids, RegionDesc* __restrict__ descs,
                                                           int32_t* __restrict__ tabs, int32_t* __restrict__ status_out, BoxCall c)
{
    box_tables_body(boxes, frame_ids, descs, tabs, status_out, c, BoxStretch{});
}
// (the name carries no other kernel family's: the resource tests count families by substring)
__global__ __launch_bounds__(kRgbaBlock) void k_fit_tables(const BoxRecord* __restrict__ boxes, const uint32_t* __restrict__ frame_ids, RegionDesc* __restrict__ descs,
                                                           int32_t* __restrict__ tabs, int32_t* __restrict__ status_out, int32_t* __restrict__ rects, int32_t top_left,
                                                           BoxCall c)
{
    box_tables_body(boxes, frame_ids, descs, tabs, status_out, c, BoxLetterbox{rects, top_left});
}
// The same rows for a batch of single axes at a fixed pitch (leon_pipeline_resize_weights_device, a diagnostic: the doubles' outcome
// compared word for word with the host's): one workgroup per axis, `max_out` rows of `max_taps` words each.  status: kRegionBox, kRegionRatioX
// (either axis: there is one), kRegionTaps (also a count above max_taps); nothing of a refused axis is written.
struct AxisRecord {
    int32_t in_size, crop_start, crop_size, out_size;
};
__global__ __launch_bounds__(kRgbaBlock) void k_axis_tables(const AxisRecord* __restrict__ axes, int32_t* __restrict__ first, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ weights, int32_t* __restrict__ status_out, int32_t cubic, int32_t max_taps, int32_t max_out)
{
    __shared__ int32_t most_s;
    const uint32_t i = blockIdx.x;
    const AxisRecord a = axes[i];
    int32_t status = region_axis_status(a.in_size, a.crop_start, a.crop_size, a.out_size, kRegionRatioX);
    ResizeAxis A{};
    if (status == kRegionOk) A = resize_axis(a.in_size, a.crop_start, a.crop_size, a.out_size, cubic != 0);
    if (threadIdx.x == 0) most_s = 0;
    __syncthreads();
    if (status == kRegionOk) atomicMax(&most_s, box_axis_most(A, a.out_size));
    __syncthreads();
    if (status == kRegionOk && most_s > max_taps) status = kRegionTaps;
    if (threadIdx.x == 0) status_out[i] = status;
    if (status != kRegionOk) return;
    const size_t at = (size_t)i * (size_t)max_out;
    for (int32_t o = (int32_t)threadIdx.x; o < a.out_size; o += kRgbaBlock)
        box_axis_row(A, o, first + at, count + at, weights + (at + (size_t)o) * (size_t)max_taps, max_taps);
}

// ---- the resampled image in a padded canvas (leon_pipeline.h, leon_pipeline_tensor_canvas) ------------------------------
// One launch writes every element of every frame's tensor.  blockIdx.y below the image's tile rows: resample_body, its stores moved
// to (x, y) of the canvas.  blockIdx.y from there on: pad workgroups, numbered (blockIdx.y - tile rows) * gridDim.x + blockIdx.x;
// they leave before any table load or staging and use no LDS.
// A pad workgroup owns kPadLinesPerGroup consecutive 16-byte lines of the tensor (which starts on a 256-byte boundary), a lane one
// line per step: consecutive lanes, consecutive lines.  In memory order the tensor is a sequence of rows -- HWC: `height` rows of
// 3 * width elements, the image in elements [3x, 3(x + ow)) of rows y .. y + oh - 1; CHW: 3 * height rows of `width` elements, the
// image in [x, x + ow) of rows y .. y + oh - 1 of each plane -- and the pad is what lies between: byte runs that start behind one
// row's image and end in front of the next one's (or at the tensor's ends, or run from plane to plane).  A line wholly inside a run
// is ONE b128 store of the pad pattern, built from the line's address (HWC: period 3 elements; CHW: the plane's element); a line
// wholly inside an image row is not touched (its tile stores it); a line shared with image elements or cut by the tensor's end
// leaves element by element, its pad elements only.  The image tiles store exactly the image's bytes, the pad workgroups exactly
// the others: no byte twice, none left out, no order between workgroups.
static constexpr int kPadLinesPerLane = 4, kPadLinesPerGroup = kPadLinesPerLane * kRgbaBlock;
template <int EB>
__device__ __forceinline__ void pad_store_elem(uint32_t v, __amdgpu_buffer_rsrc_t rs, uint32_t at)
{
    typedef typename ElemOf<EB>::type Elem;
    if constexpr (EB == 4) __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)at, 0, kAuxFrameStore);
    else if constexpr (EB == 2) __builtin_amdgcn_raw_buffer_store_b16((Elem)v, rs, (int)at, 0, kAuxFrameStore);
    else __builtin_amdgcn_raw_buffer_store_b8((Elem)v, rs, (int)at, 0, kAuxFrameStore);
}
// Which tensor a pad workgroup works on and where its image lies (`P`), asked as resample_body asks its `W`.  RingPad: frame
// blockIdx.z of the pipeline's tensor ring, the launch's one rectangle (k_letterbox).  RegionPad: what k_fitted has read from its
// region's descriptor.
struct RingPad {
    uint8_t* __restrict__ tensor_ring;
    const uint32_t* __restrict__ frame_ids;
    const LetterboxGeom& G;
    __device__ __forceinline__ const CanvasGeom& canvas() const { return G.canvas; }
    __device__ __forceinline__ int32_t image_width() const { return G.image.ow; }
    __device__ __forceinline__ int32_t image_height() const { return G.image.oh; }
    __device__ __forceinline__ uint8_t* tensor() const { return tensor_ring + (size_t)frame_ids[blockIdx.z] * join64(G.image.ring.tensor_pitch_lo, G.image.ring.tensor_pitch_hi); }
};
struct RegionPad {
    uint8_t* at;
    CanvasGeom C;
    int32_t iw, ih;
    __device__ __forceinline__ const CanvasGeom& canvas() const { return C; }
    __device__ __forceinline__ int32_t image_width() const { return iw; }
    __device__ __forceinline__ int32_t image_height() const { return ih; }
    __device__ __forceinline__ uint8_t* tensor() const { return at; }
};
template <int EB, int LAYOUT, class P>
__device__ __forceinline__ void pad_body(const P& where, const uint32_t* __restrict__ table, uint32_t group)
{
    typedef typename ElemOf<EB>::type Elem;
    constexpr bool kHwc = LAYOUT == kLayoutHwc;
    constexpr int kLineElems = 16 / EB;
    const CanvasGeom& C = where.canvas();
    const uint32_t cw = (uint32_t)C.cw, ch = (uint32_t)C.ch;
    const uint32_t row_elems = kHwc ? 3u * cw : cw;                                      // a row of the tensor in memory order
    const uint32_t total = 3u * cw * ch;                                                 // elements of the tensor (< 2^26)
    const uint32_t ix0 = (kHwc ? 3u : 1u) * (uint32_t)C.x, ix1 = ix0 + (kHwc ? 3u : 1u) * (uint32_t)where.image_width();      // the image's elements in its rows
    const uint32_t iy0 = (uint32_t)C.y, iy1 = iy0 + (uint32_t)where.image_height();
    // the pad elements T[c][pad[c]] (uint8: the value itself)
    uint32_t pe[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const uint32_t v = (C.pad >> (8 * c)) & 255u;
        if constexpr (EB == 1) pe[c] = v;
        else pe[c] = reinterpret_cast<const Elem*>(table)[c * 256 + v];
    }
    uint8_t* dst = where.tensor();
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)(total * EB), 0x00020000);
    const uint32_t n_lines = (total * EB + 15u) / 16u;
#pragma unroll 1
    for (int step = 0; step < kPadLinesPerLane; step++) {
        const uint32_t line = group * (uint32_t)kPadLinesPerGroup + (uint32_t)(step * kRgbaBlock) + threadIdx.x;
        if (line >= n_lines) break;
        const uint32_t e0 = line * (uint32_t)kLineElems;                                 // the line's first element ...
        const uint32_t row = e0 / row_elems, q = e0 - row * row_elems;                   // ... lies in this row at this element
        const uint32_t plane = kHwc ? 0u : row / ch, yrow = kHwc ? row : row - plane * ch;          // CHW: the row's channel, its row in the plane
        const bool whole = e0 + (uint32_t)kLineElems <= total;
        if (whole && q + (uint32_t)kLineElems <= row_elems) {                            // the line lies in one row
            const bool image_row = yrow >= iy0 && yrow < iy1;
            if (image_row && q >= ix0 && q + (uint32_t)kLineElems <= ix1) continue;      // image: its tile stores it
            if (!image_row || q + (uint32_t)kLineElems <= ix0 || q >= ix1) {             // inside a pad run: one store
                v4u v;
                if constexpr (kHwc) {
                    // dword j starts at channel (q + j * (4 / EB)) % 3
                    const uint32_t ph = q % 3u;
                    uint32_t d[3];
#pragma unroll
                    for (int s = 0; s < 3; s++) {
                        if constexpr (EB == 4) d[s] = pe[s];
                        else if constexpr (EB == 2) d[s] = pe[s] | (pe[(s + 1) % 3] << 16);
                        else d[s] = pe[s] | (pe[(s + 1) % 3] << 8) | (pe[(s + 2) % 3] << 16) | (pe[s] << 24);
                    }
                    constexpr uint32_t kStep = (4 / EB) % 3;                             // channels a dword advances by
                    const uint32_t p1 = (ph + kStep) % 3u, p2 = (ph + 2u * kStep) % 3u, p3 = (ph + 3u * kStep) % 3u;
                    auto pick = [&](uint32_t p) { return p == 0u ? d[0] : (p == 1u ? d[1] : d[2]); };
                    v = v4u{pick(ph), pick(p1), pick(p2), pick(p3)};
                } else {
                    const uint32_t e = plane == 0u ? pe[0] : (plane == 1u ? pe[1] : pe[2]);
                    const uint32_t dw = EB == 4 ? e : (EB == 2 ? e * 0x00010001u : e * 0x01010101u);
                    v = v4u{dw, dw, dw, dw};
                }
                __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)(line * 16u), 0, kAuxFrameStore);
                continue;
            }
        }
        // a line over a row's end, shared with the image or cut by the tensor's end: walk its elements
        uint32_t ev[kLineElems];
        uint32_t image_mask = 0u;
        {
            uint32_t r = row, qq = q, pl = plane, yy = yrow;
#pragma unroll
            for (int k = 0; k < kLineElems; k++) {
                const bool in = e0 + (uint32_t)k < total;
                const uint32_t c = kHwc ? qq % 3u : pl;
                ev[k] = c == 0u ? pe[0] : (c == 1u ? pe[1] : pe[2]);
                if (!in || (yy >= iy0 && yy < iy1 && qq >= ix0 && qq < ix1)) image_mask |= 1u << k;      // not this line's to store
                if (++qq == row_elems) {
                    qq = 0u; r++; yy++;
                    if (!kHwc && yy == ch) { yy = 0u; pl++; }
                }
            }
            (void)r;
        }
        if (image_mask == 0u) {          // over a row's end, yet wholly inside a run
            uint32_t d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if constexpr (EB == 4) d[j] = ev[j];
                else if constexpr (EB == 2) d[j] = ev[2 * j] | (ev[2 * j + 1] << 16);
                else d[j] = ev[4 * j] | (ev[4 * j + 1] << 8) | (ev[4 * j + 2] << 16) | (ev[4 * j + 3] << 24);
            }
            __builtin_amdgcn_raw_buffer_store_b128(v4u{d[0], d[1], d[2], d[3]}, rs, (int)(line * 16u), 0, kAuxFrameStore);
        } else {
#pragma unroll
            for (int k = 0; k < kLineElems; k++)
                if (!((image_mask >> k) & 1u)) pad_store_elem<EB>(ev[k], rs, line * 16u + (uint32_t)(k * EB));
        }
    }
}

template <int EB, int LAYOUT, class F>
__global__ __launch_bounds__(kRgbaBlock) void k_letterbox(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ tensor_ring, const uint32_t* __restrict__ frame_ids,
                                                          const uint32_t* __restrict__ table, const Tables* __restrict__ T, const int32_t* __restrict__ rt,
                                                          LetterboxGeom G)
{
    const uint32_t tile_rows = (uint32_t)(G.image.oh + kResTileY - 1) / (uint32_t)kResTileY;
    if (blockIdx.y >= tile_rows) {
        pad_body<EB, LAYOUT>(RingPad{tensor_ring, frame_ids, G}, table, (blockIdx.y - tile_rows) * gridDim.x + blockIdx.x);
        return;
    }
    resample_body<EB, LAYOUT, F>(RingFrame{planes_ring, tensor_ring, frame_ids}, table, T, rt, G.image, G.canvas);
}

// ---- regions letterboxed into the batch's tensor size (leon_pipeline.h, leon_pipeline_regions_fit) ------------------------------
// k_letterbox with a rectangle per region: every region of a call has the canvas's size cw x ch (G.ow x G.oh of the launch) and an
// image of its own in it, iw x ih at (ix, iy) of its descriptor -- the letterbox of its box -- with tables built for iw x ih.  One
// family for both roads: the host path's descriptors carry status 0, the device path's come from k_fit_tables.
// Grid: x = the canvas's tile columns, y = its tile rows and behind them the pad workgroup rows of a cw x ch tensor, z = the region.
// A workgroup reads its region's descriptor (one address per workgroup: scalar loads) and decides, before any table load or LDS use
// and the same for all its lanes: a refused region -- leave, not one byte of it is written, pad included; a tile row of the canvas --
// resample_body with the region's own image size and origin if the tile is one of the image's ceil(iw / 32) x ceil(ih / 8), else
// leave (the image's tiles are numbered from ITS origin, so these are the first columns and rows of the grid); behind the canvas's
// tile rows -- pad_body on the region's tensor, which stores every byte outside the image's rectangle and none inside.
template <int EB, int LAYOUT, class F>
__global__ __launch_bounds__(kRgbaBlock) void k_fitted(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ out, const RegionDesc* __restrict__ descs,
                                                       const uint32_t* __restrict__ table, const Tables* __restrict__ T, const int32_t* __restrict__ tabs,
                                                       ResampleGeom G, uint32_t pad)
{
    const RegionDesc& d = descs[blockIdx.z];
    if (d.status != kRegionOk) return;
    const CanvasGeom C{G.ow, G.oh, d.ix, d.iy, pad};
    uint8_t* dst = out + join64(d.dst_lo, d.dst_hi);
    const uint32_t tile_rows = (uint32_t)(G.oh + kResTileY - 1) / (uint32_t)kResTileY;
    if (blockIdx.y >= tile_rows) {
        pad_body<EB, LAYOUT>(RegionPad{dst, C, d.iw, d.ih}, table, (blockIdx.y - tile_rows) * gridDim.x + blockIdx.x);
        return;
    }
    if (blockIdx.x * (uint32_t)kResTileX >= (uint32_t)d.iw || blockIdx.y * (uint32_t)kResTileY >= (uint32_t)d.ih) return;
    G.ow = d.iw; G.oh = d.ih;
    G.taps_x = d.taps_x; G.taps_y = d.taps_y;
    G.off_cx = d.off_cx; G.off_wx = d.off_wx; G.off_fy = d.off_fy; G.off_cy = d.off_cy; G.off_wy = d.off_wy;
    const RegionFrame where{FramePair{planes_ring + (size_t)d.frame_id * join64(G.ring.planes_pitch_lo, G.ring.planes_pitch_hi), dst}};
    resample_body<EB, LAYOUT, F>(where, table, T, tabs + d.rt_base, G, C);
}

// ---- rotated boxes and affine crops of delivered frames (leon_pipeline.h, leon_pipeline_warp_regions) ---------------------------
// blockIdx.z is the region, blockIdx.x / y the 32 x 8 tiles of the out size, a lane one output pixel as in resample_body's vertical
// pass.  There are no tables: a workgroup reads its region's record (one address per workgroup: scalar loads), judges it with the
// host's text (leon_warp.h) -- a refused region is left before any LDS use, not one byte of it written -- and one workgroup of the
// region writes the status word.  The map is affine, so the source footprint of a rectangle of output pixels is the bounding box of
// its four corner samples and their bilinear neighbours.  The tile is walked in pieces (leon_warp.h: warp_level) whose footprint,
// aligned to 8 columns and even rows, fits the stage; per piece (1) the footprint is loaded and converted ONCE into RGBX dwords in
// LDS with resample_body's loads and conversion (8 Y bytes a row and 4 + 4 chroma bytes a row pair per lane, chroma_terms /
// tensor_px8, the fill row of an odd height) -- what lies outside the frame is staged as the pad pixel and never loaded, so the taps
// select nothing; a piece wholly outside stages nothing at all; (2) the piece's lanes accumulate their S x S x 4 taps from LDS.
// Sample positions: the definition's 64-bit numerator once per piece and axis, minus the stage's origin (scalar); what a lane adds
// to it stays inside 2^28, so its arithmetic is 32 bits.  After the last piece the pixel leaves through resample_body's store forms.
struct WarpCall {
    int32_t fw, fh, ow, oh;
    int32_t n_frames;
    uint32_t pad;                        // the pad pixel's 8-bit R, G, B in bits 0, 8, 16
    uint32_t pitch_lo, pitch_hi;         // bytes between the regions' tensors
    RingGeom ring;
};
// A tile's pixels to the tensor at `dst` (the image is the tensor): resample_body's two store forms, which see its comment.  `pack`:
// LDS nobody reads any more, kRows * kRowStride bytes.
template <int EB, int LAYOUT>
__device__ __forceinline__ void warp_store(uint32_t px, bool valid, const typename ElemOf<EB>::type* tab_s, char* pack, uint8_t* dst, int ox0, int oy0, int nox, int noy,
                                           int o, int sub, uint32_t width, uint32_t plane_elems)
{
    typedef typename ElemOf<EB>::type Elem;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)dst, 0, (int)(3u * plane_elems * EB), 0x00020000);
    if constexpr (LAYOUT == kLayoutChw && EB != 1) {
        const uint32_t at = (uint32_t)(oy0 + sub) * width + (uint32_t)(ox0 + o);
        const uint32_t oob = valid ? 0u : kOobBit;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const Elem e = tab_s[ch * 256 + ((px >> (8 * ch)) & 255u)];
            const uint32_t voff = (((uint32_t)ch * plane_elems + at) * (uint32_t)sizeof(Elem)) | oob;
            if constexpr (sizeof(Elem) == 4) __builtin_amdgcn_raw_buffer_store_b32(e, rs, (int)voff, 0, kAuxFrameStore);
            else __builtin_amdgcn_raw_buffer_store_b16(e, rs, (int)voff, 0, kAuxFrameStore);
        }
    } else {
        constexpr bool kHwc = LAYOUT == kLayoutHwc;
        constexpr int kRowElems = kHwc ? 3 * kResTileX : kResTileX, kRowStride = kRowElems * EB + 16;
        constexpr int kRows = kHwc ? kResTileY : 3 * kResTileY, kLines = (kRowElems * EB + 15) / 16 + 1;
        constexpr int kLinesP2 = kLines <= 4 ? 4 : 32;
        static_assert(kRows * kRowStride <= kWarpStagePx * 4 && kLines <= kLinesP2 && kRows * kLinesP2 <= kRgbaBlock, "the packed tile fits the stage, a lane per line");
        auto row_start = [&](int row) -> uint32_t {
            if constexpr (kHwc) return ((uint32_t)(oy0 + row) * width + (uint32_t)ox0) * 3u * EB;
            else return ((uint32_t)(row >> 3) * plane_elems + (uint32_t)(oy0 + (row & 7)) * width + (uint32_t)ox0) * EB;
        };
        if (valid) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const int row = kHwc ? sub : ch * kResTileY + sub;
                const int at = (int)(row_start(row) & 15u) + (kHwc ? (o * 3 + ch) * EB : o * EB);
                *reinterpret_cast<Elem*>(pack + row * kRowStride + at) = (Elem)image_elem<EB>(tab_s, px, ch);
            }
        }
        __syncthreads();
        const int tid = threadIdx.x;
        const int row = tid / kLinesP2, line = tid & (kLinesP2 - 1);
        if (row < kRows && (kHwc ? row : (row & 7)) < noy) {
            const uint32_t g0 = row_start(row), g1 = g0 + (uint32_t)(nox * (kHwc ? 3 : 1) * EB);      // the row's bytes in the tensor
            const uint32_t a0 = (g0 & ~15u) + 16u * (uint32_t)line;                                   // this lane's line
            const char* from = pack + row * kRowStride + 16 * line;
            if (a0 >= g0 && a0 + 16u <= g1) __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const v4u*>(from), rs, (int)a0, 0, kAuxFrameStore);
            else if (a0 + 16u > g0 && a0 < g1) {
                for (int e = 0; e < 16 / EB; e++) {          // a line at an end of the row: only the elements inside [g0, g1), one by one
                    const uint32_t a = a0 + (uint32_t)(e * EB);
                    if (a < g0 || a >= g1) continue;
                    pad_store_elem<EB>(*reinterpret_cast<const Elem*>(from + e * EB), rs, a);
                }
            }
        }
    }
}
template <int EB, int LAYOUT>
__global__ __launch_bounds__(kRgbaBlock) void k_warp(const uint8_t* __restrict__ planes_ring, uint8_t* __restrict__ out, const WarpRecord* __restrict__ recs,
                                                     const uint32_t* __restrict__ frame_ids, int32_t* __restrict__ status_out, const uint32_t* __restrict__ table,
                                                     const Tables* __restrict__ T, WarpCall c)
{
    typedef typename ElemOf<EB>::type Elem;
    static_assert(kResTileX * kResTileY == kRgbaBlock && kResTileX == 32, "lane = (tid & 31, tid >> 5)");
    __shared__ __attribute__((aligned(16))) int32_t lut_s[kLdsLut / 4];
    __shared__ __attribute__((aligned(16))) Elem tab_s[EB == 1 ? 16 : 3 * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage_s[kWarpStagePx];
    const WarpRecord r = recs[blockIdx.z];
    int32_t g;
    const int32_t status = warp_record_status(r, c.n_frames, &g);
    if (status_out && (blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) status_out[blockIdx.z] = status;
    if (status != kRegionOk) return;
    const int tid = threadIdx.x;
    {   // the conversion tables and the element table as k_tensor loads them
        display_lut_to_lds(lut_s, T);
        if constexpr (EB != 1) {
            constexpr int kDwords = 3 * 256 * EB / 4;
            for (int i = tid; i < kDwords; i += kRgbaBlock) reinterpret_cast<uint32_t*>(tab_s)[i] = table[i];
        }
        wait_vmem_all();
        __syncthreads();
    }
    const int ox0 = blockIdx.x * kResTileX, oy0 = blockIdx.y * kResTileY;
    const int nox = min(kResTileX, c.ow - ox0), noy = min(kResTileY, c.oh - oy0);
    const int o = tid & 31, sub = tid >> 5;
    const int32_t a00 = r.m[0], a01 = r.m[1], tx = r.m[2], a10 = r.m[3], a11 = r.m[4], ty = r.m[5];
    const int S = 1 << g, S2 = 2 << g;
    const int level = warp_level(r.m, g);
    const int pw = warp_piece_w(level), ph = warp_piece_h(level);
    const uint64_t planes_pitch = join64(c.ring.planes_pitch_lo, c.ring.planes_pitch_hi);
    const uint8_t* src = planes_ring + (size_t)frame_ids[r.frame] * planes_pitch;
    // (the frame's planes end where the ring's next frame starts: a wrong offset reads 0 and faults nothing)
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)min(planes_pitch, (uint64_t)0x7fffffff), 0x00020000);
    const char* lut = reinterpret_cast<const char*>(lut_s);
    uint32_t two = 2u, three = 3u;                       // SDWA shift counts live in registers (display_half)
    asm("" : "+v"(two), "+v"(three));
    uint32_t px = 0u;
    for (int py = 0; py < noy; py += ph) {
        for (int pxo = 0; pxo < nox; pxo += pw) {
            const int qw = min(pw, nox - pxo), qh = min(ph, noy - py);
            const int fx_o = ox0 + pxo, fy_o = oy0 + py;          // the piece's first pixel, and its last:
            const int lx_o = fx_o + qw - 1, ly_o = fy_o + qh - 1;
            // the four corner samples: the piece's extremes on both axes (the numerators are affine in the pixel and the sub-sample)
            const int64_t nx00 = warp_numerator(a00, a01, tx, g, fx_o, fy_o, 0, 0), nx10 = warp_numerator(a00, a01, tx, g, lx_o, fy_o, S - 1, 0);
            const int64_t nx01 = warp_numerator(a00, a01, tx, g, fx_o, ly_o, 0, S - 1), nx11 = warp_numerator(a00, a01, tx, g, lx_o, ly_o, S - 1, S - 1);
            const int64_t ny00 = warp_numerator(a10, a11, ty, g, fx_o, fy_o, 0, 0), ny10 = warp_numerator(a10, a11, ty, g, lx_o, fy_o, S - 1, 0);
            const int64_t ny01 = warp_numerator(a10, a11, ty, g, fx_o, ly_o, 0, S - 1), ny11 = warp_numerator(a10, a11, ty, g, lx_o, ly_o, S - 1, S - 1);
            const int x_lo = warp_q(min(min(nx00, nx10), min(nx01, nx11)), g) >> 8, x_hi = (warp_q(max(max(nx00, nx10), max(nx01, nx11)), g) >> 8) + 1;
            const int y_lo = warp_q(min(min(ny00, ny10), min(ny01, ny11)), g) >> 8, y_hi = (warp_q(max(max(ny00, ny10), max(ny01, ny11)), g) >> 8) + 1;
            const int sx0 = x_lo & ~7, sx1 = (x_hi + 8) & ~7, sy0 = y_lo & ~1, sy1 = (y_hi + 2) & ~1;      // [sx0, sx1) x [sy0, sy1)
            const bool mine = o >= pxo && o < pxo + qw && sub >= py && sub < py + qh;
            if (sx1 <= 0 || sx0 >= c.fw || sy1 <= 0 || sy0 >= c.fh) {          // nothing of the frame: every tap reads the pad
                if (mine) px = c.pad;
                continue;
            }
            const int sw8 = (sx1 - sx0) >> 3, n_pairs = (sy1 - sy0) >> 1;
            const int pitch = sx1 - sx0 + 1;                                  // odd (leon_warp.h)
            // (1) rows sy0 .. sy1 - 1 (whole pairs), columns sx0 .. sx1 - 1 -> RGBX in stage_s[row][pitch]; outside the frame: the pad
            const int pair_t = tid / sw8, col_t = tid - pair_t * sw8;
            const int pair_step = kRgbaBlock / sw8, col_step = kRgbaBlock - pair_step * sw8;
            for (int pair = pair_t, col = col_t; pair < n_pairs;) {
                const int row = sy0 + 2 * pair, x = sx0 + 8 * col;          // (row is even: row >= 0 is row + 1 >= 0 too)
                const bool inx = x >= 0 && x < c.fw;
                const bool in0 = inx && row >= 0 && row < c.fh, in1 = inx && row >= 0 && row + 1 < c.fh;
                const uint32_t yo = (uint32_t)row * c.ring.luma_stride + (uint32_t)x;
                const uint32_t co = (uint32_t)(row >> 1) * c.ring.chroma_stride + (uint32_t)(x >> 1);
                const v2u y0 = __builtin_amdgcn_raw_buffer_load_b64(prs, (int)(in0 ? yo : kOobBit), 0, kAuxStreamOnce);
                const v2u y1 = __builtin_amdgcn_raw_buffer_load_b64(prs, (int)(in1 ? yo + c.ring.luma_stride : kOobBit), 0, kAuxStreamOnce);
                const uint32_t cb4 = __builtin_amdgcn_raw_buffer_load_b32(prs, (int)(in0 ? c.ring.cb_off + co : kOobBit), 0, kAuxStreamOnce);
                const uint32_t cr4 = __builtin_amdgcn_raw_buffer_load_b32(prs, (int)(in0 ? c.ring.cr_off + co : kOobBit), 0, kAuxStreamOnce);
                const ChromaTerms ct[4] = {chroma_terms<0>(lut, cb4, cr4, three), chroma_terms<1>(lut, cb4, cr4, three),
                                           chroma_terms<2>(lut, cb4, cr4, three), chroma_terms<3>(lut, cb4, cr4, three)};
                uint32_t a[8], b[8];
                tensor_px8(lut, y0, ct, !in1, two, a);       // (!in1: the last row of an odd height, left at 255 by the twin)
                tensor_px8(lut, y1, ct, false, two, b);
                const int n_in = c.fw - x;                   // columns of the group inside the frame (a width that is no multiple of 8)
                uint32_t* s0 = stage_s + (2 * pair) * pitch + 8 * col;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    s0[k] = in0 && k < n_in ? a[k] : c.pad;
                    s0[pitch + k] = in1 && k < n_in ? b[k] : c.pad;
                }
                pair += pair_step; col += col_step;
                if (col >= sw8) { col -= sw8; pair++; }
            }
            __syncthreads();
            // (2) the piece's pixels: S x S bilinear samples each, positions relative to the stage's origin
            if (mine) {
                const int32_t bx = (int32_t)(nx00 - ((int64_t)sx0 << (17 + g))), by = (int32_t)(ny00 - ((int64_t)sy0 << (17 + g)));
                const int32_t dx = S2 * (o - pxo), dy = S2 * (sub - py);
                const int32_t nx0 = bx + a00 * dx + a01 * dy, ny0 = by + a10 * dx + a11 * dy;
                uint32_t ar = 0u, ag = 0u, ab = 0u;
                for (int j = 0; j < S; j++) {
                    for (int i = 0; i < S; i++) {
                        const int32_t nx = nx0 + 2 * (a00 * i + a01 * j), ny = ny0 + 2 * (a10 * i + a11 * j);
                        const int32_t qx = ((nx >> (g + 1)) + 128) >> 8, qy = ((ny >> (g + 1)) + 128) >> 8;
                        const uint32_t fx = (uint32_t)qx & 255u, fy = (uint32_t)qy & 255u;
                        const uint32_t* s = stage_s + (qy >> 8) * pitch + (qx >> 8);
                        const uint32_t p00 = s[0], p01 = s[1], p10 = s[pitch], p11 = s[pitch + 1];
                        const uint32_t w00 = (256u - fx) * (256u - fy), w01 = fx * (256u - fy), w10 = (256u - fx) * fy, w11 = fx * fy;
                        ar += __umul24(w00, p00 & 255u) + __umul24(w01, p01 & 255u) + __umul24(w10, p10 & 255u) + __umul24(w11, p11 & 255u);
                        ag += __umul24(w00, (p00 >> 8) & 255u) + __umul24(w01, (p01 >> 8) & 255u) + __umul24(w10, (p10 >> 8) & 255u) + __umul24(w11, (p11 >> 8) & 255u);
                        ab += __umul24(w00, (p00 >> 16) & 255u) + __umul24(w01, (p01 >> 16) & 255u) + __umul24(w10, (p10 >> 16) & 255u) + __umul24(w11, (p11 >> 16) & 255u);
                    }
                }
                const uint32_t half = 1u << (15 + 2 * g);
                const int sh = 16 + 2 * g;
                px = ((ar + half) >> sh) | (((ag + half) >> sh) << 8) | (((ab + half) >> sh) << 16);          // (the weights sum to 2^sh: at most 255 each)
            }
            __syncthreads();          // the stage is free for the next piece, or for the store
        }
    }
    const uint64_t dst_off = (uint64_t)blockIdx.z * join64(c.pitch_lo, c.pitch_hi);
    warp_store<EB, LAYOUT>(px, o < nox && sub < noy, tab_s, reinterpret_cast<char*>(stage_s), out + dst_off, ox0, oy0, nox, noy, o, sub, (uint32_t)c.ow,
                           (uint32_t)c.ow * (uint32_t)c.oh);
}

// ---- output MOTION: a frame's motion record (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_MOTION) ------------------------------
// One launch per window behind its reconstruction levels: blockIdx.y = the delivered frame, one workgroup of 256 lanes a frame, walking
// the picture's macroblocks in a strided loop, four consecutive macroblocks per lane and trip -- a dword of repadd and of mb_dir,
// 16 bytes of each vector map in, two 16-byte stores of vectors and a dword of info out.  The maps are padded to 256 bytes in the arenas
// (MapLayout) and the record's parts to 256 (leon_motion.h), so the last trip's lanes address whole dwords inside both; what they
// write behind macroblock mbs - 1 lies in the record's unspecified bytes, and only the summary's counting asks which macroblocks exist.
// The per-macroblock expression is the host's text (leon_motion.h).  The summary is summed per lane, across the wave by shuffles,
// across the four waves through LDS; lane 0 stores its eight words: every specified byte of the record is written by this launch,
// nothing is cleared beforehand and nothing is added to atomically.
struct MotionDesc {
    const uint8_t* repadd;       // the picture's maps in its GOP's device arena; null where the type has none
    const uint8_t* mb_dir;
    const uint32_t* mv_fwd;      // a macroblock's (h, v) as one dword
    const uint32_t* mv_bwd;
    int32_t type;                // LEON_PIC_*
    uint32_t frame;              // the frame's index in the motion ring (frame_addr)
    uint32_t reserved[2];
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

__global__ __launch_bounds__(kRgbaBlock) void k_motion(const MotionDesc* __restrict__ descs, uint8_t* __restrict__ ring, MotionLayout G)
{
    __shared__ __attribute__((aligned(16))) uint32_t part_s[kRgbaBlock / 64][8];
    const MotionDesc* __restrict__ D = descs + blockIdx.y;
    const int32_t type = D->type;
    const uint8_t* __restrict__ repadd = D->repadd;
    const uint8_t* __restrict__ mb_dir = D->mb_dir;
    const uint32_t* __restrict__ mv_fwd = D->mv_fwd;
    const uint32_t* __restrict__ mv_bwd = D->mv_bwd;
    uint8_t* __restrict__ rec = ring + (size_t)D->frame * G.record_pitch;
    const uint32_t mbs = G.mbs;
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t k0 = 4u * threadIdx.x; k0 < mbs; k0 += 4u * kRgbaBlock) {
        uint32_t ra = 0u, di = 0u;
        uint4 f = uint4{0u, 0u, 0u, 0u}, b = uint4{0u, 0u, 0u, 0u};
        if (type != 1) {
            ra = *reinterpret_cast<const uint32_t*>(repadd + k0);
            f = *reinterpret_cast<const uint4*>(mv_fwd + k0);
        }
        if (type == 3) {
            di = *reinterpret_cast<const uint32_t*>(mb_dir + k0);
            b = *reinterpret_cast<const uint4*>(mv_bwd + k0);
        }
        const uint32_t fi[4] = {f.x, f.y, f.z, f.w}, bi[4] = {b.x, b.y, b.z, b.w};
        uint32_t of[4], ob[4], info4 = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t info = motion_mb(type, (ra >> (8 * i)) & 255u, (di >> (8 * i)) & 255u, fi[i], bi[i], &of[i], &ob[i]);
            info4 |= info << (8 * i);
            if (k0 + (uint32_t)i < mbs) motion_count(info, of[i], ob[i], s);
        }
        uint4* mv = reinterpret_cast<uint4*>(rec + (size_t)k0 * 8u);
        mv[0] = uint4{of[0], ob[0], of[1], ob[1]};
        mv[1] = uint4{of[2], ob[2], of[3], ob[3]};
        *reinterpret_cast<uint32_t*>(rec + G.info_offset + k0) = info4;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = wave_sum(s[i]);
    if ((threadIdx.x & 63u) == 0u) {
        uint4* ps = reinterpret_cast<uint4*>(part_s[threadIdx.x >> 6]);
        ps[0] = uint4{s[0], s[1], s[2], s[3]};
        ps[1] = uint4{s[4], s[5], s[6], s[7]};
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 lo = uint4{0u, 0u, 0u, 0u}, hi = lo;
#pragma unroll
        for (int w = 0; w < kRgbaBlock / 64; w++) {
            const uint4 a = reinterpret_cast<const uint4*>(part_s[w])[0], c = reinterpret_cast<const uint4*>(part_s[w])[1];
            lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
            hi.x += c.x; hi.y += c.y; hi.z += c.z; hi.w += c.w;
        }
        uint4* sm = reinterpret_cast<uint4*>(rec + G.summary_offset);
        sm[0] = lo;
        sm[1] = hi;
    }
}

// ---- output ACTIVITY: a frame's activity record (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_ACTIVITY) ------------------------
// Two launches per window behind its reconstruction levels, blockIdx.y = the delivered frame in both.
// k_activity: a task is the 8 macroblocks under one chroma group c of one macroblock row my -- Cb and Cr group c of block row my, luma
// groups 2c and 2c + 1 (where the row has it) of block rows 2 my and 2 my + 1, six lists at most.  One 64-lane wave per task, four
// tasks per workgroup; the waves share nothing but the two barriers.  The wave's lanes stride over each list's entries, a dword each
// (a list starts at any entry, so nothing wider is aligned), and add what an entry counts (leon_activity.h, the host's text) to the
// task's bins in LDS -- all six lists' offsets are asked for at once and then every list's first 64 entries, before anything is counted:
// a list of the 1080p benchmark stream holds 13 entries on average and 2 % hold more than 64, so a task waits for memory three times
// (descriptor, offsets, entries) and not thirteen --: per macroblock and sum eight 64-bit words, lane l into word l & 7, so that the run of entries one block
// contributes spreads over eight addresses and no sum can wrap whatever a list holds.  The block bits travel as one 48-bit mask per lane,
// OR-ed into LDS once.  Lanes 0 .. 7 then add a macroblock's eight words each, saturate, read its qscale and store its 8 bytes: every
// cell is written once, by the task that owns it.  Both offsets of a list are clamped to the list's capacity (activity_span) before
// an entry is addressed.  LDS: 4 waves x (3 sums x 8 macroblocks x 8 words x 8 bytes + 8) = 6176 bytes.
// k_activity_summary: the eight summary words of a frame from its cells, one workgroup per frame, k_motion's reduction (shuffles, the
// four waves through LDS, lane 0 stores).  A second kernel and not the last workgroup of the first: the cells of a frame come from
// workgroups on every XCD, whose L2s are not coherent inside a launch, and a "last one reduces" hand-off needs a counter that somebody
// clears -- which the record's rule (nothing cleared beforehand, nothing added to atomically in global memory) rules out.  The launch
// boundary orders the cells at no cost, and the cells of a window are still in L2 when they are read again.  LDS: 128 bytes.
struct ActivityDesc {
    const uint32_t* grp_off;     // the picture's group offsets, entry list and qscale map in its GOP's device arena
    const uint32_t* entries;
    const uint8_t* qscale;
    uint32_t n_entries;          // the list's capacity: no entry at or behind it is read
    uint32_t frame;              // the frame's index in the activity ring (frame_addr)
};
constexpr int kActivityWaves = kRgbaBlock / 64, kActivitySpread = 8;

__global__ __launch_bounds__(kRgbaBlock) void k_activity(const ActivityDesc* __restrict__ descs, uint8_t* __restrict__ ring, ActivityGeom G, ActivityLayout L)
{
    __shared__ unsigned long long bins_s[kActivityWaves][3][8][kActivitySpread];      // [wave][ac_count, ac_mag, dc_mag][macroblock][lane & 7]
    __shared__ unsigned long long seen_s[kActivityWaves];                             // bit 6 m + j: block j of macroblock m codes something
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t task = blockIdx.x * (uint32_t)kActivityWaves + wave;
    const bool live = task < G.tasks;
    unsigned long long* const bins = &bins_s[wave][0][0][0];
    for (uint32_t i = lane; i < 3u * 8u * (uint32_t)kActivitySpread; i += 64u) bins[i] = 0ull;
    if (lane == 0u) seen_s[wave] = 0ull;
    __syncthreads();
    const ActivityDesc* __restrict__ D = descs + blockIdx.y;
    const uint32_t my = live ? task / G.groups_c : 0u, c = live ? task - my * G.groups_c : 0u;
    // lanes 0 .. 7 own a macroblock each; its qscale is needed last and asked for first, so that it travels beside the lists
    const uint32_t mx = 8u * c + lane, k = my * G.mbw + mx;
    const bool owns = live && lane < 8u && mx < G.mbw;
    const uint32_t qscale = owns ? D->qscale[k] : 0u;
    if (live) {
        const uint32_t* __restrict__ grp_off = D->grp_off;
        const uint32_t* __restrict__ entries = D->entries;
        const uint32_t cap = D->n_entries;
        // the six lists: luma (2 my, 2c), (2 my, 2c + 1), (2 my + 1, 2c), (2 my + 1, 2c + 1), Cb, Cr.  All their offsets are asked for
        // first and then every list's first 64 entries, before anything is counted: a list is seldom longer, and six loads in
        // flight wait once where a list after the other waits twelve times (offsets, then entries, each a trip to memory).
        uint32_t begin[6], end[6], first[6];
#pragma unroll
        for (uint32_t part = 0; part < 6u; part++) {
            const uint32_t plane = part < 4u ? 0u : part - 3u;
            const uint32_t R = plane == 0u ? 2u * my + (part >> 1) : my, g = plane == 0u ? 2u * c + (part & 1u) : c;
            const uint32_t gid = plane == 0u ? R * G.groups_y + g : G.n_y + (plane - 1u) * G.n_c + R * G.groups_c + g;
            begin[part] = end[part] = 0u;
            if (plane != 0u || g < G.groups_y) activity_span(grp_off[gid], grp_off[gid + 1u], cap, &begin[part], &end[part]);
        }
#pragma unroll
        for (uint32_t part = 0; part < 6u; part++) first[part] = begin[part] + lane < end[part] ? entries[begin[part] + lane] : 0u;      // (level 0 counts nothing)
        unsigned long long seen = 0ull;
        auto count = [&](uint32_t e, uint32_t plane, uint32_t R, uint32_t g) {
            const uint32_t a = activity_abs(e);
            uint32_t emx, emy, j;
            activity_place(plane, R, g, activity_b(e), &emx, &emy, &j);
            if (a == 0u || emx >= G.mbw) return;
            const uint32_t m = (emx - 8u * c) & 7u, at = m * (uint32_t)kActivitySpread + (lane & 7u);
            if (activity_is_dc(e)) {
                atomicAdd(&bins[2u * 8u * kActivitySpread + at], (unsigned long long)a);
            } else {
                atomicAdd(&bins[at], 1ull);
                atomicAdd(&bins[8u * kActivitySpread + at], (unsigned long long)a);
            }
            seen |= 1ull << (6u * m + j);
        };
#pragma unroll
        for (uint32_t part = 0; part < 6u; part++) {
            const uint32_t plane = part < 4u ? 0u : part - 3u;
            const uint32_t R = plane == 0u ? 2u * my + (part >> 1) : my, g = plane == 0u ? 2u * c + (part & 1u) : c;
            count(first[part], plane, R, g);
            for (uint32_t i = begin[part] + 64u + lane; i < end[part]; i += 64u) count(entries[i], plane, R, g);
        }
        if (seen) atomicOr(&seen_s[wave], seen);
    }
    __syncthreads();
    if (owns) {
        unsigned long long sum[3] = {0ull, 0ull, 0ull};
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int r = 0; r < kActivitySpread; r++) sum[f] += bins_s[wave][f][lane][r];
        uint32_t lo, hi;
        activity_cell(sum[0], sum[1], sum[2], (uint32_t)(seen_s[wave] >> (6u * lane)) & 63u, qscale, &lo, &hi);
        *reinterpret_cast<uint2*>(ring + (size_t)D->frame * L.record_pitch + 8u * (size_t)k) = uint2{lo, hi};
    }
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kRgbaBlock) void k_activity_summary(const ActivityDesc* __restrict__ descs, uint8_t* ring, ActivityLayout L)
{
    __shared__ __attribute__((aligned(16))) uint32_t part_s[kRgbaBlock / 64][8];
    uint8_t* rec = ring + (size_t)descs[blockIdx.y].frame * L.record_pitch;
    uint32_t s[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t k = threadIdx.x; k < L.mbs; k += kRgbaBlock) {
        const uint2 cell = reinterpret_cast<const uint2*>(rec)[k];
        activity_count(cell.x, cell.y, s);
    }
#pragma unroll
    for (int i = 0; i < 7; i++) s[i] = i == 4 ? wave_max(s[i]) : wave_sum(s[i]);
    if ((threadIdx.x & 63u) == 0u) {
        uint4* ps = reinterpret_cast<uint4*>(part_s[threadIdx.x >> 6]);
        ps[0] = uint4{s[0], s[1], s[2], s[3]};
        ps[1] = uint4{s[4], s[5], s[6], 0u};
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint4 lo = uint4{0u, 0u, 0u, 0u}, hi = lo;
#pragma unroll
        for (int w = 0; w < kRgbaBlock / 64; w++) {
            const uint4 a = reinterpret_cast<const uint4*>(part_s[w])[0], c = reinterpret_cast<const uint4*>(part_s[w])[1];
            lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
            hi.x = c.x > hi.x ? c.x : hi.x; hi.y += c.y; hi.z += c.z;
        }
        uint4* sm = reinterpret_cast<uint4*>(rec + L.summary_offset);
        sm[0] = lo;
        sm[1] = hi;
    }
}

// ---- output RESIDUAL: a frame's residual record (include/leon_pipeline.h, LEON_PIPELINE_OUTPUT_RESIDUAL) -------------------------
// One launch per window behind its reconstruction levels, blockIdx.y = the delivered frame.  A task is k_recon's (leon_residual.h): two
// block groups that share their macroblocks; one 64-lane wave per task, four per workgroup, a private LDS strip in layout 0 per wave, no
// talk between waves.  It is the sparse, non-display road of recon_task up to and including its row pass -- the same helpers, called,
// not copied: both groups' offsets, each run's first 64 entries through a buffer resource of exactly n_entries dwords (count clamped to
// 512, tile offset masked with 1022: a malformed list gives a wrong record and no access outside the list or the tile), the qscale and
// intra bytes, clear and scatter, scan_tile and column_pass on the live columns, the row pass with its shortcuts by live columns -- and
// then, in place of the prediction, truncation toward zero for EVERY picture type (k_recon may leave it out for I pictures because its
// clamp hides negative values; the record shows them), a saturating pack to int16 (v_cvt_pk_i16_i32) and one 16-byte store per lane and
// half: the 8 lanes of a row write 128 contiguous bytes of one record row.  A half without a live column stores zeros without a row
// pass.  Every specified element is written by exactly one lane of one task; lanes of blocks at or behind the plane's block width
// store nothing (residual_store).
struct ResidualDesc {
    const uint32_t* grp_off;     // the picture's group offsets, entry list and maps in its GOP's device arena
    const uint32_t* entries;
    const uint8_t* qscale;
    const uint8_t* intra;
    const QTables* qt;           // the matrices of the picture's sequence (PicDesc::qt)
    uint32_t n_entries;          // the list's capacity: no entry at or behind it is read
    uint32_t frame;              // the frame's index in the residual ring
};

__global__ __launch_bounds__(kRgbaBlock) void k_residual(const ResidualDesc* __restrict__ descs, uint8_t* __restrict__ ring, ResidualGeom G, ResidualLayout L)
{
    __shared__ __attribute__((aligned(16))) char smem[kWavesPerWG * kLdsPerWave];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * (uint32_t)kWavesPerWG + (uint32_t)wave;
    if (t >= G.tasks) return;                         // (waves share no barrier)
    char* lds = smem + wave * kLdsPerWave;
    const ResidualDesc& D = descs[blockIdx.y];
    stage_tables(D.qt, lds, lane);
    const ResidualTask T = residual_task(G, t);
    const int hi3 = lane >> 3, lo3 = lane & 7;
    // both runs' first 64 entries (one dword per lane), longer runs loop below; indices past the list read 0, whatever grp_off says
    const __amdgpu_buffer_rsrc_t ent_rs = __builtin_amdgcn_make_buffer_rsrc((void*)D.entries, 0, (int)(D.n_entries * 4u), 0x00020000);
    const LEON_GLOBAL uint32_t* go = gptr(D.grp_off);
    uint32_t ent_first[2], ent_start[2], ent_count[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t s0 = go[T.gid[h]], e0 = go[T.gid[h] + 1u];
        ent_start[h] = s0;
        ent_count[h] = e0 > s0 ? min(e0 - s0, 512u) : 0u;      // a group holds at most 8*64 coefficients
        ent_first[h] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
            ent_rs, (int)(((s0 + (uint32_t)lane) * 4u) | ((uint32_t)lane < ent_count[h] ? 0u : kOobBit)), 0, kAuxStreamOnce);
    }
    // quantiser scale and intra flag of this lane's block (lane b: block b's macroblock), for the lanes of the column pass to fetch
    const uint32_t bw = residual_block_width(L, T.chroma);
    const uint32_t Qb = 8u * T.g + (uint32_t)lo3, Qs = Qb < bw ? Qb : bw - 1u;
    const uint32_t mb = T.Rt * G.mbw + (T.chroma ? Qs : Qs >> 1);
    const int qia = (int)(ldg<uint8_t>(gptr(D.qscale), mb) & 31) | (ldg<uint8_t>(gptr(D.intra), mb) != 0 ? 256 : 0);

    *reinterpret_cast<v4i*>(lds + lane * 16) = v4i{0, 0, 0, 0};
    *reinterpret_cast<v4i*>(lds + kLdsHalf + lane * 16) = v4i{0, 0, 0, 0};
    wave_sync();
#pragma unroll
    for (int h = 0; h < 2; h++) {
        uint32_t e = ent_first[h];
        // (an entry with level 0 writes nothing: it may name a cell another entry of the list fills)
        if ((e & 0xffffu) != 0u) *reinterpret_cast<short*>(lds + h * kLdsHalf + ((e >> 16) & 1022u)) = (short)e;
#pragma unroll 1
        for (uint32_t k = 64u; k < ent_count[h]; k += 64u) {     // wave-uniform, rare
            const uint32_t idx = k + (uint32_t)lane;
            e = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(
                ent_rs, (int)(((ent_start[h] + idx) * 4u) | (idx < ent_count[h] ? 0u : kOobBit)), 0, kAuxStreamOnce);
            if ((e & 0xffffu) != 0u) *reinterpret_cast<short*>(lds + h * kLdsHalf + ((e >> 16) & 1022u)) = (short)e;
        }
    }
    // the staged tables (an LDS-direct load the compiler does not order LDS reads behind) and the maps have landed
    wait_vmem_all();
    wave_sync();
    uint64_t live[2];
    const uint32_t n_cols = scan_tile(lds, lds + Lay<0>::slots, lane, 0u, 0u, live);
    wave_sync();
    column_pass<false, true>(lds, 0u, lds + Lay<0>::slots, lds + kOffQtab, n_cols, qia, qia, lane);
    wave_sync();

    uint8_t* const rec = ring + (size_t)D.frame * L.record_pitch;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        int r[8];
        const uint64_t colbits = live[half];
        if (colbits == 0) {
#pragma unroll
            for (int m = 0; m < 8; m++) r[m] = 0;
        } else {
            // recon_task's row pass: lane (n = hi3, b = lo3), row n of block b, eight int16 w; trunc(5w/2) == trunc(w * 2.5f)
            const int cols_live = 8 - (__builtin_clzll(colbits | 1ull) >> 3);
            const v4u wv = *reinterpret_cast<const v4u*>(lds + half * kLdsHalf + hi3 * 128 + lo3 * 16);
            const v2f k25 = {2.5f, 2.5f};
            const v2f a = v2f{(float)(short)(wv.x & 0xffffu), (float)((int)wv.x >> 16)} * k25;
            const int Y0 = (int)a.x + 128, Y1 = (int)a.y;                           // "+128" of (t+128)/256
            if (cols_live <= 2) {
                butterfly8_lo2(Y0, Y1, r);
            } else {
                const v2f bb = v2f{(float)(short)(wv.y & 0xffffu), (float)((int)wv.y >> 16)} * k25;
                if (cols_live <= 4) {
                    butterfly8_lo4(Y0, Y1, (int)bb.x, (int)bb.y, r);
                } else {
                    const v2f cc = v2f{(float)(short)(wv.z & 0xffffu), (float)((int)wv.z >> 16)} * k25;
                    const v2f dd = v2f{(float)(short)(wv.w & 0xffffu), (float)((int)wv.w >> 16)} * k25;
                    const int Y[8] = {Y0, Y1, (int)bb.x, (int)bb.y, (int)cc.x, (int)cc.y, (int)dd.x, (int)dd.y};
                    butterfly8(Y, r);
                }
            }
            // t / 256 truncating toward zero, every picture type
#pragma unroll
            for (int m = 0; m < 8; m++) {
                r[m] += (r[m] >> 31) & 255;
                r[m] >>= 8;
            }
        }
        // saturated to int16: a guard, no stream and no probe has reached it
        typedef short v2s __attribute__((ext_vector_type(2)));
        v4u out;
        {
            const v2s p0 = __builtin_amdgcn_cvt_pk_i16(r[0], r[1]), p1 = __builtin_amdgcn_cvt_pk_i16(r[2], r[3]);
            const v2s p2 = __builtin_amdgcn_cvt_pk_i16(r[4], r[5]), p3 = __builtin_amdgcn_cvt_pk_i16(r[6], r[7]);
            out.x = __builtin_bit_cast(uint32_t, p0); out.y = __builtin_bit_cast(uint32_t, p1);
            out.z = __builtin_bit_cast(uint32_t, p2); out.w = __builtin_bit_cast(uint32_t, p3);
        }
        uint32_t off;
        if (residual_store(L, T, (uint32_t)half, (uint32_t)lane, &off)) __builtin_nontemporal_store(out, reinterpret_cast<LEON_GLOBAL v4u*>(gptr_mut(rec) + off));
    }
}

// ---- carry: a box along the motion vectors between two delivered frames (include/leon_pipeline.h, leon_pipeline_carry_regions) -----
// One 64-lane wave per record, four records per workgroup; the waves of a workgroup share nothing.  A wave judges its record (every lane
// the same words), picks the motion record M that votes (leon_carry.h), and its lanes stride over the macroblocks the box covers: per
// lane and trip 8 bytes of mv[k] and one byte of info[k], the weight from the box, 64-bit partial sums in registers.  The sums cross
// the wave by shuffles, two 32-bit halves each; lane 0 finishes and stores.  No LDS, no atomics, no barrier; idle waves of the last
// workgroup and waves whose record is refused leave at once, a refused record with its status word alone.
// M's record lies at ring + frames[M].ring * record_pitch, where k_motion wrote it.  A box inside the frame lies inside the coded
// grid (fw <= 16 * mbw, fh <= 16 * mbh: the callers see to it), so every macroblock index is below mbs.
struct CarryCall {
    int32_t fw, fh;                      // the frame
    int32_t mbw;                         // macroblocks a row of the coded picture
    int32_t n_frames, n;                 // frames of the window, records of the call
    uint32_t info_offset, record_pitch;  // MotionLayout's
    uint32_t reserved;
};
struct __attribute__((aligned(4))) CarryWords4 { int32_t w[4]; };          // 16 bytes at a 4-byte aligned address

__device__ __forceinline__ int64_t wave_sum64(int64_t v)
{
    uint32_t lo = (uint32_t)(uint64_t)v, hi = (uint32_t)((uint64_t)v >> 32);
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t olo = (uint32_t)__shfl_xor((int)lo, m, 64), ohi = (uint32_t)__shfl_xor((int)hi, m, 64);
        const uint64_t sum = (((uint64_t)hi << 32) | lo) + (((uint64_t)ohi << 32) | olo);
        lo = (uint32_t)sum; hi = (uint32_t)(sum >> 32);
    }
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kRgbaBlock) void k_carry(const CarryRecord* __restrict__ recs, const CarryFrame* __restrict__ frames,
                                                       const uint8_t* __restrict__ ring, int32_t* __restrict__ out, int32_t* __restrict__ votes,
                                                       int32_t* __restrict__ status, CarryCall c)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * (uint32_t)(kRgbaBlock / 64) + (threadIdx.x >> 6);
    if (i >= (uint32_t)c.n) return;
    const CarryRecord r = recs[i];
    int32_t st = carry_record_status(r, c.fw, c.fh, c.n_frames), m = 0, sense = 1, d = 0;
    if (st == kRegionOk) {
        const CarryFrame fs = frames[r.frame], ft = frames[r.target];
        st = carry_pick(r.frame, r.target, ft.fwd, ft.bwd, fs.fwd, fs.bwd, &m, &sense, &d);
    }
    if (st != kRegionOk) {
        if (lane == 0 && status) status[i] = st;
        return;
    }
    CarrySums s{0, 0, 0, 0};
    if (d) {
        const uint8_t* __restrict__ rec = ring + (size_t)frames[m].ring * c.record_pitch;
        const int32_t i0 = r.x >> 4, j0 = r.y >> 4;
        const uint32_t cols = (uint32_t)(((r.x + r.width - 1) >> 4) - i0 + 1), rows = (uint32_t)(((r.y + r.height - 1) >> 4) - j0 + 1);
        for (uint32_t k = lane; k < cols * rows; k += 64u) {
            const uint32_t jj = k / cols, ii = k - jj * cols;
            const int32_t mi = i0 + (int32_t)ii, mj = j0 + (int32_t)jj;
            const uint32_t mb = (uint32_t)mj * (uint32_t)c.mbw + (uint32_t)mi;
            const uint2 mv = *reinterpret_cast<const uint2*>(rec + (size_t)mb * 8u);
            const uint32_t info = rec[c.info_offset + mb];
            carry_vote(d, info, mv.x, mv.y, carry_weight(r.x, r.y, r.width, r.height, mi, mj), &s);
        }
        s.A = wave_sum64(s.A);
        s.I = wave_sum64(s.I);
        s.SH = wave_sum64(s.SH);
        s.SV = wave_sum64(s.SV);
    }
    if (lane != 0) return;
    int32_t o[8], v[4];
    carry_finish(r, c.fw, c.fh, sense, s, o, v);
    CarryWords4* po = reinterpret_cast<CarryWords4*>(out + (size_t)i * 8u);
    po[0] = CarryWords4{{o[0], o[1], o[2], o[3]}};
    po[1] = CarryWords4{{o[4], o[5], o[6], o[7]}};
    if (votes) *reinterpret_cast<CarryWords4*>(votes + (size_t)i * 4u) = CarryWords4{{v[0], v[1], v[2], v[3]}};
    if (status) status[i] = kRegionOk;
}

// ---- propagate: a dense map along the motion vectors, a gather through the target's record (include/leon_pipeline.h,
// leon_pipeline_propagate_maps) ----
// One launch per call: blockIdx.z the hop record, blockIdx.y a group of c.g.group planes, blockIdx.x x 256 lanes over one plane's work
// units (leon_propagate.h: a destination dword on the fast path, a cell otherwise -- chosen per call, so uniform over the grid).  A lane
// works out its macroblock, pick and source address once and loops over its group's planes: maps with few cells and many planes get
// their parallelism from y.  Consecutive lanes store consecutive dwords (cells); the source of a unit the clamp leaves alone is two
// aligned dwords funnelled by v_alignbyte, as the reconstruction kernels' reference fetch.  via is written by plane group 0 alone, the
// status word by one lane of the hop.  No LDS, no atomics, no barrier, no scratch; lanes of a refused record leave at once.
// T's record lies at ring + frames[T].ring * record_pitch, where k_motion wrote it.  A cell of the frame lies inside the coded grid
// (fw <= 16 * mbw, fh <= 16 * mbh: the callers see to it), so every macroblock index is below mbs.
struct PropagateCall {
    PropagateGeom g;
    size_t slot_pitch, maps_bytes;       // the caller's buffer: n_slots maps at slot_pitch, maps_bytes in all
    int32_t n_frames, n_slots;           // frames of the window, maps of the buffer
    uint32_t fill;
    uint32_t info_offset, record_pitch;  // MotionLayout's
    uint32_t reserved;
};

__global__ __launch_bounds__(kRgbaBlock) void k_propagate(const PropagateHop* __restrict__ hops, const CarryFrame* __restrict__ frames,
                                                           const uint8_t* __restrict__ ring, uint8_t* maps, uint8_t* __restrict__ via,
                                                           int32_t* __restrict__ status, PropagateCall c)
{
    const uint32_t i = blockIdx.z, u = blockIdx.x * (uint32_t)kRgbaBlock + threadIdx.x;
    const PropagateHop h = hops[i];
    const int32_t st = propagate_hop_status(h, c.n_frames, c.n_slots);
    if (status && u == 0 && blockIdx.y == 0) status[i] = st;
    if (st != kRegionOk || u >= c.g.units) return;
    const int32_t p0 = (int32_t)blockIdx.y * c.g.group, p1 = p0 + c.g.group < c.g.planes ? p0 + c.g.group : c.g.planes;
    uint8_t* v = via && blockIdx.y == 0 ? via + (size_t)i * (size_t)c.g.mh * (size_t)c.g.mw : nullptr;
    propagate_unit(c.g, ring + (size_t)frames[h.target].ring * c.record_pitch, c.info_offset, maps, c.maps_bytes, c.slot_pitch, h, c.fill, v, u, p0, p1);
}

// ---- accumulate: motion and residual summed along a GOP's chain, a gather through the target's records (include/leon_pipeline.h,
// leon_pipeline_accumulate) ----
// One launch per call: blockIdx.z the hop, blockIdx.y the plane among those asked for (AX AY AGE | RY RCb RCr), blockIdx.x x 256 lanes
// over the plane's work units (leon_accumulate.h: 4 destination elements, 8 bytes, never across a macroblock).  The grid's x is sized
// for a luma plane; lanes behind a chroma plane's units, and lanes of a refused hop, leave at once.  A lane works out its macroblock
// and pick as k_propagate does, reads the source's 8 bytes as the aligned dwords around their 2-byte aligned address (v_alignbyte),
// T's residual as 8 aligned bytes, adds with two packed saturating 16-bit adds and stores 8 bytes: consecutive lanes store
// consecutive 8 bytes, a wave one 512-byte run of a row.  A unit the clamp touches goes element by element.  via (a byte a
// macroblock) is written by plane 0 alone, by the lane of the macroblock's first unit; the status word by one lane of the hop.
// No LDS, no atomics, no barrier, no scratch.  T's records lie at motion + frames[T].ring * motion_pitch and residual + frames[T].ring *
// residual_pitch, where k_motion and k_residual wrote them (residual may be null where the parts do not ask for it).
struct AccumulateCall {
    AccumulateGeom g;
    size_t slot_pitch, slots_bytes;      // the caller's buffer: n_slots accumulators at slot_pitch, slots_bytes in all
    int32_t n_frames, n_slots;           // frames of the window, accumulators of the buffer
    uint32_t info_offset, motion_pitch;  // MotionLayout's
    uint32_t residual_pitch;             // ResidualLayout's
    uint32_t reserved;
};

__global__ __launch_bounds__(kRgbaBlock) void k_accumulate(const PropagateHop* __restrict__ hops, const CarryFrame* __restrict__ frames,
                                                            const uint8_t* __restrict__ motion, const uint8_t* __restrict__ residual, uint8_t* slots,
                                                            uint8_t* __restrict__ via, int32_t* __restrict__ status, AccumulateCall c)
{
    const uint32_t i = blockIdx.z, u = blockIdx.x * (uint32_t)kRgbaBlock + threadIdx.x;
    const int32_t q = (int32_t)blockIdx.y;
    const PropagateHop h = hops[i];
    const int32_t st = propagate_hop_status(h, c.n_frames, c.n_slots);
    if (status && u == 0 && q == 0) status[i] = st;
    if (st != kRegionOk || u >= accumulate_units(c.g, q)) return;
    const uint32_t ring = frames[h.target].ring;
    uint8_t* v = via && q == 0 ? via + (size_t)i * (size_t)c.g.mbw * (size_t)(c.g.ch >> 4) : nullptr;
    accumulate_unit(c.g, motion + (size_t)ring * c.motion_pitch, c.info_offset, residual ? residual + (size_t)ring * c.residual_pitch : nullptr, slots, c.slots_bytes,
                    c.slot_pitch, h, v, q, u);
}

// ---- fields: boxes of int16 fields -- motion vectors, residual planes, accumulators -- as a model's tensors (include/leon_pipeline.h,
// leon_pipeline_field_tensors) ----
// k_regions' shape behind k_box_tables: blockIdx.z the region of the chunk, blockIdx.x / y the 32 x 8 tiles of the out size.  A workgroup
// reads the region's descriptor (one address per workgroup: scalar loads) and leaves at once on a non-zero status; otherwise it takes
// the tile's rows of the region's tables into LDS once and then, per channel, runs leon_fields.h's three steps: the horizontal pass of
// the frame rows the tile's vertical taps need, gathered from the field's cells (2-byte loads; lanes of neighbouring columns read
// neighbouring or the same cells) with 64-bit multiply-adds, into LDS as int16; the vertical pass from LDS, a lane per output sample,
// whose element goes into the packed tile at its row's place in its 16-byte line; and the rows out in whole 16-byte lines, the lines
// at a row's ends element by element.  The item of a region is src + frame_id * item_pitch: a record of the ring through the window's
// table, or an item of the caller's buffer through an identity table.  Static LDS 16992 bytes, no scratch.  DTYPE: LEON_TENSOR_F16 /
// _BF16 / _F32.
struct FieldCall {
    FieldChannel ch[kFieldMaxChannels];
    int32_t fw, fh, ow, oh;
    int32_t channels, reserved;
    size_t item_pitch;
};
template <int DTYPE>
__global__ __launch_bounds__(kRgbaBlock) void k_fields(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, const RegionDesc* __restrict__ descs,
                                                       const int32_t* __restrict__ tabs, FieldCall c)
{
    static_assert(kFieldLanes == kRgbaBlock, "a lane per sample of the tile");
    __shared__ FieldTile t;
    const RegionDesc& d = descs[blockIdx.z];
    if (d.status != kRegionOk) return;   // a refused region stores nothing anywhere
    const int32_t* rt = tabs + d.rt_base;
    const FieldTables T{rt, rt + d.off_cx, rt + d.off_wx, rt + d.off_fy, rt + d.off_cy, rt + d.off_wy, d.taps_x, d.taps_y};
    const FieldTileAt a = field_tile_at(c.ow, c.oh, (int32_t)blockIdx.x, (int32_t)blockIdx.y);
    const int32_t tid = (int32_t)threadIdx.x;
    const uint8_t* item = src + (size_t)d.frame_id * c.item_pitch;
    uint8_t* dst = out + join64(d.dst_lo, d.dst_hi);
    field_step_tables(t, T, a, tid);
    __syncthreads();
    int32_t ry0, rows;
    field_tile_rows(t, a, &ry0, &rows);
    for (int32_t q = 0; q < c.channels; q++) {
        field_step_h(t, item, c.ch[q], a, ry0, rows, tid);
        __syncthreads();
        field_step_v(t, c.ch[q], a, c.ow, c.oh, q, DTYPE, ry0, rows, tid);
        __syncthreads();          // (the next channel's horizontal pass stands between this store and the next write of the packed tile)
        field_step_store(t, dst, a, c.ow, c.oh, q, DTYPE, tid);
    }
}

// ---- gauge: the statistics of a frame's motion and activity records under a box (include/leon_pipeline.h, leon_pipeline_gauge_regions) --
// k_carry's shape: one 64-lane wave per record, four records per workgroup, the waves of a workgroup share nothing.  A wave judges its
// record (leon_gauge.h; every lane the same words) and its lanes stride over the macroblocks the box covers: per lane and trip the 8
// bytes of the activity cell, the 8 bytes of mv[k] and one byte of info[k] -- whichever the call's sources ask for, a choice that is
// uniform over the grid --, the weight from the box, 64-bit partial sums in registers.  The sums of the sources asked for and the
// maximum cross the wave by shuffles; lane 0 finishes and stores 16 words.  No LDS, no atomics, no barrier; idle waves of the last
// workgroup and waves whose record is refused leave at once, a refused record with its status word alone.
// Frame f's records lie at motion + frames[f].ring * motion_pitch and activity + frames[f].ring * activity_pitch, where k_motion and
// k_activity wrote them (a ring the call does not read may be null).  A box inside the frame lies inside the coded grid
// (fw <= 16 * mbw, fh <= 16 * mbh: the callers see to it), so every macroblock index is below mbs.
struct GaugeCall {
    int32_t fw, fh;                      // the frame
    int32_t mbw;                         // macroblocks a row of the coded picture
    int32_t n_frames, n;                 // frames of the window, records of the call
    int32_t sources;                     // kGaugeMotion | kGaugeActivity
    uint32_t info_offset, motion_pitch;  // MotionLayout's
    uint32_t activity_pitch;             // ActivityLayout's
    uint32_t reserved;
};
struct __attribute__((aligned(8))) GaugeWords2 { int64_t w[2]; };          // 16 bytes at an 8-byte aligned address

__global__ __launch_bounds__(kRgbaBlock) void k_gauge(const GaugeRecord* __restrict__ recs, const CarryFrame* __restrict__ frames,
                                                       const uint8_t* __restrict__ motion, const uint8_t* __restrict__ activity,
                                                       int64_t* __restrict__ stats, int32_t* __restrict__ status, GaugeCall c)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * (uint32_t)(kRgbaBlock / 64) + (threadIdx.x >> 6);
    if (i >= (uint32_t)c.n) return;
    const GaugeRecord r = recs[i];
    const int32_t st = gauge_record_status(r, c.fw, c.fh, c.n_frames);
    if (st != kRegionOk) {
        if (lane == 0 && status) status[i] = st;
        return;
    }
    const bool act = (c.sources & kGaugeActivity) != 0, mot = (c.sources & kGaugeMotion) != 0;
    const uint32_t ring = frames[r.frame].ring;
    const uint8_t* __restrict__ mrec = motion + (mot ? (size_t)ring * c.motion_pitch : 0);
    const uint8_t* __restrict__ arec = activity + (act ? (size_t)ring * c.activity_pitch : 0);
    GaugeSums s{};
    const int32_t i0 = r.x >> 4, j0 = r.y >> 4;
    const uint32_t cols = (uint32_t)(((r.x + r.width - 1) >> 4) - i0 + 1), rows = (uint32_t)(((r.y + r.height - 1) >> 4) - j0 + 1);
    for (uint32_t k = lane; k < cols * rows; k += 64u) {
        const uint32_t jj = k / cols, ii = k - jj * cols;
        const int32_t mi = i0 + (int32_t)ii, mj = j0 + (int32_t)jj;
        const uint32_t mb = (uint32_t)mj * (uint32_t)c.mbw + (uint32_t)mi;
        uint2 cell = uint2{0u, 0u}, mv = uint2{0u, 0u};
        uint32_t info = 0u;
        if (act) cell = *reinterpret_cast<const uint2*>(arec + (size_t)mb * 8u);
        if (mot) {
            mv = *reinterpret_cast<const uint2*>(mrec + (size_t)mb * 8u);
            info = mrec[c.info_offset + mb];
        }
        gauge_cell(c.sources, carry_weight(r.x, r.y, r.width, r.height, mi, mj), cell.x, cell.y, info, mv.x, mv.y, &s);
    }
    s.w[0] = wave_sum64(s.w[0]);
    if (act) {
#pragma unroll
        for (int k = 1; k < 7; k++) s.w[k] = wave_sum64(s.w[k]);
        s.w[7] = (int64_t)wave_max((uint32_t)s.w[7]);
    }
    if (mot) {
#pragma unroll
        for (int k = 8; k < kGaugeWords; k++) s.w[k] = wave_sum64(s.w[k]);
    }
    if (lane != 0) return;
    int64_t o[kGaugeWords];
    gauge_finish(c.sources, s, o);
    GaugeWords2* po = reinterpret_cast<GaugeWords2*>(stats + (size_t)i * kGaugeWords);
#pragma unroll
    for (int k = 0; k < kGaugeWords / 2; k++) po[k] = GaugeWords2{{o[2 * k], o[2 * k + 1]}};
    if (status) status[i] = kRegionOk;
}

// ---- propose: boxes of the connected components of a frame's hot macroblocks (include/leon_pipeline.h, leon_pipeline_propose_regions) --
// One workgroup of 8 waves per request, everything between the records and the rows in LDS (leon_propose.h, ProposeLds: 16-bit
// labels, two bit masks, two dwords a row).  The steps, a barrier between each two:
//   1  the hot mask: a lane a cell, 8 + 1 + 8 bytes of the frame's records -- whichever the sources ask for --, a wave's ballot is two words;
//   2  every hot cell points to the first cell of its run in its row (bit arithmetic on the mask: a row is joined at depth 1);
//   3  union with the row above, by smallest index: the larger root is hung under the smaller with a 16-bit minimum (a compare-and-swap
//      on the label's dword), and whoever finds a root taken goes on with what it pointed to.  Labels only ever fall and a label never
//      exceeds its cell, so the root of a component is its smallest cell -- its `first` -- whatever the order of the waves;
//   4  every hot cell points to its root;
//   5  the root mask (ballot); a root's own slot, which said nothing but "root", becomes 0;
//   6  every other hot cell adds 1 to its root's slot: cells - 1, at most 65535, never a carry into the neighbouring label;
//   7  the roots with cells >= min_cells are counted, a thread a piece of the root mask, and the counts scanned by shuffles;
//   8  in raster order -- the order of `first` -- the selected roots take rows 0, 1, ...: the first K write {first, cells - 1} and
//      their own cell as the extent and keep the row in their slot, every other root keeps 0xffff;
//   9  every other hot cell of a component with a row widens the row's extent (three 8-bit maxima in a dword, compare-and-swap only
//      when a field grows);
//  10  the K rows go out, boxes first and filler behind, with count and status.
// A refused request leaves with its status word alone.  Every index into LDS is below ProposeLds's sizes for mbs = mbw * mbh and
// K = max_boxes, which the launch passes as dynamic LDS; every macroblock index is below mbs.
struct ProposeCall {
    ProposeConfig cfg;
    int32_t fw, fh, mbw, mbh;            // the frame, the coded grid
    int32_t n_frames, n;                 // frames of the window, requests of the call
    uint32_t info_offset, motion_pitch;  // MotionLayout's
    uint32_t activity_pitch;             // ActivityLayout's
    uint32_t reserved;
};

__device__ __forceinline__ uint32_t propose_get(const volatile uint32_t* lab, uint32_t c) { return (lab[c >> 1] >> ((c & 1u) << 4)) & 0xffffu; }
__device__ __forceinline__ void propose_put(volatile uint32_t* lab, uint32_t c, uint32_t v) { reinterpret_cast<volatile uint16_t*>(lab)[c] = (uint16_t)v; }
__device__ __forceinline__ uint32_t propose_find(const volatile uint32_t* lab, uint32_t c)
{
    for (uint32_t l = propose_get(lab, c); l != c; l = propose_get(lab, c)) c = l;
    return c;
}
// label a = min(label a, b); what stood there
__device__ __forceinline__ uint32_t propose_min(uint32_t* lab, uint32_t a, uint32_t b)
{
    uint32_t* const p = lab + (a >> 1);
    const uint32_t sh = (a & 1u) << 4;
    uint32_t w = *(volatile uint32_t*)p;
    for (;;) {
        const uint32_t cur = (w >> sh) & 0xffffu;
        if (cur <= b) return cur;
        const uint32_t got = atomicCAS(p, w, (w & ~(0xffffu << sh)) | (b << sh));
        if (got == w) return cur;
        w = got;
    }
}
__device__ __forceinline__ void propose_union(uint32_t* lab, uint32_t a, uint32_t b)
{
    for (;;) {
        a = propose_find(lab, a);
        b = propose_find(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = propose_min(lab, a, b);
        if (old == a) return;
        a = old;            // a was a root no longer: what it pointed to has to meet b as well
    }
}

__global__ __launch_bounds__(kProposeThreads) void k_propose(const int32_t* __restrict__ requests, const CarryFrame* __restrict__ frames,
                                                             const uint8_t* __restrict__ motion, const uint8_t* __restrict__ activity,
                                                             int32_t* __restrict__ regions, int32_t* __restrict__ info, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ status, ProposeCall c)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_propose[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, q = blockIdx.x;
    const int32_t f = requests[q];
    if (propose_request_status(f, c.n_frames) != kRegionOk) {
        if (tid == 0 && status) status[q] = kRegionFrame;
        return;
    }
    const uint32_t mbw = (uint32_t)c.mbw, mbs = mbw * (uint32_t)c.mbh, K = (uint32_t)c.cfg.max_boxes;
    const ProposeLds L = propose_lds(mbs, K);
    uint32_t* const lab = s_propose;
    uint32_t* const hot = s_propose + L.hot;
    uint32_t* const root = s_propose + L.root;
    uint32_t* const rows = s_propose + L.rows;
    uint32_t* const scan = s_propose + L.scan;
    const uint32_t padded = 32u * L.mask_words;
    const bool act = (c.cfg.sources & kProposeActivity) != 0, mot = (c.cfg.sources & kProposeMotion) != 0;
    const uint32_t ring = frames[f].ring;
    const uint8_t* __restrict__ mrec = motion + (mot ? (size_t)ring * c.motion_pitch : 0);
    const uint8_t* __restrict__ arec = activity + (act ? (size_t)ring * c.activity_pitch : 0);

    for (uint32_t k = tid; k < padded; k += kProposeThreads) {                              // 1
        bool h = false;
        if (k < mbs) {
            const uint32_t j = k / mbw, i = k - j * mbw;
            uint2 mv = uint2{0u, 0u};
            uint32_t lo = 0u, nf = 0u;
            if (act) lo = *reinterpret_cast<const uint32_t*>(arec + (size_t)k * 8u);
            if (mot) {
                mv = *reinterpret_cast<const uint2*>(mrec + (size_t)k * 8u);
                nf = mrec[c.info_offset + k];
            }
            h = propose_hot(c.cfg, c.fw, c.fh, (int32_t)i, (int32_t)j, lo, nf, mv.x, mv.y);
        }
        const uint64_t b = __ballot(h);
        if (lane == 0) {
            hot[k >> 5] = (uint32_t)b;
            hot[(k >> 5) + 1u] = (uint32_t)(b >> 32);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < mbs; k += kProposeThreads)                                   // 2
        if (propose_bit(hot, k)) propose_put(lab, k, propose_run_start(hot, k, k - k % mbw));
    __syncthreads();
    const bool corners = c.cfg.connectivity == 8;
    for (uint32_t k = tid + mbw; k < mbs; k += kProposeThreads) {                           // 3
        if (!propose_bit(hot, k)) continue;
        const uint32_t i = k % mbw, up = k - mbw;
        const bool left = i > 0u && propose_bit(hot, k - 1u);
        if (propose_bit(hot, up)) {
            // (the left neighbour joins the two runs where it and the cell above it are hot)
            if (!(left && propose_bit(hot, up - 1u))) propose_union(lab, k, up);
        } else if (corners) {
            // (the cell above is cold: a corner neighbour is a run of its own above; where the left / right neighbour is hot, that
            // corner is the cell above IT)
            if (i > 0u && !left && propose_bit(hot, up - 1u)) propose_union(lab, k, up - 1u);
            if (i + 1u < mbw && !propose_bit(hot, k + 1u) && propose_bit(hot, up + 1u)) propose_union(lab, k, up + 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < mbs; k += kProposeThreads)                                   // 4
        if (propose_bit(hot, k)) propose_put(lab, k, propose_find(lab, k));
    __syncthreads();
    for (uint32_t k = tid; k < padded; k += kProposeThreads) {                              // 5
        const bool r = k < mbs && propose_bit(hot, k) && propose_get(lab, k) == k;
        const uint64_t b = __ballot(r);
        if (lane == 0) {
            root[k >> 5] = (uint32_t)b;
            root[(k >> 5) + 1u] = (uint32_t)(b >> 32);
        }
        if (r) propose_put(lab, k, 0u);
    }
    __syncthreads();
    for (uint32_t k = tid; k < mbs; k += kProposeThreads)                                   // 6
        if (propose_bit(hot, k) && !propose_bit(root, k)) {
            const uint32_t r = propose_get(lab, k);
            atomicAdd(lab + (r >> 1), 1u << ((r & 1u) << 4));
        }
    __syncthreads();
    const uint32_t per = (L.mask_words + kProposeThreads - 1u) / kProposeThreads;           // 7
    const uint32_t w0 = min(tid * per, L.mask_words), w1 = min(w0 + per, L.mask_words), least = (uint32_t)c.cfg.min_cells;
    uint32_t sum = 0u;
    for (uint32_t w = w0; w < w1; w++)
        for (uint32_t m = root[w]; m; m &= m - 1u) sum += propose_get(lab, (w << 5) + (uint32_t)__builtin_ctz(m)) + 1u >= least ? 1u : 0u;
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += v;
    }
    if (lane == 63u) scan[wv] = incl;
    __syncthreads();
    uint32_t run = incl - sum, total = 0u;                                                  // 8
    for (uint32_t w = 0; w < (uint32_t)kProposeThreads / 64u; w++) {
        run += w < wv ? scan[w] : 0u;
        total += scan[w];
    }
    for (uint32_t w = w0; w < w1; w++)
        for (uint32_t m = root[w]; m; m &= m - 1u) {
            const uint32_t r = (w << 5) + (uint32_t)__builtin_ctz(m), less = propose_get(lab, r);
            uint32_t row = 0xffffu;
            if (less + 1u >= least) {
                if (run < K) {
                    row = run;
                    rows[2u * row] = r | (less << 16);
                    rows[2u * row + 1u] = propose_extent(r % mbw, r / mbw);
                }
                run++;
            }
            propose_put(lab, r, row);
        }
    __syncthreads();
    for (uint32_t k = tid; k < mbs; k += kProposeThreads)                                   // 9
        if (propose_bit(hot, k) && !propose_bit(root, k)) {
            const uint32_t row = propose_get(lab, propose_get(lab, k));
            if (row == 0xffffu) continue;
            const uint32_t e = propose_extent(k % mbw, k / mbw);
            uint32_t* const p = rows + 2u * row + 1u;
            uint32_t w = *(volatile uint32_t*)p;
            for (;;) {
                const uint32_t joined = propose_extent_join(w, e);
                if (joined == w) break;
                const uint32_t got = atomicCAS(p, w, joined);
                if (got == w) break;
                w = got;
            }
        }
    __syncthreads();
    const uint32_t written = total < K ? total : K;                                         // 10
    for (uint32_t k = tid; k < K; k += kProposeThreads) {
        int32_t o[8], nf[2];
        if (k < written) {
            const uint32_t a = rows[2u * k], e = rows[2u * k + 1u], first = a & 0xffffu;
            propose_box(f, c.fw, c.fh, (int32_t)(255u - (e & 255u)), (int32_t)((e >> 8) & 255u), (int32_t)(first / mbw), (int32_t)((e >> 16) & 255u), o);
            nf[0] = (int32_t)(a >> 16) + 1;
            nf[1] = (int32_t)first;
        } else {
            propose_filler(f, o, nf);
        }
        int32_t* const po = regions + ((size_t)q * K + k) * 8u;
#pragma unroll
        for (int u = 0; u < 8; u++) po[u] = o[u];
        if (info) {
            info[((size_t)q * K + k) * 2u] = nf[0];
            info[((size_t)q * K + k) * 2u + 1u] = nf[1];
        }
    }
    if (tid == 0) {
        count[q] = (int32_t)total;
        if (status) status[q] = kRegionOk;
    }
}

// ---- measured HBM roofline -----------------------------------------------------------
// One 16-byte element per thread, no loop: the fastest of the copy shapes probed on MI355X
// (tools/probe/bw_probe.cpp: 6.3 TB/s vs 4.8-5.9 TB/s for grid-stride forms).
__global__ __launch_bounds__(kRgbaBlock) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// The same shape with R source streams and W destination streams (16 B per lane and stream, no loop): the yardstick for
// launches that do not read and write in equal parts -- an I launch of the fused path writes 55-65 % of its bytes.
// R = 0: write only; W = 0: read only (the store is there for the compiler and never happens).
template <int R, int W>
__global__ __launch_bounds__(kRgbaBlock) void k_stream16(const uint4* __restrict__ s0, const uint4* __restrict__ s1,
                                                         uint4* __restrict__ d0, uint4* __restrict__ d1, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint4 v = uint4{(uint32_t)i, 0x5a5a5a5au, (uint32_t)(i >> 32), 0xa5a5a5a5u};
    if (R >= 1) v = s0[i];
    if (R >= 2) { const uint4 u = s1[i]; v.x ^= u.x; v.y ^= u.y; v.z ^= u.z; v.w ^= u.w; }
    if (W >= 1) d0[i] = v;
    if (W >= 2) d1[i] = v;
    if (W == 0 && v.x == 0x12345678u && v.y == 0x9abcdef0u && v.z == 0x0fedcba9u) d0[i] = v;      // never (sources hold 0x5a bytes)
}

}  // namespace leon
