// leon_pipeline_impl.h -- implementation of include/leon_pipeline.h; included at the end of leon_hip.cpp
// (it uses the decoder's internals: submit_batch_any, the slot ring, the decoder's stream).
#include "../../include/leon_pipeline.h"
#include "../../include/leon_vlc.h"
#include "leon_vlc_gpu.h"
#include "leon_pipe_flow.h"

#include <atomic>
#include <sys/stat.h>
#include <chrono>
#include <cmath>
#include <memory>
#include <mutex>
#include <thread>

namespace {

using Clock = std::chrono::steady_clock;

struct PipePic {                 // one parsed picture: offsets of its arrays inside the GOP's arena
    int32_t type, tref;
    uint32_t n_entries;
    double ts_ms;
    size_t grp_off, entries, qscale, intra, repadd, mb_dir, mv_fwd, mv_bwd;   // (size_t)-1: absent
    int32_t qm = -1;             // index into its GOP's `qms` (matrices of the sequence header in force), -1: the stream's first
    bool shown = true;           // false: reconstructed for the pictures that predict from it, not converted nor delivered (trim_to_target)
};

struct Arena {                   // pinned host buffer + its device twin, one GOP at a time
    PinnedBuf<> host;            // each its own allocation, or a borrowed piece of the pipeline's slabs (gpu_parser) until a GOP outgrows it
    DevBuf<> dev;
    size_t used = 0;
};

using leon_flow::PipeRun;

struct GopJob {
    std::shared_ptr<const PipeRun> run;      // the run it was parsed for
    bool open_gop = false;       // its GOP header says closed_gop = 0
    bool broken_link = false;    // ... and broken_link = 1
    // an open GOP's leading B pictures (in front of its second anchor) predict forward from the last anchor of the key-map entry
    // before it.  true: this run decodes that entry, directly before this GOP and in the same pass of `loop`, and the header does
    // not say broken_link (parser_main).  false: the leading B pictures of an open GOP are dropped (drop_leading_b)
    bool has_pred = false;
    uint64_t gop = 0;            // running index among the GOPs of this pipeline
    uint64_t key_gop = 0;        // GOP id in the stream (key-map index, counting on across loops)
    Arena* arena = nullptr;
    std::vector<PipePic> pics;
    double gop_ts_ms = 0;
    int status = LEON_OK;
    std::string err;
    // sequence headers of this shard whose quantiser matrices differ from the stream's first: the reference reloads them
    // at every header (decoders/jsv.js:540-558), a picture is dequantised with the ones in force when it was coded
    std::vector<std::array<uint8_t, 128>> qms;
    // gpu_parser: the slices of the GOP and its pictures as the device kernels want them (pointers into the arena's
    // device twin; VlcSlice::pic counts inside the GOP until submit_window rebases it), what of the arena is uploaded
    // (stream bytes) and what is cleared on the device (counters, error words, maps)
    std::vector<leon::VlcSlice> slices;
    std::vector<leon::VlcPic> vpics;
    size_t upload_bytes = 0, zero_begin = 0, zero_bytes = 0;
};

struct PipeWindow {
    std::shared_ptr<const PipeRun> run;
    int64_t id = 0;
    int ring = 0;
    std::vector<std::unique_ptr<GopJob>> jobs;
    std::vector<leon_pipeline_frame> frames;
    std::vector<uint8_t*> tensors;       // output TENSOR: frames[i]'s tensor
    std::vector<uint32_t> frame_ids;     // ... and its index in the ring entry's lanes (what k_tensor finds planes and tensor by)
    std::vector<leon_pipeline_motion_frame> motion;      // output MOTION: frames[i]'s record and references
    std::vector<leon::MotionDesc> motion_descs;          // ... and what k_motion makes the record from
    std::vector<uint32_t> carry_table;                   // ... and per frame a leon::CarryFrame (ring id, fwd, bwd, 0): what k_carry reads
    std::vector<uint8_t*> activity;                      // output ACTIVITY: frames[i]'s record
    std::vector<leon::ActivityDesc> activity_descs;      // ... and what k_activity makes the record from
    std::vector<uint8_t*> residual;                      // output RESIDUAL: frames[i]'s record
    std::vector<leon::ResidualDesc> residual_descs;      // ... and what k_residual makes the record from
    Event done;
    int status = LEON_OK;
    uint32_t n_vpics = 0;        // gpu_parser: error words of the window's pictures are in the ring entry's h_err
};

struct VlcRing {                 // gpu_parser: per ring entry, the window's slice / picture descriptors
    Mirror<char> desc;           // pinned: [VlcSlice x n][VlcPic x m]; device: the same + [slice_words x n][error x m]
    PinnedBuf<uint32_t> h_err;   // pinned copy of the error words
};

using PipeFlow = leon_flow::Flow<GopJob, PipeWindow>;       // the thread protocol: leon_pipe_flow.h

// A record output (MOTION, ACTIVITY): one record per frame in a device ring, `pitch` apart and addressed by the frame's index like its
// planes and tensor, written by a kernel on the decoder's stream behind the last level from one descriptor per frame; per ring entry
// the descriptors of its window's frames (pinned, device).  The window's own list of them is a PipeWindow vector (launch_records).
template <class Desc>
struct RecordOutput {
    DevBuf<uint8_t> ring;
    size_t pitch = 0;
    Mirror<Desc> descs;
    uint8_t* record(size_t frame) const { return ring + frame * pitch; }
};

constexpr size_t kNone = (size_t)-1;

}  // namespace

struct leon_pipeline {
    leon_pipeline_config cfg{};
    leon_pipeline_info info{};
    const uint8_t* stream = nullptr;
    size_t bytes = 0;
    leon_pipeline_callback cb = nullptr;
    void* user = nullptr;
    leon_vlc_info vinfo{};
    std::vector<uint64_t> shard_begin, shard_end;     // byte ranges of the GOP shards
    std::vector<uint32_t> shard_gops;                 // key-map ids this pipeline may decode (all, or g % shard_count == shard_index)
    bool has_keymap = false;
    int W = 32, R = 2, K = 1, max_pics = 16;
    uint64_t st_wait_ring_ns = 0, st_wait_scan_ns = 0;       // submit thread: waiting for a ring entry / for the window's GOPs to be parsed
    std::string capture_dir;     // LEON_DEBUG_CAPTURE=<dir> at create: everything a window's launches read and wrote goes to files (capture_*)
    bool unfused = false;        // frame_width % 8 != 0, or the GL flavour: planes for every picture, one display conversion launch per picture
    int flavour = LEON_RGB_CPU_TWIN;      // leon_pipeline_config.display_flavour
    size_t frame_bytes = 0;      // RGBA bytes of a frame
    int output = LEON_PIPELINE_OUTPUT_RGBA;           // leon_pipeline_config.output, 0 resolved
    FrameOut planes_geom{};      // the frames' plane layout (planes_layout)
    MapLayout maps{};            // a picture's maps in the arenas (map_layout)
    size_t planes_bytes = 0;     // one frame's planes record [Y | Cb | Cr (| A)], a multiple of 256

    leon_decoder* dec = nullptr;
    // Open GOPs across windows (submit thread only).  The leading B pictures of a window's first GOP predict from the last anchor
    // of the window before, whose slot this window's own anchors overwrite: submit_window copies it to the carry slot first.
    // What is remembered belongs to a run and a GOP of it: a window of another run, or one that does not follow directly, never
    // matches.  Behind the carry slot: one hold slot per lane (plan_levels).
    int carry_slot = -1;
    uint64_t last_run = 0;       // PipeRun::id, 0: nothing remembered
    uint64_t last_gop = 0;       // the run's GOP the remembered anchor closes
    int last_anchor = -1;        // its slot, -1: none
    int last_anchor_tref = -1;   // its display index (what the motion records of the next window's leading B pictures name)
    // (the streams stand in front of the buffers their work touches: members go in reverse order, the buffers first)
    Stream copy_stream;
    // The parser kernels of window n + 1 run beside the reconstruction of window n -- and beside the parser kernels of
    // window n + 2, on a second stream: a parse launch lasts as long as its longest slice (one lane, symbol after symbol) and
    // leaves three quarters of the issue slots idle; two of them side by side take little longer than one.
    Stream vlc_stream[2];
    DevBuf<uint8_t> d_rgba;                           // R ring entries of W * max_pics frames (output RGBA)
    DevBuf<uint8_t> d_planes;                         // the same for the frames' planes records (output YCbCr, and what the tensors are made from)
    // output TENSOR: the ring of [3][fh][fw] tensors (tensor_pitch apart), the element table T (host, device), and per ring entry
    // the frame indices of its window for k_tensor (pinned, device)
    DevBuf<uint8_t> d_tensor;
    int tensor_dtype = 0, tensor_layout = 0;          // LEON_TENSOR_*, LEON_TENSOR_LAYOUT_* (which k_tensor / k_resample: by element bytes and layout)
    size_t tensor_elem = 0, tensor_bytes = 0, tensor_pitch = 0;
    std::vector<uint8_t> tensor_table;
    DevBuf<uint32_t> d_tensor_table;
    Mirror<uint32_t> tensor_ids;
    // outputs MOTION and ACTIVITY (RecordOutput), and what k_motion and k_activity take of the picture's grid
    RecordOutput<leon::MotionDesc> motion;
    leon::MotionLayout motion_lay{};
    RecordOutput<leon::ActivityDesc> activity;
    leon::ActivityLayout activity_lay{};
    leon::ActivityGeom activity_geom{};
    RecordOutput<leon::ResidualDesc> residual;
    leon::ResidualLayout residual_lay{};
    leon::ResidualGeom residual_geom{};
    // ... resampled to a model's input size (leon_pipeline_tensor_resize; geom.resized = 0: the full-size tensor, k_tensor): the
    // tables of both axes as k_resample reads them -- first_x, count_x, Wx, first_y, count_y, Wy in one int32 buffer
    leon_pipeline_tensor_geometry tensor_geom{};
    std::vector<int32_t> resize_tabs;
    leon::ResampleGeom resample_geom{};
    int32_t resize_filter = LEON_RESIZE_TRIANGLE;      // LEON_RESIZE_*: which k_resample
    DevBuf<int32_t> d_resize_tabs;
    // ... placed in a padded canvas (leon_pipeline_tensor_canvas; canvas_on = 0: the tensor is the image): what get_tensor_canvas
    // reports and k_letterbox's constants.  tensor_geom.width / height are the canvas's then, resample_geom.ow / oh the image's.
    leon_pipeline_tensor_canvas tensor_canvas{};
    leon::CanvasGeom canvas_geom{};
    int canvas_on = 0;
    // leon_pipeline_resample_regions: a stream of its own (non-blocking, made at first use) and the scratch of a call -- pinned staging
    // and its device twin for [descriptors | tables], read_regions' device tensors -- grown to the high-water mark, all under regions_mu
    std::mutex regions_mu;
    Stream regions_stream;
    PinnedBuf<> regions_host;
    DevBuf<> regions_dev;
    DevBuf<uint8_t> regions_out;
    // leon_pipeline_resample_regions_device (regions_mu too): the scratch of a chunk [frame ids | descriptors | table slots], the event
    // behind the last call's last launch -- the next call's stream waits for it on the device, growing the scratch and destroy on the
    // host -- and a small ring of pinned staging for the frame ids, each entry with the event behind its upload
    static constexpr int kBoxesStaging = 4;
    Event boxes_done;
    DevBuf<> boxes_dev;
    bool boxes_busy = false;
    Event boxes_ids_done[kBoxesStaging];
    PinnedBuf<uint32_t> boxes_ids_host[kBoxesStaging];
    bool boxes_ids_busy[kBoxesStaging] = {};
    unsigned boxes_ids_next = 0;
    bool gpu_parser = false;
    DevBuf<leon::VlcTables> d_vlc_tables;
    leon::VlcGeom vgeom{};
    PinnedBuf<> slab_host;            // gpu_parser: the arenas' memory, one allocation each (pinned host, device): both or neither
    DevBuf<> slab_dev;
    size_t vlc_index_lds = 0;         // dynamic LDS of k_vlc_index: the group counters of one picture + its scan
    std::vector<VlcRing> vlc_ring;

    // The jobs, the windows and everything the threads wait for.  It stands behind the streams and in front of the arenas: members
    // go in reverse order, so the arenas (all_arenas; the flow holds them as tickets and never looks inside) go first, then what is
    // left of the windows with their events (leon_pipeline_destroy has emptied the flow by then), the streams last.
    PipeFlow flow;

    std::vector<std::thread> parsers;
    std::thread submitter, notifier;
    std::vector<std::unique_ptr<Arena>> all_arenas;

    // stats
    Clock::time_point t0;
    std::atomic<uint64_t> st_pictures{0}, st_gops{0}, st_entries{0}, st_parse_ns{0}, st_upload{0}, st_submit_ns{0};
};

namespace {

void pipe_fail(leon_pipeline* p, int code, const std::string& msg) { p->flow.fail(code, msg); }

// host_need bytes of pinned memory and dev_need bytes of its device twin (equal for a GOP parsed on the host: the
// arena is copied as it is; the GPU parser uploads the stream bytes only and keeps everything else on the device)
bool arena_reserve(Arena* a, size_t host_need, size_t dev_need)
{
    // (the device twin is only ever grown while the arena is being filled: nothing in flight reads it)
    return a->host.reserve(host_need, cap_for(host_need, Grow::Half, (size_t)4 << 20), a->used) &&
           a->dev.reserve(dev_need, cap_for(dev_need, Grow::Half, (size_t)8 << 20), 0, kBigArenas);
}

// The pipeline takes the picture size from the stream's FIRST sequence header (leon_create).  Every key-map entry starts
// with a sequence header of its own and the reference re-initialises at each (decoders/jsv.js:491-561): a shard whose
// header names another SIZE cannot be decoded into this pipeline's rings and is refused; other quantiser MATRICES
// (jsv.js:540-558) are carried with the shard's pictures and dequantised with (leon_add_quant_matrices, round 4 --
// round 3 refused such a stream).  Returns the index of the matrices in force in job->qms, -1 = the stream's first,
// -2 = refused (job->status / err set).
int sequence_in_force(leon_pipeline* p, GopJob* job, leon_vlc_stream* st, uint64_t g)
{
    leon_vlc_info v{};
    leon_vlc_get_info(st, &v);
    if (v.coded_width != p->vinfo.coded_width || v.coded_height != p->vinfo.coded_height ||
        v.frame_width != p->vinfo.frame_width || v.frame_height != p->vinfo.frame_height) {
        job->status = LEON_ERR_INVALID;
        job->err = std::string("GOP shard ") + std::to_string(g) + ": its sequence header changes the picture size (" +
                   std::to_string(v.frame_width) + "x" + std::to_string(v.frame_height) + " after " + std::to_string(p->vinfo.frame_width) + "x" +
                   std::to_string(p->vinfo.frame_height) + "): a pipeline decodes one size";
        return -2;
    }
    if (memcmp(v.intra_qm, p->vinfo.intra_qm, 64) == 0 && memcmp(v.non_intra_qm, p->vinfo.non_intra_qm, 64) == 0) return -1;
    std::array<uint8_t, 128> m;
    memcpy(m.data(), v.intra_qm, 64);
    memcpy(m.data() + 64, v.non_intra_qm, 64);
    for (size_t i = 0; i < job->qms.size(); i++)
        if (job->qms[i] == m) return (int)i;
    job->qms.push_back(m);
    return (int)job->qms.size() - 1;
}

// gpu_parser: the entry list a picture reserves for a slice of `bytes` stream bytes.  An entry is a coefficient symbol, and n
// of them in a block take 3 n + 1 bits at least: the shortest code is '11s' (three bits; '1s', two, in first position only),
// and the end-of-block code (or an intra block's DC size code) another two -- entries <= bits / 3.  (Round 3 reserved a
// dword per two bits.)  The kernels keep inside the bound whatever the stream says (k_vlc_blocks, and the reconstruction
// reads the list through a buffer resource of exactly this length).  The bound of a whole GOP shard covers the sum over its
// slices: each slice has a 4-byte start code of its own outside every slice's bytes, worth ten entries of the bound -- more
// than the two a slice adds.
inline size_t vlc_entry_bound(size_t bytes) { return (8 * bytes) / 3 + 2; }
constexpr size_t kVlcMinEntries = 64;       // the least a picture's entry list reserves

// gpu_parser: what a picture takes of its GOP's arena besides its entry list: the macroblock records (mb_recs), the block
// records of all its slices (blk_recs: leon_vlc_gpu.h VlcSliceOut, a record per block at most), the maps, the group offsets
struct VlcPicBytes { size_t mb_recs, blk_recs, total; };
VlcPicBytes vlc_pic_bytes(const leon_pipeline* p)
{
    VlcPicBytes b;
    b.mb_recs = pad256(p->maps.mbs * leon::kVlcMbRecBytes);
    b.blk_recs = pad256(p->maps.mbs * (size_t)leon::vlc_blocks_per_mb(p->vinfo.has_alpha == 1) * leon::kVlcRecWords * 4);
    b.total = b.mb_recs + b.blk_recs + p->maps.bytes() + p->maps.gpad;
    return b;
}

// gpu_parser: the host reads the picture layer only (leon_vlc_scan_picture) and lays the GOP's arena out for the
// device kernels of leon_vlc_gpu.h:
//   [stream bytes, zero padded]                                            uploaded
//   per picture: [macroblock records]                                      cleared on the device
//   per picture: [maps | grp_off | entries (capacity)], per slice: [block records]      written by the kernels
void scan_gop_for_gpu(leon_pipeline* p, GopJob* job, leon_vlc_stream* st, const uint8_t* bytes, size_t n, uint64_t g, int qm_now)
{
    struct Scan { leon_vlc_picture_scan s; std::vector<int32_t> code; std::vector<uint64_t> pos; int qm; };
    std::vector<Scan> scans;
    for (;;) {
        leon_vlc_picture_scan sc;
        const int rc = leon_vlc_scan_picture(st, &sc);
        if (rc == LEON_VLC_END) break;
        if (rc != LEON_VLC_PICTURE) {
            job->status = LEON_ERR_INVALID;
            job->err = std::string("GOP shard ") + std::to_string(g) + ": " + leon_vlc_last_error();
            return;
        }
        if (sc.new_sequence && (qm_now = sequence_in_force(p, job, st, g)) == -2) return;
        if (sc.open_gop & LEON_VLC_GOP_OPEN) job->open_gop = true;
        if (sc.open_gop & LEON_VLC_GOP_BROKEN_LINK) job->broken_link = true;
        Scan x;
        x.s = sc;
        x.qm = qm_now;
        x.code.assign(sc.slice_code, sc.slice_code + sc.n_slices);
        x.pos.assign(sc.slice_bit_pos, sc.slice_bit_pos + sc.n_slices);
        scans.push_back(std::move(x));
    }
    if (n >= ((size_t)1 << 28)) { job->status = LEON_ERR_INVALID; job->err = "GOP shard too large for the GPU parser"; return; }
    const MapLayout& M = p->maps;
    const VlcPicBytes pb = vlc_pic_bytes(p);
    const size_t max_entries = (size_t)p->vinfo.coded_width * p->vinfo.coded_height * (p->vinfo.has_alpha == 1 ? 5 : 3) / 2;
    const size_t stream_pad = pad256(n + 16);
    // sizes first: the arena may move when it grows
    size_t need = stream_pad;
    std::vector<size_t> ecap(scans.size());
    for (size_t k = 0; k < scans.size(); k++) {
        const Scan& x = scans[k];
        size_t pic_words = 0;
        for (size_t j = 0; j < x.code.size(); j++) {
            const uint64_t begin = x.pos[j] >> 3, end = j + 1 < x.code.size() ? (x.pos[j + 1] >> 3) - 4 : x.s.end_byte;
            pic_words += vlc_entry_bound(end > begin ? (size_t)(end - begin) : 0);
        }
        ecap[k] = std::min(std::max(pic_words, kVlcMinEntries), max_entries);
        need += pb.total + MapLayout::entries_pad(ecap[k]);
    }
    if (!arena_reserve(job->arena, stream_pad, need)) { job->status = LEON_ERR_NOMEM; job->err = "staging allocation failed"; return; }
    Arena* a = job->arena;
    memcpy(a->host, bytes, n);
    memset(a->host + n, 0, stream_pad - n);
    job->upload_bytes = stream_pad;
    size_t at = stream_pad;
    job->zero_begin = at;                                // the macroblock records of all its pictures, side by side
    job->zero_bytes = scans.size() * pb.mb_recs;
    char* dev = a->dev;
    auto take = [&](size_t bytes_) { const size_t o = at; at += bytes_; return o; };
    for (size_t k = 0; k < scans.size(); k++) {
        const Scan& x = scans[k];
        PipePic m{};
        m.type = x.s.type;
        m.tref = x.s.temporal_reference;
        m.ts_ms = x.s.ts_ms;
        m.qm = x.qm;
        leon::VlcPic v{};
        v.type = x.s.type;
        v.full_pel_fwd = x.s.full_pel_fwd; v.fwd_rsize = x.s.fwd_rsize;
        v.full_pel_bwd = x.s.full_pel_bwd; v.bwd_rsize = x.s.bwd_rsize;
        v.zbase = dev + take(pb.mb_recs);
        job->pics.push_back(m);
        job->vpics.push_back(v);
    }
    for (size_t k = 0; k < scans.size(); k++) {
        const Scan& x = scans[k];
        PipePic& m = job->pics[k];
        leon::VlcPic& v = job->vpics[k];
        const size_t maps = take(M.bytes());             // all six: the kernels write them at VlcGeom's offsets (M's)
        v.maps = dev + maps;
        m.qscale = maps + M.off(M.QSCALE);
        m.intra = maps + M.off(M.INTRA);
        m.repadd = x.s.type != LEON_PIC_I ? maps + M.off(M.REPADD) : kNone;
        m.mb_dir = x.s.type == LEON_PIC_B ? maps + M.off(M.MB_DIR) : kNone;
        m.mv_fwd = x.s.type != LEON_PIC_I ? maps + M.off(M.MV_FWD) : kNone;
        m.mv_bwd = x.s.type == LEON_PIC_B ? maps + M.off(M.MV_BWD) : kNone;
        m.grp_off = take(M.gpad);
        m.entries = take(MapLayout::entries_pad(ecap[k]));
        m.n_entries = (uint32_t)ecap[k];                 // the bound of the device lists (the kernels keep inside it)
        v.grp_off = (uint32_t*)(dev + m.grp_off);
        v.entries = (uint32_t*)(dev + m.entries);
        v.entries_cap = (uint32_t)ecap[k];
        v.recs = (uint32_t*)(dev + take(pb.blk_recs));
        for (size_t j = 0; j < x.code.size(); j++) {
            leon::VlcSlice sl{};
            sl.bytes = (const uint32_t*)dev;
            sl.n_dwords = (uint32_t)(stream_pad / 4);
            sl.n_bytes = (uint32_t)n;
            sl.bit_pos = (uint32_t)x.pos[j];
            sl.end_byte = (uint32_t)(j + 1 < x.code.size() ? (x.pos[j + 1] >> 3) - 4 : x.s.end_byte);
            sl.code = x.code[j];
            sl.pic = (uint32_t)k;
            job->slices.push_back(sl);
        }
    }
    a->used = at;
    if (!job->pics.empty()) job->gop_ts_ms = job->pics[0].ts_ms;
}

// one GOP shard: parse every picture of it straight into a pinned arena
void parse_gop(leon_pipeline* p, GopJob* job)
{
    // job->gop counts the GOPs this pipeline decodes; which key-map entry that is:
    const std::vector<uint32_t>& mine = job->run->mine;
    const uint64_t g = mine[job->gop % mine.size()];
    job->key_gop = (job->gop / mine.size()) * p->shard_begin.size() + g;      // id in the whole (looped) stream
    const uint8_t* b = p->stream + p->shard_begin[g];
    const size_t n = (size_t)(p->shard_end[g] - p->shard_begin[g]);
    leon_vlc_stream* st = nullptr;
    // a stream without key map is one shard that still carries its container header
    // gpu_parser: only the picture layer is read here -- in place, when the stream goes on behind the shard
    const int rc_open = p->gpu_parser ? leon_vlc_open_scan(b, n, p->bytes - (size_t)p->shard_begin[g], p->vinfo.has_alpha, &st)
                                      : leon_vlc_open_shard(b, n, 1, p->vinfo.has_alpha, &st);
    if (rc_open != LEON_VLC_OK) {
        job->status = LEON_ERR_INVALID;
        job->err = std::string("GOP shard ") + std::to_string(g) + ": " + leon_vlc_last_error();
        return;
    }
    int qm_now = sequence_in_force(p, job, st, g);        // the shard's own sequence header (read by leon_vlc_open*)
    if (qm_now == -2) {
        leon_vlc_close(st);
        return;
    }
    Arena* a = job->arena;
    a->used = 0;
    if (p->gpu_parser) {
        scan_gop_for_gpu(p, job, st, b, n, g, qm_now);
        leon_vlc_close(st);
        return;
    }
    leon_vlc_picture pic;
    for (;;) {
        const int rc = leon_vlc_next_picture_sync(st, &pic);      // parsed here, on this thread: no second thread per shard
        if (rc == LEON_VLC_END) break;
        if (rc != LEON_VLC_PICTURE) {
            job->status = LEON_ERR_INVALID;
            job->err = std::string("GOP shard ") + std::to_string(g) + ": " + leon_vlc_last_error();
            break;
        }
        if (pic.new_sequence && (qm_now = sequence_in_force(p, job, st, g)) == -2) break;
        if (pic.open_gop & LEON_VLC_GOP_OPEN) job->open_gop = true;
        if (pic.open_gop & LEON_VLC_GOP_BROKEN_LINK) job->broken_link = true;
        const MapLayout& M = p->maps;
        const size_t epad = MapLayout::entries_pad(pic.n_entries), mbs = M.mbs;
        const size_t need = a->used + M.gpad + epad + M.bytes();      // (absent maps are left out: no more than this)
        if (!arena_reserve(a, need, need)) {
            job->status = LEON_ERR_NOMEM;
            job->err = "pinned staging allocation failed";
            break;
        }
        PipePic m{};
        m.type = pic.type;
        m.tref = pic.temporal_reference;
        m.n_entries = pic.n_entries;
        m.ts_ms = pic.ts_ms;
        m.qm = qm_now;
        auto put = [&](const void* src, size_t nbytes, size_t reserve) -> size_t {
            if (!src) return kNone;
            const size_t at = a->used;
            memcpy(a->host + at, src, nbytes);
            a->used += reserve;
            return at;
        };
        m.grp_off = put(pic.grp_off, ((size_t)pic.n_groups + 1) * 4, M.gpad);
        m.entries = put(pic.entries ? (const void*)pic.entries : (const void*)pic.grp_off, (size_t)pic.n_entries * 4, epad);
        m.qscale = put(pic.qscale, mbs, M.mpad);
        m.intra = put(pic.intra, mbs, M.mpad);
        m.repadd = put(pic.type != LEON_PIC_I ? pic.repadd : nullptr, mbs, M.mpad);
        m.mb_dir = put(pic.type == LEON_PIC_B ? pic.mb_dir : nullptr, mbs, M.mpad);
        m.mv_fwd = put(pic.type != LEON_PIC_I ? pic.mv_fwd : nullptr, mbs * 4, M.vpad);
        m.mv_bwd = put(pic.type == LEON_PIC_B ? pic.mv_bwd : nullptr, mbs * 4, M.vpad);
        if (job->pics.empty()) job->gop_ts_ms = pic.ts_ms;
        job->pics.push_back(m);
        p->st_entries += pic.n_entries;
    }
    leon_vlc_close(st);
}

// a frame's presentation time: its GOP's time code + its display index at the picture rate (25 when the stream names none)
double frame_ts_ms(const leon_pipeline* p, const GopJob* job, int display_index)
{
    const double rate = p->vinfo.picture_rate > 0 ? p->vinfo.picture_rate : 25.0;
    return job->gop_ts_ms + 1000.0 * (double)display_index / rate;
}

// a frame's RGBA and planes record in the output rings (null: that output is off): ring entry, lane (GOP of the window),
// display index
struct FrameAddr { uint8_t* rgba; uint8_t* planes; uint8_t* tensor; size_t index; };
FrameAddr frame_addr(const leon_pipeline* p, int ring, size_t lane, size_t k)
{
    const size_t i = ((size_t)ring * p->W + lane) * p->max_pics + k;
    return {p->d_rgba ? p->d_rgba + i * p->frame_bytes : nullptr, p->d_planes ? p->d_planes + i * p->planes_bytes : nullptr,
            p->d_tensor ? p->d_tensor + i * p->tensor_pitch : nullptr, i};
}

// ---- output TENSOR: the element table (the definition of include/leon_pipeline.h) ------------------------

// binary32 -> binary16 / bfloat16 bits, round to nearest even (finite input)
uint16_t f32_to_f16_bits(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);          // 65536 and beyond (65520 .. 65536 round up below)
    if (x < 0x38800000u) {                                             // below 2^-14: a subnormal half -- the adder rounds at 2^-24
        float a;
        memcpy(&a, &x, 4);
        a += 0.5f;
        uint32_t y;
        memcpy(&y, &a, 4);
        return (uint16_t)(sign | (y - 0x3f000000u));
    }
    const uint32_t r = x - 0x38000000u;                                // exponent rebased from 127 to 15
    return (uint16_t)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
}
uint16_t f32_to_bf16_bits(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
}

// What create and leon_pipeline_tensor_table make of the settings: the element type, scale and bias with the defaults resolved,
// and T itself (3 x 256 elements) into `out` (may be null).  Every refusal of the header is here.
int tensor_table_build(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tc, int* dtype_out, void* out)
{
    const bool bit = (cfg->output & LEON_PIPELINE_OUTPUT_TENSOR) != 0;
    if (!bit) return fail(LEON_ERR_INVALID, "tensor settings (dtype %d) without LEON_PIPELINE_OUTPUT_TENSOR in output %d", tc ? tc->dtype : 0, cfg->output);
    const int dtype = tc && tc->dtype ? tc->dtype : LEON_TENSOR_F16;
    if (dtype != LEON_TENSOR_F16 && dtype != LEON_TENSOR_BF16 && dtype != LEON_TENSOR_F32 && dtype != LEON_TENSOR_U8) return fail(LEON_ERR_INVALID, "tensor dtype %d", dtype);
    if (dtype == LEON_TENSOR_U8) {          // the element is the colour value itself: nothing to scale
        for (int c = 0; c < 3 && tc; c++)
            if (tc->scale[c] != 0.0f || tc->bias[c] != 0.0f) return fail(LEON_ERR_INVALID, "tensor dtype %d (LEON_TENSOR_U8) takes no scale / bias (channel %d: they must be 0)", dtype, c);
        for (int i = 0; i < 3 * 256 && out; i++) ((uint8_t*)out)[i] = (uint8_t)(i & 255);
        if (dtype_out) *dtype_out = dtype;
        return LEON_OK;
    }
    float scale[3] = {0, 0, 0}, bias[3] = {0, 0, 0};
    bool all_zero = true;
    for (int c = 0; c < 3 && tc; c++) {
        scale[c] = tc->scale[c];
        bias[c] = tc->bias[c];
        if (!std::isfinite(scale[c]) || !std::isfinite(bias[c])) return fail(LEON_ERR_INVALID, "tensor scale / bias of channel %d is not finite", c);
        all_zero = all_zero && scale[c] == 0.0f && bias[c] == 0.0f;
    }
    if (all_zero)
        for (int c = 0; c < 3; c++) scale[c] = (float)(1.0 / 255.0);
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < 256; v++) {
            const float f = (float)((double)v * (double)scale[c] + (double)bias[c]);
            const int i = c * 256 + v;
            bool finite = std::isfinite(f);
            if (dtype == LEON_TENSOR_F32) {
                if (out) memcpy((char*)out + 4 * i, &f, 4);
            } else if (finite) {
                const uint16_t h = dtype == LEON_TENSOR_F16 ? f32_to_f16_bits(f) : f32_to_bf16_bits(f);
                finite = dtype == LEON_TENSOR_F16 ? (h & 0x7c00u) != 0x7c00u : (h & 0x7f80u) != 0x7f80u;
                if (out) memcpy((char*)out + 2 * i, &h, 2);
            }
            if (!finite) return fail(LEON_ERR_INVALID, "tensor table: value %d of channel %d is not finite in the element type (dtype %d)", v, c, dtype);
        }
    if (dtype_out) *dtype_out = dtype;
    return LEON_OK;
}

// ---- output TENSOR at a model's input size: the tables of one axis (the definition of include/leon_pipeline.h) --------

// first[o], count[o], weights[o * max_taps + k] (zero behind count[o]); *taps = the largest count.  Every refusal of one axis is here.
// Doubles, evaluated as written (the library is compiled with -ffp-contract=off; the pragma holds it for other builds).  What one
// output sample's row is -- the window, the filter functions, the sum in index order, the normalisation and the rounding -- is
// leon_resize_row.h, the text the device evaluates too (k_box_tables).

// the most taps an output sample of `filter` has at the largest ratio (0: no such filter)
int32_t resize_filter_max_taps(int32_t filter)
{
    return filter == LEON_RESIZE_TRIANGLE ? LEON_RESIZE_MAX_TAPS : filter == LEON_RESIZE_BICUBIC ? LEON_RESIZE_MAX_TAPS_BICUBIC : 0;
}
int resize_axis_build(const char* axis, int32_t in_size, int32_t crop_start, int32_t crop_size, int32_t out_size, int32_t filter,
                      int32_t* first, int32_t* count, int32_t* weights, int32_t max_taps, int32_t* taps)
{
#pragma clang fp contract(off)
    const int32_t filter_taps = resize_filter_max_taps(filter);
    if (!filter_taps) return fail(LEON_ERR_INVALID, "resize filter %d (LEON_RESIZE_TRIANGLE and LEON_RESIZE_BICUBIC are the filters)", filter);
    const bool cubic = filter == LEON_RESIZE_BICUBIC;
    if (out_size < 1 || out_size > 4096) return fail(LEON_ERR_INVALID, "resize: output %s %d is outside 1 .. 4096", axis, out_size);
    if (in_size < 1 || crop_size < 1 || crop_start < 0 || crop_start > in_size || crop_size > in_size - crop_start)
        return fail(LEON_ERR_INVALID, "resize: the crop box (%s: start %d, size %d) is empty or leaves the frame (%d)", axis, crop_start, crop_size, in_size);
    if ((int64_t)crop_size > 16 * (int64_t)out_size) return fail(LEON_ERR_INVALID, "resize: %s %d -> %d reduces by more than 16", axis, crop_size, out_size);
    if (max_taps < 1) return fail(LEON_ERR_INVALID, "resize: max_taps %d", max_taps);
    const leon::ResizeAxis A = leon::resize_axis(in_size, crop_start, crop_size, out_size, cubic);
    int32_t most = 0;
    double w[LEON_RESIZE_MAX_TAPS_BICUBIC + 2];
    for (int32_t o = 0; o < out_size; o++) {
        const leon::ResizeWindow R = leon::resize_row_window(A, o);
        const int32_t lo = R.lo, n = R.n;
        if (n < 1 || n > filter_taps) return fail(LEON_ERR_INVALID, "resize: %s output %d has %d taps", axis, o, n);
        if (n > max_taps) return fail(LEON_ERR_INVALID, "resize: %s output %d has %d taps, max_taps is %d", axis, o, n, max_taps);
        double sum = 0.0;
        for (int32_t k = 0; k < n; k++) {
            w[k] = leon::resize_row_tap(A, R, k);
            sum += w[k];
        }
        if (!(sum > 0.0)) return fail(LEON_ERR_INVALID, "resize: %s output %d has no weight", axis, o);
        // what the kernels' 24-bit multiplies and 32-bit sums rest on: every |W| < 2^23, and neither the positive nor the negative
        // part of a row can carry a sum of 8-bit samples out of 31 bits (with these filters it never happens)
        int64_t pos = 0, neg = 0;
        for (int32_t k = 0; k < n; k++) {
            const int32_t W = leon::resize_row_weight(w[k], sum);
            if (W <= -(1 << 23) || W >= (1 << 23)) return fail(LEON_ERR_INVALID, "resize: %s output %d has a weight of %d", axis, o, W);
            if (W < 0) neg -= W; else pos += W;
            if (weights) weights[(size_t)o * max_taps + k] = W;
        }
        if ((1 << 21) + 255 * pos >= ((int64_t)1 << 31) || 255 * neg >= ((int64_t)1 << 31)) return fail(LEON_ERR_INVALID, "resize: the weights of %s output %d overflow 32 bits", axis, o);
        if (first) first[o] = lo;
        if (count) count[o] = n;
        if (weights)
            for (int32_t k = n; k < max_taps; k++) weights[(size_t)o * max_taps + k] = 0;
        if (n > most) most = n;
    }
    if (taps) *taps = most;
    return LEON_OK;
}

// The largest count of resize_axis_build for arguments it accepts, without the weights: the same window expressions, no filter
// evaluated.  0: arguments it refuses (the caller asks resize_axis_build itself for the message).  A caller that sizes table rows by it
// and builds them with max_taps = this value is told by resize_axis_build should the two ever disagree ("max_taps is").
int32_t resize_axis_taps(int32_t in_size, int32_t crop_start, int32_t crop_size, int32_t out_size, int32_t filter)
{
#pragma clang fp contract(off)
    const int32_t filter_taps = resize_filter_max_taps(filter);
    if (!filter_taps || out_size < 1 || out_size > 4096 || in_size < 1 || crop_size < 1 || crop_start < 0 || crop_start > in_size || crop_size > in_size - crop_start ||
        (int64_t)crop_size > 16 * (int64_t)out_size) return 0;
    const leon::ResizeAxis A = leon::resize_axis(in_size, crop_start, crop_size, out_size, filter == LEON_RESIZE_BICUBIC);
    int32_t most = 0;
    for (int32_t o = 0; o < out_size; o++) {
        const int32_t n = leon::resize_row_window(A, o).n;
        if (n < 1 || n > filter_taps) return 0;
        if (n > most) most = n;
    }
    return most;
}

// Every refusal of the format settings is here
int tensor_format_check(const leon_pipeline_config* cfg, const leon_pipeline_tensor_format* fm, int* layout_out)
{
    int32_t any = 0;
    if (fm) {
        any = fm->layout;
        for (int i = 0; i < 7; i++) any |= fm->reserved[i];
    }
    if (layout_out) *layout_out = LEON_TENSOR_LAYOUT_CHW;
    if (!any) return LEON_OK;
    if (!(cfg->output & LEON_PIPELINE_OUTPUT_TENSOR)) return fail(LEON_ERR_INVALID, "tensor format settings (layout %d) without LEON_PIPELINE_OUTPUT_TENSOR in output %d", fm->layout, cfg->output);
    for (int i = 0; i < 7; i++)
        if (fm->reserved[i]) return fail(LEON_ERR_INVALID, "tensor format: reserved word %d is %d, not 0", i, fm->reserved[i]);
    if (fm->layout != LEON_TENSOR_LAYOUT_CHW && fm->layout != LEON_TENSOR_LAYOUT_HWC) return fail(LEON_ERR_INVALID, "tensor format: layout %d", fm->layout);
    if (layout_out) *layout_out = fm->layout;
    return LEON_OK;
}

bool canvas_asked(const leon_pipeline_tensor_canvas* cv)
{
    if (!cv) return false;
    int32_t any = cv->width | cv->height | cv->x | cv->y | cv->pad[0] | cv->pad[1] | cv->pad[2] | cv->image_width | cv->image_height;
    for (int i = 0; i < 7; i++) any |= cv->reserved[i];
    return any != 0;
}

// Every refusal of the canvas settings is here (the resize settings' own are resize_axis_build's)
int tensor_canvas_check(const leon_pipeline_config* cfg, const leon_pipeline_tensor_resize* rz, const leon_pipeline_tensor_canvas* cv)
{
    if (!canvas_asked(cv)) return LEON_OK;
    if (!(cfg->output & LEON_PIPELINE_OUTPUT_TENSOR)) return fail(LEON_ERR_INVALID, "tensor canvas settings (width %d, height %d) without LEON_PIPELINE_OUTPUT_TENSOR in output %d", cv->width, cv->height, cfg->output);
    for (int i = 0; i < 7; i++)
        if (cv->reserved[i]) return fail(LEON_ERR_INVALID, "tensor canvas: reserved word %d is %d, not 0", i, cv->reserved[i]);
    if (!rz || rz->out_width < 1 || rz->out_height < 1) return fail(LEON_ERR_INVALID, "tensor canvas: no resize settings (out_width %d, out_height %d): the canvas places the resampled image", rz ? rz->out_width : 0, rz ? rz->out_height : 0);
    if (cv->width < 1 || cv->width > 4096) return fail(LEON_ERR_INVALID, "tensor canvas: width %d is outside 1 .. 4096", cv->width);
    if (cv->height < 1 || cv->height > 4096) return fail(LEON_ERR_INVALID, "tensor canvas: height %d is outside 1 .. 4096", cv->height);
    if (cv->x < 0) return fail(LEON_ERR_INVALID, "tensor canvas: x %d is negative", cv->x);
    if (cv->y < 0) return fail(LEON_ERR_INVALID, "tensor canvas: y %d is negative", cv->y);
    if ((int64_t)cv->x + rz->out_width > cv->width) return fail(LEON_ERR_INVALID, "tensor canvas: x %d + out_width %d leaves the width %d", cv->x, rz->out_width, cv->width);
    if ((int64_t)cv->y + rz->out_height > cv->height) return fail(LEON_ERR_INVALID, "tensor canvas: y %d + out_height %d leaves the height %d", cv->y, rz->out_height, cv->height);
    for (int c = 0; c < 3; c++)
        if (cv->pad[c] < 0 || cv->pad[c] > 255) return fail(LEON_ERR_INVALID, "tensor canvas: pad[%d] %d is outside 0 .. 255", c, cv->pad[c]);
    if (cv->image_width && cv->image_width != rz->out_width) return fail(LEON_ERR_INVALID, "tensor canvas: image_width %d is not out_width %d", cv->image_width, rz->out_width);
    if (cv->image_height && cv->image_height != rz->out_height) return fail(LEON_ERR_INVALID, "tensor canvas: image_height %d is not out_height %d", cv->image_height, rz->out_height);
    return LEON_OK;
}

// What create makes of the canvas settings, behind plan_resize: the tensor takes the canvas's size, the image keeps resample_geom's
void plan_canvas(leon_pipeline* p, const leon_pipeline_tensor_canvas* cv)
{
    leon_pipeline_tensor_geometry& g = p->tensor_geom;
    leon_pipeline_tensor_canvas& c = p->tensor_canvas;
    c = leon_pipeline_tensor_canvas{};
    c.width = g.width; c.height = g.height; c.image_width = g.width; c.image_height = g.height;
    if (!canvas_asked(cv)) return;
    c.width = cv->width; c.height = cv->height; c.x = cv->x; c.y = cv->y;
    for (int i = 0; i < 3; i++) c.pad[i] = cv->pad[i];
    g.width = c.width; g.height = c.height;
    p->canvas_on = 1;
    p->canvas_geom = leon::CanvasGeom{c.width, c.height, c.x, c.y, (uint32_t)c.pad[0] | ((uint32_t)c.pad[1] << 8) | ((uint32_t)c.pad[2] << 16)};
}

bool resize_asked(const leon_pipeline_tensor_resize* rz)
{
    return rz && (rz->crop_x | rz->crop_y | rz->crop_width | rz->crop_height | rz->out_width | rz->out_height | rz->filter) != 0;
}

// What the kernel's LDS is sized for (by filter: ResTriangle, ResCubic), of the tables `t` laid out by G.  Within the limits of
// resize_axis_build neither check can fail (at most 544 columns and 147 rows, bicubic 576 and 179: leon_kernels.h has the arithmetic);
// they stand guard for the kernel's chunk loop, which needs at least one row pair per chunk (rc >= 2) to advance, should a limit ever
// be widened without the kernel.
int resize_footprint_check(const int32_t* t, const leon::ResampleGeom& G, int32_t filter)
{
    for (int32_t o = 0; o < G.ow; o += leon::kResTileX) {
        const int32_t l = std::min(o + leon::kResTileX, G.ow) - 1;
        const int32_t sw = (t[l] + t[G.off_cx + l] - (t[o] & ~7) + 7) & ~7;
        if (leon::resample_col(sw) * 2 > leon::kResStagePx) return fail(LEON_ERR_INVALID, "resize: a tile's source footprint of %d columns does not fit the staging buffer", sw);
    }
    for (int32_t o = 0; o < G.oh; o += leon::kResTileY) {
        const int32_t l = std::min(o + leon::kResTileY, G.oh) - 1;
        const int32_t rows = t[G.off_fy + l] + t[G.off_cy + l] - (t[G.off_fy + o] & ~1);
        if (rows + 1 > (filter == LEON_RESIZE_BICUBIC ? leon::ResCubic::kHRows : leon::ResTriangle::kHRows)) return fail(LEON_ERR_INVALID, "resize: a tile's source footprint of %d rows does not fit", rows);
    }
    return LEON_OK;
}

// The tables of an image ow x oh in one buffer: first_x | count_x | Wx | first_y | count_y | Wy, rows of taps_x and taps_y words (zero
// behind count[o]).  Fills G's row lengths and off_* and returns the int32 words of the whole; box_tables_body is the device's statement.
size_t resize_tables_layout(int32_t ow, int32_t oh, int32_t taps_x, int32_t taps_y, leon::ResampleGeom* G)
{
    G->taps_x = taps_x; G->taps_y = taps_y;
    G->off_cx = (uint32_t)ow;
    G->off_wx = G->off_cx + (uint32_t)ow;
    G->off_fy = G->off_wx + (uint32_t)ow * (uint32_t)taps_x;
    G->off_cy = G->off_fy + (uint32_t)oh;
    G->off_wy = G->off_cy + (uint32_t)oh;
    return (size_t)G->off_wy + (size_t)oh * (size_t)taps_y;
}

// What create makes of the resize settings: the geometry in force, the table buffer and k_resample's constants
int plan_resize(leon_pipeline* p, const leon_pipeline_tensor_resize* rz)
{
    const int32_t fw = p->vinfo.frame_width, fh = p->vinfo.frame_height;
    leon_pipeline_tensor_geometry& g = p->tensor_geom;
    g = leon_pipeline_tensor_geometry{fw, fh, 0, 0, fw, fh, 1, 1, 0};
    if (!resize_asked(rz)) return LEON_OK;
    g.resized = 1;
    p->resize_filter = rz->filter;
    g.width = rz->out_width;
    g.height = rz->out_height;
    if (rz->crop_x | rz->crop_y | rz->crop_width | rz->crop_height) {
        g.crop_x = rz->crop_x; g.crop_y = rz->crop_y; g.crop_width = rz->crop_width; g.crop_height = rz->crop_height;
    }
    int rc;
    // once for the refusals and the tap counts, then into the buffer with rows of exactly that length
    if ((rc = resize_axis_build("width", fw, g.crop_x, g.crop_width, g.width, rz->filter, nullptr, nullptr, nullptr, LEON_RESIZE_MAX_TAPS_BICUBIC, &g.taps_x)) != LEON_OK) return rc;
    if ((rc = resize_axis_build("height", fh, g.crop_y, g.crop_height, g.height, rz->filter, nullptr, nullptr, nullptr, LEON_RESIZE_MAX_TAPS_BICUBIC, &g.taps_y)) != LEON_OK) return rc;
    leon::ResampleGeom& G = p->resample_geom;
    G = leon::ResampleGeom{};
    G.fw = fw; G.fh = fh; G.ow = g.width; G.oh = g.height;
    // rows of Wx are an odd number of entries long (zero behind count[o]): the horizontal pass's lanes are output columns and read
    // Wx[o][k] for one k together -- 32 entries a row (ratio 16) would put them all on one LDS bank, 18 (1080p -> 224) on every other
    // (bicubic: up to 65, odd as well)
    p->resize_tabs.assign(resize_tables_layout(g.width, g.height, g.taps_x | 1, g.taps_y, &G), 0);
    int32_t* t = p->resize_tabs.data();
    if ((rc = resize_axis_build("width", fw, g.crop_x, g.crop_width, g.width, rz->filter, t, t + G.off_cx, t + G.off_wx, G.taps_x, nullptr)) != LEON_OK) return rc;
    if ((rc = resize_axis_build("height", fh, g.crop_y, g.crop_height, g.height, rz->filter, t + G.off_fy, t + G.off_cy, t + G.off_wy, g.taps_y, nullptr)) != LEON_OK) return rc;
    return resize_footprint_check(t, G, rz->filter);
}

// the GOP without the pictures whose `keep` is 0: they leave pics, and vpics / slices (gpu_parser) with them
void keep_pictures(GopJob* job, const std::vector<uint8_t>& keep)
{
    std::vector<PipePic> pics;
    std::vector<leon::VlcPic> vpics;
    std::vector<int> renum(job->pics.size(), -1);
    for (size_t k = 0; k < job->pics.size(); k++) {
        if (!keep[k]) continue;
        renum[k] = (int)pics.size();
        pics.push_back(job->pics[k]);
        if (k < job->vpics.size()) vpics.push_back(job->vpics[k]);
    }
    std::vector<leon::VlcSlice> slices;       // (in picture order, as launch_gpu_parser walks them)
    for (leon::VlcSlice sl : job->slices)
        if (renum[sl.pic] >= 0) {
            sl.pic = (uint32_t)renum[sl.pic];
            slices.push_back(sl);
        }
    job->pics.swap(pics);
    job->vpics.swap(vpics);
    job->slices.swap(slices);
}

// LEON_PIPELINE_SEEK_EXACT: the first GOP of the run delivers its frames from the one on screen at t_ms on (the largest
// ts_ms <= t_ms; none: the GOP's first frame, i.e. all of them).  B pictures before it are dropped -- neither parsed on the
// GPU nor launched --, I and P pictures before it are still reconstructed (later pictures predict from them) but not
// converted to RGBA and not delivered.  (After drop_leading_b: a target on a dropped frame finds no picture at or before it and
// the GOP delivers from its I picture.)
void trim_to_target(leon_pipeline* p, GopJob* job, double t_ms)
{
    int target = -1;
    for (const PipePic& m : job->pics)
        if (frame_ts_ms(p, job, m.tref) <= t_ms) target = std::max(target, m.tref);
    if (target < 0) return;
    std::vector<uint8_t> keep(job->pics.size(), 1);
    for (size_t k = 0; k < job->pics.size(); k++) {
        PipePic& m = job->pics[k];
        if (m.tref >= target) continue;
        if (m.type == LEON_PIC_B) keep[k] = 0;
        else m.shown = false;
    }
    keep_pictures(job, keep);
}

// A GOP that is open (closed_gop = 0) and does not have its predecessor (GopJob::has_pred): its leading B pictures -- those in
// front of its second anchor in coded order -- would predict from pictures that are not there, or, behind a broken_link, from the
// wrong ones.  They are dropped as trim_to_target drops pictures: neither parsed on the GPU nor launched nor delivered.  The GOP's
// frames then start at its I picture's display index (ISO 11172-2 2.4.3.4: broken_link; what a player does after random access).
void drop_leading_b(GopJob* job)
{
    std::vector<uint8_t> keep(job->pics.size(), 1);
    int n_anchor = 0;
    bool any = false;
    for (size_t k = 0; k < job->pics.size(); k++) {
        if (job->pics[k].type != LEON_PIC_B) n_anchor++;
        else if (n_anchor == 1) { keep[k] = 0; any = true; }
    }
    if (any) keep_pictures(job, keep);
}

void parser_main(leon_pipeline* p)
{
    hipSetDevice(p->cfg.device_id);
    for (;;) {
        std::unique_ptr<GopJob> owned = p->flow.take_gop();
        if (!owned) return;
        const std::shared_ptr<const PipeRun> run = owned->run;
        const uint64_t g = owned->gop;
        const uint32_t key = run->mine[g % run->mine.size()];
        // a stream that is still arriving (leon_pipeline_create_partial): the GOP's bytes must be there -- the decoder of the
        // reference stalls the same way when its buffer runs dry (features/bitreader.js:135-189)
        const PipeFlow::Bytes bytes = p->flow.await_bytes(owned, p->shard_end[key]);
        if (bytes == PipeFlow::Bytes::Stop) return;
        if (bytes == PipeFlow::Bytes::Replaced) continue;
        GopJob* const job = owned.get();
        {
            const uint8_t* b = p->stream + p->shard_begin[key];
            if (b[0] != 0 || b[1] != 0 || b[2] != 1) {
                job->status = LEON_ERR_INVALID;
                job->err = "key map entry " + std::to_string(key) + " does not point at a start code";
            }
        }
        const auto t = Clock::now();
        if (job->status == LEON_OK) parse_gop(p, job);
        if (job->status == LEON_OK && (int)job->pics.size() > p->max_pics) {        // (either parser)
            job->status = LEON_ERR_INVALID;
            job->err = "a GOP has " + std::to_string(job->pics.size()) + " pictures; raise max_gop_pictures (" + std::to_string(p->max_pics) + ")";
        }
        if (job->status == LEON_OK && job->open_gop && p->cfg.shard_count <= 1) {
            // (a shard never holds a GOP's neighbour: there plan_levels refuses the GOP)
            job->has_pred = g % run->mine.size() != 0 && !job->broken_link;
            if (!job->has_pred) drop_leading_b(job);
        }
        if (job->status == LEON_OK && g == 0 && run->exact_ms >= 0) trim_to_target(p, job, run->exact_ms);
        p->st_parse_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t).count();
        p->flow.hand_parsed(std::move(owned));
    }
}


// which of the two parser streams a window's parser kernels run on: they alternate
inline size_t vlc_stream_of(int64_t window) { return (size_t)(window & 1); }

// gpu_parser: the slices of the whole window in one launch each of k_vlc_parse / k_vlc_index / k_vlc_blocks
// (leon_vlc_gpu.h), on a parser stream, in front of the reconstruction launches that read their output
int launch_gpu_parser(leon_pipeline* p, PipeWindow* w)
{
    hipStream_t vs = p->vlc_stream[vlc_stream_of(w->id)];
    size_t n_slices = 0, n_pics = 0;
    for (const auto& job : w->jobs) { n_slices += job->slices.size(); n_pics += job->vpics.size(); }
    w->n_vpics = (uint32_t)n_pics;
    if (!n_slices || !n_pics) return LEON_OK;
    VlcRing& R = p->vlc_ring[(size_t)w->ring];
    const size_t desc_bytes = pad256(n_slices * sizeof(leon::VlcSlice)) + pad256(n_pics * sizeof(leon::VlcPic)) + pad256(w->jobs.size() * sizeof(leon::VlcClear));
    const size_t dev_bytes = desc_bytes + pad256(n_slices * sizeof(leon::VlcSliceOut)) + pad256(n_pics * 4);
    // (the ring entry is ours: its previous window has been released)
    if (!R.desc.reserve(dev_bytes, cap_for(dev_bytes, Grow::Half))) return fail(LEON_ERR_NOMEM, "descriptor ring of the GPU parser");
    if (!R.h_err.reserve(n_pics * 4, cap_for(n_pics, Grow::Half) * 4)) return fail(LEON_ERR_NOMEM, "error words of the GPU parser");
    leon::VlcSlice* hs = (leon::VlcSlice*)R.desc.host();
    leon::VlcPic* hp = (leon::VlcPic*)(R.desc.host() + pad256(n_slices * sizeof(leon::VlcSlice)));
    leon::VlcSliceOut* d_words = (leon::VlcSliceOut*)(R.desc.dev() + desc_bytes);      // what k_vlc_parse leaves per slice for the two kernels behind it
    uint32_t* d_err = (uint32_t*)(R.desc.dev() + desc_bytes + pad256(n_slices * sizeof(leon::VlcSliceOut)));
    leon::VlcClear* hc = (leon::VlcClear*)(R.desc.host() + pad256(n_slices * sizeof(leon::VlcSlice)) + pad256(n_pics * sizeof(leon::VlcPic)));
    size_t pi = 0, ci = 0;
    // Slice order of the launch: picture by picture, the I pictures first, then P, then B -- the 64 lanes of a wave
    // then hold slices of ONE picture type (in coded order most waves straddled two pictures of different types, and
    // a wave executes the union of its lanes' paths), and the longest waves (I: three times the symbols) start first.
    // The opposite -- the k-th slice of every picture side by side, so that every wave carries a few I slices -- was
    // measured too: 76 k against 97 k pictures/s.
    struct PicRun { const leon::VlcSlice* first; uint32_t n, pic; int type; };
    std::vector<PicRun> runs;
    runs.reserve(n_pics);
    for (const auto& job : w->jobs) {
        // what the kernels count in and report through starts at zero (regions are multiples of 256 bytes)
        hc[ci].ptr = (uint4*)(job->arena->dev + job->zero_begin);
        hc[ci].n16 = job->zero_bytes / 16;
        ci++;
        size_t at = 0;
        for (size_t k = 0; k < job->vpics.size(); k++) {
            uint32_t n = 0;
            while (at + n < job->slices.size() && job->slices[at + n].pic == k) n++;
            runs.push_back(PicRun{job->slices.data() + at, n, (uint32_t)(pi + k), job->vpics[k].type});
            at += n;
        }
        for (const leon::VlcPic& v : job->vpics) hp[pi++] = v;
    }
    // Inside a type: picture by picture -- a picture's slices stay together (k_vlc_index walks them).  (The k-th slice of
    // every picture side by side, so that the 64 lanes of a wave hold slices that are alike, was measured in round 3:
    // 30 % fewer instructions in all, and 25-30 % SLOWER end to end -- the launch has fewer waves than the chip has
    // room for, it lasts as long as its longest wave, and a wave of 64 long slices is longer than a wave with one.)
    size_t si = 0;
    for (int type = 1; type <= 3; type++)
        for (const PicRun& pr : runs)
            if (pr.type == type) {
                hp[pr.pic].first_slice = (uint32_t)si;
                hp[pr.pic].n_slices = pr.n;
                for (uint32_t k = 0; k < pr.n; k++) {
                    hs[si] = pr.first[k];
                    hs[si].pic = pr.pic;
                    si++;
                }
            }
    HIP_TRY(hipMemcpyAsync(R.desc.dev(), R.desc.host(), desc_bytes, hipMemcpyHostToDevice, vs));
    HIP_TRY(hipMemsetAsync(d_err, 0, n_pics * 4, vs));
    const leon::VlcClear* dc = (const leon::VlcClear*)(R.desc.dev() + pad256(n_slices * sizeof(leon::VlcSlice)) + pad256(n_pics * sizeof(leon::VlcPic)));
    hipLaunchKernelGGL(leon::k_vlc_clear, dim3(32, (unsigned)w->jobs.size()), dim3(256), 0, vs, dc);
    const leon::VlcSlice* ds = (const leon::VlcSlice*)R.desc.dev();
    const leon::VlcPic* dp = (const leon::VlcPic*)(R.desc.dev() + pad256(n_slices * sizeof(leon::VlcSlice)));
    const int blocks = (int)((n_slices + 255) / 256);
    hipLaunchKernelGGL(leon::k_vlc_parse, dim3(blocks), dim3(256), 4 * leon::kVlcRingDwords * 64 * 4, vs, ds, d_words, (int)n_slices, dp, d_err, p->vgeom, p->d_vlc_tables);
    hipLaunchKernelGGL(leon::k_vlc_index, dim3((unsigned)n_pics), dim3(leon::kVlcIndexThreads), p->vlc_index_lds, vs, ds, d_words, dp, d_err, p->vgeom);
    hipLaunchKernelGGL(leon::k_vlc_blocks, dim3((unsigned)((n_slices + 3) / 4)), dim3(256), 0, vs, ds, d_words, (int)n_slices, dp, d_err, p->vgeom, p->d_vlc_tables);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R.h_err, d_err, n_pics * 4, hipMemcpyDeviceToHost, vs));
    return LEON_OK;
}

// LEON_DEBUG_CAPTURE=<dir> (read when the pipeline is created; tests/test_pipeline_gpu.py sets it for its small streams):
// what the reconstruction launches of a window READ and WROTE is written to <dir>/w<window>/ -- after every level, with
// the decoder's stream idle, the planes of the slot each picture of the level wrote and of the slots it predicted from
// (L<level>_g<lane>_t<tref>_{out,fwd,bwd}.planes); after the last level every GOP's device arena as the kernels left it
// (arena_<lane>.bin: stream bytes, the GPU parser's records, maps, group offsets, entry lists) with an index of where each
// picture's arrays lie (index.txt).  A wrong frame then comes with the inputs that produced it: which buffer held wrong
// bytes separates a late write into reused pages from a read of memory nobody wrote.  Serialises the levels.
void capture_file(const std::string& path, const void* dev, size_t bytes)
{
    std::vector<char> h(bytes);
    if (bytes && hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
    if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(h.data(), 1, bytes, f); fclose(f); }
}

// a picture of a level: the lane of its GOP in the window, the slots it writes and predicts from
// (fwd_tref, bwd_tref: the display indices of the pictures in those slots, -1: none; fwd_before: the forward one is of the GOP before)
struct LevelPic { size_t lane; const PipePic* pic; int fwd, bwd, out; int fwd_tref = -1, bwd_tref = -1; bool fwd_before = false; };

// after a level, the decoder's stream idle: the planes its pictures wrote and predicted from, a line each in the index
// (the first level begins the index with the geometry)
int capture_level(const leon_pipeline* p, const PipeWindow* w, const std::string& dir, const std::vector<LevelPic>& lvl, size_t lvl_no)
{
    const leon_decoder* d = p->dec;
    HIP_TRY(hipStreamSynchronize(d->stream));
    FILE* idx = fopen((dir + "/index.txt").c_str(), lvl_no ? "a" : "w");
    if (idx && !lvl_no)
        fprintf(idx, "geom coded=%dx%d frame=%dx%d mbs=%d n_groups=%d gpu_parser=%d unfused=%d slot_bytes=%zu\n", p->vinfo.coded_width, p->vinfo.coded_height,
                p->vinfo.frame_width, p->vinfo.frame_height, p->vinfo.mb_width * p->vinfo.mb_height, p->vinfo.n_groups, (int)p->gpu_parser, (int)p->unfused, d->plane_bytes);
    for (const LevelPic& it : lvl) {
        const PipePic& m = *it.pic;
        const std::string stem = dir + "/L" + std::to_string(lvl_no) + "_g" + std::to_string(it.lane) + "_t" + std::to_string(m.tref);
        if (it.out >= 0) capture_file(stem + "_out.planes", d->d_slots + (size_t)it.out * d->slot_stride, d->plane_bytes);
        if (it.fwd >= 0) capture_file(stem + "_fwd.planes", d->d_slots + (size_t)it.fwd * d->slot_stride, d->plane_bytes);
        if (it.bwd >= 0) capture_file(stem + "_bwd.planes", d->d_slots + (size_t)it.bwd * d->slot_stride, d->plane_bytes);
        if (idx) fprintf(idx, "pic lane=%zu gop=%llu tref=%d type=%d level=%zu out=%d fwd=%d bwd=%d n_entries=%u qm=%d grp_off=%zd entries=%zd qscale=%zd intra=%zd repadd=%zd "
                              "mb_dir=%zd mv_fwd=%zd mv_bwd=%zd\n", it.lane, (unsigned long long)w->jobs[it.lane]->key_gop, m.tref, m.type, lvl_no, it.out, it.fwd, it.bwd,
                         m.n_entries, m.qm, (ssize_t)m.grp_off, (ssize_t)m.entries, (ssize_t)m.qscale, (ssize_t)m.intra, (ssize_t)m.repadd, (ssize_t)m.mb_dir, (ssize_t)m.mv_fwd, (ssize_t)m.mv_bwd);
    }
    if (idx) fclose(idx);
    return LEON_OK;
}

// The pictures of one window as levels of launches: per GOP the anchors rotate through three slots (on the unfused road a B
// picture has one of its own until it is converted); a picture's level is one more than the deepest picture it predicts from.
// The leading B pictures of an open GOP that has its predecessor predict forward from that GOP's last anchor: the lane before
// owns its slots, so the slot is final once that anchor has run; for the window's first GOP it is `carry`, the slot
// submit_window copies the window before's last anchor to in front of the first level (-1: nothing to copy, *uses_carry tells
// whether it is needed).  *last_anchor: the slot of the last GOP's last anchor, -1 without one.
// Invariant: a slot is not written again before the last picture that reads it has run.  Three rotating slots keep it for a GOP
// on its own -- anchor k + 3 (level k + 3) replaces anchor k, whose last readers are the B pictures in front of anchor k + 1
// (level k + 2) -- and for leading B pictures at level 1 (closed GOPs, and lane 0 with the carry slot).  In lane j > 0 the leading
// B pictures of an open GOP wait for the lane before's last anchor, level 4 behind an IBBP-12, while the lane's own fourth anchor
// would replace the I picture, their backward reference, at level 3.  So the I picture of such a GOP is written to the lane's HOLD
// slot (behind the carry slot, one per lane), which nothing else of the window writes; its other anchors rotate as before.
int plan_levels(const leon_pipeline* p, const PipeWindow* w, std::vector<std::vector<LevelPic>>& levels, int carry, bool* uses_carry, int* last_anchor,
                int* last_anchor_tref)
{
    const int per_lane = 3 + (p->unfused ? p->max_pics : 0);
    int prev_last = -1, lv_prev_last = -1;       // the lane before's last anchor and its level
    int tr_prev_last = p->last_anchor_tref;      // ... and its display index (lane 0: the carried anchor's)
    *uses_carry = false;
    for (size_t j = 0; j < w->jobs.size(); j++) {
        const GopJob* job = w->jobs[j].get();
        int older = -1, newer = -1, lv_older = -1, lv_newer = -1, n_anchor = 0;      // anchor slots (0..2 of the lane) and their levels
        int n_b = 0;
        int tr_older = -1, tr_newer = -1;        // the anchors' display indices
        for (const PipePic& m : job->pics) {
            LevelPic it{j, &m, -1, -1, -1};
            int lv = 0;
            if (m.type == LEON_PIC_I) {
                it.out = j && n_anchor == 0 && job->open_gop && job->has_pred ? p->carry_slot + 1 + (int)j : (int)(per_lane * j) + n_anchor % 3;
            } else if (m.type == LEON_PIC_P) {
                if (newer < 0) return fail(LEON_ERR_INVALID, "GOP %llu: a P picture without a preceding anchor", (unsigned long long)job->gop);
                it.fwd = newer;
                it.fwd_tref = tr_newer;
                lv = lv_newer + 1;
                it.out = (int)(per_lane * j) + n_anchor % 3;
            } else {
                if (newer < 0) return fail(LEON_ERR_INVALID, "GOP %llu: a B picture without an anchor (open GOPs cannot be sharded)", (unsigned long long)job->key_gop);
                // the leading B pictures of a CLOSED GOP predict backward only (both references = the I picture); in an
                // open GOP (closed_gop = 0) they may predict from the GOP before, which a shard does not have
                if (older < 0 && job->open_gop && !job->has_pred)
                    return fail(LEON_ERR_INVALID, "GOP %llu is open (closed_gop = 0) and its leading B pictures may predict from the GOP before it: "
                                                  "GOP shards must be closed", (unsigned long long)job->key_gop);
                it.bwd = newer;
                it.bwd_tref = tr_newer;
                if (older >= 0 || !job->open_gop) {
                    it.fwd = older >= 0 ? older : newer;
                    it.fwd_tref = older >= 0 ? tr_older : tr_newer;
                    lv = std::max(lv_newer, lv_older) + 1;
                } else {
                    it.fwd = j ? prev_last : carry;
                    it.fwd_tref = tr_prev_last;
                    it.fwd_before = true;
                    if (it.fwd < 0) return fail(LEON_ERR_INVALID, "GOP %llu is open and the last anchor of the GOP before it is not at hand", (unsigned long long)job->key_gop);
                    if (!j) *uses_carry = true;
                    lv = std::max(lv_newer, j ? lv_prev_last : -1) + 1;
                }
                if (p->unfused) it.out = (int)(per_lane * j) + 3 + n_b++ % p->max_pics;
            }
            if (m.type != LEON_PIC_B) {
                older = newer; lv_older = lv_newer; tr_older = tr_newer;
                newer = it.out; lv_newer = lv; tr_newer = m.tref;
                n_anchor++;
            }
            if ((size_t)lv >= levels.size()) levels.resize((size_t)lv + 1);
            levels[(size_t)lv].push_back(it);
            if (m.tref < 0 || m.tref >= p->max_pics) return fail(LEON_ERR_INVALID, "temporal reference %d outside the GOP", m.tref);
        }
        // two pictures of a GOP with one temporal reference would be rendered into the same frame of the ring
        std::vector<uint8_t> seen((size_t)p->max_pics, 0);
        for (const PipePic& m : job->pics) {
            if (seen[(size_t)m.tref]) return fail(LEON_ERR_INVALID, "GOP %llu: two pictures with temporal reference %d", (unsigned long long)job->key_gop, m.tref);
            seen[(size_t)m.tref] = 1;
        }
        prev_last = newer; lv_prev_last = lv_newer; tr_prev_last = tr_newer;
    }
    *last_anchor = prev_last;
    *last_anchor_tref = tr_prev_last;
    return LEON_OK;
}

// Every GOP's arena goes up on the copy stream before the window's first launch; then the chain copy stream -> (gpu_parser:
// the parser kernels, on a parser stream ->) the decoder's stream.
int upload_and_chain(leon_pipeline* p, PipeWindow* w, bool serial, bool poison)
{
    leon_decoder* d = p->dec;
    for (const auto& job : w->jobs) {
        const size_t up = p->gpu_parser ? job->upload_bytes : job->arena->used;
        if (poison && p->gpu_parser && job->arena->used > up) HIP_TRY(hipMemsetAsync(job->arena->dev + up, 0xCD, job->arena->used - up, p->copy_stream));
        if (up) {
            HIP_TRY(hipMemcpyAsync(job->arena->dev, job->arena->host, up, hipMemcpyHostToDevice, p->copy_stream));
            p->st_upload += up;
        }
    }
    Event ready = get_event(d->ev_pool);        // what the decoder's stream waits for: the upload, or the parser kernels
    if (!ready) return LEON_ERR_HIP;
    HIP_TRY(hipEventRecord(ready, p->copy_stream));
    if (serial) HIP_TRY(hipStreamSynchronize(p->copy_stream));
    if (p->gpu_parser) {
        hipStream_t vs = p->vlc_stream[vlc_stream_of(w->id)];
        HIP_TRY(hipStreamWaitEvent(vs, ready, 0));
        d->ev_pool.push_back(std::move(ready));
        const int rc = launch_gpu_parser(p, w);
        if (rc != LEON_OK) return rc;
        if (serial) HIP_TRY(hipStreamSynchronize(vs));
        if (!(ready = get_event(d->ev_pool))) return LEON_ERR_HIP;
        HIP_TRY(hipEventRecord(ready, vs));
    }
    HIP_TRY(hipStreamWaitEvent(d->stream, ready, 0));
    d->ev_pool.push_back(std::move(ready));
    return LEON_OK;
}

// the matrix sets of shards whose sequence headers carry other matrices than the stream's first: registered with the
// decoder here, on the one thread that drives it (the upload is ordered in front of the launches by the stream)
int register_qsets(leon_pipeline* p, const PipeWindow* w, std::vector<std::vector<int32_t>>& qset)
{
    for (size_t j = 0; j < w->jobs.size(); j++)
        for (const auto& m : w->jobs[j]->qms) {
            int32_t id = 0;
            const int rc = leon_add_quant_matrices(p->dec, m.data(), m.data() + 64, &id);
            if (rc != LEON_OK) return rc;
            qset[j].push_back(id);
        }
    return LEON_OK;
}

// One level, one batch.  Fused road: a shown picture's launch writes its frame (RGBA and / or planes), B pictures nothing
// else.  Unfused road: every picture writes its planes, then each shown one is converted (leon_convert_rgba) and the level's
// shown pictures are cropped into their frames' planes (k_planes_crop, one launch).
int launch_level(leon_pipeline* p, const PipeWindow* w, const std::vector<LevelPic>& lvl, const std::vector<std::vector<int32_t>>& qset)
{
    leon_decoder* d = p->dec;
    std::vector<AnyPic> batch;
    for (const LevelPic& it : lvl) {
        const char* base = w->jobs[it.lane]->arena->dev;
        const PipePic& m = *it.pic;
        auto ptr = [&](size_t off) -> const void* { return off == kNone ? nullptr : (const void*)(base + off); };
        const bool writes_frame = !p->unfused && m.shown;
        const FrameAddr f = frame_addr(p, w->ring, it.lane, (size_t)m.tref);
        AnyPic a;
        a.sparse = true;
        a.p.type = m.type;
        a.p.out_slot = it.out;
        a.p.ref_fwd_slot = it.fwd;
        a.p.ref_bwd_slot = it.bwd;
        a.grp_off = (const uint32_t*)ptr(m.grp_off);
        a.entries = (const uint32_t*)ptr(m.entries);
        a.n_entries = m.n_entries;
        a.p.qscale = (const uint8_t*)ptr(m.qscale);
        a.p.intra = (const uint8_t*)ptr(m.intra);
        a.p.repadd = (const uint8_t*)ptr(m.repadd);
        a.p.mb_dir = (const uint8_t*)ptr(m.mb_dir);
        a.p.mv_fwd = (const int16_t*)ptr(m.mv_fwd);
        a.p.mv_bwd = (const int16_t*)ptr(m.mv_bwd);
        a.p.rgba_out = writes_frame ? f.rgba : nullptr;
        a.planes_out = writes_frame ? f.planes : nullptr;
        a.p.no_planes = !p->unfused && m.type == LEON_PIC_B;
        a.p.qm_set = m.qm >= 0 ? qset[it.lane][(size_t)m.qm] : 0;
        batch.push_back(a);
    }
    int rc = submit_batch_any(d, batch.data(), (int)batch.size(), LEON_MEM_DEVICE);
    if (rc != LEON_OK || !p->unfused) return rc;
    std::vector<int32_t> crop_slots;
    std::vector<uint8_t*> crop_frames;
    for (const LevelPic& it : lvl) {
        if (!it.pic->shown) continue;
        const FrameAddr f = frame_addr(p, w->ring, it.lane, (size_t)it.pic->tref);
        if (f.rgba && (rc = leon_convert_rgba(d, it.out, f.rgba, LEON_MEM_DEVICE, p->flavour)) != LEON_OK) return rc;
        if (f.planes) {
            crop_slots.push_back(it.out);
            crop_frames.push_back(f.planes);
        }
    }
    return crop_planes_batch(d, crop_slots.data(), crop_frames.data(), (int)crop_slots.size());
}

// carry: which window frames a frame's vectors point into (include/leon_pipeline.h, "References inside a window"): the frames sorted
// by (gop, display_index) once, every reference looked up in them
void carry_refs_host(const leon_pipeline_frame* frames, const leon_pipeline_motion_frame* motion, int32_t n, int32_t* fwd, int32_t* bwd)
{
    std::vector<int32_t> order((size_t)n);
    for (int32_t i = 0; i < n; i++) order[(size_t)i] = i;
    const auto key_less = [&](uint64_t ga, int32_t da, uint64_t gb, int32_t db) { return ga != gb ? ga < gb : da < db; };
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key_less(frames[a].gop, frames[a].display_index, frames[b].gop, frames[b].display_index); });
    const auto find = [&](uint64_t gop, int32_t display) -> int32_t {
        if (display < 0) return -1;
        const auto it = std::lower_bound(order.begin(), order.end(), 0, [&](int32_t a, int32_t) { return key_less(frames[a].gop, frames[a].display_index, gop, display); });
        return it != order.end() && frames[*it].gop == gop && frames[*it].display_index == display ? *it : -1;
    };
    for (int32_t i = 0; i < n; i++) {
        fwd[i] = find(motion[i].fwd_gop, motion[i].fwd_display);
        bwd[i] = find(frames[i].gop, motion[i].bwd_display);
    }
}

// the window's frames in display order, GOP-major
void list_frames(leon_pipeline* p, PipeWindow* w, const std::vector<std::vector<LevelPic>>& levels, const std::vector<std::vector<int32_t>>& qset)
{
    w->frames.clear();
    w->tensors.clear();
    w->frame_ids.clear();
    w->motion.clear();
    w->motion_descs.clear();
    w->activity.clear();
    w->activity_descs.clear();
    w->residual.clear();
    w->residual_descs.clear();
    // output MOTION: what plan_levels gave each picture's launch to predict from, by lane and display index
    std::vector<const LevelPic*> planned;
    if (p->motion.ring) {
        planned.assign(w->jobs.size() * (size_t)p->max_pics, nullptr);
        for (const auto& lvl : levels)
            for (const LevelPic& it : lvl) planned[it.lane * (size_t)p->max_pics + (size_t)it.pic->tref] = &it;
    }
    for (size_t j = 0; j < w->jobs.size(); j++) {
        const GopJob* job = w->jobs[j].get();
        // by temporal reference: a GOP cut short by the encoder may skip display positions
        std::vector<const PipePic*> by_disp((size_t)p->max_pics, nullptr);
        for (const PipePic& m : job->pics) by_disp[(size_t)m.tref] = &m;
        for (size_t k = 0; k < by_disp.size(); k++) {
            if (!by_disp[k] || !by_disp[k]->shown) continue;
            const FrameAddr a = frame_addr(p, w->ring, j, k);
            leon_pipeline_frame f{};
            f.gop = job->key_gop;
            f.display_index = (int32_t)k;
            f.type = by_disp[k]->type;
            f.ts_ms = frame_ts_ms(p, job, (int)k);
            f.rgba = a.rgba;
            if (a.tensor) {
                w->tensors.push_back(a.tensor);
                w->frame_ids.push_back((uint32_t)(a.index - (size_t)w->ring * p->W * p->max_pics));
            }
            if (a.planes && (p->output & LEON_PIPELINE_OUTPUT_YCBCR)) {
                f.y = a.planes;
                f.cb = a.planes + p->planes_geom.cb_off;
                f.cr = a.planes + p->planes_geom.cr_off;
                f.a = p->vinfo.has_alpha == 1 ? a.planes + p->planes_geom.a_off : nullptr;
            }
            const PipePic& m = *by_disp[k];
            const char* base = job->arena->dev;
            auto ptr = [&](size_t off) -> const void* { return off == kNone ? nullptr : (const void*)(base + off); };
            if (p->motion.ring) {
                const LevelPic* it = planned[j * (size_t)p->max_pics + k];
                leon_pipeline_motion_frame mf{};
                mf.record = p->motion.record(a.index);
                mf.fwd_gop = it && it->fwd_before ? job->key_gop - 1 : job->key_gop;
                mf.fwd_display = it ? it->fwd_tref : -1;
                mf.bwd_display = it ? it->bwd_tref : -1;
                w->motion.push_back(mf);
                leon::MotionDesc d{};
                d.type = m.type;
                d.frame = (uint32_t)a.index;
                d.repadd = (const uint8_t*)ptr(m.type != LEON_PIC_I ? m.repadd : kNone);
                d.mv_fwd = (const uint32_t*)ptr(m.type != LEON_PIC_I ? m.mv_fwd : kNone);
                d.mb_dir = (const uint8_t*)ptr(m.type == LEON_PIC_B ? m.mb_dir : kNone);
                d.mv_bwd = (const uint32_t*)ptr(m.type == LEON_PIC_B ? m.mv_bwd : kNone);
                w->motion_descs.push_back(d);
            }
            if (p->activity.ring) {
                w->activity.push_back(p->activity.record(a.index));
                leon::ActivityDesc d{};
                d.grp_off = (const uint32_t*)ptr(m.grp_off);
                d.entries = (const uint32_t*)ptr(m.entries);
                d.qscale = (const uint8_t*)ptr(m.qscale);
                d.n_entries = m.n_entries;
                d.frame = (uint32_t)a.index;
                w->activity_descs.push_back(d);
            }
            if (p->residual.ring) {
                w->residual.push_back(p->residual.record(a.index));
                leon::ResidualDesc d{};
                d.grp_off = (const uint32_t*)ptr(m.grp_off);
                d.entries = (const uint32_t*)ptr(m.entries);
                d.qscale = (const uint8_t*)ptr(m.qscale);
                d.intra = (const uint8_t*)ptr(m.intra);
                // the matrices its reconstruction launch was given (launch_level, fill_desc)
                const int32_t set = m.qm >= 0 ? qset[j][(size_t)m.qm] : 0;
                d.qt = set > 0 ? &p->dec->qset_tabs.dev()[set] : &p->dec->d_tables->q;
                d.n_entries = m.n_entries;
                d.frame = (uint32_t)a.index;
                w->residual_descs.push_back(d);
            }
            w->frames.push_back(f);
        }
        p->st_pictures += job->pics.size();
    }
    p->st_gops += w->jobs.size();
    w->carry_table.clear();
    // the table of either record output: both rings are indexed by the frame's own index, so one ring id serves both; without MOTION
    // there are no references (-1), and the carry and propagate calls refuse such a pipeline before they look at the table
    if ((p->motion.ring || p->activity.ring) && !w->frames.empty()) {
        const size_t n = w->frames.size();
        std::vector<int32_t> fwd(n, -1), bwd(n, -1);
        if (p->motion.ring) carry_refs_host(w->frames.data(), w->motion.data(), (int32_t)n, fwd.data(), bwd.data());
        w->carry_table.resize(4 * n);
        for (size_t i = 0; i < n; i++) {
            const leon::CarryFrame f{p->motion.ring ? w->motion_descs[i].frame : w->activity_descs[i].frame, fwd[i], bwd[i], 0u};
            std::memcpy(&w->carry_table[4 * i], &f, sizeof(f));
        }
    }
}

// output TENSOR: the window's frames -> their tensors, one launch on the decoder's stream behind the last level (at most 65535 frames
// per launch: blockIdx.z).  Pictures decoded for prediction only (EXACT seek) are not among the frames.
// The kernels by element bytes (1, 2, 4 -> 0, 1, 2) and layout: k_tensor at the frame's size, k_resample at a model's input size, by
// filter as well (no entry: no such filter -- create refuses it).
typedef void (*TensorKernel)(const uint8_t*, uint8_t*, const uint32_t*, const uint32_t*, const leon::Tables*, leon::TensorGeom);
typedef void (*ResampleKernel)(const uint8_t*, uint8_t*, const uint32_t*, const uint32_t*, const leon::Tables*, const int32_t*, leon::ResampleGeom);
static_assert(leon::kLayoutChw == LEON_TENSOR_LAYOUT_CHW && leon::kLayoutHwc == LEON_TENSOR_LAYOUT_HWC, "the tables' layout index is LEON_TENSOR_LAYOUT_*");
static_assert(LEON_RESIZE_TRIANGLE == 0 && LEON_RESIZE_BICUBIC == 3, "kResampleKernels is indexed by LEON_RESIZE_*");
constexpr TensorKernel kTensorKernels[3][2] = {{leon::k_tensor<1, leon::kLayoutChw>, leon::k_tensor<1, leon::kLayoutHwc>},
                                               {leon::k_tensor<2, leon::kLayoutChw>, leon::k_tensor<2, leon::kLayoutHwc>},
                                               {leon::k_tensor<4, leon::kLayoutChw>, leon::k_tensor<4, leon::kLayoutHwc>}};
struct ResampleKernelsOfFilter { ResampleKernel k[3][2]; };
template <class F> constexpr ResampleKernelsOfFilter kResampleKernelsOf = {{{leon::k_resample<1, leon::kLayoutChw, F>, leon::k_resample<1, leon::kLayoutHwc, F>},
                                                                            {leon::k_resample<2, leon::kLayoutChw, F>, leon::k_resample<2, leon::kLayoutHwc, F>},
                                                                            {leon::k_resample<4, leon::kLayoutChw, F>, leon::k_resample<4, leon::kLayoutHwc, F>}}};
constexpr ResampleKernelsOfFilter kResampleKernels[4] = {kResampleKernelsOf<leon::ResTriangle>, {}, {}, kResampleKernelsOf<leon::ResCubic>};
// ... and k_letterbox where the resampled image lies in a padded canvas
typedef void (*LetterboxKernel)(const uint8_t*, uint8_t*, const uint32_t*, const uint32_t*, const leon::Tables*, const int32_t*, leon::LetterboxGeom);
struct LetterboxKernelsOfFilter { LetterboxKernel k[3][2]; };
template <class F> constexpr LetterboxKernelsOfFilter kLetterboxKernelsOf = {{{leon::k_letterbox<1, leon::kLayoutChw, F>, leon::k_letterbox<1, leon::kLayoutHwc, F>},
                                                                              {leon::k_letterbox<2, leon::kLayoutChw, F>, leon::k_letterbox<2, leon::kLayoutHwc, F>},
                                                                              {leon::k_letterbox<4, leon::kLayoutChw, F>, leon::k_letterbox<4, leon::kLayoutHwc, F>}}};
constexpr LetterboxKernelsOfFilter kLetterboxKernels[4] = {kLetterboxKernelsOf<leon::ResTriangle>, {}, {}, kLetterboxKernelsOf<leon::ResCubic>};

// where the kernels find a frame's planes and its tensor
leon::RingGeom ring_geom(const leon_pipeline* p)
{
    leon::RingGeom g{};
    g.luma_stride = p->planes_geom.luma_stride; g.chroma_stride = p->planes_geom.chroma_stride;
    g.cb_off = p->planes_geom.cb_off; g.cr_off = p->planes_geom.cr_off;
    g.planes_pitch_lo = (uint32_t)(p->planes_bytes & 0xffffffffu); g.planes_pitch_hi = (uint32_t)((uint64_t)p->planes_bytes >> 32);
    g.tensor_pitch_lo = (uint32_t)(p->tensor_pitch & 0xffffffffu); g.tensor_pitch_hi = (uint32_t)((uint64_t)p->tensor_pitch >> 32);
    return g;
}

int launch_tensors(leon_pipeline* p, const PipeWindow* w)
{
    const size_t n = w->frame_ids.size();
    if (!p->d_tensor || !n) return LEON_OK;
    const size_t entry = (size_t)p->W * p->max_pics;
    uint32_t* h = p->tensor_ids.host() + (size_t)w->ring * entry;       // the ring entry is this window's: its previous launch has finished
    uint32_t* dv = p->tensor_ids.dev() + (size_t)w->ring * entry;
    for (size_t i = 0; i < n; i++) h[i] = (uint32_t)((size_t)w->ring * entry) + w->frame_ids[i];
    HIP_TRY(hipMemcpyAsync(dv, h, n * 4, hipMemcpyHostToDevice, p->dec->stream));
    const bool resized = p->tensor_geom.resized != 0;
    const int eb = (int)p->tensor_elem, layout = p->tensor_layout, filter = p->resize_filter;
    leon::TensorGeom G{};
    leon::ResampleGeom R = p->resample_geom;
    unsigned gx, gy = 1;
    if (resized) {          // a workgroup per tile of kResTileX x kResTileY output pixels
        R.ring = ring_geom(p);
        gx = (unsigned)((R.ow + leon::kResTileX - 1) / leon::kResTileX);
        gy = (unsigned)((R.oh + leon::kResTileY - 1) / leon::kResTileY);
    } else {                // lanes numbered linearly through the frame
        G.fw = p->vinfo.frame_width; G.fh = p->vinfo.frame_height;
        G.fast = (G.fw & 7) == 0;
        G.per_row = (uint32_t)(G.fast ? G.fw / leon::lane_px(eb) : G.fw / 2);
        G.n_items = G.per_row * (uint32_t)((G.fh + 1) / 2);
        G.ring = ring_geom(p);
        if (!G.n_items) return LEON_OK;
        gx = (G.n_items + leon::kRgbaBlock - 1) / leon::kRgbaBlock;
    }
    const bool listed = (eb == 1 || eb == 2 || eb == 4) && (layout == leon::kLayoutChw || layout == leon::kLayoutHwc) && filter >= 0 && filter < 4;
    const TensorKernel kt = listed && !resized ? kTensorKernels[eb >> 1][layout] : nullptr;
    const bool canvas = resized && p->canvas_on;
    const ResampleKernel kr = listed && resized && !canvas ? kResampleKernels[filter].k[eb >> 1][layout] : nullptr;
    const LetterboxKernel kl = listed && canvas ? kLetterboxKernels[filter].k[eb >> 1][layout] : nullptr;
    leon::LetterboxGeom L{R, p->canvas_geom};
    if (canvas) {
        // the pad's workgroups behind the image's tile rows: whole rows of gx workgroups that cover every 16-byte line of the tensor,
        // kPadLinesPerGroup each (the last ones may find nothing); none when the image fills the canvas
        const bool pad = L.canvas.cw != R.ow || L.canvas.ch != R.oh;
        const size_t lines = (p->tensor_bytes + 15) / 16, groups = pad ? (lines + leon::kPadLinesPerGroup - 1) / leon::kPadLinesPerGroup : 0;
        gy += (unsigned)((groups + gx - 1) / gx);
        if (gy > 65535u) return fail(LEON_ERR_INVALID, "tensor canvas: %u workgroup rows", gy);
    }
    if (!kt && !kr && !kl) return fail(LEON_ERR_INVALID, "tensor: no kernel for %d-byte elements, layout %d, filter %d", eb, layout, filter);
    for (size_t at = 0; at < n; at += 65535) {
        const dim3 grid(gx, gy, (unsigned)std::min<size_t>(65535, n - at)), block(leon::kRgbaBlock);
        if (canvas) hipLaunchKernelGGL(kl, grid, block, 0, p->dec->stream, (const uint8_t*)p->d_planes, p->d_tensor, (const uint32_t*)(dv + at),
                                       (const uint32_t*)p->d_tensor_table, (const leon::Tables*)p->dec->d_tables, (const int32_t*)p->d_resize_tabs, L);
        else if (resized) hipLaunchKernelGGL(kr, grid, block, 0, p->dec->stream, (const uint8_t*)p->d_planes, p->d_tensor, (const uint32_t*)(dv + at),
                                        (const uint32_t*)p->d_tensor_table, (const leon::Tables*)p->dec->d_tables, (const int32_t*)p->d_resize_tabs, R);
        else hipLaunchKernelGGL(kt, grid, block, 0, p->dec->stream, (const uint8_t*)p->d_planes, p->d_tensor, (const uint32_t*)(dv + at),
                                (const uint32_t*)p->d_tensor_table, (const leon::Tables*)p->dec->d_tables, G);
    }
    HIP_TRY(hipGetLastError());
    return LEON_OK;
}

// ---- the refusals that several motion and region calls state, each under the caller's own prefix ----------------------------------------
int record_count_check(const char* who, const char* noun, int32_t n)
{
    return n < 1 || n > 65535 ? fail(LEON_ERR_INVALID, "%s: %d %s (a call takes 1 .. 65535)", who, n, noun) : LEON_OK;
}
int no_output(const char* name, const char* flag)          // a call for an output the pipeline was made without: its lower-case name, its flag's
{
    return fail(LEON_ERR_INVALID, "the pipeline has no %s output (leon_pipeline_config.output without LEON_PIPELINE_OUTPUT_%s)", name, flag);
}
// The n per-frame items of a delivered window -- `items`: which PipeWindow vector; `noun`: what the count message calls them -- for the
// window_* calls, and frame `index`'s item alone for the read_* calls.  Not through window_delivered: a window delivered with an error
// still answers these.
template <class T, class Out>
int window_items(leon_pipeline* p, int64_t window, std::vector<T> PipeWindow::*items, const char* noun, Out* out, int32_t n)
{
    size_t has = 0;
    const bool delivered = p->flow.with_delivered(window, [&](const PipeWindow& w) {
        has = (w.*items).size();
        if (n >= 0 && (size_t)n == has) std::copy((w.*items).begin(), (w.*items).end(), out);
    });
    if (!delivered) return fail(LEON_ERR_INVALID, "window %lld is not out for delivery", (long long)window);
    if (n < 0 || (size_t)n != has) return fail(LEON_ERR_INVALID, "window %lld has %zu %s, not %d", (long long)window, has, noun, n);
    return LEON_OK;
}
template <class T>
int window_item(leon_pipeline* p, int64_t window, int32_t index, std::vector<T> PipeWindow::*items, T* out)
{
    bool has = false;
    const bool delivered = p->flow.with_delivered(window, [&](const PipeWindow& w) {
        if ((has = index >= 0 && (size_t)index < (w.*items).size())) *out = (w.*items)[(size_t)index];
    });
    if (!delivered) return fail(LEON_ERR_INVALID, "window %lld is not out for delivery", (long long)window);
    if (!has) return fail(LEON_ERR_INVALID, "window %lld has no frame %d", (long long)window, index);
    return LEON_OK;
}
int mb_grid_check(const char* who, int32_t mbw, int32_t mbh)
{
    if (mbw >= 1 && mbw <= leon::kMotionMaxMb && mbh >= 1 && mbh <= leon::kMotionMaxMb) return LEON_OK;
    return fail(LEON_ERR_INVALID, "%s: %d x %d macroblocks (1 .. %d each)", who, mbw, mbh, leon::kMotionMaxMb);
}
// a picture of `type` has the maps k_motion reads of it
bool motion_maps_present(int32_t type, const void* repadd, const void* mb_dir, const void* mv_fwd, const void* mv_bwd)
{
    return (type == LEON_PIC_I || (repadd && mv_fwd)) && (type != LEON_PIC_B || (mb_dir && mv_bwd));
}

// output MOTION: the window's frames -> their motion records, one launch on the decoder's stream behind the last level and in front of
// the window's event (at most 65535 frames per launch: blockIdx.y), while the maps are still in the GOPs' arenas.  The descriptors are
// staged in the ring entry's part of the mirror and go up with one copy.
static_assert(sizeof(leon::MotionDesc) == 48, "a descriptor is 12 dwords");
static_assert(sizeof(leon_pipeline_motion_frame) == 32 && sizeof(struct leon_pipeline_motion_layout) == 64, "include/leon_pipeline.h states the sizes");
// k_motion over n descriptors in device memory, frame i of them in workgroup i: the one place that cuts them into launches
// (launch_motion for a window, motion_kernel for a caller's maps)
void motion_launch(const leon::MotionDesc* descs, size_t n, uint8_t* ring, const leon::MotionLayout& lay, hipStream_t stream)
{
    for (size_t at = 0; at < n; at += 65535) {
        const dim3 grid(1, (unsigned)std::min<size_t>(65535, n - at)), block(leon::kRgbaBlock);
        hipLaunchKernelGGL(leon::k_motion, grid, block, 0, stream, descs + at, ring, lay);
    }
}

// A window's records: its descriptors, each checked (`check(i, d)`: LEON_OK or the refusal it states), staged in the ring entry's part
// of the mirror, up with one copy on the decoder's stream, then `launch(device descriptors, n)`
template <class Desc, class Check, class Launch>
int launch_records(leon_pipeline* p, const PipeWindow* w, const RecordOutput<Desc>& out, const std::vector<Desc>& descs, Check check, Launch launch)
{
    const size_t n = descs.size();
    if (!out.ring || !n) return LEON_OK;
    const size_t at = (size_t)w->ring * p->W * p->max_pics;      // the ring entry is this window's: its previous launch has finished
    Desc *h = out.descs.host() + at, *dv = out.descs.dev() + at;
    for (size_t i = 0; i < n; i++) {
        if (const int rc = check(i, descs[i]); rc != LEON_OK) return rc;
        h[i] = descs[i];
    }
    HIP_TRY(hipMemcpyAsync(dv, h, n * sizeof(Desc), hipMemcpyHostToDevice, p->dec->stream));
    launch(dv, n);
    HIP_TRY(hipGetLastError());
    return LEON_OK;
}

int launch_motion(leon_pipeline* p, const PipeWindow* w)
{
    return launch_records(p, w, p->motion, w->motion_descs, [&](size_t i, const leon::MotionDesc& d) {
        if (motion_maps_present(d.type, d.repadd, d.mb_dir, d.mv_fwd, d.mv_bwd)) return (int)LEON_OK;
        return fail(LEON_ERR_INVALID, "motion: frame %zu of window %lld (type %d) lacks a map", i, (long long)w->id, d.type);
    }, [&](const leon::MotionDesc* dv, size_t n) { motion_launch(dv, n, p->motion.ring, p->motion_lay, p->dec->stream); });
}

// the definition on the CPU: the same per-macroblock text (leon_motion.h), the specified bytes of one record
int motion_record_host(int32_t type, int32_t mbw, int32_t mbh, const uint8_t* repadd, const uint8_t* mb_dir, const int16_t* mv_fwd, const int16_t* mv_bwd,
                       void* record)
{
    if (!record) return fail(LEON_ERR_INVALID, "null argument");
    if (type != LEON_PIC_I && type != LEON_PIC_P && type != LEON_PIC_B) return fail(LEON_ERR_INVALID, "motion record: picture type %d", type);
    if (const int rc = mb_grid_check("motion record", mbw, mbh); rc != LEON_OK) return rc;
    if (!motion_maps_present(type, repadd, mb_dir, mv_fwd, mv_bwd))
        return fail(LEON_ERR_INVALID, "motion record: a picture of type %d without one of its maps", type);
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    uint8_t* rec = static_cast<uint8_t*>(record);
    uint32_t s[8] = {};
    for (uint32_t k = 0; k < L.mbs; k++) {
        uint32_t f = 0, b = 0, of, ob;
        if (type != LEON_PIC_I) memcpy(&f, mv_fwd + 2 * (size_t)k, 4);
        if (type == LEON_PIC_B) memcpy(&b, mv_bwd + 2 * (size_t)k, 4);
        const uint32_t info = leon::motion_mb(type, type != LEON_PIC_I ? repadd[k] : 0u, type == LEON_PIC_B ? mb_dir[k] : 0u, f, b, &of, &ob);
        leon::motion_count(info, of, ob, s);
        memcpy(rec + 8 * (size_t)k, &of, 4);
        memcpy(rec + 8 * (size_t)k + 4, &ob, 4);
        rec[L.info_offset + k] = (uint8_t)info;
    }
    memcpy(rec + L.summary_offset, s, 32);
    return LEON_OK;
}

static_assert(sizeof(leon_pipeline_motion_picture) == 40 && sizeof(leon_pipeline_motion_kernel_frame) == 8, "include/leon_pipeline.h states the sizes");
// what the diagnostics that run a record kernel on a caller's pictures (motion_kernel, activity_kernel) refuse of their counts and frames
int kernel_counts_check(const char* who, int32_t n_pics, int32_t n_frames, int32_t ring_frames, int32_t pad_byte)
{
    if (n_pics < 1 || n_pics > LEON_MOTION_KERNEL_MAX_FRAMES) return fail(LEON_ERR_INVALID, "%s: %d pictures (1 .. %d)", who, n_pics, LEON_MOTION_KERNEL_MAX_FRAMES);
    if (ring_frames < 1 || ring_frames > LEON_MOTION_KERNEL_MAX_FRAMES)
        return fail(LEON_ERR_INVALID, "%s: a ring of %d records (1 .. %d)", who, ring_frames, LEON_MOTION_KERNEL_MAX_FRAMES);
    if (n_frames < 1 || n_frames > ring_frames) return fail(LEON_ERR_INVALID, "%s: %d frames (1 .. the ring's %d records)", who, n_frames, ring_frames);
    if (pad_byte < 0 || pad_byte > 255) return fail(LEON_ERR_INVALID, "%s: pad_byte %d (0 .. 255)", who, pad_byte);
    return LEON_OK;
}
int kernel_frames_check(const char* who, int32_t n_pics, const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames)
{
    std::vector<bool> named((size_t)ring_frames, false);
    for (int32_t i = 0; i < n_frames; i++) {
        const leon_pipeline_motion_kernel_frame& f = frames[i];
        if (f.picture < 0 || f.picture >= n_pics) return fail(LEON_ERR_INVALID, "%s: frame %d names picture %d of %d", who, i, f.picture, n_pics);
        if (f.ring < 0 || f.ring >= ring_frames) return fail(LEON_ERR_INVALID, "%s: frame %d names record %d of a ring of %d", who, i, f.ring, ring_frames);
        if (named[(size_t)f.ring]) return fail(LEON_ERR_INVALID, "%s: frame %d names record %d, which an earlier frame names", who, i, f.ring);
        named[(size_t)f.ring] = true;
    }
    return LEON_OK;
}
// The pieces of one device allocation that a synchronous call makes for itself (the host roads, the diagnostics on a caller's records,
// resize_weights_device): `src` goes up if there is one, `dst` is brought back if there is one, `bytes` of either.  A piece without
// a source holds what the allocation happens to hold; where a caller's array is both, the words the kernel leaves alone come back
// as they were.  Every piece lies on a 256-byte boundary and takes 256 bytes at the least, so one of no bytes (no frames, no slots)
// still has an address of its own that nothing reads.  alloc() lays them out and allocates, after which at() gives the device
// address of piece i; up() and down() copy on the null stream, and down()'s copies wait: nothing in flight reads the allocation when
// it goes.
struct Piece { const void* src; void* dst; size_t bytes; };
class Pieces {
public:
    int alloc(const char* who, std::initializer_list<Piece> pieces)
    {
        pieces_ = pieces;
        size_t bytes = 0;
        for (const Piece& q : pieces_) bytes += pad256(std::max<size_t>(q.bytes, 1));
        if (!d_.alloc(bytes)) { (void)hipGetLastError(); return fail(LEON_ERR_NOMEM, "%s: %zu bytes of device memory", who, bytes); }
        uint8_t* at = d_;
        for (const Piece& q : pieces_) {
            at_.push_back(at);
            at += pad256(std::max<size_t>(q.bytes, 1));
        }
        return LEON_OK;
    }
    template <class T = uint8_t> T* at(size_t i) const { return reinterpret_cast<T*>(at_[i]); }
    int up() const
    {
        for (size_t i = 0; i < pieces_.size(); i++)
            if (pieces_[i].src && pieces_[i].bytes) HIP_TRY(hipMemcpy(at_[i], pieces_[i].src, pieces_[i].bytes, hipMemcpyHostToDevice));
        return LEON_OK;
    }
    int down() const
    {
        for (size_t i = 0; i < pieces_.size(); i++)
            if (pieces_[i].dst && pieces_[i].bytes) HIP_TRY(hipMemcpy(pieces_[i].dst, at_[i], pieces_[i].bytes, hipMemcpyDeviceToHost));
        return LEON_OK;
    }

private:
    DevBuf<uint8_t> d_;
    std::vector<Piece> pieces_;
    std::vector<uint8_t*> at_;
};
// One such call whose sources are complete before the allocation: the pieces up, run(pieces) -- which enqueues on the null stream, or
// is a device road that has waited -- the runtime's last error, the pieces down.  Nothing touches the device before it.
template <class Run>
int pieces_run(int32_t device_id, const char* who, std::initializer_list<Piece> pieces, Run run)
{
    HIP_TRY(hipSetDevice(device_id));
    Pieces s;
    int rc;
    if ((rc = s.alloc(who, pieces)) != LEON_OK || (rc = s.up()) != LEON_OK || (rc = run(s)) != LEON_OK) return rc;
    HIP_TRY(hipGetLastError());
    return s.down();
}

// A record kernel on a caller's pictures (motion_kernel, activity_kernel): memory of its own, the null stream.  One device allocation
// [descriptors | payload | ring]: every array of every picture in a piece of its own, padded with pad_byte; the caller's ring of
// records `pitch` apart goes up and comes back whole.  `sized(i, picture, &bytes)` refuses picture i or gives the bytes its pieces
// take; `fill(picture, place)` makes its descriptor, `place(src, n, padded)` copying n bytes into the next piece of `padded` and
// returning where the device will hold it; `launch(descriptors, n_frames, ring)`.  Nothing touches the device before every refusal.
template <class Desc, class Pic, class Sized, class Fill, class Launch>
int record_kernel(const char* who, int32_t device_id, int32_t mbw, int32_t mbh, const Pic* pics, int32_t n_pics, const leon_pipeline_motion_kernel_frame* frames,
                  int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring, size_t pitch, Sized sized, Fill fill, Launch launch)
{
    if (!pics || !frames || !ring) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = mb_grid_check(who, mbw, mbh); rc != LEON_OK) return rc;
    if (const int rc = kernel_counts_check(who, n_pics, n_frames, ring_frames, pad_byte); rc != LEON_OK) return rc;
    size_t payload_bytes = 0;
    for (int32_t i = 0; i < n_pics; i++) {
        size_t b = 0;
        if (const int rc = sized(i, pics[i], &b); rc != LEON_OK) return rc;
        payload_bytes += b;
    }
    if (const int rc = kernel_frames_check(who, n_pics, frames, n_frames, ring_frames); rc != LEON_OK) return rc;
    // the payload as the device will hold it, staged on the host: the pad byte everywhere, then each array into its piece
    std::vector<uint8_t> payload(payload_bytes, (uint8_t)pad_byte);
    std::vector<Desc> pic_descs((size_t)n_pics), descs((size_t)n_frames);
    HIP_TRY(hipSetDevice(device_id));
    Pieces s;
    if (const int rc = s.alloc(who, {{descs.data(), nullptr, descs.size() * sizeof(Desc)}, {payload.data(), nullptr, payload_bytes},      // (I pictures alone have no payload)
                                     {ring, ring, (size_t)ring_frames * pitch}}); rc != LEON_OK)
        return rc;
    const uint8_t* d_payload = s.at(1);
    size_t at = 0;
    auto place = [&](const void* src, size_t n, size_t padded) {
        if (n) memcpy(payload.data() + at, src, n);          // (a picture's empty list may be null)
        const uint8_t* dev = d_payload + at;
        at += padded;
        return dev;
    };
    for (int32_t i = 0; i < n_pics; i++) pic_descs[(size_t)i] = fill(pics[i], place);
    for (int32_t i = 0; i < n_frames; i++) {
        descs[(size_t)i] = pic_descs[(size_t)frames[i].picture];
        descs[(size_t)i].frame = (uint32_t)frames[i].ring;
    }
    if (const int rc = s.up(); rc != LEON_OK) return rc;
    launch(s.at<const Desc>(0), (size_t)n_frames, s.at(2));
    HIP_TRY(hipGetLastError());
    return s.down();
}

// k_motion on maps the caller supplies (leon_pipeline_motion_kernel): every map padded as MapLayout pads it (mpad, vpad)
int motion_kernel(int32_t device_id, int32_t mbw, int32_t mbh, const leon_pipeline_motion_picture* pics, int32_t n_pics, const leon_pipeline_motion_kernel_frame* frames,
                  int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring)
{
    const MapLayout M = map_layout((size_t)mbw * (size_t)mbh, 0);
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    return record_kernel<leon::MotionDesc>("motion kernel", device_id, mbw, mbh, pics, n_pics, frames, n_frames, ring_frames, pad_byte, ring, L.record_pitch,
        [&](int32_t i, const leon_pipeline_motion_picture& q, size_t* bytes) {
            if (q.type != LEON_PIC_I && q.type != LEON_PIC_P && q.type != LEON_PIC_B) return fail(LEON_ERR_INVALID, "motion kernel: picture %d has type %d", i, q.type);
            if (q.reserved0) return fail(LEON_ERR_INVALID, "motion kernel: a reserved word of picture %d is not 0", i);
            if (!motion_maps_present(q.type, q.repadd, q.mb_dir, q.mv_fwd, q.mv_bwd))
                return fail(LEON_ERR_INVALID, "motion kernel: picture %d (type %d) lacks a map", i, q.type);
            *bytes = q.type == LEON_PIC_I ? 0 : (q.type == LEON_PIC_P ? 1 : 2) * (M.mpad + M.vpad);
            return (int)LEON_OK;
        },
        [&](const leon_pipeline_motion_picture& q, auto& place) {
            leon::MotionDesc D{};
            D.type = q.type;
            if (q.type != LEON_PIC_I) {
                D.repadd = place(q.repadd, M.mbs, M.mpad);
                D.mv_fwd = reinterpret_cast<const uint32_t*>(place(q.mv_fwd, M.mbs * 4, M.vpad));
            }
            if (q.type == LEON_PIC_B) {
                D.mb_dir = place(q.mb_dir, M.mbs, M.mpad);
                D.mv_bwd = reinterpret_cast<const uint32_t*>(place(q.mv_bwd, M.mbs * 4, M.vpad));
            }
            return D;
        },
        [&](const leon::MotionDesc* descs, size_t n, uint8_t* d_ring) { motion_launch(descs, n, d_ring, L, nullptr); });
}

int motion_layout_host(int32_t mbw, int32_t mbh, struct leon_pipeline_motion_layout* out)
{
    if (!out) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = mb_grid_check("motion layout", mbw, mbh); rc != LEON_OK) return rc;
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    memset(out, 0, sizeof(*out));
    out->mb_width = mbw; out->mb_height = mbh; out->mbs = (int32_t)L.mbs;
    out->info_offset = L.info_offset; out->summary_offset = L.summary_offset;
    out->record_bytes = L.record_bytes; out->record_pitch = L.record_pitch;
    return LEON_OK;
}

// output ACTIVITY: the window's frames -> their activity records, k_activity and k_activity_summary on the decoder's stream behind the
// last level and in front of the window's event, while the lists are still in the GOPs' arenas.  The descriptors go up as k_motion's do.
static_assert(sizeof(leon::ActivityDesc) == 32, "a descriptor is 8 dwords");
static_assert(sizeof(struct leon_pipeline_activity_layout) == 64 && sizeof(leon_pipeline_activity_picture) == 32, "include/leon_pipeline.h states the sizes");
static_assert(sizeof(leon::ActivityGeom) == 32 && sizeof(leon::ActivityLayout) == 16, "kernel arguments");
static_assert(leon::kActivityMaxMb == leon::kMotionMaxMb, "mb_grid_check states one bound");
// both kernels over n descriptors in device memory, frame i of them in workgroup row i: the one place that cuts them into launches
// (launch_activity for a window, activity_kernel for a caller's lists)
void activity_launch(const leon::ActivityDesc* descs, size_t n, uint8_t* ring, const leon::ActivityGeom& geom, const leon::ActivityLayout& lay, hipStream_t stream)
{
    const unsigned task_blocks = (geom.tasks + leon::kActivityWaves - 1) / leon::kActivityWaves;
    for (size_t at = 0; at < n; at += 65535) {
        const unsigned frames = (unsigned)std::min<size_t>(65535, n - at);
        hipLaunchKernelGGL(leon::k_activity, dim3(task_blocks, frames), dim3(leon::kRgbaBlock), 0, stream, descs + at, ring, geom, lay);
        hipLaunchKernelGGL(leon::k_activity_summary, dim3(1, frames), dim3(leon::kRgbaBlock), 0, stream, descs + at, ring, lay);
    }
}

int launch_activity(leon_pipeline* p, const PipeWindow* w)
{
    return launch_records(p, w, p->activity, w->activity_descs, [&](size_t i, const leon::ActivityDesc& d) {
        if (d.grp_off && d.entries && d.qscale) return (int)LEON_OK;
        return fail(LEON_ERR_INVALID, "activity: frame %zu of window %lld lacks its lists or its qscale map", i, (long long)w->id);
    }, [&](const leon::ActivityDesc* dv, size_t n) { activity_launch(dv, n, p->activity.ring, p->activity_geom, p->activity_lay, p->dec->stream); });
}

// what the host calls refuse of a picture's lists: they walk them without a clamp
int activity_lists_check(const char* who, const leon::ActivityGeom& G, const uint32_t* grp_off, const uint32_t* entries, uint32_t n_entries, const uint8_t* qscale)
{
    if (!grp_off || !qscale || (!entries && n_entries)) return fail(LEON_ERR_INVALID, "%s: null argument", who);
    const uint32_t n_groups = G.n_y + 2u * G.n_c;
    for (uint32_t g = 0; g < n_groups; g++)
        if (grp_off[g + 1] < grp_off[g]) return fail(LEON_ERR_INVALID, "%s: grp_off decreases at group %u (%u after %u)", who, g, grp_off[g + 1], grp_off[g]);
    if (grp_off[n_groups] > n_entries) return fail(LEON_ERR_INVALID, "%s: grp_off ends at %u, the list has %u entries", who, grp_off[n_groups], n_entries);
    return LEON_OK;
}

// the definition on the CPU: the same per-entry and per-macroblock text (leon_activity.h), the specified bytes of one record
int activity_record_host(int32_t mbw, int32_t mbh, const uint32_t* grp_off, const uint32_t* entries, uint32_t n_entries, const uint8_t* qscale, void* record)
{
    if (!record) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = mb_grid_check("activity record", mbw, mbh); rc != LEON_OK) return rc;
    const leon::ActivityGeom G = leon::activity_geom((uint32_t)mbw, (uint32_t)mbh);
    if (const int rc = activity_lists_check("activity record", G, grp_off, entries, n_entries, qscale); rc != LEON_OK) return rc;
    const leon::ActivityLayout L = leon::activity_layout((uint32_t)mbw, (uint32_t)mbh);
    std::vector<uint64_t> sums(3 * (size_t)L.mbs, 0);          // [ac_count | ac_mag | dc_mag][mbs]
    std::vector<uint8_t> blocks(L.mbs, 0);
    for (uint32_t plane = 0; plane < 3u; plane++) {
        const uint32_t rows = plane == 0u ? 2u * G.mbh : G.mbh, groups = plane == 0u ? G.groups_y : G.groups_c;
        const uint32_t first = plane == 0u ? 0u : G.n_y + (plane - 1u) * G.n_c;
        for (uint32_t R = 0; R < rows; R++)
            for (uint32_t g = 0; g < groups; g++) {
                const uint32_t gid = first + R * groups + g;
                uint32_t begin, end;
                leon::activity_span(grp_off[gid], grp_off[gid + 1], n_entries, &begin, &end);
                for (uint32_t i = begin; i < end; i++) {
                    const uint32_t e = entries[i], a = leon::activity_abs(e);
                    uint32_t mx, my, j;
                    leon::activity_place(plane, R, g, leon::activity_b(e), &mx, &my, &j);
                    if (a == 0u || mx >= G.mbw) continue;
                    const size_t k = (size_t)my * G.mbw + mx;
                    if (leon::activity_is_dc(e)) sums[2 * (size_t)L.mbs + k] += a;
                    else { sums[k] += 1; sums[(size_t)L.mbs + k] += a; }
                    blocks[k] |= (uint8_t)(1u << j);
                }
            }
    }
    uint8_t* rec = static_cast<uint8_t*>(record);
    uint32_t s[8] = {};
    for (size_t k = 0; k < L.mbs; k++) {
        uint32_t cell[2];
        leon::activity_cell(sums[k], sums[(size_t)L.mbs + k], sums[2 * (size_t)L.mbs + k], blocks[k], qscale[k], &cell[0], &cell[1]);
        leon::activity_count(cell[0], cell[1], s);
        memcpy(rec + 8 * k, cell, 8);
    }
    memcpy(rec + L.summary_offset, s, 32);
    return LEON_OK;
}

int activity_layout_host(int32_t mbw, int32_t mbh, struct leon_pipeline_activity_layout* out)
{
    if (!out) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = mb_grid_check("activity layout", mbw, mbh); rc != LEON_OK) return rc;
    const leon::ActivityLayout L = leon::activity_layout((uint32_t)mbw, (uint32_t)mbh);
    memset(out, 0, sizeof(*out));
    out->mb_width = mbw; out->mb_height = mbh; out->mbs = (int32_t)L.mbs;
    out->summary_offset = L.summary_offset; out->record_bytes = L.record_bytes; out->record_pitch = L.record_pitch;
    return LEON_OK;
}

// both kernels on lists the caller supplies (leon_pipeline_activity_kernel): every array padded as MapLayout pads it (gpad,
// entries_pad, mpad)
int activity_kernel(int32_t device_id, int32_t mbw, int32_t mbh, const leon_pipeline_activity_picture* pics, int32_t n_pics, const leon_pipeline_motion_kernel_frame* frames,
                    int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring)
{
    const leon::ActivityGeom G = leon::activity_geom((uint32_t)mbw, (uint32_t)mbh);
    const size_t n_off = (size_t)G.n_y + 2 * (size_t)G.n_c + 1;
    const MapLayout M = map_layout((size_t)mbw * (size_t)mbh, n_off - 1);
    const leon::ActivityLayout L = leon::activity_layout((uint32_t)mbw, (uint32_t)mbh);
    return record_kernel<leon::ActivityDesc>("activity kernel", device_id, mbw, mbh, pics, n_pics, frames, n_frames, ring_frames, pad_byte, ring, L.record_pitch,
        [&](int32_t i, const leon_pipeline_activity_picture& q, size_t* bytes) {
            if (q.reserved0) return fail(LEON_ERR_INVALID, "activity kernel: a reserved word of picture %d is not 0", i);
            if (q.n_entries > (1u << 30)) return fail(LEON_ERR_INVALID, "activity kernel: picture %d has %u entries (at most 2^30)", i, q.n_entries);
            *bytes = M.gpad + MapLayout::entries_pad(q.n_entries) + M.mpad;
            return activity_lists_check("activity kernel", G, q.grp_off, q.entries, q.n_entries, q.qscale);
        },
        [&](const leon_pipeline_activity_picture& q, auto& place) {
            leon::ActivityDesc D{};
            D.grp_off = reinterpret_cast<const uint32_t*>(place(q.grp_off, n_off * 4, M.gpad));
            D.entries = reinterpret_cast<const uint32_t*>(place(q.entries, (size_t)q.n_entries * 4, MapLayout::entries_pad(q.n_entries)));
            D.qscale = place(q.qscale, M.mbs, M.mpad);
            D.n_entries = q.n_entries;
            return D;
        },
        [&](const leon::ActivityDesc* descs, size_t n, uint8_t* d_ring) { activity_launch(descs, n, d_ring, G, L, nullptr); });
}

// output RESIDUAL: the window's frames -> their residual records, k_residual on the decoder's stream behind k_activity and in front of
// the window's event, while the lists and maps are still in the GOPs' arenas.  The descriptors go up as k_motion's do.
static_assert(sizeof(leon::ResidualDesc) == 48, "a descriptor is 12 dwords");
static_assert(sizeof(struct leon_pipeline_residual_layout) == 64 && sizeof(leon_pipeline_residual_picture) == 56, "include/leon_pipeline.h states the sizes");
static_assert(sizeof(leon::ResidualGeom) == 32 && sizeof(leon::ResidualLayout) == 32, "kernel arguments");
// k_residual over n descriptors in device memory, frame i of them in workgroup row i: the one place that cuts them into launches
// (launch_residual for a window, residual_kernel for a caller's lists)
void residual_launch(const leon::ResidualDesc* descs, size_t n, uint8_t* ring, const leon::ResidualGeom& geom, const leon::ResidualLayout& lay, hipStream_t stream)
{
    const unsigned task_blocks = (geom.tasks + leon::kWavesPerWG - 1) / leon::kWavesPerWG;
    for (size_t at = 0; at < n; at += 65535) {
        const unsigned frames = (unsigned)std::min<size_t>(65535, n - at);
        hipLaunchKernelGGL(leon::k_residual, dim3(task_blocks, frames), dim3(leon::kRgbaBlock), 0, stream, descs + at, ring, geom, lay);
    }
}

int launch_residual(leon_pipeline* p, const PipeWindow* w)
{
    return launch_records(p, w, p->residual, w->residual_descs, [&](size_t i, const leon::ResidualDesc& d) {
        if (d.grp_off && d.entries && d.qscale && d.intra && d.qt) return (int)LEON_OK;
        return fail(LEON_ERR_INVALID, "residual: frame %zu of window %lld lacks its lists or a map", i, (long long)w->id);
    }, [&](const leon::ResidualDesc* dv, size_t n) { residual_launch(dv, n, p->residual.ring, p->residual_geom, p->residual_lay, p->dec->stream); });
}

// ACTIVITY's size rules on a coded size
int residual_size_check(const char* who, int32_t cw, int32_t ch)
{
    if (cw < 16 || ch < 16 || (cw & 15) || (ch & 15)) return fail(LEON_ERR_INVALID, "%s: a coded size of %d x %d (multiples of 16)", who, cw, ch);
    return mb_grid_check(who, cw / 16, ch / 16);
}

int residual_layout_host(int32_t cw, int32_t ch, struct leon_pipeline_residual_layout* out)
{
    if (!out) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = residual_size_check("residual layout", cw, ch); rc != LEON_OK) return rc;
    const leon::ResidualLayout L = leon::residual_layout((uint32_t)cw, (uint32_t)ch);
    memset(out, 0, sizeof(*out));
    out->coded_width = cw; out->coded_height = ch;
    out->luma_stride = (int32_t)L.luma_stride; out->chroma_stride = (int32_t)L.chroma_stride;
    out->cb_offset = L.cb_offset; out->cr_offset = L.cr_offset;
    out->record_bytes = L.record_bytes; out->record_pitch = L.record_pitch;
    return LEON_OK;
}

// k_residual on lists, maps and matrices the caller supplies (leon_pipeline_residual_kernel): every array padded as activity_kernel
// pads it, the intra map like qscale, the picture's QTables (fill_qtables: what the decoder builds its own with) in 256 bytes
int residual_kernel(int32_t device_id, int32_t cw, int32_t ch, const leon_pipeline_residual_picture* pics, int32_t n_pics, const leon_pipeline_motion_kernel_frame* frames,
                    int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring)
{
    if (const int rc = residual_size_check("residual kernel", cw, ch); rc != LEON_OK) return rc;
    const int32_t mbw = cw / 16, mbh = ch / 16;
    const leon::ResidualGeom G = leon::residual_geom((uint32_t)mbw, (uint32_t)mbh);
    const leon::ActivityGeom AG = leon::activity_geom((uint32_t)mbw, (uint32_t)mbh);
    const size_t n_off = (size_t)G.n_y + 2 * (size_t)G.n_c + 1;
    const MapLayout M = map_layout((size_t)mbw * (size_t)mbh, n_off - 1);
    const leon::ResidualLayout L = leon::residual_layout((uint32_t)cw, (uint32_t)ch);
    static_assert(sizeof(QTables) == 256, "a picture's tables take one padded piece");
    return record_kernel<leon::ResidualDesc>("residual kernel", device_id, mbw, mbh, pics, n_pics, frames, n_frames, ring_frames, pad_byte, ring, L.record_pitch,
        [&](int32_t i, const leon_pipeline_residual_picture& q, size_t* bytes) {
            if (q.reserved0) return fail(LEON_ERR_INVALID, "residual kernel: a reserved word of picture %d is not 0", i);
            if (q.n_entries > (1u << 29)) return fail(LEON_ERR_INVALID, "residual kernel: picture %d has %u entries (at most 2^29)", i, q.n_entries);
            if (!q.intra || !q.matrices || !q.premultiplier) return fail(LEON_ERR_INVALID, "residual kernel: picture %d lacks its intra map, matrices or premultiplier", i);
            *bytes = M.gpad + MapLayout::entries_pad(q.n_entries) + 2 * M.mpad + sizeof(QTables);
            return activity_lists_check("residual kernel", AG, q.grp_off, q.entries, q.n_entries, q.qscale);
        },
        [&](const leon_pipeline_residual_picture& q, auto& place) {
            leon::ResidualDesc D{};
            D.grp_off = reinterpret_cast<const uint32_t*>(place(q.grp_off, n_off * 4, M.gpad));
            D.entries = reinterpret_cast<const uint32_t*>(place(q.entries, (size_t)q.n_entries * 4, MapLayout::entries_pad(q.n_entries)));
            D.qscale = place(q.qscale, M.mbs, M.mpad);
            D.intra = place(q.intra, M.mbs, M.mpad);
            QTables qt;
            fill_qtables(qt, q.matrices, q.premultiplier);
            D.qt = reinterpret_cast<const QTables*>(place(&qt, sizeof(qt), sizeof(qt)));
            D.n_entries = q.n_entries;
            return D;
        },
        [&](const leon::ResidualDesc* descs, size_t n, uint8_t* d_ring) { residual_launch(descs, n, d_ring, G, L, nullptr); });
}

// ---- regions of delivered frames as a tensor batch (leon_pipeline_resample_regions) ------------------------------------
typedef void (*RegionsKernel)(const uint8_t*, uint8_t*, const leon::RegionDesc*, const uint32_t*, const leon::Tables*, const int32_t*, leon::ResampleGeom);
struct RegionsKernelsOfFilter { RegionsKernel k[3][2]; };
template <class F> constexpr RegionsKernelsOfFilter kRegionsKernelsOf = {{{leon::k_regions<1, leon::kLayoutChw, F>, leon::k_regions<1, leon::kLayoutHwc, F>},
                                                                          {leon::k_regions<2, leon::kLayoutChw, F>, leon::k_regions<2, leon::kLayoutHwc, F>},
                                                                          {leon::k_regions<4, leon::kLayoutChw, F>, leon::k_regions<4, leon::kLayoutHwc, F>}}};
constexpr RegionsKernelsOfFilter kRegionsKernels[4] = {kRegionsKernelsOf<leon::ResTriangle>, {}, {}, kRegionsKernelsOf<leon::ResCubic>};
static_assert(sizeof(leon::RegionDesc) == 64, "a descriptor is 16 dwords");
static_assert(sizeof(leon_pipeline_region) == 32 && sizeof(leon_pipeline_regions_config) == 32, "include/leon_pipeline.h states the sizes");

// ... and k_fitted where every region is letterboxed into the call's out size (leon_pipeline_regions_fit), on both roads
typedef void (*FittedKernel)(const uint8_t*, uint8_t*, const leon::RegionDesc*, const uint32_t*, const leon::Tables*, const int32_t*, leon::ResampleGeom, uint32_t);
struct FittedKernelsOfFilter { FittedKernel k[3][2]; };
template <class F> constexpr FittedKernelsOfFilter kFittedKernelsOf = {{{leon::k_fitted<1, leon::kLayoutChw, F>, leon::k_fitted<1, leon::kLayoutHwc, F>},
                                                                        {leon::k_fitted<2, leon::kLayoutChw, F>, leon::k_fitted<2, leon::kLayoutHwc, F>},
                                                                        {leon::k_fitted<4, leon::kLayoutChw, F>, leon::k_fitted<4, leon::kLayoutHwc, F>}}};
constexpr FittedKernelsOfFilter kFittedKernels[4] = {kFittedKernelsOf<leon::ResTriangle>, {}, {}, kFittedKernelsOf<leon::ResCubic>};
// the pad's workgroup rows behind the canvas's tile rows: whole rows of gx workgroups that cover every 16-byte line of a region's
// tensor, kPadLinesPerGroup each (launch_tensors' rule; here always, since a call's regions differ in what they pad)
unsigned fitted_pad_rows(size_t region_bytes, unsigned gx)
{
    const size_t lines = (region_bytes + 15) / 16, groups = (lines + leon::kPadLinesPerGroup - 1) / leon::kPadLinesPerGroup;
    return (unsigned)((groups + gx - 1) / gx);
}

struct RegionTaps { int32_t x, y; };       // the largest tap count of a region's columns and rows

// what a call's config, window and n can be refused for, whichever memory the regions lie in
int regions_config_check(int32_t fw, int32_t fh, int32_t n_frames, int32_t n, const leon_pipeline_regions_config* cfg)
{
    for (int i = 0; i < 5; i++)
        if (cfg->reserved[i]) return fail(LEON_ERR_INVALID, "regions config: reserved word %d is %d, not 0", i, cfg->reserved[i]);
    if (cfg->out_width < 1 || cfg->out_width > 4096) return fail(LEON_ERR_INVALID, "regions config: out_width %d is outside 1 .. 4096", cfg->out_width);
    if (cfg->out_height < 1 || cfg->out_height > 4096) return fail(LEON_ERR_INVALID, "regions config: out_height %d is outside 1 .. 4096", cfg->out_height);
    if (!resize_filter_max_taps(cfg->filter)) return fail(LEON_ERR_INVALID, "regions config: filter %d (LEON_RESIZE_TRIANGLE and LEON_RESIZE_BICUBIC are the filters)", cfg->filter);
    if (fw < 1 || fh < 1 || n_frames < 0) return fail(LEON_ERR_INVALID, "regions: %d frames of %d x %d", n_frames, fw, fh);
    return record_count_check("regions", "regions", n);
}

// The fit of a call as the kernels take it (leon_pipeline_regions_fit); every refusal of the settings is in regions_fit_check
struct RegionsFit {
    bool letterbox = false, top_left = false;
    uint32_t pad = 0;                    // R, G, B in bits 0, 8, 16 (CanvasGeom::pad)
};
static_assert(sizeof(leon_pipeline_regions_fit) == 32, "include/leon_pipeline.h states the size");
int regions_fit_check(const leon_pipeline_regions_fit* f, RegionsFit* out)
{
    *out = RegionsFit{};
    if (!f) return LEON_OK;
    for (int i = 0; i < 3; i++)
        if (f->reserved[i]) return fail(LEON_ERR_INVALID, "regions fit: reserved word %d is %d, not 0", i, f->reserved[i]);
    if (f->mode != LEON_REGIONS_FIT_STRETCH && f->mode != LEON_REGIONS_FIT_LETTERBOX) return fail(LEON_ERR_INVALID, "regions fit: mode %d", f->mode);
    if (f->anchor != LEON_REGIONS_ANCHOR_CENTRE && f->anchor != LEON_REGIONS_ANCHOR_TOP_LEFT) return fail(LEON_ERR_INVALID, "regions fit: anchor %d", f->anchor);
    for (int i = 0; i < 3; i++)
        if (f->pad[i] < 0 || f->pad[i] > 255) return fail(LEON_ERR_INVALID, "regions fit: pad value %d is %d, outside 0 .. 255", i, f->pad[i]);
    if (f->mode == LEON_REGIONS_FIT_STRETCH && (f->anchor | f->pad[0] | f->pad[1] | f->pad[2]))
        return fail(LEON_ERR_INVALID, "regions fit: an anchor or a pad value with LEON_REGIONS_FIT_STRETCH, which has neither");
    out->letterbox = f->mode == LEON_REGIONS_FIT_LETTERBOX;
    out->top_left = f->anchor == LEON_REGIONS_ANCHOR_TOP_LEFT;
    out->pad = (uint32_t)f->pad[0] | ((uint32_t)f->pad[1] << 8) | ((uint32_t)f->pad[2] << 16);
    return LEON_OK;
}
// a region's image in its tensor: the tensor itself when stretched, else the letterbox of its box (leon_resize_row.h, the device's text too)
leon::FitRect region_image(const leon_pipeline_region& r, const leon_pipeline_regions_config& cfg, const RegionsFit& fit)
{
    if (!fit.letterbox) return leon::FitRect{cfg.out_width, cfg.out_height, 0, 0};
    return leon::region_fit_rect(r.width, r.height, cfg.out_width, cfg.out_height, fit.top_left);
}

// Every refusal that needs no device is here (leon_pipeline_regions_check is this function); taps: per region, for the table layout
int regions_check(int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_region* regions, int32_t n, const leon_pipeline_regions_config* cfg,
                  const RegionsFit& fit, int32_t* bad, std::vector<RegionTaps>* taps)
{
    if (bad) *bad = -1;
    if (!regions || !cfg) return fail(LEON_ERR_INVALID, "null argument");
    const int crc = regions_config_check(fw, fh, n_frames, n, cfg);
    if (crc != LEON_OK) return crc;
    if (taps) taps->resize((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const leon_pipeline_region& r = regions[i];
        if (bad) *bad = i;
        for (int k = 0; k < 3; k++)
            if (r.reserved[k]) return fail(LEON_ERR_INVALID, "region %d: reserved word %d is %d, not 0", i, k, r.reserved[k]);
        if (r.frame < 0 || r.frame >= n_frames) return fail(LEON_ERR_INVALID, "region %d: frame %d is outside the window's %d frames", i, r.frame, n_frames);
        // a call that goes on to build the tables (taps != NULL) needs the row lengths only: the weights are judged when they are built
        RegionTaps t{};
        const leon::FitRect image = region_image(r, *cfg, fit);          // (the limits are judged on the region's own out size)
        if (taps) {
            t.x = resize_axis_taps(fw, r.x, r.width, image.ow, cfg->filter);
            t.y = resize_axis_taps(fh, r.y, r.height, image.oh, cfg->filter);
        }
        int rc = LEON_OK;
        if ((!t.x && (rc = resize_axis_build("width", fw, r.x, r.width, image.ow, cfg->filter, nullptr, nullptr, nullptr, LEON_RESIZE_MAX_TAPS_BICUBIC, &t.x)) != LEON_OK) ||
            (!t.y && (rc = resize_axis_build("height", fh, r.y, r.height, image.oh, cfg->filter, nullptr, nullptr, nullptr, LEON_RESIZE_MAX_TAPS_BICUBIC, &t.y)) != LEON_OK)) {
            const std::string why = g_err;
            return fail(rc, "region %d: %s", i, why.c_str());
        }
        if (taps) (*taps)[(size_t)i] = t;
    }
    if (bad) *bad = -1;
    return LEON_OK;
}

// the host roads' scratch (regions_mu held; the regions stream is idle between calls): each buffer grown to half again what is
// asked and never shrunk
int regions_reserve(leon_pipeline* p, size_t upload_bytes, size_t out_bytes)
{
    const auto cap = [](size_t bytes) { return cap_for(bytes, Grow::Half, (size_t)1 << 20); };
    const auto no = [](size_t bytes, const char* what) { (void)hipGetLastError(); return fail(LEON_ERR_NOMEM, "regions: %zu bytes %s", bytes, what); };
    if (!p->regions_host.reserve(upload_bytes, cap(upload_bytes))) return no(cap(upload_bytes), "of pinned staging");
    if (!p->regions_dev.reserve(upload_bytes, cap(upload_bytes), 0, kBigCaller)) return no(cap(upload_bytes), "of device scratch");
    if (!p->regions_out.reserve(out_bytes, cap(out_bytes), 0, kBigCaller)) return no(cap(out_bytes), "for the tensors");
    return LEON_OK;
}

// fn(w) on a window that is out for delivery and was delivered whole: the one lookup of the region, carry and propagate calls
template <class Fn>
int window_delivered(leon_pipeline* p, int64_t window, Fn fn)
{
    int status = LEON_OK;
    const bool out = p->flow.with_delivered(window, [&](const PipeWindow& w) {
        if ((status = w.status) == LEON_OK) fn(w);
    });
    if (!out) return fail(LEON_ERR_INVALID, "window %lld is not out for delivery", (long long)window);
    if (status != LEON_OK) return fail(LEON_ERR_INVALID, "window %lld was delivered with an error (status %d)", (long long)window, status);
    return LEON_OK;
}
// the ring ids of a delivered window's frames
int regions_window_ids(leon_pipeline* p, int64_t window, std::vector<uint32_t>* ids)
{
    return window_delivered(p, window, [&](const PipeWindow& w) {
        const uint32_t base = (uint32_t)((size_t)w.ring * p->W * p->max_pics);
        ids->reserve(w.frame_ids.size());
        for (uint32_t id : w.frame_ids) ids->push_back(base + id);
    });
}
// ... and its table of ring ids and references, as k_carry and k_propagate take it
int carry_window_table(leon_pipeline* p, int64_t window, std::vector<uint32_t>* table)
{
    return window_delivered(p, window, [&](const PipeWindow& w) { *table = w.carry_table; });
}

// ---- what the four roads share (stretch / fit and warp, each from host records and from device records) --------------------------
// the pipeline of a call: one with tensors, of an element size and layout the kernel tables list (create admits no other)
int regions_pipeline_check(const leon_pipeline* p)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    if (!(p->output & LEON_PIPELINE_OUTPUT_TENSOR) || !p->d_tensor || !p->d_planes)
        return no_output("tensor", "TENSOR");
    const int eb = (int)p->tensor_elem, layout = p->tensor_layout;
    if (!((eb == 1 || eb == 2 || eb == 4) && (layout == leon::kLayoutChw || layout == leon::kLayoutHwc)))
        return fail(LEON_ERR_INVALID, "regions: no kernel for %d-byte elements, layout %d", eb, layout);
    return LEON_OK;
}
// ... and its kernel of a family, by filter (the config checks admit the two that have kernels), element bytes and layout
template <class T> auto regions_kernel(const T (&family)[4], const leon_pipeline* p, int32_t filter) { return family[filter].k[p->tensor_elem >> 1][p->tensor_layout]; }

// the caller's buffer; *pitch: the bytes from one region's tensor to the next
int regions_out_check(const char* who, const void* device_out, uint64_t out_pitch, size_t region_bytes, uint64_t* pitch)
{
    if (!device_out) return fail(LEON_ERR_INVALID, "%s: null device_out", who);
    if ((uintptr_t)device_out & 255u) return fail(LEON_ERR_INVALID, "%s: device_out %p is not 256-byte aligned", who, device_out);
    if (out_pitch && (out_pitch % 256 || out_pitch < region_bytes))
        return fail(LEON_ERR_INVALID, "%s: out_pitch_bytes %llu (0, or a multiple of 256 not below the region's %zu bytes)", who, (unsigned long long)out_pitch, region_bytes);
    *pitch = out_pitch ? out_pitch : (uint64_t)pad256(region_bytes);
    return LEON_OK;
}

// the stream a call enqueues on: the caller's, or (NULL) the pipeline's regions stream, made at first use
int regions_call_stream(leon_pipeline* p, void* caller_stream, hipStream_t* st)
{
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    if (!caller_stream && !p->regions_stream && !p->regions_stream.create(hipStreamNonBlocking)) return refused(LEON_ERR_HIP, "regions stream");
    *st = caller_stream ? static_cast<hipStream_t>(caller_stream) : p->regions_stream.get();
    return LEON_OK;
}

// The tail of a host road, all on the regions stream `st`: the staging uploaded, the road's launch, the tensors packed to `host` when
// they went into the pooled scratch, the wait.  launch(out) enqueues on `st` and returns nothing: its error is asked here.
template <class Launch>
int regions_host_run(leon_pipeline* p, hipStream_t st, size_t upload_bytes, void* host, void* device_out, size_t pitch, size_t region_bytes, int32_t n, Launch launch)
{
    uint8_t* out = host ? p->regions_out.get() : static_cast<uint8_t*>(device_out);
    HIP_TRY(hipMemcpyAsync(p->regions_dev, p->regions_host, upload_bytes, hipMemcpyHostToDevice, st));
    launch(out);
    HIP_TRY(hipGetLastError());
    if (host) HIP_TRY(hipMemcpy2DAsync(host, region_bytes, out, pitch, region_bytes, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LEON_OK;
}

// the grid of m regions: the out size's tiles and, letterboxed, the pad's rows behind them
dim3 regions_grid(int32_t ow, int32_t oh, size_t region_bytes, bool letterbox, unsigned m)
{
    const unsigned gx = (unsigned)((ow + leon::kResTileX - 1) / leon::kResTileX), gy = (unsigned)((oh + leon::kResTileY - 1) / leon::kResTileY);
    return dim3(gx, letterbox ? gy + fitted_pad_rows(region_bytes, gx) : gy, m);
}
// the launch both roads share: descriptors and the tables they point into, in device memory -- k_regions, letterboxed k_fitted
void regions_launch(leon_pipeline* p, hipStream_t st, const RegionsFit& fit, int32_t filter, const leon::ResampleGeom& G, dim3 grid, uint8_t* out,
                    const leon::RegionDesc* d_descs, const int32_t* d_tabs)
{
    const dim3 block(leon::kRgbaBlock);
    if (fit.letterbox)
        hipLaunchKernelGGL(regions_kernel(kFittedKernels, p, filter), grid, block, 0, st, (const uint8_t*)p->d_planes, out, d_descs, (const uint32_t*)p->d_tensor_table,
                           (const leon::Tables*)p->dec->d_tables, d_tabs, G, fit.pad);
    else
        hipLaunchKernelGGL(regions_kernel(kRegionsKernels, p, filter), grid, block, 0, st, (const uint8_t*)p->d_planes, out, d_descs, (const uint32_t*)p->d_tensor_table,
                           (const leon::Tables*)p->dec->d_tables, d_tabs, G);
}

// One call: refusals, the regions' descriptors and tables into pinned staging, then regions_host_run.  device_out NULL with `host`:
// into the pooled scratch at the default pitch, then packed to the host.
int resample_regions(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n, const leon_pipeline_regions_config* cfg,
                     const leon_pipeline_regions_fit* fit_settings, void* device_out, uint64_t out_pitch, void* host)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    RegionsFit fit;
    int rc = regions_fit_check(fit_settings, &fit);
    if (rc != LEON_OK || (rc = regions_pipeline_check(p)) != LEON_OK) return rc;
    std::lock_guard<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> ids;
    if ((rc = regions_window_ids(p, window, &ids)) != LEON_OK) return rc;
    std::vector<RegionTaps> taps;
    const int32_t fw = p->vinfo.frame_width, fh = p->vinfo.frame_height;
    if ((rc = regions_check(fw, fh, (int32_t)ids.size(), regions, n, cfg, fit, nullptr, &taps)) != LEON_OK) return rc;
    const int32_t ow = cfg->out_width, oh = cfg->out_height, filter = cfg->filter;
    const size_t region_bytes = (size_t)3 * oh * ow * p->tensor_elem;
    uint64_t pitch = pad256(region_bytes);
    if (!host && (rc = regions_out_check("regions", device_out, out_pitch, region_bytes, &pitch)) != LEON_OK) return rc;

    // [descriptors | tables]: a region's tables as plan_resize lays out a pipeline's, rows of its own tap counts -- and, letterboxed,
    // of its own image size
    const size_t desc_bytes = pad256((size_t)n * sizeof(leon::RegionDesc));
    leon::ResampleGeom G{};
    G.fw = fw; G.fh = fh; G.ow = ow; G.oh = oh;
    G.ring = ring_geom(p);
    size_t words = 0;
    for (int32_t i = 0; i < n; i++) {
        const leon::FitRect image = region_image(regions[i], *cfg, fit);
        leon::ResampleGeom R;
        words += resize_tables_layout(image.ow, image.oh, taps[(size_t)i].x | 1, taps[(size_t)i].y, &R);          // (odd rows of Wx: plan_resize says why)
    }
    if (words >= ((size_t)1 << 32)) return fail(LEON_ERR_INVALID, "regions: the tables of %d regions take %zu bytes (4 GiB a call at most)", n, words * 4);
    const size_t upload_bytes = desc_bytes + words * 4;
    hipStream_t st;
    if ((rc = regions_call_stream(p, nullptr, &st)) != LEON_OK || (rc = regions_reserve(p, upload_bytes, host ? (size_t)n * pitch : 0)) != LEON_OK) return rc;
    leon::RegionDesc* descs = reinterpret_cast<leon::RegionDesc*>(p->regions_host.get());
    int32_t* tabs = reinterpret_cast<int32_t*>(p->regions_host + desc_bytes);
    size_t at = 0;
    for (int32_t i = 0; i < n; i++) {
        const leon_pipeline_region& r = regions[i];
        const leon::FitRect image = region_image(r, *cfg, fit);
        leon::ResampleGeom R = G;
        R.ow = image.ow; R.oh = image.oh;
        const size_t region_words = resize_tables_layout(image.ow, image.oh, taps[(size_t)i].x | 1, taps[(size_t)i].y, &R);
        int32_t* t = tabs + at;
        if ((rc = resize_axis_build("width", fw, r.x, r.width, image.ow, filter, t, t + R.off_cx, t + R.off_wx, R.taps_x, nullptr)) != LEON_OK ||
            (rc = resize_axis_build("height", fh, r.y, r.height, image.oh, filter, t + R.off_fy, t + R.off_cy, t + R.off_wy, R.taps_y, nullptr)) != LEON_OK ||
            (rc = resize_footprint_check(t, R, filter)) != LEON_OK) {
            const std::string why = g_err;
            return fail(rc, "region %d: %s", i, why.c_str());
        }
        leon::RegionDesc d{};          // (status 0: kRegionOk)
        d.frame_id = ids[(size_t)r.frame];
        d.rt_base = (uint32_t)at;
        d.off_cx = R.off_cx; d.off_wx = R.off_wx; d.off_fy = R.off_fy; d.off_cy = R.off_cy; d.off_wy = R.off_wy;
        d.taps_x = R.taps_x; d.taps_y = R.taps_y;
        const uint64_t dst = (uint64_t)i * pitch;
        d.dst_lo = (uint32_t)(dst & 0xffffffffu); d.dst_hi = (uint32_t)(dst >> 32);
        if (fit.letterbox) { d.iw = image.ow; d.ih = image.oh; d.ix = image.x; d.iy = image.y; }
        descs[i] = d;
        at += region_words;
    }
    const dim3 grid = regions_grid(ow, oh, region_bytes, fit.letterbox, (unsigned)n);          // (blockIdx.z; one launch: n <= 65535)
    if (grid.y > 65535u) return fail(LEON_ERR_INVALID, "regions fit: %u workgroup rows", grid.y);
    return regions_host_run(p, st, upload_bytes, host, device_out, (size_t)pitch, region_bytes, n, [&](uint8_t* out) {
        regions_launch(p, st, fit, filter, G, grid, out, reinterpret_cast<const leon::RegionDesc*>(p->regions_dev.get()), reinterpret_cast<const int32_t*>(p->regions_dev + desc_bytes));
    });
}

// ---- regions whose boxes lie in device memory (leon_pipeline_resample_regions_device) -----------------------------------
static_assert(sizeof(leon::BoxRecord) == sizeof(leon_pipeline_region) && sizeof(leon_pipeline_regions_device) == 64, "include/leon_pipeline.h states the sizes");
static_assert(leon::kRegionOk == LEON_REGION_OK && leon::kRegionReserved == LEON_REGION_RESERVED && leon::kRegionFrame == LEON_REGION_FRAME &&
              leon::kRegionBox == LEON_REGION_BOX && leon::kRegionRatioX == LEON_REGION_RATIO_X && leon::kRegionRatioY == LEON_REGION_RATIO_Y &&
              leon::kRegionTaps == LEON_REGION_TAPS, "the kernels' codes are the header's");
static_assert(leon::kResizeMaxTapsTriangle == LEON_RESIZE_MAX_TAPS && leon::kResizeMaxTapsCubic == LEON_RESIZE_MAX_TAPS_BICUBIC, "one limit");

// int32 words of a region's table slot: the layout at the filter's worst case for the out size (rows of Wx are an odd number of words: both maxima are odd)
size_t boxes_slot_words(int32_t ow, int32_t oh, int32_t filter)
{
    leon::ResampleGeom worst;
    return resize_tables_layout(ow, oh, resize_filter_max_taps(filter), resize_filter_max_taps(filter), &worst);
}

// The CPU twin of k_box_tables' judgement: the same functions of leon_resize_row.h in the same order
int32_t region_status(int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_region& r, const leon_pipeline_regions_config& cfg, const RegionsFit& fit)
{
    if (r.reserved[0] | r.reserved[1] | r.reserved[2]) return LEON_REGION_RESERVED;
    if (r.frame < 0 || r.frame >= n_frames) return LEON_REGION_FRAME;
    const bool cubic = cfg.filter == LEON_RESIZE_BICUBIC;
    const leon::FitRect image = region_image(r, cfg, fit);
    const int32_t in[2] = {fw, fh}, start[2] = {r.x, r.y}, size[2] = {r.width, r.height}, out[2] = {image.ow, image.oh};
    const int32_t ratio[2] = {LEON_REGION_RATIO_X, LEON_REGION_RATIO_Y};
    for (int a = 0; a < 2; a++) {
        const int32_t s = leon::region_axis_status(in[a], start[a], size[a], out[a], ratio[a]);
        if (s) return s;
        const leon::ResizeAxis A = leon::resize_axis(in[a], start[a], size[a], out[a], cubic);
        for (int32_t o = 0; o < out[a]; o++)
            if (!leon::resize_row_count_ok(leon::resize_row_window(A, o).n, cubic)) return LEON_REGION_TAPS;
    }
    return LEON_REGION_OK;
}

// the chunk's scratch, grown and never shrunk (regions_mu held): nothing of an earlier call may still run in the old one
int boxes_reserve(leon_pipeline* p, size_t bytes)
{
    if (bytes <= p->boxes_dev.bytes()) return LEON_OK;
    if (p->boxes_busy) { HIP_TRY(hipEventSynchronize(p->boxes_done)); p->boxes_busy = false; }
    const size_t cap = cap_for(bytes, Grow::Exact, (size_t)1 << 20);
    if (!p->boxes_dev.reserve(bytes, cap, 0, kBigCaller)) { (void)hipGetLastError(); return fail(LEON_ERR_NOMEM, "regions: %zu bytes of device scratch", cap); }
    return LEON_OK;
}

// the window's frame ids into a pinned staging entry whose last upload has run (four calls back: as good as always); regions_mu held.
// The entry is (boxes_ids_next - 1) % kBoxesStaging afterwards: the caller records its event behind the upload.
int boxes_ids_stage(leon_pipeline* p, const std::vector<uint32_t>& ids, uint32_t** host)
{
    const unsigned e = p->boxes_ids_next++ % leon_pipeline::kBoxesStaging;
    if (p->boxes_ids_busy[e]) { HIP_TRY(hipEventSynchronize(p->boxes_ids_done[e])); p->boxes_ids_busy[e] = false; }
    if (!p->boxes_ids_done[e] && !p->boxes_ids_done[e].create(hipEventDisableTiming)) return refused(LEON_ERR_HIP, "hipEventCreate");
    const size_t cap = cap_for(ids.size(), Grow::Twice, 1024) * 4;
    if (!p->boxes_ids_host[e].reserve(ids.size() * 4, cap)) { (void)hipGetLastError(); return fail(LEON_ERR_NOMEM, "regions: %zu bytes of pinned staging", cap); }
    std::copy(ids.begin(), ids.end(), p->boxes_ids_host[e].get());
    *host = p->boxes_ids_host[e];
    return LEON_OK;
}

// what the two device roads' call structs share (leon_pipeline_regions_device, leon_pipeline_warp_regions_call); *pitch as regions_out_check's
int boxes_call_check(const char* who, const void* regions, bool reserved_set, const int32_t* device_status, const void* device_out, uint64_t out_pitch,
                     size_t region_bytes, uint64_t* pitch)
{
    if (reserved_set) return fail(LEON_ERR_INVALID, "%s: a reserved word of the call is not 0", who);
    if (!regions) return fail(LEON_ERR_INVALID, "%s: null regions", who);
    if ((uintptr_t)regions & 3u) return fail(LEON_ERR_INVALID, "%s: regions %p is not 4-byte aligned", who, regions);
    if ((uintptr_t)device_status & 3u) return fail(LEON_ERR_INVALID, "%s: device_status %p is not 4-byte aligned", who, (const void*)device_status);
    return regions_out_check(who, device_out, out_pitch, region_bytes, pitch);
}

// The bracket of a device road's enqueue, regions_mu held in `call`: on the caller's stream, or (NULL) on the regions stream with a wait at
// the end.  The scratch (boxes_dev) at `scratch_bytes` or more, the stream behind the call before's use of it (boxes_done), `table` -- the
// window's frame ids, or its carry table -- uploaded to the scratch's start with the staging entry's event recorded behind the upload; then
// launch(st, d_table), which only enqueues, while nothing has failed, and the runtime's last error folded in.  From the upload on the stream
// holds work, so whatever failed since, boxes_done is recorded to keep the scratch covered; the lock is dropped (regions_mu is held while
// enqueuing only); then the road's error, and the wait.
template <class Launch>
int boxes_run(leon_pipeline* p, void* caller_stream, std::unique_lock<std::mutex>& call, const std::vector<uint32_t>& table, size_t scratch_bytes, Launch launch)
{
    int rc;
    hipStream_t st;
    if ((rc = regions_call_stream(p, caller_stream, &st)) != LEON_OK) return rc;
    if (!p->boxes_done && !p->boxes_done.create(hipEventDisableTiming)) return refused(LEON_ERR_HIP, "hipEventCreate");
    if ((rc = boxes_reserve(p, scratch_bytes)) != LEON_OK) return rc;
    uint32_t* table_host = nullptr;
    if ((rc = boxes_ids_stage(p, table, &table_host)) != LEON_OK) return rc;
    const unsigned e = (p->boxes_ids_next - 1) % leon_pipeline::kBoxesStaging;
    if (p->boxes_busy) HIP_TRY(hipStreamWaitEvent(st, p->boxes_done, 0));
    uint32_t* d_table = reinterpret_cast<uint32_t*>(p->boxes_dev.get());
    hipError_t he = hipMemcpyAsync(d_table, table_host, table.size() * 4, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && (he = hipEventRecord(p->boxes_ids_done[e], st)) == hipSuccess) p->boxes_ids_busy[e] = true;
    if (he == hipSuccess) {
        launch(st, d_table);
        he = hipGetLastError();
    }
    if (hipEventRecord(p->boxes_done, st) == hipSuccess) p->boxes_busy = true;
    else if (he == hipSuccess) he = hipGetLastError();
    call.unlock();
    HIP_TRY(he);
    if (!caller_stream) HIP_TRY(hipStreamSynchronize(st));
    return LEON_OK;
}

// One call: the host's refusals, then inside the bracket per chunk k_box_tables and k_regions (letterboxed: k_fit_tables and k_fitted) on the
// caller's stream (or the pipeline's regions stream and a wait)
int resample_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit_settings,
                            const leon_pipeline_regions_device* c, int32_t* device_rects)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    if (!cfg || !c) return fail(LEON_ERR_INVALID, "null argument");
    RegionsFit fit;
    int rc = regions_fit_check(fit_settings, &fit);
    if (rc != LEON_OK) return rc;
    if (device_rects && !fit.letterbox) return fail(LEON_ERR_INVALID, "regions: device_rects without LEON_REGIONS_FIT_LETTERBOX (every region's rectangle is its tensor)");
    if ((uintptr_t)device_rects & 3u) return fail(LEON_ERR_INVALID, "regions: device_rects %p is not 4-byte aligned", (void*)device_rects);
    if ((rc = regions_pipeline_check(p)) != LEON_OK) return rc;
    std::unique_lock<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> ids;
    if ((rc = regions_window_ids(p, window, &ids)) != LEON_OK) return rc;
    const int32_t fw = p->vinfo.frame_width, fh = p->vinfo.frame_height, n = c->n;
    if ((rc = regions_config_check(fw, fh, (int32_t)ids.size(), n, cfg)) != LEON_OK) return rc;
    const int32_t ow = cfg->out_width, oh = cfg->out_height, filter = cfg->filter;
    const size_t region_bytes = (size_t)3 * oh * ow * p->tensor_elem;
    uint64_t pitch;
    if ((rc = boxes_call_check("regions", c->regions, c->reserved0 || c->reserved[0], c->device_status, c->device_out, c->out_pitch_bytes, region_bytes, &pitch)) != LEON_OK)
        return rc;
    // as many regions a chunk as fit the limit (and 32 bits of table words, which rt_base counts)
    const size_t slot_words = boxes_slot_words(ow, oh, filter), per_region = slot_words * 4 + sizeof(leon::RegionDesc);
    const uint64_t limit = c->scratch_limit_bytes ? c->scratch_limit_bytes : LEON_REGIONS_SCRATCH_DEFAULT;
    if (limit < per_region) return fail(LEON_ERR_INVALID, "regions: scratch_limit_bytes %llu is below one region's %zu bytes", (unsigned long long)limit, per_region);
    const size_t chunk = (size_t)std::min<uint64_t>({(uint64_t)n, limit / per_region, (((uint64_t)1 << 32) - 1) / slot_words});
    const size_t ids_bytes = pad256(ids.size() * 4), desc_bytes = pad256(chunk * sizeof(leon::RegionDesc));
    leon::ResampleGeom G{};
    G.fw = fw; G.fh = fh; G.ow = ow; G.oh = oh;
    G.ring = ring_geom(p);
    leon::BoxCall B{};
    B.fw = fw; B.fh = fh; B.ow = ow; B.oh = oh;
    B.n_frames = (int32_t)ids.size(); B.cubic = filter == LEON_RESIZE_BICUBIC;
    B.slot_words = (uint32_t)slot_words;
    B.pitch_lo = (uint32_t)(pitch & 0xffffffffu); B.pitch_hi = (uint32_t)(pitch >> 32);
    const leon::BoxRecord* boxes = reinterpret_cast<const leon::BoxRecord*>(c->regions);
    // the scratch: [frame ids | a chunk's descriptors | its tables]; the chunks in turn, none behind one whose launch failed
    return boxes_run(p, c->stream, call, ids, ids_bytes + desc_bytes + chunk * slot_words * 4, [&](hipStream_t st, uint32_t* d_ids) {
        leon::RegionDesc* d_descs = reinterpret_cast<leon::RegionDesc*>(p->boxes_dev + ids_bytes);
        int32_t* d_tabs = reinterpret_cast<int32_t*>(p->boxes_dev + ids_bytes + desc_bytes);
        for (size_t first = 0; first < (size_t)n; first += chunk) {
            const unsigned m = (unsigned)std::min(chunk, (size_t)n - first);          // (blockIdx.z: m <= n <= 65535; at most 512 tile rows and 96 pad rows)
            B.first = (uint32_t)first;
            int32_t* status = c->device_status ? c->device_status + first : nullptr;
            if (fit.letterbox)
                hipLaunchKernelGGL(leon::k_fit_tables, dim3(m), dim3(leon::kRgbaBlock), 0, st, boxes + first, (const uint32_t*)d_ids, d_descs, d_tabs, status,
                                   device_rects ? device_rects + first * 4 : nullptr, fit.top_left ? 1 : 0, B);
            else
                hipLaunchKernelGGL(leon::k_box_tables, dim3(m), dim3(leon::kRgbaBlock), 0, st, boxes + first, (const uint32_t*)d_ids, d_descs, d_tabs, status, B);
            regions_launch(p, st, fit, filter, G, regions_grid(ow, oh, region_bytes, fit.letterbox, m), static_cast<uint8_t*>(c->device_out), d_descs, d_tabs);
            if (hipPeekAtLastError() != hipSuccess) break;          // (boxes_run asks for it)
        }
    });
}

// ---- rotated boxes and affine crops (leon_pipeline_warp_regions) ---------------------------------------------------------------
typedef void (*WarpKernel)(const uint8_t*, uint8_t*, const leon::WarpRecord*, const uint32_t*, int32_t*, const uint32_t*, const leon::Tables*, leon::WarpCall);
constexpr WarpKernel kWarpKernels[3][2] = {{leon::k_warp<1, leon::kLayoutChw>, leon::k_warp<1, leon::kLayoutHwc>},
                                           {leon::k_warp<2, leon::kLayoutChw>, leon::k_warp<2, leon::kLayoutHwc>},
                                           {leon::k_warp<4, leon::kLayoutChw>, leon::k_warp<4, leon::kLayoutHwc>}};
static_assert(sizeof(leon_pipeline_warp_region) == 32 && sizeof(leon_pipeline_warp_config) == 32 && sizeof(leon_pipeline_warp_regions_call) == 64 &&
              sizeof(leon::WarpRecord) == sizeof(leon_pipeline_warp_region), "include/leon_pipeline.h states the sizes");
static_assert(leon::kRegionScale == LEON_REGION_SCALE && leon::kRegionOffset == LEON_REGION_OFFSET, "the kernels' codes are the header's");

// what a call's config, window and n can be refused for, whichever memory the records lie in; *pad: the pad pixel as the kernel takes it
int warp_config_check(int32_t fw, int32_t fh, int32_t n_frames, int32_t n, const leon_pipeline_warp_config* cfg, uint32_t* pad)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; i++)
        if (cfg->reserved[i]) return fail(LEON_ERR_INVALID, "warp config: reserved word %d is %d, not 0", i, cfg->reserved[i]);
    if (cfg->out_width < 1 || cfg->out_width > 4096) return fail(LEON_ERR_INVALID, "warp config: out_width %d is outside 1 .. 4096", cfg->out_width);
    if (cfg->out_height < 1 || cfg->out_height > 4096) return fail(LEON_ERR_INVALID, "warp config: out_height %d is outside 1 .. 4096", cfg->out_height);
    for (int i = 0; i < 3; i++)
        if (cfg->pad[i] < 0 || cfg->pad[i] > 255) return fail(LEON_ERR_INVALID, "warp config: pad value %d is %d, outside 0 .. 255", i, cfg->pad[i]);
    if (fw < 1 || fh < 1 || n_frames < 0) return fail(LEON_ERR_INVALID, "warp regions: %d frames of %d x %d", n_frames, fw, fh);
    if (const int rc = record_count_check("warp regions", "regions", n); rc != LEON_OK) return rc;
    if (pad) *pad = (uint32_t)cfg->pad[0] | ((uint32_t)cfg->pad[1] << 8) | ((uint32_t)cfg->pad[2] << 16);
    return LEON_OK;
}

inline const leon::WarpRecord& warp_record(const leon_pipeline_warp_region& r) { return reinterpret_cast<const leon::WarpRecord&>(r); }

// Every refusal that needs no device (leon_pipeline_warp_regions_check is this function): the kernel's judgement, named
int warp_regions_check(int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_warp_region* regions, int32_t n, const leon_pipeline_warp_config* cfg,
                       int32_t* bad, uint32_t* pad)
{
    if (bad) *bad = -1;
    if (!regions || !cfg) return fail(LEON_ERR_INVALID, "null argument");
    const int crc = warp_config_check(fw, fh, n_frames, n, cfg, pad);
    if (crc != LEON_OK) return crc;
    for (int32_t i = 0; i < n; i++) {
        const leon_pipeline_warp_region& r = regions[i];
        int32_t g;
        const int32_t status = leon::warp_record_status(warp_record(r), n_frames, &g);
        if (status == LEON_REGION_OK) continue;
        if (bad) *bad = i;
        switch (status) {
        case LEON_REGION_RESERVED: return fail(LEON_ERR_INVALID, "region %d: the reserved word is %d, not 0", i, r.reserved);
        case LEON_REGION_FRAME: return fail(LEON_ERR_INVALID, "region %d: frame %d is outside the window's %d frames", i, r.frame, n_frames);
        case LEON_REGION_SCALE: return fail(LEON_ERR_INVALID, "region %d: the matrix (%d %d / %d %d, Q16) reduces by more than 4", i, r.m[0], r.m[1], r.m[3], r.m[4]);
        default: return fail(LEON_ERR_INVALID, "region %d: offset (%d, %d) is outside +-2^29 (Q16)", i, r.m[2], r.m[5]);
        }
    }
    return LEON_OK;
}

int warp_quantise(const double* A, int32_t* m)
{
    if (!A || !m) return fail(LEON_ERR_INVALID, "null argument");
    int32_t q[6];
    for (int k = 0; k < 6; k++) {
        if (!std::isfinite(A[k])) return fail(LEON_ERR_INVALID, "warp matrix: entry %d is not finite", k);
        const double v = std::floor(A[k] * 65536.0 + 0.5);
        if (v < -2147483648.0 || v > 2147483647.0) return fail(LEON_ERR_INVALID, "warp matrix: entry %d (%g) is outside Q16 in 32 bits", k, A[k]);
        q[k] = (int32_t)v;
    }
    for (int k = 0; k < 6; k++) m[k] = q[k];
    return LEON_OK;
}

// the launch both roads share: records and frame ids in device memory
void warp_launch(leon_pipeline* p, hipStream_t st, const leon::WarpRecord* d_recs, const uint32_t* d_ids, int32_t n_frames, int32_t n, const leon_pipeline_warp_config& cfg,
                 uint32_t pad, uint8_t* out, uint64_t pitch, int32_t* d_status)
{
    leon::WarpCall C{};
    C.fw = p->vinfo.frame_width; C.fh = p->vinfo.frame_height; C.ow = cfg.out_width; C.oh = cfg.out_height;
    C.n_frames = n_frames;
    C.pad = pad;
    C.pitch_lo = (uint32_t)(pitch & 0xffffffffu); C.pitch_hi = (uint32_t)(pitch >> 32);
    C.ring = ring_geom(p);
    const unsigned gx = (unsigned)((cfg.out_width + leon::kResTileX - 1) / leon::kResTileX), gy = (unsigned)((cfg.out_height + leon::kResTileY - 1) / leon::kResTileY);
    hipLaunchKernelGGL(kWarpKernels[p->tensor_elem >> 1][p->tensor_layout], dim3(gx, gy, (unsigned)n), dim3(leon::kRgbaBlock), 0, st, (const uint8_t*)p->d_planes, out, d_recs,
                       d_ids, d_status, (const uint32_t*)p->d_tensor_table, (const leon::Tables*)p->dec->d_tables, C);
}

// One call of the host road: refusals, [frame ids | records] into the regions staging, then regions_host_run
int warp_regions(leon_pipeline* p, int64_t window, const leon_pipeline_warp_region* regions, int32_t n, const leon_pipeline_warp_config* cfg, void* device_out,
                 uint64_t out_pitch, void* host)
{
    int rc = regions_pipeline_check(p);
    if (rc != LEON_OK) return rc;
    std::lock_guard<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> ids;
    if ((rc = regions_window_ids(p, window, &ids)) != LEON_OK) return rc;
    uint32_t pad = 0;
    if ((rc = warp_regions_check(p->vinfo.frame_width, p->vinfo.frame_height, (int32_t)ids.size(), regions, n, cfg, nullptr, &pad)) != LEON_OK) return rc;
    const size_t region_bytes = (size_t)3 * cfg->out_height * cfg->out_width * p->tensor_elem;
    uint64_t pitch = pad256(region_bytes);
    if (!host && (rc = regions_out_check("warp regions", device_out, out_pitch, region_bytes, &pitch)) != LEON_OK) return rc;
    const size_t ids_bytes = pad256(ids.size() * 4), upload_bytes = ids_bytes + (size_t)n * sizeof(leon::WarpRecord);
    hipStream_t st;
    if ((rc = regions_call_stream(p, nullptr, &st)) != LEON_OK || (rc = regions_reserve(p, upload_bytes, host ? (size_t)n * pitch : 0)) != LEON_OK) return rc;
    std::copy(ids.begin(), ids.end(), reinterpret_cast<uint32_t*>(p->regions_host.get()));
    std::memcpy(p->regions_host + ids_bytes, regions, (size_t)n * sizeof(leon::WarpRecord));
    return regions_host_run(p, st, upload_bytes, host, device_out, (size_t)pitch, region_bytes, n, [&](uint8_t* out) {
        warp_launch(p, st, reinterpret_cast<const leon::WarpRecord*>(p->regions_dev + ids_bytes), reinterpret_cast<const uint32_t*>(p->regions_dev.get()), (int32_t)ids.size(), n, *cfg,
                    pad, out, pitch, nullptr);
    });
}

// One call of the device road: the host's refusals, then inside the boxes bracket (the frame ids are all of the scratch it needs) one launch
// on the caller's stream (or the regions stream and a wait)
int warp_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_warp_config* cfg, const leon_pipeline_warp_regions_call* c)
{
    int rc = regions_pipeline_check(p);
    if (rc != LEON_OK) return rc;
    if (!cfg || !c) return fail(LEON_ERR_INVALID, "null argument");
    std::unique_lock<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> ids;
    if ((rc = regions_window_ids(p, window, &ids)) != LEON_OK) return rc;
    uint32_t pad = 0;
    const int32_t n = c->n;
    if ((rc = warp_config_check(p->vinfo.frame_width, p->vinfo.frame_height, (int32_t)ids.size(), n, cfg, &pad)) != LEON_OK) return rc;
    const size_t region_bytes = (size_t)3 * cfg->out_height * cfg->out_width * p->tensor_elem;
    uint64_t pitch;
    if ((rc = boxes_call_check("warp regions", c->regions, c->reserved0 || c->reserved[0] || c->reserved[1], c->device_status, c->device_out, c->out_pitch_bytes, region_bytes,
                               &pitch)) != LEON_OK)
        return rc;
    return boxes_run(p, c->stream, call, ids, pad256(ids.size() * 4), [&](hipStream_t st, uint32_t* d_ids) {
        warp_launch(p, st, reinterpret_cast<const leon::WarpRecord*>(c->regions), d_ids, (int32_t)ids.size(), n, *cfg, pad, static_cast<uint8_t*>(c->device_out), pitch,
                    c->device_status);
    });
}

// ---- boxes carried along the motion vectors (leon_pipeline_carry_regions) -------------------------------------------------------
static_assert(sizeof(leon_pipeline_carry_region) == 32 && sizeof(leon_pipeline_carry_regions_call) == 64 && sizeof(leon::CarryRecord) == sizeof(leon_pipeline_carry_region) &&
              sizeof(leon::CarryFrame) == 16, "include/leon_pipeline.h states the sizes");
static_assert(leon::kRegionNoReference == LEON_REGION_NO_REFERENCE, "the kernel's code is the header's");

// the geometry a carry call may have: a coded grid of 1 .. 256 macroblocks an axis and a frame inside it
int carry_geometry_check(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames)
{
    if (const int rc = mb_grid_check("carry", mbw, mbh); rc != LEON_OK) return rc;
    if (fw < 1 || fw > 16 * mbw || fh < 1 || fh > 16 * mbh) return fail(LEON_ERR_INVALID, "carry: a frame of %d x %d in a grid of %d x %d macroblocks", fw, fh, mbw, mbh);
    if (n_frames < 0) return fail(LEON_ERR_INVALID, "carry: %d frames", n_frames);
    return LEON_OK;
}

// the launch every road shares: records, the window's table and the motion ring in device memory; ceil(n / 4) workgroups
void carry_launch(hipStream_t st, const leon::CarryRecord* d_recs, const leon::CarryFrame* d_frames, const uint8_t* d_ring, int32_t fw, int32_t fh, int32_t mbw,
                  const leon::MotionLayout& lay, int32_t n_frames, int32_t n, int32_t* d_out, int32_t* d_votes, int32_t* d_status)
{
    leon::CarryCall C{};
    C.fw = fw; C.fh = fh; C.mbw = mbw;
    C.n_frames = n_frames; C.n = n;
    C.info_offset = lay.info_offset; C.record_pitch = lay.record_pitch;
    const unsigned per = leon::kRgbaBlock / 64;
    hipLaunchKernelGGL(leon::k_carry, dim3(((unsigned)n + per - 1) / per), dim3(leon::kRgbaBlock), 0, st, d_recs, d_frames, d_ring, d_out, d_votes, d_status, C);
}

int carry_pipeline_check(const leon_pipeline* p)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    if (!p->motion.ring) return no_output("motion", "MOTION");
    return LEON_OK;
}

// The head of the device roads that read the record rings through the window's table (carry, gauge, propagate), after the family's
// judgement of its pipeline: regions_mu, the table, what every such call refuses alike under its prefix `who` -- a reserved word, the
// count of its `noun` -- then the family's own (`checks()`: null pointers, alignment, propagate's config), then inside the boxes
// bracket (the table is all of the scratch it needs) `launch(st, frames, n_frames)` on the caller's stream (or the regions stream and a
// wait)
template <class Checks, class Launch>
int table_road(leon_pipeline* p, int64_t window, void* stream, const char* who, const char* noun, int32_t n, bool reserved_set, Checks checks, Launch launch)
{
    std::unique_lock<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> table;
    int rc = carry_window_table(p, window, &table);
    if (rc != LEON_OK) return rc;
    if (reserved_set) return fail(LEON_ERR_INVALID, "%s: a reserved word of the call is not 0", who);
    if ((rc = record_count_check(who, noun, n)) != LEON_OK || (rc = checks()) != LEON_OK) return rc;
    return boxes_run(p, stream, call, table, pad256(std::max<size_t>(table.size(), 1) * 4), [&](hipStream_t st, uint32_t* d_table) {
        launch(st, reinterpret_cast<const leon::CarryFrame*>(d_table), (int32_t)(table.size() / 4));
    });
}
// Their host roads, after the family's argument checks: the window's refusals before anything is allocated or uploaded (the device
// road judges it again under the same lock), then between the pieces going up and coming back `device(pieces)`: the device road with
// stream NULL, which has waited when it returns
template <class Device>
int table_host_road(leon_pipeline* p, int64_t window, const char* who, std::initializer_list<Piece> pieces, Device device)
{
    {
        std::unique_lock<std::mutex> call(p->regions_mu);
        std::vector<uint32_t> table;
        if (const int rc = carry_window_table(p, window, &table); rc != LEON_OK) return rc;
    }
    return pieces_run(p->cfg.device_id, who, pieces, device);
}
// Their diagnostics' window: the table -- a frame that `has(i)` a record gets the next slot of the ring(s), a frame without gets none:
// its ring id stays 0 and nothing of the call reads it; fwd, bwd: null where the family reads no references -- and a ring of `slots`
// records `pitch` apart staged on the host as record_kernel stages its payload, frame i's record at its slot, to go up as one piece
// (records null: a ring the call does not read, of no bytes)
template <class Has>
std::vector<leon::CarryFrame> kernel_table(int32_t n_frames, const int32_t* fwd, const int32_t* bwd, Has has, uint32_t* slots)
{
    std::vector<leon::CarryFrame> table((size_t)n_frames);
    *slots = 0;
    for (size_t i = 0; i < table.size(); i++) table[i] = leon::CarryFrame{has(i) ? (*slots)++ : 0u, fwd ? fwd[i] : -1, bwd ? bwd[i] : -1, 0u};
    return table;
}
std::vector<uint8_t> kernel_ring(const std::vector<leon::CarryFrame>& table, uint32_t slots, const void* const* records, size_t record_bytes, size_t pitch)
{
    std::vector<uint8_t> ring(records ? (size_t)slots * pitch : 0);
    for (size_t i = 0; records && i < table.size(); i++)
        if (records[i]) memcpy(ring.data() + (size_t)table[i].ring * pitch, records[i], record_bytes);
    return ring;
}

// One call of the device road: the host's refusals, then one launch
int carry_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_carry_regions_call* c)
{
    if (const int rc = carry_pipeline_check(p); rc != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    return table_road(p, window, c->stream, "carry regions", "regions", c->n, c->reserved0 || c->reserved[0] || c->reserved[1], [&] {
        if (!c->regions) return fail(LEON_ERR_INVALID, "carry regions: null regions");
        if (!c->device_out) return fail(LEON_ERR_INVALID, "carry regions: null device_out");
        if (((uintptr_t)c->regions | (uintptr_t)c->device_out | (uintptr_t)c->device_votes | (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "carry regions: regions %p, device_out %p, device_votes %p, device_status %p: not all 4-byte aligned", (const void*)c->regions,
                        (void*)c->device_out, (void*)c->device_votes, (void*)c->device_status);
        return (int)LEON_OK;
    }, [&](hipStream_t st, const leon::CarryFrame* d_frames, int32_t n_frames) {
        carry_launch(st, reinterpret_cast<const leon::CarryRecord*>(c->regions), d_frames, p->motion.ring, p->vinfo.frame_width, p->vinfo.frame_height, p->vinfo.mb_width,
                     p->motion_lay, n_frames, c->n, reinterpret_cast<int32_t*>(c->device_out), c->device_votes, c->device_status);
    });
}

// One call of the host road: [records | out | votes | status], what the caller has in out, votes and status going up first
int carry_regions(leon_pipeline* p, int64_t window, const leon_pipeline_carry_region* regions, int32_t n, leon_pipeline_region* out, int32_t* votes, int32_t* status)
{
    int rc = carry_pipeline_check(p);
    if (rc != LEON_OK) return rc;
    if (!regions || !out) return fail(LEON_ERR_INVALID, "carry regions: null %s", regions ? "out" : "regions");
    if ((rc = record_count_check("carry regions", "regions", n)) != LEON_OK) return rc;
    return table_host_road(p, window, "carry", {{regions, nullptr, (size_t)n * 32}, {out, out, (size_t)n * 32}, {votes, votes, (size_t)n * 16}, {status, status, (size_t)n * 4}},
                           [&](const Pieces& s) {
        leon_pipeline_carry_regions_call c{};
        c.regions = s.at<const leon_pipeline_carry_region>(0);
        c.n = n;
        c.device_out = s.at<leon_pipeline_region>(1);
        c.device_votes = votes ? s.at<int32_t>(2) : nullptr;
        c.device_status = status ? s.at<int32_t>(3) : nullptr;
        return carry_regions_device(p, window, &c);
    });
}

// the definition on the CPU: the same text (leon_carry.h) over a record in host memory; the status word, or a negative error
int32_t carry_record_host(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const int32_t* fwd, const int32_t* bwd, const void* const* records,
                          const leon_pipeline_carry_region* rec, leon_pipeline_region* out, int32_t* votes, bool dry)
{
    if (!fwd || !bwd || !records || !rec || (!dry && !out)) return fail(LEON_ERR_INVALID, "null argument");
    const int rc = carry_geometry_check(fw, fh, mbw, mbh, n_frames);
    if (rc != LEON_OK) return rc;
    const leon::CarryRecord& r = reinterpret_cast<const leon::CarryRecord&>(*rec);
    int32_t st = leon::carry_record_status(r, fw, fh, n_frames), m = 0, sense = 1, d = 0;
    if (st != leon::kRegionOk) return st;
    if ((st = leon::carry_pick(r.frame, r.target, fwd[r.target], bwd[r.target], fwd[r.frame], bwd[r.frame], &m, &sense, &d)) != leon::kRegionOk) return st;
    leon::CarrySums s{0, 0, 0, 0};
    if (d) {
        const uint8_t* record = static_cast<const uint8_t*>(records[m]);
        if (!record) return fail(LEON_ERR_INVALID, "carry: frame %d votes (frame %d to %d) and has no record", m, r.frame, r.target);
        if (dry) return leon::kRegionOk;
        const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
        for (int32_t j = r.y >> 4; j <= (r.y + r.height - 1) >> 4; j++)
            for (int32_t i = r.x >> 4; i <= (r.x + r.width - 1) >> 4; i++) {
                const size_t mb = (size_t)j * (size_t)mbw + (size_t)i;
                uint32_t f, b;
                memcpy(&f, record + 8 * mb, 4);
                memcpy(&b, record + 8 * mb + 4, 4);
                leon::carry_vote(d, record[L.info_offset + mb], f, b, leon::carry_weight(r.x, r.y, r.width, r.height, i, j), &s);
            }
    }
    if (dry) return leon::kRegionOk;
    int32_t o[8], v[4];
    leon::carry_finish(r, fw, fh, sense, s, o, v);
    memcpy(out, o, 32);
    if (votes) memcpy(votes, v, 16);
    return leon::kRegionOk;
}

// k_carry on records the caller supplies (leon_pipeline_carry_device): memory of its own, the null stream
int carry_device(int32_t device_id, int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const int32_t* fwd, const int32_t* bwd,
                 const void* const* records, const leon_pipeline_carry_region* regions, int32_t n, leon_pipeline_region* out, int32_t* votes, int32_t* status)
{
    if (!fwd || !bwd || !records || !regions || !out) return fail(LEON_ERR_INVALID, "null argument");
    int rc = carry_geometry_check(fw, fh, mbw, mbh, n_frames);
    if (rc != LEON_OK) return rc;
    if ((rc = record_count_check("carry regions", "regions", n)) != LEON_OK) return rc;
    for (int32_t i = 0; i < n_frames; i++)
        if (fwd[i] < -1 || fwd[i] >= n_frames || bwd[i] < -1 || bwd[i] >= n_frames)
            return fail(LEON_ERR_INVALID, "carry: frame %d points into frames %d and %d of %d", i, fwd[i], bwd[i], n_frames);
    for (int32_t i = 0; i < n; i++)          // a record that votes must be there: the judgement alone, nothing summed
        if (carry_record_host(fw, fh, mbw, mbh, n_frames, fwd, bwd, records, regions + i, nullptr, nullptr, true) < 0) return LEON_ERR_INVALID;
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    uint32_t slots;
    const std::vector<leon::CarryFrame> table = kernel_table(n_frames, fwd, bwd, [&](size_t i) { return records[i] != nullptr; }, &slots);
    const std::vector<uint8_t> ring = kernel_ring(table, slots, records, L.record_bytes, L.record_pitch);
    return pieces_run(device_id, "carry", {{regions, nullptr, (size_t)n * 32}, {out, out, (size_t)n * 32}, {votes, votes, (size_t)n * 16}, {status, status, (size_t)n * 4},
                                           {table.data(), nullptr, table.size() * sizeof(leon::CarryFrame)}, {ring.data(), nullptr, ring.size()}}, [&](const Pieces& s) {
        carry_launch(nullptr, s.at<const leon::CarryRecord>(0), s.at<const leon::CarryFrame>(4), s.at(5), fw, fh, mbw, L, n_frames, n, s.at<int32_t>(1),
                     votes ? s.at<int32_t>(2) : nullptr, status ? s.at<int32_t>(3) : nullptr);
        return (int)LEON_OK;
    });
}

// ---- boxes gauged: a frame's motion and activity records under each box (leon_pipeline_gauge_regions) ------------------------------
static_assert(sizeof(leon_pipeline_gauge_config) == 32 && sizeof(leon_pipeline_gauge_regions_call) == 64 && sizeof(leon::GaugeRecord) == sizeof(leon_pipeline_region) &&
              sizeof(leon::GaugeCall) == 40, "include/leon_pipeline.h states the sizes");
static_assert(leon::kGaugeMotion == LEON_GAUGE_MOTION && leon::kGaugeActivity == LEON_GAUGE_ACTIVITY, "the kernel's bits are the header's");

int gauge_config_check(const leon_pipeline_gauge_config* cfg)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "null argument");
    if (cfg->sources < 1 || cfg->sources > (LEON_GAUGE_MOTION | LEON_GAUGE_ACTIVITY))
        return fail(LEON_ERR_INVALID, "gauge regions: sources %d (LEON_GAUGE_MOTION | LEON_GAUGE_ACTIVITY: 1 .. 3)", cfg->sources);
    for (int32_t v : cfg->reserved)
        if (v) return fail(LEON_ERR_INVALID, "gauge regions: a reserved word of the config is not 0");
    return LEON_OK;
}

// the launch every road shares: records, the window's table and the two rings in device memory (a ring the sources do not ask for is
// not read); ceil(n / 4) workgroups
void gauge_launch(hipStream_t st, const leon::GaugeRecord* d_recs, const leon::CarryFrame* d_frames, const uint8_t* d_motion, const uint8_t* d_activity, int32_t fw,
                  int32_t fh, int32_t mbw, const leon::MotionLayout& ml, const leon::ActivityLayout& al, int32_t n_frames, int32_t sources, int32_t n, int64_t* d_stats,
                  int32_t* d_status)
{
    leon::GaugeCall C{};
    C.fw = fw; C.fh = fh; C.mbw = mbw;
    C.n_frames = n_frames; C.n = n; C.sources = sources;
    C.info_offset = ml.info_offset; C.motion_pitch = ml.record_pitch; C.activity_pitch = al.record_pitch;
    const unsigned per = leon::kRgbaBlock / 64;
    hipLaunchKernelGGL(leon::k_gauge, dim3(((unsigned)n + per - 1) / per), dim3(leon::kRgbaBlock), 0, st, d_recs, d_frames, d_motion, d_activity, d_stats, d_status, C);
}

// the record outputs a call's sources ask for are the pipeline's
int gauge_outputs_check(const leon_pipeline* p, int32_t sources)
{
    if ((sources & LEON_GAUGE_MOTION) && !p->motion.ring) return no_output("motion", "MOTION");
    if ((sources & LEON_GAUGE_ACTIVITY) && !p->activity.ring) return no_output("activity", "ACTIVITY");
    return LEON_OK;
}

// One call of the device road: the host's refusals (the config's before the window's), then one launch
int gauge_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg, const leon_pipeline_gauge_regions_call* c)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = gauge_config_check(cfg);
    if (rc != LEON_OK || (rc = gauge_outputs_check(p, cfg->sources)) != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    return table_road(p, window, c->stream, "gauge regions", "regions", c->n, c->reserved0 || c->reserved[0] || c->reserved[1] || c->reserved[2], [&] {
        if (!c->regions) return fail(LEON_ERR_INVALID, "gauge regions: null regions");
        if (!c->device_stats) return fail(LEON_ERR_INVALID, "gauge regions: null device_stats");
        if (((uintptr_t)c->regions | (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "gauge regions: regions %p, device_status %p: not both 4-byte aligned", (const void*)c->regions, (void*)c->device_status);
        if ((uintptr_t)c->device_stats & 7u) return fail(LEON_ERR_INVALID, "gauge regions: device_stats %p is not 8-byte aligned", (void*)c->device_stats);
        return (int)LEON_OK;
    }, [&](hipStream_t st, const leon::CarryFrame* d_frames, int32_t n_frames) {
        gauge_launch(st, reinterpret_cast<const leon::GaugeRecord*>(c->regions), d_frames, p->motion.ring, p->activity.ring, p->vinfo.frame_width, p->vinfo.frame_height,
                     p->vinfo.mb_width, p->motion_lay, p->activity_lay, n_frames, cfg->sources, c->n, c->device_stats, c->device_status);
    });
}

// One call of the host road: [stats | records | status], what the caller has in stats and status going up first.  The outputs are
// judged here as well, behind the count and in front of the window: the order in which a caller of this road meets the refusals.
int gauge_regions(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* regions, int32_t n, int64_t* stats, int32_t* status)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = gauge_config_check(cfg);
    if (rc != LEON_OK) return rc;
    if (!regions || !stats) return fail(LEON_ERR_INVALID, "gauge regions: null %s", regions ? "stats" : "regions");
    if ((rc = record_count_check("gauge regions", "regions", n)) != LEON_OK || (rc = gauge_outputs_check(p, cfg->sources)) != LEON_OK) return rc;
    return table_host_road(p, window, "gauge", {{stats, stats, (size_t)n * 8 * leon::kGaugeWords}, {regions, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4}},
                           [&](const Pieces& s) {
        leon_pipeline_gauge_regions_call c{};
        c.regions = s.at<const leon_pipeline_region>(1);
        c.n = n;
        c.device_stats = s.at<int64_t>(0);
        c.device_status = status ? s.at<int32_t>(2) : nullptr;
        return gauge_regions_device(p, window, cfg, &c);
    });
}

// the definition on the CPU: the same text (leon_gauge.h) over records in host memory; the status word, or a negative error
int32_t gauge_record_host(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* motion_records, const void* const* activity_records,
                          const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* rec, int64_t* stats, bool dry)
{
    int rc = gauge_config_check(cfg);
    if (rc != LEON_OK) return rc;
    const bool mot = (cfg->sources & LEON_GAUGE_MOTION) != 0, act = (cfg->sources & LEON_GAUGE_ACTIVITY) != 0;
    if (!rec || (!dry && !stats) || (mot && !motion_records) || (act && !activity_records)) return fail(LEON_ERR_INVALID, "null argument");
    if ((rc = carry_geometry_check(fw, fh, mbw, mbh, n_frames)) != LEON_OK) return rc;
    const leon::GaugeRecord& r = reinterpret_cast<const leon::GaugeRecord&>(*rec);
    const int32_t st = leon::gauge_record_status(r, fw, fh, n_frames);
    if (st != leon::kRegionOk) return st;
    const uint8_t* mrec = mot ? static_cast<const uint8_t*>(motion_records[r.frame]) : nullptr;
    const uint8_t* arec = act ? static_cast<const uint8_t*>(activity_records[r.frame]) : nullptr;
    if ((mot && !mrec) || (act && !arec)) return fail(LEON_ERR_INVALID, "gauge: frame %d has no %s record", r.frame, mot && !mrec ? "motion" : "activity");
    if (dry) return leon::kRegionOk;
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    leon::GaugeSums s{};
    for (int32_t j = r.y >> 4; j <= (r.y + r.height - 1) >> 4; j++)
        for (int32_t i = r.x >> 4; i <= (r.x + r.width - 1) >> 4; i++) {
            const size_t mb = (size_t)j * (size_t)mbw + (size_t)i;
            uint32_t lo = 0, hi = 0, f = 0, b = 0, info = 0;
            if (act) {
                memcpy(&lo, arec + 8 * mb, 4);
                memcpy(&hi, arec + 8 * mb + 4, 4);
            }
            if (mot) {
                memcpy(&f, mrec + 8 * mb, 4);
                memcpy(&b, mrec + 8 * mb + 4, 4);
                info = mrec[L.info_offset + mb];
            }
            leon::gauge_cell(cfg->sources, leon::carry_weight(r.x, r.y, r.width, r.height, i, j), lo, hi, info, f, b, &s);
        }
    int64_t o[leon::kGaugeWords];
    leon::gauge_finish(cfg->sources, s, o);
    memcpy(stats, o, sizeof(o));
    return leon::kRegionOk;
}

// k_gauge on records the caller supplies (leon_pipeline_gauge_kernel): memory of its own, the null stream
int gauge_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* motion_records,
                 const void* const* activity_records, const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* regions, int32_t n, int64_t* stats, int32_t* status)
{
    int rc = gauge_config_check(cfg);
    if (rc != LEON_OK) return rc;
    if (!regions || !stats) return fail(LEON_ERR_INVALID, "null argument");
    if ((rc = record_count_check("gauge regions", "regions", n)) != LEON_OK) return rc;
    for (int32_t i = 0; i < n; i++)          // a record a valid region names must be there: the judgement alone, nothing summed
        if (gauge_record_host(fw, fh, mbw, mbh, n_frames, motion_records, activity_records, cfg, regions + i, nullptr, true) < 0) return LEON_ERR_INVALID;
    const bool mot = (cfg->sources & LEON_GAUGE_MOTION) != 0, act = (cfg->sources & LEON_GAUGE_ACTIVITY) != 0;
    const leon::MotionLayout ML = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    const leon::ActivityLayout AL = leon::activity_layout((uint32_t)mbw, (uint32_t)mbh);
    // a frame with a record of either kind gets a slot in both rings, as the pipeline's rings share an index
    uint32_t slots;
    const std::vector<leon::CarryFrame> table =
        kernel_table(n_frames, nullptr, nullptr, [&](size_t i) { return (mot && motion_records[i]) || (act && activity_records[i]); }, &slots);
    const std::vector<uint8_t> motion = kernel_ring(table, slots, mot ? motion_records : nullptr, ML.record_bytes, ML.record_pitch);
    const std::vector<uint8_t> activity = kernel_ring(table, slots, act ? activity_records : nullptr, AL.record_bytes, AL.record_pitch);
    return pieces_run(device_id, "gauge", {{stats, stats, (size_t)n * 8 * leon::kGaugeWords}, {regions, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4},
                                           {table.data(), nullptr, table.size() * sizeof(leon::CarryFrame)}, {motion.data(), nullptr, motion.size()},
                                           {activity.data(), nullptr, activity.size()}}, [&](const Pieces& s) {
        gauge_launch(nullptr, s.at<const leon::GaugeRecord>(1), s.at<const leon::CarryFrame>(3), mot ? s.at(4) : nullptr, act ? s.at(5) : nullptr, fw, fh, mbw, ML, AL, n_frames,
                     cfg->sources, n, s.at<int64_t>(0), status ? s.at<int32_t>(2) : nullptr);
        return (int)LEON_OK;
    });
}

// ---- boxes proposed: the components of a frame's hot macroblocks as region records (leon_pipeline_propose_regions) -----------------
static_assert(sizeof(leon_pipeline_propose_config) == 32 && sizeof(leon_pipeline_propose_regions_call) == 64 && sizeof(leon::ProposeConfig) == 32 &&
              sizeof(leon::ProposeCall) == 72, "include/leon_pipeline.h states the sizes");
static_assert(leon::kProposeMotion == LEON_PROPOSE_MOTION && leon::kProposeActivity == LEON_PROPOSE_ACTIVITY && leon::kProposeIntra == LEON_PROPOSE_INTRA,
              "the kernel's bits are the header's");
static_assert(LEON_PROPOSE_MOTION == LEON_GAUGE_MOTION && LEON_PROPOSE_ACTIVITY == LEON_GAUGE_ACTIVITY, "one judgement of the outputs a call's sources need (gauge_outputs_check)");
// a CU's LDS holds the largest request: every grid up to 256 x 256 with every K up to 1024
static_assert(leon::propose_lds(leon::kProposeMaxCells, leon::kProposeMaxBoxes).bytes == 155680 && 155680 <= 160 * 1024, "include/leon_pipeline.h states the LDS");

int propose_config_check(const leon_pipeline_propose_config* cfg)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "null argument");
    if (cfg->sources < 1 || cfg->sources > (LEON_PROPOSE_MOTION | LEON_PROPOSE_ACTIVITY))
        return fail(LEON_ERR_INVALID, "propose regions: sources %d (LEON_PROPOSE_MOTION | LEON_PROPOSE_ACTIVITY: 1 .. 3)", cfg->sources);
    const bool mot = (cfg->sources & LEON_PROPOSE_MOTION) != 0, act = (cfg->sources & LEON_PROPOSE_ACTIVITY) != 0;
    if ((cfg->flags & ~LEON_PROPOSE_INTRA) || (cfg->flags && !mot))
        return fail(LEON_ERR_INVALID, "propose regions: flags %d (LEON_PROPOSE_INTRA, with LEON_PROPOSE_MOTION only)", cfg->flags);
    if (mot ? cfg->mv_min < 1 || cfg->mv_min > 32768 : cfg->mv_min != 0)
        return fail(LEON_ERR_INVALID, "propose regions: mv_min %d (1 .. 32768 with the motion source, 0 without)", cfg->mv_min);
    if (act ? cfg->ac_min < 1 || cfg->ac_min > 65535 : cfg->ac_min != 0)
        return fail(LEON_ERR_INVALID, "propose regions: ac_min %d (1 .. 65535 with the activity source, 0 without)", cfg->ac_min);
    if (cfg->connectivity != 4 && cfg->connectivity != 8) return fail(LEON_ERR_INVALID, "propose regions: connectivity %d (4 or 8)", cfg->connectivity);
    if (cfg->min_cells < 1 || cfg->min_cells > leon::kProposeMaxCells) return fail(LEON_ERR_INVALID, "propose regions: min_cells %d (1 .. 65536)", cfg->min_cells);
    if (cfg->max_boxes < 1 || cfg->max_boxes > leon::kProposeMaxBoxes) return fail(LEON_ERR_INVALID, "propose regions: max_boxes %d (1 .. 1024)", cfg->max_boxes);
    if (cfg->reserved) return fail(LEON_ERR_INVALID, "propose regions: a reserved word of the config is not 0");
    return LEON_OK;
}

// the launch every road shares: requests, the window's table and the two rings in device memory (a ring the sources do not ask for is
// not read); a workgroup a request, its LDS as leon_propose.h lays it out for this grid and K -- above 48 KiB the kernel is told so
int propose_launch(hipStream_t st, const int32_t* d_requests, const leon::CarryFrame* d_frames, const uint8_t* d_motion, const uint8_t* d_activity, int32_t fw, int32_t fh,
                   int32_t mbw, int32_t mbh, const leon::MotionLayout& ml, const leon::ActivityLayout& al, int32_t n_frames, const leon_pipeline_propose_config& cfg, int32_t n,
                   int32_t* d_regions, int32_t* d_info, int32_t* d_count, int32_t* d_status)
{
    leon::ProposeCall C{};
    memcpy(&C.cfg, &cfg, sizeof(C.cfg));
    C.fw = fw; C.fh = fh; C.mbw = mbw; C.mbh = mbh;
    C.n_frames = n_frames; C.n = n;
    C.info_offset = ml.info_offset; C.motion_pitch = ml.record_pitch; C.activity_pitch = al.record_pitch;
    const uint32_t lds = leon::propose_lds((uint32_t)mbw * (uint32_t)mbh, (uint32_t)cfg.max_boxes).bytes;
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)leon::k_propose, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(leon::k_propose, dim3((unsigned)n), dim3(leon::kProposeThreads), lds, st, d_requests, d_frames, d_motion, d_activity, d_regions, d_info, d_count,
                       d_status, C);
    return LEON_OK;
}

// One call of the device road: the host's refusals (the config's before the window's), then one launch
int propose_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg, const leon_pipeline_propose_regions_call* c)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = propose_config_check(cfg);
    if (rc != LEON_OK || (rc = gauge_outputs_check(p, cfg->sources)) != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    int launched = LEON_OK;
    rc = table_road(p, window, c->stream, "propose regions", "frames", c->n, c->reserved0 || c->reserved[0], [&] {
        if (!c->frames) return fail(LEON_ERR_INVALID, "propose regions: null frames");
        if (!c->device_regions) return fail(LEON_ERR_INVALID, "propose regions: null device_regions");
        if (!c->device_count) return fail(LEON_ERR_INVALID, "propose regions: null device_count");
        if (((uintptr_t)c->frames | (uintptr_t)c->device_regions | (uintptr_t)c->device_info | (uintptr_t)c->device_count | (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "propose regions: frames %p, device_regions %p, device_info %p, device_count %p, device_status %p: not all 4-byte aligned",
                        (const void*)c->frames, (void*)c->device_regions, (void*)c->device_info, (void*)c->device_count, (void*)c->device_status);
        return (int)LEON_OK;
    }, [&](hipStream_t st, const leon::CarryFrame* d_frames, int32_t n_frames) {
        launched = propose_launch(st, c->frames, d_frames, p->motion.ring, p->activity.ring, p->vinfo.frame_width, p->vinfo.frame_height, p->vinfo.mb_width,
                                  p->vinfo.mb_height, p->motion_lay, p->activity_lay, n_frames, *cfg, c->n, reinterpret_cast<int32_t*>(c->device_regions), c->device_info,
                                  c->device_count, c->device_status);
    });
    return rc != LEON_OK ? rc : launched;
}

// One call of the host road: [regions | info | count | status | requests], what the caller has in the outputs going up first.  The
// outputs are judged here as well, behind the count and in front of the window, as the gauge family's host road does.
int propose_regions(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg, const int32_t* frames, int32_t n, leon_pipeline_region* regions, int32_t* info,
                    int32_t* count, int32_t* status)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = propose_config_check(cfg);
    if (rc != LEON_OK) return rc;
    if (!frames || !regions || !count) return fail(LEON_ERR_INVALID, "propose regions: null %s", !frames ? "frames" : !regions ? "regions" : "count");
    if ((rc = record_count_check("propose regions", "frames", n)) != LEON_OK || (rc = gauge_outputs_check(p, cfg->sources)) != LEON_OK) return rc;
    const size_t rows = (size_t)n * (size_t)cfg->max_boxes;
    return table_host_road(p, window, "propose", {{regions, regions, rows * 32}, {info, info, rows * 8}, {count, count, (size_t)n * 4}, {status, status, (size_t)n * 4},
                                                  {frames, nullptr, (size_t)n * 4}}, [&](const Pieces& s) {
        leon_pipeline_propose_regions_call c{};
        c.frames = s.at<const int32_t>(4);
        c.n = n;
        c.device_regions = s.at<leon_pipeline_region>(0);
        c.device_info = info ? s.at<int32_t>(1) : nullptr;
        c.device_count = s.at<int32_t>(2);
        c.device_status = status ? s.at<int32_t>(3) : nullptr;
        return propose_regions_device(p, window, cfg, &c);
    });
}

// the definition on the CPU: the checks, then leon_propose.h's host text (propose_request_host: a flood fill, nothing of the kernel's
// search) over records in host memory; the status word, or a negative error
int32_t propose_record_host(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* motion_records, const void* const* activity_records,
                            const leon_pipeline_propose_config* cfg, int32_t frame, leon_pipeline_region* regions, int32_t* info, int32_t* count, bool dry)
{
    int rc = propose_config_check(cfg);
    if (rc != LEON_OK) return rc;
    const bool mot = (cfg->sources & LEON_PROPOSE_MOTION) != 0, act = (cfg->sources & LEON_PROPOSE_ACTIVITY) != 0;
    if ((!dry && (!regions || !count)) || (mot && !motion_records) || (act && !activity_records)) return fail(LEON_ERR_INVALID, "null argument");
    if ((rc = carry_geometry_check(fw, fh, mbw, mbh, n_frames)) != LEON_OK) return rc;
    const int32_t st = leon::propose_request_status(frame, n_frames);
    if (st != leon::kRegionOk) return st;
    const uint8_t* mrec = mot ? static_cast<const uint8_t*>(motion_records[frame]) : nullptr;
    const uint8_t* arec = act ? static_cast<const uint8_t*>(activity_records[frame]) : nullptr;
    if ((mot && !mrec) || (act && !arec)) return fail(LEON_ERR_INVALID, "propose: frame %d has no %s record", frame, mot && !mrec ? "motion" : "activity");
    if (dry) return leon::kRegionOk;
    leon::ProposeConfig C;
    memcpy(&C, cfg, sizeof(C));
    leon::propose_request_host(C, fw, fh, mbw, mbh, mrec, arec, frame, reinterpret_cast<int32_t*>(regions), info, count);
    return leon::kRegionOk;
}

// k_propose on records the caller supplies (leon_pipeline_propose_kernel): memory of its own, the null stream
int propose_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* motion_records,
                   const void* const* activity_records, const leon_pipeline_propose_config* cfg, const int32_t* frames, int32_t n, leon_pipeline_region* regions, int32_t* info,
                   int32_t* count, int32_t* status)
{
    int rc = propose_config_check(cfg);
    if (rc != LEON_OK) return rc;
    if (!frames || !regions || !count) return fail(LEON_ERR_INVALID, "null argument");
    if ((rc = record_count_check("propose regions", "frames", n)) != LEON_OK) return rc;
    for (int32_t i = 0; i < n; i++)          // a record a valid request names must be there: the judgement alone, nothing searched
        if (propose_record_host(fw, fh, mbw, mbh, n_frames, motion_records, activity_records, cfg, frames[i], nullptr, nullptr, nullptr, true) < 0) return LEON_ERR_INVALID;
    const bool mot = (cfg->sources & LEON_PROPOSE_MOTION) != 0, act = (cfg->sources & LEON_PROPOSE_ACTIVITY) != 0;
    const leon::MotionLayout ML = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    const leon::ActivityLayout AL = leon::activity_layout((uint32_t)mbw, (uint32_t)mbh);
    uint32_t slots;
    const std::vector<leon::CarryFrame> table =
        kernel_table(n_frames, nullptr, nullptr, [&](size_t i) { return (mot && motion_records[i]) || (act && activity_records[i]); }, &slots);
    const std::vector<uint8_t> motion = kernel_ring(table, slots, mot ? motion_records : nullptr, ML.record_bytes, ML.record_pitch);
    const std::vector<uint8_t> activity = kernel_ring(table, slots, act ? activity_records : nullptr, AL.record_bytes, AL.record_pitch);
    const size_t rows = (size_t)n * (size_t)cfg->max_boxes;
    return pieces_run(device_id, "propose", {{regions, regions, rows * 32}, {info, info, rows * 8}, {count, count, (size_t)n * 4}, {status, status, (size_t)n * 4},
                                             {frames, nullptr, (size_t)n * 4}, {table.data(), nullptr, table.size() * sizeof(leon::CarryFrame)},
                                             {motion.data(), nullptr, motion.size()}, {activity.data(), nullptr, activity.size()}}, [&](const Pieces& s) {
        return propose_launch(nullptr, s.at<const int32_t>(4), s.at<const leon::CarryFrame>(5), mot ? s.at(6) : nullptr, act ? s.at(7) : nullptr, fw, fh, mbw, mbh, ML, AL,
                              n_frames, *cfg, n, s.at<int32_t>(0), info ? s.at<int32_t>(1) : nullptr, s.at<int32_t>(2), status ? s.at<int32_t>(3) : nullptr);
    });
}

// ---- boxes compared by overlap: suppression inside a set, matching of two sets (leon_pipeline_suppress_regions, _match_regions) ----
static_assert(sizeof(leon_pipeline_overlap_config) == 16 && sizeof(leon_pipeline_suppress_regions_call) == 96 && sizeof(leon_pipeline_match_regions_call) == 96 &&
              sizeof(leon::OverlapConfig) == 16 && sizeof(leon::OverlapCall) == 40, "include/leon_pipeline.h states the sizes");
static_assert(leon::kOverlapIou == LEON_OVERLAP_IOU && leon::kOverlapIomin == LEON_OVERLAP_IOMIN && leon::kOverlapMaxRows == leon::kProposeMaxBoxes,
              "the kernels' words are the header's");
// a CU's LDS holds the largest set and the largest pair
static_assert(leon::suppress_lds(leon::kOverlapMaxRows).bytes == 32768 && leon::match_lds(leon::kOverlapMaxRows, leon::kOverlapMaxRows).bytes == 49156 && 49156 <= 160 * 1024,
              "include/leon_pipeline.h states the LDS");

int overlap_config_check(const char* who, const leon_pipeline_overlap_config* cfg)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "null argument");
    if (cfg->measure != LEON_OVERLAP_IOU && cfg->measure != LEON_OVERLAP_IOMIN) return fail(LEON_ERR_INVALID, "%s: measure %d (LEON_OVERLAP_IOU 0, LEON_OVERLAP_IOMIN 1)", who, cfg->measure);
    if (cfg->threshold < 1 || cfg->threshold > leon::kOverlapMaxThreshold) return fail(LEON_ERR_INVALID, "%s: threshold %d (Q16, 1 .. 65536)", who, cfg->threshold);
    if (cfg->reserved[0] || cfg->reserved[1]) return fail(LEON_ERR_INVALID, "%s: a reserved word of the config is not 0", who);
    return LEON_OK;
}
// the rows of a set, and a suppress call's stride
int overlap_rows_check(const char* who, const char* noun, int32_t k)
{
    return k < 1 || k > leon::kOverlapMaxRows ? fail(LEON_ERR_INVALID, "%s: %s %d (a set has 1 .. 1024 rows)", who, noun, k) : LEON_OK;
}
int overlap_stride_check(int32_t score_stride)
{
    return score_stride < 1 || score_stride > leon::kOverlapMaxStride ? fail(LEON_ERR_INVALID, "suppress regions: score_stride %d (1 .. 8 words)", score_stride) : LEON_OK;
}
// the frame a record or diagnostic call names itself
int overlap_geometry_check(const char* who, int32_t fw, int32_t fh, int32_t n_frames)
{
    if (fw < 1 || fw > leon::kOverlapMaxFrame || fh < 1 || fh > leon::kOverlapMaxFrame) return fail(LEON_ERR_INVALID, "%s: a frame of %d x %d (1 .. 4096 an axis)", who, fw, fh);
    if (n_frames < 0) return fail(LEON_ERR_INVALID, "%s: %d frames", who, n_frames);
    return LEON_OK;
}
leon::OverlapCall overlap_call(const leon_pipeline_overlap_config& cfg, int32_t fw, int32_t fh, int32_t n_frames, int32_t n, int32_t ka, int32_t kb, int32_t score_stride)
{
    leon::OverlapCall C{};
    C.measure = cfg.measure; C.threshold = cfg.threshold;
    C.fw = fw; C.fh = fh; C.n_frames = n_frames;
    C.n = n; C.ka = ka; C.kb = kb;
    C.score_stride = score_stride;
    return C;
}

// the launches every road shares: a workgroup a set (pair), its LDS as leon_overlap.h lays it out for this K -- above 48 KiB the kernel
// is told so
int suppress_launch(hipStream_t st, const leon::OverlapCall& C, const int32_t* d_rows, const int32_t* d_scores, int32_t* d_out, int32_t* d_order, int32_t* d_by,
                    int32_t* d_count, int32_t* d_status)
{
    const uint32_t lds = leon::suppress_lds((uint32_t)C.ka).bytes;
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)leon::k_suppress, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(leon::k_suppress, dim3((unsigned)C.n), dim3(leon::kOverlapThreads), lds, st, d_rows, d_scores, d_out, d_order, d_by, d_count, d_status, C);
    return LEON_OK;
}
int match_launch(hipStream_t st, const leon::OverlapCall& C, const int32_t* d_a, const int32_t* d_b, int32_t* d_match_a, int32_t* d_match_b, int32_t* d_overlap,
                 int32_t* d_count, int32_t* d_status_a, int32_t* d_status_b)
{
    const uint32_t lds = leon::match_lds((uint32_t)C.ka, (uint32_t)C.kb).bytes;
    if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)leon::k_match, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(leon::k_match, dim3((unsigned)C.n), dim3(leon::kOverlapThreads), lds, st, d_a, d_b, d_match_a, d_match_b, d_overlap, d_count, d_status_a, d_status_b, C);
    return LEON_OK;
}

// the frames of a window that is out for delivery: from the window itself -- its tables are only built for the outputs that need them
int overlap_window_frames(leon_pipeline* p, int64_t window, int32_t* n_frames)
{
    return window_delivered(p, window, [&](const PipeWindow& w) { *n_frames = (int32_t)w.frames.size(); });
}

// The head of both device roads: the config, the call, regions_mu, the window, the call's reserved words, then the family's own checks
// (`checks()`: counts, null pointers, alignment), then inside the boxes bracket -- whose table is the window's frame count alone: the
// kernels read no ring -- `launch(st, n_frames)` on the caller's stream (or the regions stream and a wait)
template <class Call, class Checks, class Launch>
int overlap_road(leon_pipeline* p, int64_t window, const char* who, const leon_pipeline_overlap_config* cfg, const Call* c, Checks checks, Launch launch)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = overlap_config_check(who, cfg);
    if (rc != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    std::unique_lock<std::mutex> call(p->regions_mu);
    int32_t n_frames = 0;
    if ((rc = overlap_window_frames(p, window, &n_frames)) != LEON_OK) return rc;
    if ((rc = checks()) != LEON_OK) return rc;
    int launched = LEON_OK;
    const std::vector<uint32_t> table(1, (uint32_t)n_frames);
    rc = boxes_run(p, c->stream, call, table, pad256(4), [&](hipStream_t st, uint32_t*) { launched = launch(st, n_frames); });
    return rc != LEON_OK ? rc : launched;
}

int suppress_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_suppress_regions_call* c)
{
    const char* who = "suppress regions";
    return overlap_road(p, window, who, cfg, c, [&] {
        if (c->reserved0 || c->reserved[0] || c->reserved[1]) return fail(LEON_ERR_INVALID, "%s: a reserved word of the call is not 0", who);
        int rc = record_count_check(who, "sets", c->n);
        if (rc != LEON_OK || (rc = overlap_rows_check(who, "k", c->k)) != LEON_OK || (rc = overlap_stride_check(c->score_stride)) != LEON_OK) return rc;
        if (!c->regions || !c->device_by || !c->device_count)
            return fail(LEON_ERR_INVALID, "%s: null %s", who, !c->regions ? "regions" : !c->device_by ? "device_by" : "device_count");
        if (((uintptr_t)c->regions | (uintptr_t)c->scores | (uintptr_t)c->device_out | (uintptr_t)c->device_order | (uintptr_t)c->device_by | (uintptr_t)c->device_count |
             (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "%s: regions %p, scores %p, device_out %p, device_order %p, device_by %p, device_count %p, device_status %p: not all 4-byte aligned",
                        who, (const void*)c->regions, (const void*)c->scores, (void*)c->device_out, (void*)c->device_order, (void*)c->device_by, (void*)c->device_count,
                        (void*)c->device_status);
        return (int)LEON_OK;
    }, [&](hipStream_t st, int32_t n_frames) {
        return suppress_launch(st, overlap_call(*cfg, p->vinfo.frame_width, p->vinfo.frame_height, n_frames, c->n, c->k, 0, c->score_stride),
                               reinterpret_cast<const int32_t*>(c->regions), c->scores, reinterpret_cast<int32_t*>(c->device_out), c->device_order, c->device_by, c->device_count,
                               c->device_status);
    });
}

int match_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_match_regions_call* c)
{
    const char* who = "match regions";
    return overlap_road(p, window, who, cfg, c, [&] {
        if (c->reserved0 || c->reserved[0]) return fail(LEON_ERR_INVALID, "%s: a reserved word of the call is not 0", who);
        int rc = record_count_check(who, "pairs of sets", c->n);
        if (rc != LEON_OK || (rc = overlap_rows_check(who, "ka", c->ka)) != LEON_OK || (rc = overlap_rows_check(who, "kb", c->kb)) != LEON_OK) return rc;
        if (!c->a || !c->b || !c->device_match_a || !c->device_match_b || !c->device_overlap || !c->device_count)
            return fail(LEON_ERR_INVALID, "%s: null %s", who,
                        !c->a ? "a" : !c->b ? "b" : !c->device_match_a ? "device_match_a" : !c->device_match_b ? "device_match_b" : !c->device_overlap ? "device_overlap" : "device_count");
        if (((uintptr_t)c->a | (uintptr_t)c->b | (uintptr_t)c->device_match_a | (uintptr_t)c->device_match_b | (uintptr_t)c->device_overlap | (uintptr_t)c->device_count |
             (uintptr_t)c->device_status_a | (uintptr_t)c->device_status_b) & 3u)
            return fail(LEON_ERR_INVALID, "%s: a %p, b %p, device_match_a %p, device_match_b %p, device_overlap %p, device_count %p, device_status_a %p, device_status_b %p: "
                        "not all 4-byte aligned", who, (const void*)c->a, (const void*)c->b, (void*)c->device_match_a, (void*)c->device_match_b, (void*)c->device_overlap,
                        (void*)c->device_count, (void*)c->device_status_a, (void*)c->device_status_b);
        return (int)LEON_OK;
    }, [&](hipStream_t st, int32_t n_frames) {
        return match_launch(st, overlap_call(*cfg, p->vinfo.frame_width, p->vinfo.frame_height, n_frames, c->n, c->ka, c->kb, 1), reinterpret_cast<const int32_t*>(c->a),
                            reinterpret_cast<const int32_t*>(c->b), c->device_match_a, c->device_match_b, c->device_overlap, c->device_count, c->device_status_a,
                            c->device_status_b);
    });
}

// what the host roads, the record calls and the diagnostics judge of their own arguments, in the device road's order
int suppress_args_check(const leon_pipeline_overlap_config* cfg, int32_t n, int32_t k, int32_t score_stride, const void* regions, const void* by, const void* count)
{
    const char* who = "suppress regions";
    int rc = overlap_config_check(who, cfg);
    if (rc != LEON_OK || (rc = record_count_check(who, "sets", n)) != LEON_OK || (rc = overlap_rows_check(who, "k", k)) != LEON_OK ||
        (rc = overlap_stride_check(score_stride)) != LEON_OK)
        return rc;
    if (!regions || !by || !count) return fail(LEON_ERR_INVALID, "%s: null %s", who, !regions ? "regions" : !by ? "by" : "count");
    return LEON_OK;
}
int match_args_check(const leon_pipeline_overlap_config* cfg, int32_t n, int32_t ka, int32_t kb, const void* a, const void* b, const void* match_a, const void* match_b,
                     const void* overlap, const void* count)
{
    const char* who = "match regions";
    int rc = overlap_config_check(who, cfg);
    if (rc != LEON_OK || (rc = record_count_check(who, "pairs of sets", n)) != LEON_OK || (rc = overlap_rows_check(who, "ka", ka)) != LEON_OK ||
        (rc = overlap_rows_check(who, "kb", kb)) != LEON_OK)
        return rc;
    if (!a || !b || !match_a || !match_b || !overlap || !count)
        return fail(LEON_ERR_INVALID, "%s: null %s", who, !a ? "a" : !b ? "b" : !match_a ? "match_a" : !match_b ? "match_b" : !overlap ? "overlap" : "count");
    return LEON_OK;
}

// the pieces of a suppress call that goes up and comes back: [out | order | by | count | status | rows | scores]
#define LEON_SUPPRESS_PIECES {{out, out, rows * 32}, {order, order, rows * 4}, {by, by, rows * 4}, {count, count, (size_t)n * 4}, {status, status, rows * 4}, \
                              {regions, nullptr, rows * 32}, {scores, nullptr, scores ? rows * 4 * (size_t)score_stride : 0}}
#define LEON_MATCH_PIECES {{match_a, match_a, ra * 4}, {match_b, match_b, rb * 4}, {overlap, overlap, ra * 4}, {count, count, (size_t)n * 4}, {status_a, status_a, ra * 4}, \
                           {status_b, status_b, rb * 4}, {a, nullptr, ra * 32}, {b, nullptr, rb * 32}}

int suppress_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* regions, int32_t n, int32_t k,
                     const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = overlap_config_check("suppress regions", cfg);
    if (rc != LEON_OK) return rc;
    int32_t n_frames = 0;
    {
        std::unique_lock<std::mutex> call(p->regions_mu);
        if ((rc = overlap_window_frames(p, window, &n_frames)) != LEON_OK) return rc;
    }
    if ((rc = suppress_args_check(cfg, n, k, score_stride, regions, by, count)) != LEON_OK) return rc;
    const size_t rows = (size_t)n * (size_t)k;
    return pieces_run(p->cfg.device_id, "suppress", LEON_SUPPRESS_PIECES, [&](const Pieces& s) {
        leon_pipeline_suppress_regions_call c{};
        c.regions = s.at<const leon_pipeline_region>(5);
        c.scores = scores ? s.at<const int32_t>(6) : nullptr;
        c.n = n; c.k = k; c.score_stride = score_stride;
        c.device_out = out ? s.at<leon_pipeline_region>(0) : nullptr;
        c.device_order = order ? s.at<int32_t>(1) : nullptr;
        c.device_by = s.at<int32_t>(2);
        c.device_count = s.at<int32_t>(3);
        c.device_status = status ? s.at<int32_t>(4) : nullptr;
        return suppress_regions_device(p, window, cfg, &c);
    });
}

int match_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a, int32_t ka, const leon_pipeline_region* b,
                  int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count, int32_t* status_a, int32_t* status_b)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = overlap_config_check("match regions", cfg);
    if (rc != LEON_OK) return rc;
    int32_t n_frames = 0;
    {
        std::unique_lock<std::mutex> call(p->regions_mu);
        if ((rc = overlap_window_frames(p, window, &n_frames)) != LEON_OK) return rc;
    }
    if ((rc = match_args_check(cfg, n, ka, kb, a, b, match_a, match_b, overlap, count)) != LEON_OK) return rc;
    const size_t ra = (size_t)n * (size_t)ka, rb = (size_t)n * (size_t)kb;
    return pieces_run(p->cfg.device_id, "match", LEON_MATCH_PIECES, [&](const Pieces& s) {
        leon_pipeline_match_regions_call c{};
        c.a = s.at<const leon_pipeline_region>(6);
        c.b = s.at<const leon_pipeline_region>(7);
        c.n = n; c.ka = ka; c.kb = kb;
        c.device_match_a = s.at<int32_t>(0);
        c.device_match_b = s.at<int32_t>(1);
        c.device_overlap = s.at<int32_t>(2);
        c.device_count = s.at<int32_t>(3);
        c.device_status_a = status_a ? s.at<int32_t>(4) : nullptr;
        c.device_status_b = status_b ? s.at<int32_t>(5) : nullptr;
        return match_regions_device(p, window, cfg, &c);
    });
}

// the definitions on the CPU for one set (pair): the checks, then leon_overlap.h's host texts
int32_t suppress_record_host(int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* regions, int32_t k,
                             const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    int rc = overlap_config_check("suppress regions", cfg);
    if (rc != LEON_OK || (rc = overlap_geometry_check("suppress regions", fw, fh, n_frames)) != LEON_OK ||
        (rc = suppress_args_check(cfg, 1, k, score_stride, regions, by, count)) != LEON_OK)
        return rc;
    leon::suppress_set_host(overlap_call(*cfg, fw, fh, n_frames, 1, k, 0, score_stride), reinterpret_cast<const int32_t*>(regions), scores, reinterpret_cast<int32_t*>(out),
                            order, by, count, status);
    return LEON_OK;
}
int32_t match_record_host(int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a, int32_t ka,
                          const leon_pipeline_region* b, int32_t kb, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count, int32_t* status_a, int32_t* status_b)
{
    int rc = overlap_config_check("match regions", cfg);
    if (rc != LEON_OK || (rc = overlap_geometry_check("match regions", fw, fh, n_frames)) != LEON_OK ||
        (rc = match_args_check(cfg, 1, ka, kb, a, b, match_a, match_b, overlap, count)) != LEON_OK)
        return rc;
    leon::match_set_host(overlap_call(*cfg, fw, fh, n_frames, 1, ka, kb, 1), reinterpret_cast<const int32_t*>(a), reinterpret_cast<const int32_t*>(b), match_a, match_b,
                         overlap, count, status_a, status_b);
    return LEON_OK;
}

// k_suppress / k_match on rows the caller supplies (leon_pipeline_suppress_kernel, _match_kernel): memory of their own, the null stream
int suppress_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* regions, int32_t n,
                    int32_t k, const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    int rc = overlap_config_check("suppress regions", cfg);
    if (rc != LEON_OK || (rc = overlap_geometry_check("suppress regions", fw, fh, n_frames)) != LEON_OK ||
        (rc = suppress_args_check(cfg, n, k, score_stride, regions, by, count)) != LEON_OK)
        return rc;
    const size_t rows = (size_t)n * (size_t)k;
    return pieces_run(device_id, "suppress", LEON_SUPPRESS_PIECES, [&](const Pieces& s) {
        return suppress_launch(nullptr, overlap_call(*cfg, fw, fh, n_frames, n, k, 0, score_stride), s.at<const int32_t>(5), scores ? s.at<const int32_t>(6) : nullptr,
                               out ? s.at<int32_t>(0) : nullptr, order ? s.at<int32_t>(1) : nullptr, s.at<int32_t>(2), s.at<int32_t>(3), status ? s.at<int32_t>(4) : nullptr);
    });
}
int match_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a, int32_t ka,
                 const leon_pipeline_region* b, int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count, int32_t* status_a,
                 int32_t* status_b)
{
    int rc = overlap_config_check("match regions", cfg);
    if (rc != LEON_OK || (rc = overlap_geometry_check("match regions", fw, fh, n_frames)) != LEON_OK ||
        (rc = match_args_check(cfg, n, ka, kb, a, b, match_a, match_b, overlap, count)) != LEON_OK)
        return rc;
    const size_t ra = (size_t)n * (size_t)ka, rb = (size_t)n * (size_t)kb;
    return pieces_run(device_id, "match", LEON_MATCH_PIECES, [&](const Pieces& s) {
        return match_launch(nullptr, overlap_call(*cfg, fw, fh, n_frames, n, ka, kb, 1), s.at<const int32_t>(6), s.at<const int32_t>(7), s.at<int32_t>(0), s.at<int32_t>(1),
                            s.at<int32_t>(2), s.at<int32_t>(3), status_a ? s.at<int32_t>(4) : nullptr, status_b ? s.at<int32_t>(5) : nullptr);
    });
}
#undef LEON_SUPPRESS_PIECES
#undef LEON_MATCH_PIECES

// ---- dense maps propagated along the motion vectors (leon_pipeline_propagate_maps) ------------------------------------------------
static_assert(sizeof(leon_pipeline_propagate_hop) == 32 && sizeof(leon_pipeline_propagate_config) == 40 && sizeof(struct leon_pipeline_propagate_layout) == 32 &&
              sizeof(leon_pipeline_propagate_maps_call) == 64 && sizeof(leon::PropagateHop) == sizeof(leon_pipeline_propagate_hop), "include/leon_pipeline.h states the sizes");
static_assert(leon::kRegionSlot == LEON_REGION_SLOT, "the kernel's code is the header's");

// what a call's maps may be: the geometry (leon_propagate.h) and the caller's buffer around it
int propagate_config_check(int32_t fw, int32_t fh, int32_t mbw, const leon_pipeline_propagate_config* cfg, leon::PropagateGeom* g)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "propagate: null cfg");
    if (cfg->reserved0) return fail(LEON_ERR_INVALID, "propagate: a reserved word of cfg is not 0");
    if (!leon::propagate_geometry(fw, fh, mbw, cfg->stride, cfg->planes, cfg->elem_bytes, g))
        return fail(LEON_ERR_INVALID, "propagate: stride %d (1, 2, 4, 8, 16), %d planes (1 .. %d), elem_bytes %d (1, 2, 4)", cfg->stride, cfg->planes, leon::kPropagateMaxPlanes,
                    cfg->elem_bytes);
    if (cfg->n_slots < 1 || cfg->n_slots > leon::kPropagateMaxSlots) return fail(LEON_ERR_INVALID, "propagate: %d slots (1 .. %d)", cfg->n_slots, leon::kPropagateMaxSlots);
    const uint64_t slot_bytes = (uint64_t)g->planes * g->plane_bytes;
    if (cfg->slot_pitch_bytes % 4 || cfg->slot_pitch_bytes < slot_bytes)
        return fail(LEON_ERR_INVALID, "propagate: slot_pitch_bytes %llu (a multiple of 4 not below the map's %llu bytes)", (unsigned long long)cfg->slot_pitch_bytes,
                    (unsigned long long)slot_bytes);
    if (cfg->maps_bytes / (uint64_t)cfg->n_slots < cfg->slot_pitch_bytes)
        return fail(LEON_ERR_INVALID, "propagate: maps_bytes %llu is below %d slots of %llu bytes", (unsigned long long)cfg->maps_bytes, cfg->n_slots,
                    (unsigned long long)cfg->slot_pitch_bytes);
    return LEON_OK;
}

// the launch every road shares: hops, the window's table, the motion ring and the maps in device memory
void propagate_launch(hipStream_t st, const leon::PropagateHop* d_hops, const leon::CarryFrame* d_frames, const uint8_t* d_ring, const leon::PropagateGeom& g,
                      const leon::MotionLayout& lay, int32_t n_frames, const leon_pipeline_propagate_config& cfg, int32_t n, uint8_t* d_maps, uint8_t* d_via, int32_t* d_status)
{
    leon::PropagateCall C{};
    C.g = g;
    C.slot_pitch = (size_t)cfg.slot_pitch_bytes; C.maps_bytes = (size_t)cfg.maps_bytes;
    C.n_frames = n_frames; C.n_slots = cfg.n_slots;
    C.fill = cfg.fill;
    C.info_offset = lay.info_offset; C.record_pitch = lay.record_pitch;
    const dim3 grid((g.units + leon::kRgbaBlock - 1) / leon::kRgbaBlock, (unsigned)((g.planes + g.group - 1) / g.group), (unsigned)n);
    hipLaunchKernelGGL(leon::k_propagate, grid, dim3(leon::kRgbaBlock), 0, st, d_hops, d_frames, d_ring, d_maps, d_via, d_status, C);
}

// One call of the device road: the host's refusals (the config's behind the alignment's), then one launch
int propagate_maps_device(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_maps_call* c)
{
    if (const int rc = carry_pipeline_check(p); rc != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    leon::PropagateGeom g;
    return table_road(p, window, c->stream, "propagate maps", "hops", c->n, c->reserved0 || c->reserved[0] || c->reserved[1], [&] {
        if (!c->hops) return fail(LEON_ERR_INVALID, "propagate maps: null hops");
        if (!c->maps) return fail(LEON_ERR_INVALID, "propagate maps: null maps");
        if (((uintptr_t)c->hops | (uintptr_t)c->maps | (uintptr_t)c->device_via | (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "propagate maps: hops %p, maps %p, device_via %p, device_status %p: not all 4-byte aligned", (const void*)c->hops, c->maps,
                        (void*)c->device_via, (void*)c->device_status);
        return propagate_config_check(p->vinfo.frame_width, p->vinfo.frame_height, p->vinfo.mb_width, cfg, &g);
    }, [&](hipStream_t st, const leon::CarryFrame* d_frames, int32_t n_frames) {
        propagate_launch(st, reinterpret_cast<const leon::PropagateHop*>(c->hops), d_frames, p->motion.ring, g, p->motion_lay, n_frames, *cfg, c->n,
                         static_cast<uint8_t*>(c->maps), c->device_via, c->device_status);
    });
}

// One call of the host road: [hops | status | via | maps], the maps and what the caller has in via and status going up first
int propagate_maps(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* maps, uint8_t* via,
                   int32_t* status)
{
    int rc = carry_pipeline_check(p);
    if (rc != LEON_OK) return rc;
    if (!hops || !maps) return fail(LEON_ERR_INVALID, "propagate maps: null %s", hops ? "maps" : "hops");
    if ((rc = record_count_check("propagate maps", "hops", n)) != LEON_OK) return rc;
    leon::PropagateGeom g;
    if ((rc = propagate_config_check(p->vinfo.frame_width, p->vinfo.frame_height, p->vinfo.mb_width, cfg, &g)) != LEON_OK) return rc;
    const size_t via_bytes = (size_t)n * (size_t)g.mh * (size_t)g.mw;
    return table_host_road(p, window, "propagate", {{hops, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4}, {via, via, via_bytes}, {maps, maps, (size_t)cfg->maps_bytes}},
                           [&](const Pieces& s) {
        leon_pipeline_propagate_maps_call c{};
        c.hops = s.at<const leon_pipeline_propagate_hop>(0);
        c.n = n;
        c.maps = s.at(3);
        c.device_via = via ? s.at(2) : nullptr;
        c.device_status = status ? s.at<int32_t>(1) : nullptr;
        return propagate_maps_device(p, window, cfg, &c);
    });
}

// what the CPU road and the diagnostic refuse of their geometry
int propagate_host_check(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* records, const leon_pipeline_propagate_config* cfg,
                         const void* hops, const void* maps, leon::PropagateGeom* g)
{
    if (!records || !cfg || !hops || !maps) return fail(LEON_ERR_INVALID, "null argument");
    int rc = carry_geometry_check(fw, fh, mbw, mbh, n_frames);
    if (rc != LEON_OK || (rc = propagate_config_check(fw, fh, mbw, cfg, g)) != LEON_OK) return rc;
    if ((uintptr_t)maps & 3u) return fail(LEON_ERR_INVALID, "propagate: maps %p is not 4-byte aligned", maps);
    return LEON_OK;
}

// the definition on the CPU: the same text (leon_propagate.h), every unit of every plane; the status word, or a negative error
int32_t propagate_record_host(int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* records, const leon_pipeline_propagate_config* cfg,
                              const leon_pipeline_propagate_hop* hop, void* maps, uint8_t* via)
{
    leon::PropagateGeom g;
    const int rc = propagate_host_check(fw, fh, mbw, mbh, n_frames, records, cfg, hop, maps, &g);
    if (rc != LEON_OK) return rc;
    const leon::PropagateHop& h = reinterpret_cast<const leon::PropagateHop&>(*hop);
    const int32_t st = leon::propagate_hop_status(h, n_frames, cfg->n_slots);
    if (st != leon::kRegionOk) return st;
    const uint8_t* record = static_cast<const uint8_t*>(records[h.target]);
    if (!record) return fail(LEON_ERR_INVALID, "propagate: frame %d is the target and has no record", h.target);
    if ((uintptr_t)record & 3u) return fail(LEON_ERR_INVALID, "propagate: record %p is not 4-byte aligned", (const void*)record);
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    for (uint32_t u = 0; u < g.units; u++)
        leon::propagate_unit(g, record, L.info_offset, static_cast<uint8_t*>(maps), (size_t)cfg->maps_bytes, (size_t)cfg->slot_pitch_bytes, h, cfg->fill, via, u, 0, g.planes);
    return leon::kRegionOk;
}

// k_propagate on records the caller supplies (leon_pipeline_propagate_kernel): memory of its own, the null stream
int propagate_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t mbw, int32_t mbh, int32_t n_frames, const void* const* records,
                     const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* maps, uint8_t* via, int32_t* status)
{
    leon::PropagateGeom g;
    int rc = propagate_host_check(fw, fh, mbw, mbh, n_frames, records, cfg, hops, maps, &g);
    if (rc != LEON_OK) return rc;
    if ((rc = record_count_check("propagate maps", "hops", n)) != LEON_OK) return rc;
    for (int32_t i = 0; i < n; i++) {          // a record that is read must be there
        const leon::PropagateHop& h = reinterpret_cast<const leon::PropagateHop&>(hops[i]);
        if (leon::propagate_hop_status(h, n_frames, cfg->n_slots) == leon::kRegionOk && !records[h.target])
            return fail(LEON_ERR_INVALID, "propagate: frame %d is the target of hop %d and has no record", h.target, i);
    }
    const leon::MotionLayout L = leon::motion_layout((uint32_t)mbw, (uint32_t)mbh);
    uint32_t slots;
    const std::vector<leon::CarryFrame> table = kernel_table(n_frames, nullptr, nullptr, [&](size_t i) { return records[i] != nullptr; }, &slots);
    const std::vector<uint8_t> ring = kernel_ring(table, slots, records, L.record_bytes, L.record_pitch);
    const size_t via_bytes = (size_t)n * (size_t)g.mh * (size_t)g.mw;
    return pieces_run(device_id, "propagate", {{hops, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4}, {via, via, via_bytes}, {maps, maps, (size_t)cfg->maps_bytes},
                                               {table.data(), nullptr, table.size() * sizeof(leon::CarryFrame)}, {ring.data(), nullptr, ring.size()}}, [&](const Pieces& s) {
        propagate_launch(nullptr, s.at<const leon::PropagateHop>(0), s.at<const leon::CarryFrame>(4), s.at(5), g, L, n_frames, *cfg, n, s.at(3), via ? s.at(2) : nullptr,
                         status ? s.at<int32_t>(1) : nullptr);
        return (int)LEON_OK;
    });
}

// ---- motion and residual accumulated along a GOP's chain (leon_pipeline_accumulate) -------------------------------------------------
static_assert(sizeof(leon_pipeline_accumulate_config) == 32 && sizeof(struct leon_pipeline_accumulate_layout) == 64 && sizeof(leon_pipeline_accumulate_call) == 64,
              "include/leon_pipeline.h states the sizes");
static_assert(leon::kAccumulateMotion == LEON_ACCUMULATE_MOTION && leon::kAccumulateResidual == LEON_ACCUMULATE_RESIDUAL, "the kernel's bits are the header's");

// what a call's accumulators may be: the geometry (leon_accumulate.h) and the caller's buffer around it
int accumulate_config_check(int32_t cw, int32_t ch, const leon_pipeline_accumulate_config* cfg, leon::AccumulateGeom* g)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "accumulate: null cfg");
    if (cfg->reserved[0] | cfg->reserved[1]) return fail(LEON_ERR_INVALID, "accumulate: a reserved word of cfg is not 0");
    if (cfg->parts < 1 || cfg->parts > (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL))
        return fail(LEON_ERR_INVALID, "accumulate: parts %d (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3)", cfg->parts);
    if (const int rc = residual_size_check("accumulate", cw, ch); rc != LEON_OK) return rc;
    leon::accumulate_geometry(cw, ch, cfg->parts, g);
    if (cfg->n_slots < 1 || cfg->n_slots > leon::kPropagateMaxSlots) return fail(LEON_ERR_INVALID, "accumulate: %d slots (1 .. %d)", cfg->n_slots, leon::kPropagateMaxSlots);
    if (cfg->slot_pitch_bytes % 4 || cfg->slot_pitch_bytes < g->slot_bytes)
        return fail(LEON_ERR_INVALID, "accumulate: slot_pitch_bytes %llu (a multiple of 4 not below the accumulator's %u bytes)", (unsigned long long)cfg->slot_pitch_bytes,
                    g->slot_bytes);
    if (cfg->slots_bytes / (uint64_t)cfg->n_slots < cfg->slot_pitch_bytes)
        return fail(LEON_ERR_INVALID, "accumulate: slots_bytes %llu is below %d slots of %llu bytes", (unsigned long long)cfg->slots_bytes, cfg->n_slots,
                    (unsigned long long)cfg->slot_pitch_bytes);
    return LEON_OK;
}

int accumulate_layout_host(int32_t cw, int32_t ch, int32_t parts, struct leon_pipeline_accumulate_layout* out)
{
    if (!out) return fail(LEON_ERR_INVALID, "null argument");
    if (const int rc = residual_size_check("accumulate layout", cw, ch); rc != LEON_OK) return rc;
    leon::AccumulateGeom g;
    if (!leon::accumulate_geometry(cw, ch, parts, &g)) return fail(LEON_ERR_INVALID, "accumulate layout: parts %d (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3)", parts);
    memset(out, 0, sizeof(*out));
    out->coded_width = cw; out->coded_height = ch; out->parts = parts; out->planes = g.planes;
    out->luma_stride = (int32_t)g.luma_stride; out->chroma_stride = (int32_t)g.chroma_stride;
    out->ax_offset = g.off[leon::kAccAX]; out->ay_offset = g.off[leon::kAccAY]; out->age_offset = g.off[leon::kAccAGE];
    out->ry_offset = g.off[leon::kAccRY]; out->rcb_offset = g.off[leon::kAccRCb]; out->rcr_offset = g.off[leon::kAccRCr];
    out->slot_bytes = g.slot_bytes; out->slot_pitch = (uint32_t)pad256(g.slot_bytes);
    return LEON_OK;
}

// the launch every road shares: hops, the window's table, the two rings (the residual ring null where the parts do not read it) and
// the accumulators in device memory; x sized for a luma plane
void accumulate_launch(hipStream_t st, const leon::PropagateHop* d_hops, const leon::CarryFrame* d_frames, const uint8_t* d_motion, const uint8_t* d_residual,
                       const leon::AccumulateGeom& g, const leon::MotionLayout& ml, const leon::ResidualLayout& rl, int32_t n_frames,
                       const leon_pipeline_accumulate_config& cfg, int32_t n, uint8_t* d_slots, uint8_t* d_via, int32_t* d_status)
{
    leon::AccumulateCall C{};
    C.g = g;
    C.slot_pitch = (size_t)cfg.slot_pitch_bytes; C.slots_bytes = (size_t)cfg.slots_bytes;
    C.n_frames = n_frames; C.n_slots = cfg.n_slots;
    C.info_offset = ml.info_offset; C.motion_pitch = ml.record_pitch; C.residual_pitch = rl.record_pitch;
    const dim3 grid((g.units_luma + leon::kRgbaBlock - 1) / leon::kRgbaBlock, (unsigned)g.planes, (unsigned)n);
    hipLaunchKernelGGL(leon::k_accumulate, grid, dim3(leon::kRgbaBlock), 0, st, d_hops, d_frames, d_motion, (cfg.parts & LEON_ACCUMULATE_RESIDUAL) ? d_residual : nullptr, d_slots,
                       d_via, d_status, C);
}

// the record outputs a call's parts need are the pipeline's: MOTION always, RESIDUAL for its part
int accumulate_outputs_check(const leon_pipeline* p, int32_t parts)
{
    if (!p->motion.ring) return no_output("motion", "MOTION");
    if ((parts & LEON_ACCUMULATE_RESIDUAL) && !p->residual.ring) return no_output("residual", "RESIDUAL");
    return LEON_OK;
}
int accumulate_parts_check(const leon_pipeline_accumulate_config* cfg)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "accumulate: null cfg");
    if (cfg->parts < 1 || cfg->parts > (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL))
        return fail(LEON_ERR_INVALID, "accumulate: parts %d (LEON_ACCUMULATE_MOTION | LEON_ACCUMULATE_RESIDUAL: 1 .. 3)", cfg->parts);
    return LEON_OK;
}

// One call of the device road: the host's refusals (the parts' and the outputs' before the window's, as gauge's), then one launch
int accumulate_device(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_accumulate_call* c)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = accumulate_parts_check(cfg);
    if (rc != LEON_OK || (rc = accumulate_outputs_check(p, cfg->parts)) != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    leon::AccumulateGeom g;
    return table_road(p, window, c->stream, "accumulate", "hops", c->n, c->reserved0 || c->reserved[0] || c->reserved[1], [&] {
        if (!c->hops) return fail(LEON_ERR_INVALID, "accumulate: null hops");
        if (!c->slots) return fail(LEON_ERR_INVALID, "accumulate: null slots");
        if (((uintptr_t)c->hops | (uintptr_t)c->slots | (uintptr_t)c->device_status) & 3u)
            return fail(LEON_ERR_INVALID, "accumulate: hops %p, slots %p, device_status %p: not all 4-byte aligned", (const void*)c->hops, c->slots, (void*)c->device_status);
        return accumulate_config_check(p->vinfo.coded_width, p->vinfo.coded_height, cfg, &g);
    }, [&](hipStream_t st, const leon::CarryFrame* d_frames, int32_t n_frames) {
        accumulate_launch(st, reinterpret_cast<const leon::PropagateHop*>(c->hops), d_frames, p->motion.ring, p->residual.ring, g, p->motion_lay, p->residual_lay, n_frames, *cfg,
                          c->n, static_cast<uint8_t*>(c->slots), c->device_via, c->device_status);
    });
}

// One call of the host road: [hops | status | via | slots], the accumulators and what the caller has in via and status going up first
int accumulate(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* slots, uint8_t* via,
               int32_t* status)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = accumulate_parts_check(cfg);
    if (rc != LEON_OK || (rc = accumulate_outputs_check(p, cfg->parts)) != LEON_OK) return rc;
    if (!hops || !slots) return fail(LEON_ERR_INVALID, "accumulate: null %s", hops ? "slots" : "hops");
    if ((rc = record_count_check("accumulate", "hops", n)) != LEON_OK) return rc;
    leon::AccumulateGeom g;
    if ((rc = accumulate_config_check(p->vinfo.coded_width, p->vinfo.coded_height, cfg, &g)) != LEON_OK) return rc;
    const size_t via_bytes = (size_t)n * (size_t)g.mbw * (size_t)(g.ch >> 4);
    return table_host_road(p, window, "accumulate", {{hops, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4}, {via, via, via_bytes}, {slots, slots, (size_t)cfg->slots_bytes}},
                           [&](const Pieces& s) {
        leon_pipeline_accumulate_call c{};
        c.hops = s.at<const leon_pipeline_propagate_hop>(0);
        c.n = n;
        c.slots = s.at(3);
        c.device_via = via ? s.at(2) : nullptr;
        c.device_status = status ? s.at<int32_t>(1) : nullptr;
        return accumulate_device(p, window, cfg, &c);
    });
}

// what the CPU road and the diagnostic refuse of their geometry
int accumulate_host_check(int32_t cw, int32_t ch, int32_t n_frames, const void* const* motion, const void* const* residual, const leon_pipeline_accumulate_config* cfg,
                          const void* hops, const void* slots, leon::AccumulateGeom* g)
{
    if (!motion || !cfg || !hops || !slots) return fail(LEON_ERR_INVALID, "null argument");
    if (n_frames < 0) return fail(LEON_ERR_INVALID, "accumulate: %d frames", n_frames);
    if (const int rc = accumulate_config_check(cw, ch, cfg, g); rc != LEON_OK) return rc;
    if ((cfg->parts & LEON_ACCUMULATE_RESIDUAL) && !residual) return fail(LEON_ERR_INVALID, "accumulate: null residual records with LEON_ACCUMULATE_RESIDUAL");
    if ((uintptr_t)slots & 3u) return fail(LEON_ERR_INVALID, "accumulate: slots %p is not 4-byte aligned", slots);
    return LEON_OK;
}
// the records a valid hop reads must be there
int accumulate_records_check(const leon::PropagateHop& h, int32_t i, int32_t parts, const void* const* motion, const void* const* residual)
{
    if (!motion[h.target]) return fail(LEON_ERR_INVALID, "accumulate: frame %d is the target of hop %d and has no motion record", h.target, i);
    if ((parts & LEON_ACCUMULATE_RESIDUAL) && !residual[h.target]) return fail(LEON_ERR_INVALID, "accumulate: frame %d is the target of hop %d and has no residual record", h.target, i);
    return LEON_OK;
}

// the definition on the CPU: the same text (leon_accumulate.h), every unit of every plane asked for; the status word, or a negative error
int32_t accumulate_record_host(int32_t cw, int32_t ch, int32_t n_frames, const void* const* motion, const void* const* residual, const leon_pipeline_accumulate_config* cfg,
                               const leon_pipeline_propagate_hop* hop, void* slots, uint8_t* via)
{
    leon::AccumulateGeom g;
    int rc = accumulate_host_check(cw, ch, n_frames, motion, residual, cfg, hop, slots, &g);
    if (rc != LEON_OK) return rc;
    const leon::PropagateHop& h = reinterpret_cast<const leon::PropagateHop&>(*hop);
    const int32_t st = leon::propagate_hop_status(h, n_frames, cfg->n_slots);
    if (st != leon::kRegionOk) return st;
    if ((rc = accumulate_records_check(h, 0, cfg->parts, motion, residual)) != LEON_OK) return rc;
    const uint8_t* mrec = static_cast<const uint8_t*>(motion[h.target]);
    const uint8_t* rrec = (cfg->parts & LEON_ACCUMULATE_RESIDUAL) ? static_cast<const uint8_t*>(residual[h.target]) : nullptr;
    if (((uintptr_t)mrec & 3u) || ((uintptr_t)rrec & 7u)) return fail(LEON_ERR_INVALID, "accumulate: records %p (4-byte aligned), %p (8-byte aligned)", (const void*)mrec, (const void*)rrec);
    const leon::MotionLayout L = leon::motion_layout((uint32_t)g.mbw, (uint32_t)(ch >> 4));
    for (int32_t q = 0; q < g.planes; q++)
        for (uint32_t u = 0; u < leon::accumulate_units(g, q); u++)
            leon::accumulate_unit(g, mrec, L.info_offset, rrec, static_cast<uint8_t*>(slots), (size_t)cfg->slots_bytes, (size_t)cfg->slot_pitch_bytes, h, q == 0 ? via : nullptr, q, u);
    return leon::kRegionOk;
}

// k_accumulate on records the caller supplies (leon_pipeline_accumulate_kernel): memory of its own, the null stream
int accumulate_kernel(int32_t device_id, int32_t cw, int32_t ch, int32_t n_frames, const void* const* motion, const void* const* residual,
                      const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* slots, uint8_t* via, int32_t* status)
{
    leon::AccumulateGeom g;
    int rc = accumulate_host_check(cw, ch, n_frames, motion, residual, cfg, hops, slots, &g);
    if (rc != LEON_OK) return rc;
    if ((rc = record_count_check("accumulate", "hops", n)) != LEON_OK) return rc;
    const bool res = (cfg->parts & LEON_ACCUMULATE_RESIDUAL) != 0;
    for (int32_t i = 0; i < n; i++) {
        const leon::PropagateHop& h = reinterpret_cast<const leon::PropagateHop&>(hops[i]);
        if (leon::propagate_hop_status(h, n_frames, cfg->n_slots) == leon::kRegionOk && (rc = accumulate_records_check(h, i, cfg->parts, motion, residual)) != LEON_OK) return rc;
    }
    const int32_t mbh = ch >> 4;
    const leon::MotionLayout ML = leon::motion_layout((uint32_t)g.mbw, (uint32_t)mbh);
    const leon::ResidualLayout RL = leon::residual_layout((uint32_t)cw, (uint32_t)ch);
    // a frame with a record of either kind gets a slot in both rings, as the pipeline's rings share an index
    uint32_t ring_slots;
    const std::vector<leon::CarryFrame> table = kernel_table(n_frames, nullptr, nullptr, [&](size_t i) { return motion[i] || (res && residual[i]); }, &ring_slots);
    const std::vector<uint8_t> mring = kernel_ring(table, ring_slots, motion, ML.record_bytes, ML.record_pitch);
    const std::vector<uint8_t> rring = kernel_ring(table, ring_slots, res ? residual : nullptr, RL.record_bytes, RL.record_pitch);
    const size_t via_bytes = (size_t)n * (size_t)g.mbw * (size_t)mbh;
    return pieces_run(device_id, "accumulate", {{hops, nullptr, (size_t)n * 32}, {status, status, (size_t)n * 4}, {via, via, via_bytes}, {slots, slots, (size_t)cfg->slots_bytes},
                                                {table.data(), nullptr, table.size() * sizeof(leon::CarryFrame)}, {mring.data(), nullptr, mring.size()},
                                                {rring.data(), nullptr, rring.size()}}, [&](const Pieces& s) {
        accumulate_launch(nullptr, s.at<const leon::PropagateHop>(0), s.at<const leon::CarryFrame>(4), s.at(5), res ? s.at(6) : nullptr, g, ML, RL, n_frames, *cfg, n, s.at(3),
                          via ? s.at(2) : nullptr, status ? s.at<int32_t>(1) : nullptr);
        return (int)LEON_OK;
    });
}

// ---- boxes of int16 fields as a model's tensors (leon_pipeline_field_tensors) ---------------------------------------------------------
static_assert(sizeof(leon_pipeline_field_channel) == 32 && sizeof(leon_pipeline_field_config) == 304 && sizeof(leon_pipeline_field_tensors_call) == 64 &&
              sizeof(leon::FieldChannel) == sizeof(leon_pipeline_field_channel), "include/leon_pipeline.h states the sizes");
static_assert(leon::kFieldSourceBuffer == LEON_FIELD_SOURCE_BUFFER && leon::kFieldSourceMotion == LEON_FIELD_SOURCE_MOTION && leon::kFieldSourceResidual == LEON_FIELD_SOURCE_RESIDUAL &&
              leon::kFieldF16 == LEON_TENSOR_F16 && leon::kFieldBF16 == LEON_TENSOR_BF16 && leon::kFieldF32 == LEON_TENSOR_F32 && leon::kFieldMaxChannels == LEON_FIELD_MAX_CHANNELS,
              "the kernel's codes are the header's");
static_assert(sizeof(leon::FieldTile) <= 65536, "k_fields' static LDS");
typedef void (*FieldsKernel)(const uint8_t*, uint8_t*, const leon::RegionDesc*, const int32_t*, leon::FieldCall);
constexpr FieldsKernel kFieldsKernels[3] = {leon::k_fields<LEON_TENSOR_F16>, leon::k_fields<LEON_TENSOR_BF16>, leon::k_fields<LEON_TENSOR_F32>};

int field_source_check(const leon_pipeline_field_config* cfg)
{
    if (!cfg) return fail(LEON_ERR_INVALID, "field tensors: null cfg");
    if (cfg->source < LEON_FIELD_SOURCE_BUFFER || cfg->source > LEON_FIELD_SOURCE_RESIDUAL)
        return fail(LEON_ERR_INVALID, "field tensors: source %d (LEON_FIELD_SOURCE_BUFFER, _MOTION, _RESIDUAL: 0 .. 2)", cfg->source);
    return LEON_OK;
}
// What a call's config can be refused for.  limit: the bytes of an item its channels must lie in, 0: item_pitch_bytes; items: whether
// the item geometry is the caller's (a BUFFER source, and every source of the CPU road and the diagnostic)
int field_config_check(int32_t fw, int32_t fh, const leon_pipeline_field_config* cfg, uint64_t limit, bool items)
{
    if (const int rc = field_source_check(cfg); rc != LEON_OK) return rc;
    if (cfg->reserved) return fail(LEON_ERR_INVALID, "field tensors: the reserved word of cfg is not 0");
    if (cfg->dtype != LEON_TENSOR_F16 && cfg->dtype != LEON_TENSOR_BF16 && cfg->dtype != LEON_TENSOR_F32)
        return fail(LEON_ERR_INVALID, "field tensors: dtype %d (LEON_TENSOR_F16, _BF16, _F32)", cfg->dtype);
    if (cfg->filter != LEON_RESIZE_TRIANGLE) return fail(LEON_ERR_INVALID, "field tensors: filter %d (LEON_RESIZE_TRIANGLE is the filter)", cfg->filter);
    if (cfg->channels < 1 || cfg->channels > LEON_FIELD_MAX_CHANNELS) return fail(LEON_ERR_INVALID, "field tensors: %d channels (1 .. %d)", cfg->channels, LEON_FIELD_MAX_CHANNELS);
    if (cfg->out_width < 1 || cfg->out_width > 4096) return fail(LEON_ERR_INVALID, "field tensors: out_width %d is outside 1 .. 4096", cfg->out_width);
    if (cfg->out_height < 1 || cfg->out_height > 4096) return fail(LEON_ERR_INVALID, "field tensors: out_height %d is outside 1 .. 4096", cfg->out_height);
    if (fw < 1 || fw > 4096 || fh < 1 || fh > 4096) return fail(LEON_ERR_INVALID, "field tensors: a frame of %d x %d (1 .. 4096 each)", fw, fh);
    if (items) {
        if (cfg->n_items < 1 || cfg->n_items > 65535) return fail(LEON_ERR_INVALID, "field tensors: %d items (1 .. 65535)", cfg->n_items);
        if (cfg->item_pitch_bytes & 1u) return fail(LEON_ERR_INVALID, "field tensors: item_pitch_bytes %llu is not a multiple of 2", (unsigned long long)cfg->item_pitch_bytes);
        if (limit > cfg->item_pitch_bytes)
            return fail(LEON_ERR_INVALID, "field tensors: item_pitch_bytes %llu is below the record's %llu bytes", (unsigned long long)cfg->item_pitch_bytes, (unsigned long long)limit);
        if (cfg->source_bytes / (uint64_t)cfg->n_items < cfg->item_pitch_bytes)
            return fail(LEON_ERR_INVALID, "field tensors: source_bytes %llu is below %d items of %llu bytes", (unsigned long long)cfg->source_bytes, cfg->n_items,
                        (unsigned long long)cfg->item_pitch_bytes);
        if (!limit) limit = cfg->item_pitch_bytes;
    }
    for (int32_t q = 0; q < cfg->channels; q++) {
        const leon::FieldChannel& c = reinterpret_cast<const leon::FieldChannel&>(cfg->channel[q]);
        switch (leon::field_channel_judge(c, fw, fh, cfg->dtype, limit)) {
        case leon::kFieldOk: break;
        case leon::kFieldBadReserved: return fail(LEON_ERR_INVALID, "field tensors: channel %d: a reserved word is not 0", q);
        case leon::kFieldBadShift: return fail(LEON_ERR_INVALID, "field tensors: channel %d: shift %d (0 .. %d)", q, c.shift, leon::kFieldMaxShift);
        case leon::kFieldBadElemStride: return fail(LEON_ERR_INVALID, "field tensors: channel %d: elem_stride %d (1 .. %d)", q, c.elem_stride, leon::kFieldMaxElemStride);
        case leon::kFieldBadRowStride: return fail(LEON_ERR_INVALID, "field tensors: channel %d: row_stride %d is negative", q, c.row_stride);
        case leon::kFieldBadOffset: return fail(LEON_ERR_INVALID, "field tensors: channel %d: offset_bytes %u is not a multiple of 2", q, c.offset_bytes);
        case leon::kFieldBadScale: return fail(LEON_ERR_INVALID, "field tensors: channel %d: scale %g, bias %g: not finite", q, (double)c.scale, (double)c.bias);
        case leon::kFieldBadRange:
            return fail(LEON_ERR_INVALID, "field tensors: channel %d: scale %g, bias %g: 32768 * |scale| + |bias| is not finite in the element type", q, (double)c.scale, (double)c.bias);
        default:
            return fail(LEON_ERR_INVALID, "field tensors: channel %d: its last element ends at byte %llu of an item of %llu bytes", q,
                        (unsigned long long)leon::field_channel_end(c, fw, fh), (unsigned long long)limit);
        }
    }
    return LEON_OK;
}
inline size_t field_region_bytes(const leon_pipeline_field_config& cfg)
{
    return (size_t)cfg.channels * (size_t)cfg.out_height * (size_t)cfg.out_width * (size_t)leon::field_elem_bytes(cfg.dtype);
}
// the bytes of a record source's record over a coded picture (0: a BUFFER source), for the roads with explicit sizes
int field_record_bytes(const leon_pipeline_field_config* cfg, int32_t cw, int32_t ch, uint64_t* bytes)
{
    if (const int rc = field_source_check(cfg); rc != LEON_OK) return rc;
    *bytes = 0;
    if (cfg->source == LEON_FIELD_SOURCE_BUFFER) return LEON_OK;
    if (const int rc = residual_size_check("field tensors", cw, ch); rc != LEON_OK) return rc;
    *bytes = cfg->source == LEON_FIELD_SOURCE_MOTION ? leon::motion_layout((uint32_t)cw / 16u, (uint32_t)ch / 16u).record_bytes : leon::residual_layout((uint32_t)cw, (uint32_t)ch).record_bytes;
    return LEON_OK;
}

// regions a chunk and the scratch behind the table: as many as fit the limit (and 32 bits of table words, which rt_base counts)
struct FieldsPlan {
    size_t slot_words, chunk, desc_bytes, tabs_bytes;
};
int fields_plan(const leon_pipeline_field_config& cfg, int32_t n, uint64_t limit, FieldsPlan* P)
{
    P->slot_words = boxes_slot_words(cfg.out_width, cfg.out_height, LEON_RESIZE_TRIANGLE);
    const size_t per_region = P->slot_words * 4 + sizeof(leon::RegionDesc);
    if (!limit) limit = LEON_REGIONS_SCRATCH_DEFAULT;
    if (limit < per_region) return fail(LEON_ERR_INVALID, "field tensors: scratch_limit_bytes %llu is below one region's %zu bytes", (unsigned long long)limit, per_region);
    P->chunk = (size_t)std::min<uint64_t>({(uint64_t)n, limit / per_region, (((uint64_t)1 << 32) - 1) / P->slot_words});
    P->desc_bytes = pad256(P->chunk * sizeof(leon::RegionDesc));
    P->tabs_bytes = P->chunk * P->slot_words * 4;
    return LEON_OK;
}
// the launches every device road shares: per chunk k_box_tables, which judges the records and builds their tables, and k_fields behind
// the descriptors' status words; none behind a chunk whose launch failed
void fields_launch(hipStream_t st, const leon_pipeline_field_config& cfg, int32_t fw, int32_t fh, int32_t n_frames, const leon::BoxRecord* boxes, int32_t n, const uint32_t* d_ids,
                   leon::RegionDesc* d_descs, int32_t* d_tabs, const FieldsPlan& P, const uint8_t* src, size_t item_pitch, uint8_t* out, uint64_t pitch, int32_t* d_status)
{
    const int32_t ow = cfg.out_width, oh = cfg.out_height;
    leon::BoxCall B{};
    B.fw = fw; B.fh = fh; B.ow = ow; B.oh = oh;
    B.n_frames = n_frames; B.cubic = 0;
    B.slot_words = (uint32_t)P.slot_words;
    B.pitch_lo = (uint32_t)(pitch & 0xffffffffu); B.pitch_hi = (uint32_t)(pitch >> 32);
    leon::FieldCall F{};
    for (int32_t q = 0; q < cfg.channels; q++) F.ch[q] = reinterpret_cast<const leon::FieldChannel&>(cfg.channel[q]);
    F.fw = fw; F.fh = fh; F.ow = ow; F.oh = oh;
    F.channels = cfg.channels;
    F.item_pitch = item_pitch;
    const FieldsKernel k = kFieldsKernels[cfg.dtype - LEON_TENSOR_F16];
    for (size_t first = 0; first < (size_t)n; first += P.chunk) {
        const unsigned m = (unsigned)std::min(P.chunk, (size_t)n - first);          // (blockIdx.z: m <= n <= 65535; at most 512 tile rows)
        B.first = (uint32_t)first;
        hipLaunchKernelGGL(leon::k_box_tables, dim3(m), dim3(leon::kRgbaBlock), 0, st, boxes + first, d_ids, d_descs, d_tabs, d_status ? d_status + first : nullptr, B);
        const dim3 grid((unsigned)((ow + leon::kFieldTileX - 1) / leon::kFieldTileX), (unsigned)((oh + leon::kFieldTileY - 1) / leon::kFieldTileY), m);
        hipLaunchKernelGGL(k, grid, dim3(leon::kRgbaBlock), 0, st, src, out, (const leon::RegionDesc*)d_descs, (const int32_t*)d_tabs, F);
        if (hipPeekAtLastError() != hipSuccess) break;
    }
}

int field_outputs_check(const leon_pipeline* p, int32_t source)
{
    if (source == LEON_FIELD_SOURCE_MOTION && !p->motion.ring) return no_output("motion", "MOTION");
    if (source == LEON_FIELD_SOURCE_RESIDUAL && !p->residual.ring) return no_output("residual", "RESIDUAL");
    return LEON_OK;
}
// the caller's pointers of a device call; *pitch as regions_out_check's
int field_call_check(const leon_pipeline_field_config* cfg, const leon_pipeline_field_tensors_call* c, uint64_t* pitch)
{
    if (const int rc = boxes_call_check("field tensors", c->records, false, c->device_status, c->device_out, c->out_pitch_bytes, field_region_bytes(*cfg), pitch); rc != LEON_OK) return rc;
    if (cfg->source == LEON_FIELD_SOURCE_BUFFER) {
        if (!c->source) return fail(LEON_ERR_INVALID, "field tensors: null source with LEON_FIELD_SOURCE_BUFFER");
        if ((uintptr_t)c->source & 1u) return fail(LEON_ERR_INVALID, "field tensors: source %p is not 2-byte aligned", c->source);
    } else if (c->source) return fail(LEON_ERR_INVALID, "field tensors: a source pointer with a record source (the window's records are the source)");
    return LEON_OK;
}

// One call of the device road: the host's refusals (the source's and the output's before the window's, as gauge's), then inside the boxes
// bracket the chunks' launches.  The scratch: [the table of item ids | a chunk's descriptors | its tables] -- the ids the ring slots of
// the window's records, taken from the table the carry family reads them through, or an identity for the caller's buffer.
int field_tensors_device(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_field_tensors_call* c)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = field_source_check(cfg);
    if (rc != LEON_OK || (rc = field_outputs_check(p, cfg->source)) != LEON_OK) return rc;
    if (!c) return fail(LEON_ERR_INVALID, "null argument");
    const bool buffer = cfg->source == LEON_FIELD_SOURCE_BUFFER, motion = cfg->source == LEON_FIELD_SOURCE_MOTION;
    std::unique_lock<std::mutex> call(p->regions_mu);
    std::vector<uint32_t> ids;
    if (!buffer) {
        // the ring slots of the window's records: the first word of the rows of the table the carry, gauge and propagate calls read (a
        // CarryFrame: ring, fwd, bwd, a spare word); a pipeline with the RESIDUAL output alone has no such table, and the slots are the
        // ones its residual descriptors name -- the rings share the index
        rc = window_delivered(p, window, [&](const PipeWindow& w) {
            if (!w.carry_table.empty())
                for (size_t i = 0; i + 3 < w.carry_table.size(); i += 4) ids.push_back(w.carry_table[i]);
            else
                for (const leon::ResidualDesc& d : w.residual_descs) ids.push_back(d.frame);
        });
        if (rc != LEON_OK) return rc;
    }
    if (c->reserved0 || c->reserved) return fail(LEON_ERR_INVALID, "field tensors: a reserved word of the call is not 0");
    if ((rc = record_count_check("field tensors", "records", c->n)) != LEON_OK) return rc;
    const int32_t fw = p->vinfo.frame_width, fh = p->vinfo.frame_height;
    const uint64_t record_bytes = buffer ? 0 : motion ? p->motion_lay.record_bytes : p->residual_lay.record_bytes;
    if ((rc = field_config_check(fw, fh, cfg, record_bytes, buffer)) != LEON_OK) return rc;
    uint64_t pitch;
    if ((rc = field_call_check(cfg, c, &pitch)) != LEON_OK) return rc;
    if (buffer)
        for (int32_t i = 0; i < cfg->n_items; i++) ids.push_back((uint32_t)i);
    FieldsPlan P;
    if ((rc = fields_plan(*cfg, c->n, 0, &P)) != LEON_OK) return rc;
    const uint8_t* src = buffer ? static_cast<const uint8_t*>(c->source) : motion ? (const uint8_t*)p->motion.ring : (const uint8_t*)p->residual.ring;
    const size_t item_pitch = buffer ? (size_t)cfg->item_pitch_bytes : motion ? p->motion_lay.record_pitch : p->residual_lay.record_pitch;
    const size_t ids_bytes = pad256(std::max<size_t>(ids.size(), 1) * 4);
    return boxes_run(p, c->stream, call, ids, ids_bytes + P.desc_bytes + P.tabs_bytes, [&](hipStream_t st, uint32_t* d_ids) {
        fields_launch(st, *cfg, fw, fh, (int32_t)ids.size(), reinterpret_cast<const leon::BoxRecord*>(c->records), c->n, d_ids,
                      reinterpret_cast<leon::RegionDesc*>(p->boxes_dev + ids_bytes), reinterpret_cast<int32_t*>(p->boxes_dev + ids_bytes + P.desc_bytes), P, src, item_pitch,
                      static_cast<uint8_t*>(c->device_out), pitch, c->device_status);
    });
}

// One call of the host road: [records | source | tensors | status], the tensors and status going up first so that what the kernel leaves
// alone comes back as it was
int field_tensors(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_region* records, int32_t n, const void* source, void* out,
                  uint64_t out_pitch, int32_t* status)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    int rc = field_source_check(cfg);
    if (rc != LEON_OK || (rc = field_outputs_check(p, cfg->source)) != LEON_OK) return rc;
    if (!records || !out) return fail(LEON_ERR_INVALID, "field tensors: null %s", records ? "out" : "records");
    const bool buffer = cfg->source == LEON_FIELD_SOURCE_BUFFER, motion = cfg->source == LEON_FIELD_SOURCE_MOTION;
    if (buffer != (source != nullptr)) return fail(LEON_ERR_INVALID, "field tensors: %s", buffer ? "null source with LEON_FIELD_SOURCE_BUFFER" : "a source pointer with a record source");
    if ((rc = record_count_check("field tensors", "records", n)) != LEON_OK) return rc;
    const uint64_t record_bytes = buffer ? 0 : motion ? p->motion_lay.record_bytes : p->residual_lay.record_bytes;
    if ((rc = field_config_check(p->vinfo.frame_width, p->vinfo.frame_height, cfg, record_bytes, buffer)) != LEON_OK) return rc;
    const size_t region_bytes = field_region_bytes(*cfg);
    if (out_pitch && (out_pitch % 256 || out_pitch < region_bytes))
        return fail(LEON_ERR_INVALID, "field tensors: out_pitch_bytes %llu (0, or a multiple of 256 not below the region's %zu bytes)", (unsigned long long)out_pitch, region_bytes);
    const size_t pitch = out_pitch ? (size_t)out_pitch : pad256(region_bytes);
    const auto device = [&](const Pieces& s) {
        leon_pipeline_field_tensors_call c{};
        c.records = s.at<const leon_pipeline_region>(0);
        c.n = n;
        c.source = buffer ? s.at(1) : nullptr;
        c.device_out = s.at(2);
        c.out_pitch_bytes = pitch;
        c.device_status = status ? s.at<int32_t>(3) : nullptr;
        return field_tensors_device(p, window, cfg, &c);
    };
    const std::initializer_list<Piece> pieces = {{records, nullptr, (size_t)n * 32}, {source, nullptr, buffer ? (size_t)cfg->source_bytes : 0}, {out, out, (size_t)n * pitch},
                                                 {status, status, (size_t)n * 4}};
    if (buffer) return pieces_run(p->cfg.device_id, "field tensors", pieces, device);
    return table_host_road(p, window, "field tensors", pieces, device);
}

// what the CPU road and the diagnostic refuse alike: the sizes, the config with the caller's item geometry, the pointers
int field_host_check(int32_t fw, int32_t fh, int32_t cw, int32_t ch, const leon_pipeline_field_config* cfg, const void* items, const void* records, const void* out)
{
    if (!cfg || !items || !records || !out) return fail(LEON_ERR_INVALID, "null argument");
    uint64_t record_bytes;
    int rc = field_record_bytes(cfg, cw, ch, &record_bytes);
    if (rc != LEON_OK || (rc = field_config_check(fw, fh, cfg, record_bytes, true)) != LEON_OK) return rc;
    if ((uintptr_t)items & 1u) return fail(LEON_ERR_INVALID, "field tensors: items %p is not 2-byte aligned", items);
    if ((uintptr_t)records & 3u) return fail(LEON_ERR_INVALID, "field tensors: records %p is not 4-byte aligned", records);
    return LEON_OK;
}

// the definition on the CPU: the record judged by the regions' own function, the tables by the pixel road's builder, then the plain loop
// over every sample of every channel (leon_fields.h); the status word, or a negative error
int32_t field_tensor_record_host(int32_t fw, int32_t fh, int32_t cw, int32_t ch, const leon_pipeline_field_config* cfg, const void* items, const leon_pipeline_region* record,
                                 void* out)
{
    int rc = field_host_check(fw, fh, cw, ch, cfg, items, record, out);
    if (rc != LEON_OK) return rc;
    const int32_t eb = leon::field_elem_bytes(cfg->dtype), ow = cfg->out_width, oh = cfg->out_height;
    if ((uintptr_t)out & (uintptr_t)(eb - 1)) return fail(LEON_ERR_INVALID, "field tensors: out %p is not aligned to its %d-byte elements", out, eb);
    leon_pipeline_regions_config rcfg{};
    rcfg.out_width = ow; rcfg.out_height = oh; rcfg.filter = LEON_RESIZE_TRIANGLE;
    const int32_t st = region_status(fw, fh, cfg->n_items, *record, rcfg, RegionsFit{});
    if (st != LEON_REGION_OK) return st;
    const int32_t taps = LEON_RESIZE_MAX_TAPS;
    std::vector<int32_t> t((size_t)(ow + oh) * (size_t)(2 + taps));
    int32_t* tx = t.data();
    int32_t* ty = tx + (size_t)ow * (size_t)(2 + taps);
    if ((rc = resize_axis_build("width", fw, record->x, record->width, ow, LEON_RESIZE_TRIANGLE, tx, tx + ow, tx + 2 * ow, taps, nullptr)) != LEON_OK) return rc;
    if ((rc = resize_axis_build("height", fh, record->y, record->height, oh, LEON_RESIZE_TRIANGLE, ty, ty + oh, ty + 2 * oh, taps, nullptr)) != LEON_OK) return rc;
    const leon::FieldTables T{tx, tx + ow, tx + 2 * ow, ty, ty + oh, ty + 2 * oh, taps, taps};
    const uint8_t* item = static_cast<const uint8_t*>(items) + (size_t)record->frame * (size_t)cfg->item_pitch_bytes;
    uint8_t* o = static_cast<uint8_t*>(out);
    for (int32_t q = 0; q < cfg->channels; q++) {
        const leon::FieldChannel& c = reinterpret_cast<const leon::FieldChannel&>(cfg->channel[q]);
        for (int32_t oy = 0; oy < oh; oy++)
            for (int32_t ox = 0; ox < ow; ox++)
                leon::field_store_elem(o + (((size_t)q * oh + oy) * ow + ox) * eb, leon::field_elem(leon::field_value(leon::field_sample(item, c, T, ox, oy), c.scale, c.bias), cfg->dtype), eb);
    }
    return LEON_REGION_OK;
}

// k_box_tables and k_fields on items the caller supplies (leon_pipeline_field_tensors_kernel): memory of its own, the null stream, an
// identity table of item ids
int field_tensors_kernel(int32_t device_id, int32_t fw, int32_t fh, int32_t cw, int32_t ch, const leon_pipeline_field_config* cfg, const void* items,
                         const leon_pipeline_region* records, int32_t n, void* out, uint64_t out_pitch, int32_t* status, uint64_t scratch_limit)
{
    int rc = field_host_check(fw, fh, cw, ch, cfg, items, records, out);
    if (rc != LEON_OK || (rc = record_count_check("field tensors", "records", n)) != LEON_OK) return rc;
    const size_t region_bytes = field_region_bytes(*cfg);
    if (out_pitch && (out_pitch % 256 || out_pitch < region_bytes))
        return fail(LEON_ERR_INVALID, "field tensors: out_pitch_bytes %llu (0, or a multiple of 256 not below the region's %zu bytes)", (unsigned long long)out_pitch, region_bytes);
    const size_t pitch = out_pitch ? (size_t)out_pitch : pad256(region_bytes);
    FieldsPlan P;
    if ((rc = fields_plan(*cfg, n, scratch_limit, &P)) != LEON_OK) return rc;
    std::vector<uint32_t> ids((size_t)cfg->n_items);
    for (size_t i = 0; i < ids.size(); i++) ids[i] = (uint32_t)i;
    return pieces_run(device_id, "field tensors", {{records, nullptr, (size_t)n * 32}, {items, nullptr, (size_t)cfg->source_bytes}, {out, out, (size_t)n * pitch},
                                                   {status, status, (size_t)n * 4}, {ids.data(), nullptr, ids.size() * 4}, {nullptr, nullptr, P.desc_bytes},
                                                   {nullptr, nullptr, P.tabs_bytes}}, [&](const Pieces& s) {
        fields_launch(nullptr, *cfg, fw, fh, cfg->n_items, s.at<const leon::BoxRecord>(0), n, s.at<const uint32_t>(4), s.at<leon::RegionDesc>(5), s.at<int32_t>(6), P, s.at(1),
                      (size_t)cfg->item_pitch_bytes, s.at(2), pitch, status ? s.at<int32_t>(3) : nullptr);
        return (int)LEON_OK;
    });
}

// The device's rows of a batch of single axes, copied back (leon_pipeline_resize_weights_device): memory of its own, the null stream
int resize_weights_device(int32_t device_id, int32_t n_axes, const int32_t* axes, int32_t filter, int32_t max_taps, int32_t* first, int32_t* count,
                          int32_t* weights, int32_t* status)
{
    if (!axes || !first || !count || !weights || !status) return fail(LEON_ERR_INVALID, "null argument");
    if (n_axes < 1) return fail(LEON_ERR_INVALID, "resize: %d axes", n_axes);
    if (max_taps < 1) return fail(LEON_ERR_INVALID, "resize: max_taps %d", max_taps);
    if (!resize_filter_max_taps(filter)) return fail(LEON_ERR_INVALID, "resize filter %d (LEON_RESIZE_TRIANGLE and LEON_RESIZE_BICUBIC are the filters)", filter);
    int32_t max_out = 0;
    for (int32_t a = 0; a < n_axes; a++) {
        if (axes[4 * a] < 1 || axes[4 * a] > 4096) return fail(LEON_ERR_INVALID, "resize: axis %d: in_size %d is outside 1 .. 4096", a, axes[4 * a]);
        if (axes[4 * a + 3] < 1 || axes[4 * a + 3] > 4096) return fail(LEON_ERR_INVALID, "resize: axis %d: output %d is outside 1 .. 4096", a, axes[4 * a + 3]);
        max_out = std::max(max_out, axes[4 * a + 3]);
    }
    static_assert(sizeof(leon::AxisRecord) == 16, "four words an axis");
    const size_t rows = (size_t)n_axes * (size_t)max_out;
    // [axes | first | count | weights | status]: the caller's rows go up and come back whole, so what the kernel does not write stays as
    // the caller had it
    return pieces_run(device_id, "resize", {{axes, nullptr, (size_t)n_axes * 16}, {first, first, rows * 4}, {count, count, rows * 4},
                                            {weights, weights, rows * (size_t)max_taps * 4}, {nullptr, status, (size_t)n_axes * 4}}, [&](const Pieces& s) {
        hipLaunchKernelGGL(leon::k_axis_tables, dim3((unsigned)n_axes), dim3(leon::kRgbaBlock), 0, nullptr, s.at<const leon::AxisRecord>(0), s.at<int32_t>(1), s.at<int32_t>(2),
                           s.at<int32_t>(3), s.at<int32_t>(4), filter == LEON_RESIZE_BICUBIC ? 1 : 0, max_taps, max_out);
        return (int)LEON_OK;
    });
}

// one window: its levels planned, its arenas uploaded (and parsed on the GPU), its levels launched, its frames listed
int submit_window(leon_pipeline* p, PipeWindow* w)
{
    // LEON_DEBUG_SERIAL=1: the host waits behind every stage (uploads, parser kernels, reconstruction) -- takes every
    // cross-stream dependency out of the picture when a wrong frame is being hunted
    static const bool serial = env_int("LEON_DEBUG_SERIAL", 0) == 1;
    // LEON_DEBUG_POISON=1: everything of the arena that the kernels are expected to write before they read it starts
    // as 0xCD bytes -- a read of something nobody wrote then shows in every run, not only when the memory's history
    // happens to differ from zero
    static const bool poison = env_int("LEON_DEBUG_POISON", 0) == 1;
    std::vector<std::vector<LevelPic>> levels;
    std::vector<std::vector<int32_t>> qset(w->jobs.size());
    // the window before's last anchor, if this window follows it directly in one run
    const bool follows = p->last_anchor >= 0 && p->last_run == w->run->id && !w->jobs.empty() && p->last_gop + 1 == w->jobs[0]->gop;
    bool uses_carry = false;
    int last_anchor = -1, last_anchor_tref = -1;
    if (!follows) p->last_anchor_tref = -1;
    int rc = plan_levels(p, w, levels, follows ? p->carry_slot : -1, &uses_carry, &last_anchor, &last_anchor_tref);
    if (rc == LEON_OK) rc = upload_and_chain(p, w, serial, poison);
    if (rc == LEON_OK) rc = register_qsets(p, w, qset);
    if (rc != LEON_OK) return rc;
    if (uses_carry) {
        // Every reconstruction launch of every window goes through the decoder's stream in submit order (submit_batch_any,
        // leon_convert_rgba, crop_planes_batch): the copy runs behind the window before's last launch and in front of this
        // window's first, which may overwrite the source; the carry slot's readers of the window before have run as well.
        const leon_decoder* d = p->dec;
        HIP_TRY(hipMemcpyAsync(d->d_slots + (size_t)p->carry_slot * d->slot_stride, d->d_slots + (size_t)p->last_anchor * d->slot_stride, d->plane_bytes,
                               hipMemcpyDeviceToDevice, d->stream));
    }
    const std::string cdir = p->capture_dir.empty() ? "" : p->capture_dir + "/w" + std::to_string(w->id);
    if (!cdir.empty()) {
        (void)mkdir(p->capture_dir.c_str(), 0777);          // (both may exist)
        (void)mkdir(cdir.c_str(), 0777);
    }
    size_t lvl_no = 0;
    for (const auto& lvl : levels) {
        if (lvl.empty()) continue;
        if ((rc = launch_level(p, w, lvl, qset)) != LEON_OK) return rc;
        if (!cdir.empty() && (rc = capture_level(p, w, cdir, lvl, lvl_no)) != LEON_OK) return rc;
        lvl_no++;
    }
    if (!cdir.empty())
        for (size_t j = 0; j < w->jobs.size(); j++) capture_file(cdir + "/arena_" + std::to_string(j) + ".bin", w->jobs[j]->arena->dev, w->jobs[j]->arena->used);
    p->last_run = w->run->id;
    p->last_gop = w->jobs.empty() ? 0 : w->jobs.back()->gop;
    p->last_anchor = last_anchor;
    p->last_anchor_tref = last_anchor_tref;
    list_frames(p, w, levels, qset);
    if ((rc = launch_tensors(p, w)) != LEON_OK) return rc;
    if ((rc = launch_motion(p, w)) != LEON_OK) return rc;
    if ((rc = launch_activity(p, w)) != LEON_OK) return rc;
    if ((rc = launch_residual(p, w)) != LEON_OK) return rc;
    if (serial) HIP_TRY(hipStreamSynchronize(p->dec->stream));
    HIP_TRY(hipEventRecord(w->done, p->dec->stream));
    return LEON_OK;
}

void submit_loop(leon_pipeline* p)
{
    for (;;) {
        const auto t_begin = Clock::now();
        auto t_ring = t_begin, t_scanned = t_begin;
        std::unique_ptr<PipeWindow> owned = p->flow.take_window(&t_ring, &t_scanned);
        if (!owned) return;
        PipeWindow* const w = owned.get();
        int rc = LEON_OK;
        std::string msg;
        for (const auto& j : w->jobs)
            if (j->status != LEON_OK && rc == LEON_OK) { rc = j->status; msg = j->err; }
        if (rc == LEON_OK) {
            if (!w->done.create(hipEventDisableTiming)) { rc = LEON_ERR_HIP; msg = "hipEventCreate failed"; }
            else {
                const auto t = Clock::now();
                rc = submit_window(p, w);
                p->st_submit_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t).count();
                if (rc != LEON_OK) msg = g_err;
            }
        }
        w->status = rc;
        {   // where the submit thread's time goes, per window (LEON_DEBUG_PIPE_TIMING=1 prints it when the pipeline is destroyed)
            const auto ns = [](Clock::time_point a, Clock::time_point b) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); };
            p->st_wait_ring_ns += ns(t_begin, t_ring);
            p->st_wait_scan_ns += ns(t_ring, t_scanned);
        }
        if (rc != LEON_OK) pipe_fail(p, rc, msg);
        p->flow.submitted(std::move(owned));
        if (rc != LEON_OK) return;
    }
}

void submit_main(leon_pipeline* p)
{
    hipSetDevice(p->cfg.device_id);
    submit_loop(p);
    p->flow.submit_exited();
}

void notify_main(leon_pipeline* p)
{
    hipSetDevice(p->cfg.device_id);
    for (;;) {
        PipeFlow::Event ev = p->flow.next_event();
        if (ev.exit()) break;
        if (ev.ended) {
            if (p->cb && !ev.quiet) p->cb(p->user, -1, nullptr, 0, LEON_OK);
            p->flow.ended_returned(ev.ended);
            continue;
        }
        std::unique_ptr<PipeWindow>& w = ev.window;
        if (w->status == LEON_OK && hipEventSynchronize(w->done) != hipSuccess) {
            w->status = LEON_ERR_HIP;
            pipe_fail(p, LEON_ERR_HIP, std::string("window ") + std::to_string(w->id) + ": " + hipGetErrorString(hipGetLastError()));
        }
        if (!p->flow.keep_or_retire(w)) continue;
        if (w->status == LEON_OK && p->gpu_parser && w->n_vpics) {          // the GPU parser's verdict on every picture of the window
            const uint32_t* e = p->vlc_ring[(size_t)w->ring].h_err;
            for (uint32_t k = 0; k < w->n_vpics; k++)
                if (e[k]) {
                    static const char* const what[] = {"", "invalid macroblock address increment", "macroblock address outside the picture",
                        "invalid macroblock type", "invalid motion code", "invalid coded block pattern", "invalid coefficient code",
                        "coefficient index overflow", "bitstream ends inside a slice", "invalid DC size code", "more block records than the picture has blocks",
                                           "slices of a picture overlap (the GPU parser decodes them side by side: gpu_parser = -1 decodes such a stream)"};
                    const uint32_t code = e[k] & 255u;
                    w->status = LEON_ERR_INVALID;
                    pipe_fail(p, LEON_ERR_INVALID, std::string("window ") + std::to_string(w->id) + ", picture " + std::to_string(k) + ", slice " +
                              std::to_string(e[k] >> 8) + ": " + (code < sizeof(what) / sizeof(what[0]) ? what[code] : "malformed slice"));
                    break;
                }
        }
        const int64_t id = w->id;
        const int st = w->status;
        const std::shared_ptr<const PipeRun> run = w->run;
        bool quiet = false;
        const PipeWindow* out = p->flow.deliver(std::move(w), std::chrono::duration<double>(Clock::now() - p->t0).count(), &quiet);
        // frames are handed over outside the lock: the callback may release the window at once
        if (p->cb && !quiet) p->cb(p->user, id, st == LEON_OK ? out->frames.data() : nullptr, st == LEON_OK ? (int32_t)out->frames.size() : 0, st);
        else leon_pipeline_release_window(p, id);
        p->flow.callback_returned(run);
    }
    // 'ended' (or the error that stopped the run) BEFORE leon_pipeline_wait returns: a host that waits and then
    // looks at what its callback recorded must find the end recorded
    if (p->cb && !p->flow.quiet()) p->cb(p->user, -1, nullptr, 0, p->flow.status());
    p->flow.finish();
}

// The run that starts at `seconds`: the key-map entry the front end's own seek finds (leon_vlc_seek, decoders/jsv.js
// :327-350), then this shard's entries from it on, in windows of p->W GOPs.  leon_pipeline_create (start_seconds) and
// leon_pipeline_seek both ask here; `st` is a stream opened on the pipeline's bytes (its container header and key map).
std::shared_ptr<PipeRun> make_run(const leon_pipeline* p, leon_vlc_stream* st, double seconds, int loops)
{
    static std::atomic<uint64_t> next_id{1};
    auto run = std::make_shared<PipeRun>();
    run->id = next_id++;
    if (p->has_keymap && seconds > 0) {
        uint64_t off = 0;
        if (leon_vlc_seek(st, seconds, &off) == LEON_VLC_OK)
            for (size_t g = 0; g < p->shard_begin.size(); g++)
                if (p->shard_begin[g] == off) run->first_key = (uint32_t)g;
    }
    for (uint32_t g : p->shard_gops)
        if (g >= run->first_key) run->mine.push_back(g);
    run->total_gops = (uint64_t)run->mine.size() * (uint64_t)loops;
    run->total_windows = (int64_t)((run->total_gops + p->W - 1) / p->W);
    return run;
}

// k_vlc_index counts a picture's groups in LDS (one workgroup may have all 160 KiB of a CU)
constexpr size_t kMaxVlcIndexLds = 160 * 1024 - 512;

// Create, stage 1: what the config and the stream decide -- the shards, the run, W / R / K, the longest GOP, the front
// end, the output and its roads, info.  No HIP call and no allocation: a refused config leaves nothing to free but p.
int plan_pipeline(leon_pipeline* p, const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tcfg, const leon_pipeline_tensor_resize* rz,
                  const leon_pipeline_tensor_format* fm, const leon_pipeline_tensor_canvas* cv, const uint8_t* stream, size_t bytes, size_t valid_bytes)
{
    leon_vlc_stream* st = nullptr;
    // the container header, the key map and the first sequence header must have arrived
    if (leon_vlc_open(stream, valid_bytes, 1, &st) != LEON_VLC_OK) return fail(LEON_ERR_INVALID, "stream: %s", leon_vlc_last_error());
    const std::unique_ptr<leon_vlc_stream, decltype(&leon_vlc_close)> st_owner(st, &leon_vlc_close);
    leon_vlc_get_info(st, &p->vinfo);
    const int n_keys = leon_vlc_get_keymap(st, nullptr, nullptr, 0);
    std::vector<uint32_t> offs((size_t)std::max(n_keys, 0));
    if (n_keys > 0) leon_vlc_get_keymap(st, offs.data(), nullptr, (uint32_t)n_keys);
    p->cfg = *cfg;
    p->stream = stream;
    p->bytes = bytes;
    if (const char* cd = getenv("LEON_DEBUG_CAPTURE")) p->capture_dir = cd;
    if (n_keys > 0) {
        for (int g = 0; g < n_keys; g++) {
            const uint64_t b = offs[(size_t)g], e = g + 1 < n_keys ? offs[(size_t)g + 1] : bytes;
            // (an entry behind what has arrived of a partial stream is looked at when its bytes are there: parser_main)
            if (b >= e || e > bytes || b + 4 > bytes || (b + 4 <= valid_bytes && (stream[b] != 0 || stream[b + 1] != 0 || stream[b + 2] != 1)))
                return fail(LEON_ERR_INVALID, "key map entry %d does not point at a start code", g);
            p->shard_begin.push_back(b);
            // the shard takes the start code PREFIX of what follows along (00 00 01, not the code byte): its last slice
            // then ends exactly as it does in the whole stream.  Cut at the key-map offset, a last macroblock coded in
            // two bytes or less would look like the end of the data to the slice loop (jsv.js:1710-1760) and be dropped.
            p->shard_end.push_back(std::min<uint64_t>(e + 3, bytes));
        }
    } else {            // no key map: the whole stream is one shard
        p->shard_begin.push_back(0);
        p->shard_end.push_back(bytes);
    }
    const int loops = cfg->loop > 0 ? cfg->loop : 1;
    const uint32_t sc = cfg->shard_count > 1 ? (uint32_t)cfg->shard_count : 1u, si = sc > 1 ? (uint32_t)cfg->shard_index : 0u;
    if (si >= sc) return fail(LEON_ERR_INVALID, "shard_index %d of %d", cfg->shard_index, cfg->shard_count);
    p->has_keymap = n_keys > 0;
    for (uint32_t g = si; g < p->shard_begin.size(); g += sc) p->shard_gops.push_back(g);
    p->W = cfg->gops_per_window > 0 ? cfg->gops_per_window : 32;
    const std::shared_ptr<const PipeRun> first_run = make_run(p, st, cfg->start_seconds, loops);
    p->flow.begin(first_run, valid_bytes);
    const PipeRun& run = *first_run;
    p->info.first_gop = run.first_key;
    if (run.mine.empty()) return fail(LEON_ERR_INVALID, "shard %u of %u gets no GOP: the stream has %zu", si, sc, p->shard_begin.size());
    if ((uint64_t)p->W > run.total_gops) p->W = (int)run.total_gops;      // (one window either way: run.total_windows stands)
    p->gpu_parser = cfg->gpu_parser >= 0;          // 0 = default: the GPU (a pipeline has a device by construction); < 0: the parser threads
    p->vlc_index_lds = ((size_t)p->vinfo.n_groups + leon::kVlcIndexThreads) * 4;      // the group counters of one picture + its scan
    if (cfg->gpu_parser == LEON_PIPELINE_PARSER_DEFAULT) {
        // a caller who did not ASK for the GPU parser is not refused for its limits: a picture whose group counters do not fit
        // k_vlc_index's LDS, or a GOP shard of 2^28 bytes and more (the kernels count bits in 32), goes to the parser threads
        bool fits = p->vlc_index_lds <= kMaxVlcIndexLds;
        for (uint32_t g : p->shard_gops) fits = fits && p->shard_end[g] - p->shard_begin[g] < ((uint64_t)1 << 28);
        if (p->vinfo.n_groups > env_int("LEON_DEBUG_GPU_PARSER_LIMIT", INT_MAX)) fits = false;      // tests: a mocked n_groups limit
        if (!fits) p->gpu_parser = false;
    }
    p->info.gpu_parser = p->gpu_parser ? 1 : 0;
    p->R = cfg->windows_in_flight > 0 ? cfg->windows_in_flight : (p->gpu_parser ? 3 : 2);      // GPU parser: one window being parsed beside one reconstructed and one read
    if (cfg->max_gop_pictures > 0) p->max_pics = cfg->max_gop_pictures;
    else if (valid_bytes < bytes) p->max_pics = 16;          // still arriving: nothing to count yet
    else {
        // the frames a GOP can fill in a window's ring entry: the longest GOP of this pipeline's shards, from the picture
        // start codes (00 00 01 00 -- the syntax keeps that pattern out of everything else); a fixed 16 would reserve a
        // third more than IBBP-12 streams use.  (Every GOP of the shard, not only those from start_seconds on: a seek may
        // go back to them.)
        size_t longest = 1;
        for (uint64_t g : p->shard_gops) {
            const uint8_t* b = stream + p->shard_begin[g];
            const uint8_t* const e = stream + p->shard_end[g];
            size_t n = 0;
            while (b + 4 <= e) {
                const uint8_t* z = (const uint8_t*)memchr(b, 0, (size_t)(e - b) - 3);
                if (!z) break;
                if (z[1] == 0 && z[2] == 1 && z[3] == 0) { n++; b = z + 4; } else b = z + 1;
            }
            longest = std::max(longest, n);
        }
        p->max_pics = (int)std::min<size_t>(longest, 1024);
    }
    int k = cfg->parser_threads;
    if (k <= 0) { k = (int)std::thread::hardware_concurrency(); if (k < 1) k = 1; if (k > 16) k = 16; }
    p->K = k;
    p->frame_bytes = (size_t)p->vinfo.frame_width * p->vinfo.frame_height * 4;
    p->info.coded_width = p->vinfo.coded_width; p->info.coded_height = p->vinfo.coded_height;
    p->info.frame_width = p->vinfo.frame_width; p->info.frame_height = p->vinfo.frame_height;
    p->info.picture_rate = p->vinfo.picture_rate; p->info.duration = p->vinfo.duration;
    p->info.gops = (uint32_t)p->shard_begin.size();
    p->info.shard_gops = (uint32_t)run.mine.size();
    p->info.parser_threads = p->K; p->info.gops_per_window = p->W;
    // the fused display conversion writes eight pixels per lane: it needs frame_width % 8 == 0.  The reference crops to
    // any width (player/easybits.player.js:2818): such a stream takes the slow road -- every picture (B pictures too)
    // writes its planes, and one leon_convert_rgba per picture (the generic k_rgba_twin) fills the window's frames.
    // The GL flavour (the reference's live display arithmetic, fp32) exists as a launch of its own only: the same road.
    if (cfg->display_flavour != LEON_RGB_CPU_TWIN && cfg->display_flavour != LEON_RGB_GL) return fail(LEON_ERR_INVALID, "display_flavour %d", cfg->display_flavour);
    if (cfg->output & ~(LEON_PIPELINE_OUTPUT_RGBA | LEON_PIPELINE_OUTPUT_YCBCR | LEON_PIPELINE_OUTPUT_TENSOR | LEON_PIPELINE_OUTPUT_MOTION | LEON_PIPELINE_OUTPUT_ACTIVITY |
                        LEON_PIPELINE_OUTPUT_RESIDUAL))
        return fail(LEON_ERR_INVALID, "output %d", cfg->output);
    if (cfg->output && !(cfg->output & (LEON_PIPELINE_OUTPUT_RGBA | LEON_PIPELINE_OUTPUT_YCBCR | LEON_PIPELINE_OUTPUT_TENSOR)))
        return fail(LEON_ERR_INVALID, "output %d: LEON_PIPELINE_OUTPUT_MOTION, _ACTIVITY and _RESIDUAL need RGBA, YCBCR or TENSOR beside them (a pipeline that only parses is not built)", cfg->output);
    if (cfg->output & LEON_PIPELINE_OUTPUT_TENSOR) {
        // the tensor is defined through the CPU twin's RGBA, whose index drifts over an odd width (k_rgba_twin): refused, as yuva is
        if (p->vinfo.frame_width & 1) return fail(LEON_ERR_INVALID, "the tensor output needs an even frame_width (it is %d)", p->vinfo.frame_width);
        p->tensor_table.resize(3 * 256 * 4);
        const int rc = tensor_table_build(cfg, tcfg, &p->tensor_dtype, p->tensor_table.data());
        if (rc != LEON_OK) return rc;
        p->tensor_elem = p->tensor_dtype == LEON_TENSOR_F32 ? 4 : (p->tensor_dtype == LEON_TENSOR_U8 ? 1 : 2);
        const int frc = tensor_format_check(cfg, fm, &p->tensor_layout);
        if (frc != LEON_OK) return frc;
        p->tensor_table.resize(3 * 256 * p->tensor_elem);
        const int rrc = plan_resize(p, rz);
        if (rrc != LEON_OK) return rrc;
        const int crc = tensor_canvas_check(cfg, rz, cv);
        if (crc != LEON_OK) return crc;
        plan_canvas(p, cv);
        p->tensor_bytes = (size_t)3 * p->tensor_geom.height * p->tensor_geom.width * p->tensor_elem;
        p->tensor_pitch = pad256(p->tensor_bytes);
        p->info.tensor_dtype = p->tensor_dtype;
        p->info.tensor_element_bytes = (int32_t)p->tensor_elem;
        p->info.tensor_frame_bytes = p->tensor_bytes;
        p->info.tensor_frame_pitch = p->tensor_pitch;
        p->info.tensor_gop_pitch = (uint64_t)p->tensor_pitch * (uint64_t)p->max_pics;
    } else if (tcfg && tcfg->dtype) return fail(LEON_ERR_INVALID, "tensor dtype %d without LEON_PIPELINE_OUTPUT_TENSOR in output", tcfg->dtype);
    else if (resize_asked(rz)) return fail(LEON_ERR_INVALID, "resize settings (%d x %d) without LEON_PIPELINE_OUTPUT_TENSOR in output %d", rz->out_width, rz->out_height, cfg->output);
    else if (const int frc = tensor_format_check(cfg, fm, nullptr)) return frc;
    else if (const int crc = tensor_canvas_check(cfg, rz, cv)) return crc;
    // the frames' planes (output YCbCr): the layout of include/leon_pipeline.h, one record per frame, A behind Cr for yuva
    p->output = cfg->output ? cfg->output : LEON_PIPELINE_OUTPUT_RGBA;
    p->planes_geom = planes_layout(p->vinfo.frame_width, p->vinfo.frame_height, &p->planes_bytes);
    if (p->vinfo.has_alpha == 1) p->planes_bytes = p->planes_geom.a_off + ((size_t)p->planes_geom.luma_stride * p->vinfo.frame_height + 255) / 256 * 256;
    p->info.output = p->output;
    p->info.chroma_width = (p->vinfo.frame_width + 1) / 2;
    p->info.chroma_height = p->planes_geom.chroma_height;
    p->info.luma_stride = (int32_t)p->planes_geom.luma_stride;
    p->info.chroma_stride = (int32_t)p->planes_geom.chroma_stride;
    p->flavour = cfg->display_flavour;
    p->info.display_flavour = p->flavour;
    p->unfused = (p->vinfo.frame_width & 7) != 0 || p->flavour == LEON_RGB_GL;
    if (p->unfused && p->vinfo.has_alpha == 1)
        return fail(LEON_ERR_INVALID, "a yuva stream needs frame_width %% 8 == 0 (it is %d) and the CPU-twin display flavour in the pipeline", p->vinfo.frame_width);
    p->maps = map_layout((size_t)p->vinfo.mb_width * p->vinfo.mb_height, (size_t)p->vinfo.n_groups);
    if (p->output & LEON_PIPELINE_OUTPUT_MOTION) {
        if (const int mrc = mb_grid_check("motion output", p->vinfo.mb_width, p->vinfo.mb_height); mrc != LEON_OK) return mrc;
        p->motion_lay = leon::motion_layout((uint32_t)p->vinfo.mb_width, (uint32_t)p->vinfo.mb_height);
        p->motion.pitch = p->motion_lay.record_pitch;
    }
    if (p->output & LEON_PIPELINE_OUTPUT_ACTIVITY) {
        if (const int arc = mb_grid_check("activity output", p->vinfo.mb_width, p->vinfo.mb_height); arc != LEON_OK) return arc;
        p->activity_lay = leon::activity_layout((uint32_t)p->vinfo.mb_width, (uint32_t)p->vinfo.mb_height);
        p->activity.pitch = p->activity_lay.record_pitch;
        p->activity_geom = leon::activity_geom((uint32_t)p->vinfo.mb_width, (uint32_t)p->vinfo.mb_height);
        if ((int32_t)p->activity_geom.groups_y != p->vinfo.groups_y || (int32_t)p->activity_geom.groups_c != p->vinfo.groups_c)
            return fail(LEON_ERR_INVALID, "activity output: the stream's groups (%d, %d) are not those of %d macroblocks a row", p->vinfo.groups_y, p->vinfo.groups_c, p->vinfo.mb_width);
    }
    if (p->output & LEON_PIPELINE_OUTPUT_RESIDUAL) {
        if (const int rrc = mb_grid_check("residual output", p->vinfo.mb_width, p->vinfo.mb_height); rrc != LEON_OK) return rrc;
        p->residual_lay = leon::residual_layout((uint32_t)p->vinfo.coded_width, (uint32_t)p->vinfo.coded_height);
        p->residual.pitch = p->residual_lay.record_pitch;
        p->residual_geom = leon::residual_geom((uint32_t)p->vinfo.mb_width, (uint32_t)p->vinfo.mb_height);
        if (p->vinfo.coded_width != 16 * p->vinfo.mb_width || p->vinfo.coded_height != 16 * p->vinfo.mb_height ||
            (int32_t)p->residual_geom.groups_y != p->vinfo.groups_y || (int32_t)p->residual_geom.groups_c != p->vinfo.groups_c)
            return fail(LEON_ERR_INVALID, "residual output: the stream's coded size %d x %d and groups (%d, %d) are not those of %d x %d macroblocks", p->vinfo.coded_width,
                        p->vinfo.coded_height, p->vinfo.groups_y, p->vinfo.groups_c, p->vinfo.mb_width, p->vinfo.mb_height);
    }
    // the GPU parser's geometry; it writes a picture's maps at the offsets of the layout the arenas give them
    p->vgeom.mbw = p->vinfo.mb_width; p->vgeom.mbh = p->vinfo.mb_height;
    p->vgeom.gy = p->vinfo.groups_y; p->vgeom.gc = p->vinfo.groups_c;
    p->vgeom.n_y = 2 * p->vinfo.mb_height * p->vinfo.groups_y;
    p->vgeom.n_c = p->vinfo.mb_height * p->vinfo.groups_c;
    p->vgeom.n_groups = p->vinfo.n_groups;
    p->vgeom.alpha = p->vinfo.has_alpha == 1;
    const MapLayout& M = p->maps;
    p->vgeom.off_qscale = (uint32_t)M.off(M.QSCALE);
    p->vgeom.off_intra = (uint32_t)M.off(M.INTRA);
    p->vgeom.off_repadd = (uint32_t)M.off(M.REPADD);
    p->vgeom.off_mb_dir = (uint32_t)M.off(M.MB_DIR);
    p->vgeom.off_mv_fwd = (uint32_t)M.off(M.MV_FWD);
    p->vgeom.off_mv_bwd = (uint32_t)M.off(M.MV_BWD);
    return LEON_OK;
}

// The front end's tables as the GPU parser's kernels copy them to LDS (leon_vlc_gpu.h), 16 bits per entry.  Returns what
// does not fit, "" when everything does.
std::string pack_vlc_tables(const leon_vlc_gpu_tables& src, leon::VlcTables& t)
{
    // fast12 as {length:4, end of block:1, run:5, level:6}, the others as (length << 8) | value
    for (int i = 0; i < 4096; i++) {
        const uint32_t f = src.fast12[i];
        const int len = (int)(f & 0x7f), run = (int)((f >> 8) & 0xff), level = (int)(int16_t)(f >> 16);
        if (len > 15 || run > 31 || level < -32 || level > 31) return "coefficient table does not fit 16 bits";
        t.fast12[i] = (uint16_t)(len | ((f & 0x80u) ? 0x10 : 0) | (run << 5) | ((level & 63) << 10));
    }
    // multi12: every symbol that lies complete in the next 12 bits, taken together (a prefix code is decided by its own
    // bits: the entry of the pattern shifted up, whatever follows, names the symbol if its length fits what is left)
    for (int i = 0; i < leon::kVlcMulti; i++) {
        const int B = leon::kVlcMultiBits;
        int pos = 0, nsym = 0, adv = 0, eob = 0;
        while (pos < B) {
            // the 12 bits from `pos` on, zeros behind the pattern's end
            const uint32_t f = src.fast12[(((uint32_t)i << pos) & (uint32_t)(leon::kVlcMulti - 1)) << 12 >> B];
            const int len = (int)(f & 0x7f);
            if (len == 0 || len > B - pos) break;
            pos += len;
            if (f & 0x80u) { eob = 1; break; }
            nsym++;
            adv += (int)((f >> 8) & 0xff) + 1;
        }
        if (pos > 15 || nsym > 7 || adv > 255) return "multi-symbol table does not fit 16 bits";
        t.multi12[i] = (uint16_t)(pos | (nsym << 4) | (eob << 7) | (adv << 8));
    }
    auto pack = [](int32_t e) { return (uint16_t)(((e >> 16) << 8) | (e & 0xff)); };
    for (int i = 0; i < 2048; i++) { t.motion_s[i] = pack(src.motion_s[i]); t.mba[i] = pack(src.mba[i]); }
    for (int i = 0; i < 512; i++) t.cbp[i] = pack(src.cbp[i]);
    for (int k = 0; k < 4; k++) for (int i = 0; i < 64; i++) t.mbtype[k][i] = pack(src.mbtype[k][i]);
    for (int i = 0; i < 128; i++) t.dc_lum[i] = pack(src.dc_lum[i]);
    for (int i = 0; i < 256; i++) t.dc_chr[i] = pack(src.dc_chr[i]);
    for (int i = 0; i < 64; i++) t.zz_off[i] = src.zz_off[i];
    // the codes of 12 .. 16 bits start with seven zeros: by the nine bits behind them (= the first 512 entries of the
    // 16-bit table)
    for (int i = 0; i < 512; i++) {
        const int32_t e = src.coef16[i];
        const int len = e >> 16, cf = e & 0xffff, run = cf >> 8, level = cf & 0xff;
        if (e == 0) { t.long9[i] = 0; continue; }
        if (cf == 0xffff || len < 8 || len > 16 || run > 31 || level > 63 || level == 0) return "long coefficient code does not fit 16 bits";
        t.long9[i] = (uint16_t)(len | (run << 5) | (level << 10));
    }
    return "";
}

// "<what>: <the runtime's last error>"
int hip_fail(int code, const std::string& what)
{
    return fail(code, "%s: %s", what.c_str(), hipGetErrorString(hipGetLastError()));
}

// one output ring: R entries of W * max_pics frames of `frame` bytes
int alloc_ring(leon_pipeline* p, DevBuf<uint8_t>* ring, size_t frame, const char* name)
{
    const size_t bytes = (size_t)p->R * p->W * p->max_pics * frame;
    if (ring->alloc(bytes, kBigRgbaRing)) return LEON_OK;
    return hip_fail(LEON_ERR_NOMEM, std::string(name) + " ring of " + std::to_string(bytes >> 20) + " MiB (windows_in_flight " + std::to_string(p->R) +
                                        " x gops_per_window " + std::to_string(p->W) + " x max_gop_pictures " + std::to_string(p->max_pics) + " x " +
                                        std::to_string(frame) + " bytes per frame)");
}

// Create, stage 2: the decoder, the copy stream, the output rings, the GPU parser's tables and streams, the arenas and
// their slabs.  A failure returns its code with the message set and leaves what it allocated to leon_pipeline_destroy.
int allocate_pipeline(leon_pipeline* p)
{
    leon_config dc{};
    dc.coded_width = p->vinfo.coded_width; dc.coded_height = p->vinfo.coded_height;
    dc.frame_width = p->vinfo.frame_width; dc.frame_height = p->vinfo.frame_height;
    // three rotating anchors per GOP of a window (+ its B pictures); behind them the carry slot (open GOPs across windows) and
    // a hold slot per lane (the I picture of an open GOP whose leading B pictures wait for the lane before: plan_levels)
    p->carry_slot = (3 + (p->unfused ? p->max_pics : 0)) * p->W;
    dc.n_slots = p->carry_slot + 1 + p->W;
    dc.alpha = p->vinfo.has_alpha == 1;        // yuva: the frames' A bytes come from the stream's fourth component
    dc.device_id = p->cfg.device_id;
    int rc = leon_create(&dc, &p->dec);
    if (rc == LEON_OK) rc = leon_set_quant_matrices(p->dec, p->vinfo.intra_qm, p->vinfo.non_intra_qm);
    if (rc != LEON_OK) return rc;
    if (!p->copy_stream.create(hipStreamNonBlocking)) return hip_fail(LEON_ERR_HIP, "copy stream");
    // (the tensors are made from the frames' planes: TENSOR runs the YCbCr road inside whether or not the planes are handed out)
    if ((p->output & (LEON_PIPELINE_OUTPUT_YCBCR | LEON_PIPELINE_OUTPUT_TENSOR)) && (rc = alloc_ring(p, &p->d_planes, p->planes_bytes, "planes")) != LEON_OK) return rc;
    if (p->output & LEON_PIPELINE_OUTPUT_TENSOR) {
        if ((rc = alloc_ring(p, &p->d_tensor, p->tensor_pitch, "tensor")) != LEON_OK) return rc;
        const size_t ids = (size_t)p->R * p->W * p->max_pics;
        if (!p->d_tensor_table.alloc(p->tensor_table.size()) || !p->tensor_ids.alloc(ids)) return hip_fail(LEON_ERR_NOMEM, "tensor table and frame index ring");
        if (hipMemcpy(p->d_tensor_table, p->tensor_table.data(), p->tensor_table.size(), hipMemcpyHostToDevice) != hipSuccess) return hip_fail(LEON_ERR_HIP, "tensor table");
        if (p->tensor_geom.resized) {
            const size_t tb = p->resize_tabs.size() * 4;
            if (!p->d_resize_tabs.alloc(tb)) return hip_fail(LEON_ERR_NOMEM, "resize tables");
            if (hipMemcpy(p->d_resize_tabs, p->resize_tabs.data(), tb, hipMemcpyHostToDevice) != hipSuccess) return hip_fail(LEON_ERR_HIP, "resize tables");
        }
    }
    if ((p->output & LEON_PIPELINE_OUTPUT_RGBA) && (rc = alloc_ring(p, &p->d_rgba, p->frame_bytes, "RGBA")) != LEON_OK) return rc;
    const auto alloc_records = [&](auto& out, const char* name) {          // a record output's ring (out.pitch: plan_pipeline) and its descriptor mirror
        if (const int rrc = alloc_ring(p, &out.ring, out.pitch, name); rrc != LEON_OK) return rrc;
        return out.descs.alloc((size_t)p->R * p->W * p->max_pics) ? (int)LEON_OK : hip_fail(LEON_ERR_NOMEM, std::string(name) + " descriptor ring");
    };
    if ((p->output & LEON_PIPELINE_OUTPUT_MOTION) && (rc = alloc_records(p->motion, "motion")) != LEON_OK) return rc;
    if ((p->output & LEON_PIPELINE_OUTPUT_ACTIVITY) && (rc = alloc_records(p->activity, "activity")) != LEON_OK) return rc;
    if ((p->output & LEON_PIPELINE_OUTPUT_RESIDUAL) && (rc = alloc_records(p->residual, "residual")) != LEON_OK) return rc;
    if (p->gpu_parser) {
        std::vector<leon_vlc_gpu_tables> src(1);
        std::vector<leon::VlcTables> t(1);
        leon_vlc_get_gpu_tables(src.data());
        const std::string bad = pack_vlc_tables(src[0], t[0]);
        if (!bad.empty()) return fail(LEON_ERR_INVALID, "%s", bad.c_str());
        // The parser kernels want little of the chip (a quarter of the issue slots of the SIMDs they sit on) but all of it
        // for as long as their longest slice takes; the reconstruction launches beside them fill every CU.  Highest
        // stream priority: a freed slot goes to a waiting parser workgroup first.
        int prio_lo = 0, prio_hi = 0;
        hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        for (Stream& vs : p->vlc_stream)
            if (!vs.create(hipStreamNonBlocking, prio_hi)) return hip_fail(LEON_ERR_HIP, "parser stream");
        if (!p->d_vlc_tables.alloc(sizeof(leon::VlcTables))) return hip_fail(LEON_ERR_NOMEM, "GPU parser tables");
        if (hipMemcpy(p->d_vlc_tables, t.data(), sizeof(leon::VlcTables), hipMemcpyHostToDevice) != hipSuccess) return hip_fail(LEON_ERR_HIP, "GPU parser tables");
        if (p->vlc_index_lds > kMaxVlcIndexLds)
            return hip_fail(LEON_ERR_INVALID, "picture too large for the GPU parser (its group counters do not fit in LDS): use LEON_PIPELINE_PARSER_HOST or LEON_PIPELINE_PARSER_DEFAULT");
        if (p->vlc_index_lds > 48 * 1024 &&
            hipFuncSetAttribute((const void*)leon::k_vlc_index, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->vlc_index_lds) != hipSuccess)
            return hip_fail(LEON_ERR_HIP, "LDS of the GPU parser's index kernel");
        p->vlc_ring.resize((size_t)p->R);
    }
    const int n_arenas = p->W * (p->R + 1);
    std::vector<Arena*> tickets;
    for (int i = 0; i < n_arenas; i++) {
        p->all_arenas.push_back(std::make_unique<Arena>());
        tickets.push_back(p->all_arenas.back().get());
    }
    p->flow.equip(p->W, p->R, tickets);
    if (p->gpu_parser) {
        // The arenas of the GPU parser come out of two slabs allocated HERE, sized for the largest GOP shard of the key
        // map by the bounds scan_gop_for_gpu sizes a GOP's arena with: vlc_entry_bound over the whole shard (32 / 3 bytes of
        // entry list per stream byte -- an entry takes three bits at least), vlc_pic_bytes and the least entry list of
        // max_gop_pictures pictures.  (Round 3 asked for 48 bytes per stream byte, 35 GB at W = 128 in 1080p.)  Allocated one
        // by one at their first use -- and again when a larger GOP came by, hipFree waits for the device -- the first four
        // windows of a 1080p run took 35-40 ms each instead of 8.6.  A GOP that does not fit all the same gets an allocation
        // of its own (arena_reserve); without the memory for the slabs everything does.
        size_t largest = 0;
        for (uint64_t g : p->shard_gops) largest = std::max(largest, (size_t)(p->shard_end[g] - p->shard_begin[g]));
        const size_t host_each = pad256(largest + 16) + 4096;
        const size_t dev_each = (pad256(largest + 16) + 4 * vlc_entry_bound(largest) +
                                 (size_t)p->max_pics * (vlc_pic_bytes(p).total + MapLayout::entries_pad(kVlcMinEntries)) + 65535) / 65536 * 65536;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)n_arenas * dev_each < free_b / 2 && !getenv("LEON_DEBUG_NO_SLABS")) {
            DevBuf<> dev;
            PinnedBuf<> host;
            if (dev.alloc((size_t)n_arenas * dev_each, kBigArenas) && host.alloc((size_t)n_arenas * host_each)) {
                p->slab_dev = std::move(dev);
                p->slab_host = std::move(host);
                for (int i = 0; i < n_arenas; i++) {
                    Arena* a = p->all_arenas[(size_t)i].get();
                    a->dev.borrow(p->slab_dev + (size_t)i * dev_each, dev_each);
                    a->host.borrow(p->slab_host + (size_t)i * host_each, host_each);
                }
            } else (void)hipGetLastError();
        }
    }
    return LEON_OK;
}

}  // namespace

extern "C" {

int leon_pipeline_create(const leon_pipeline_config* cfg, const uint8_t* stream, size_t bytes,
                         leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    return leon_pipeline_create_tensor(cfg, nullptr, stream, bytes, bytes, cb, user, out);
}

int leon_pipeline_create_partial(const leon_pipeline_config* cfg, const uint8_t* stream, size_t bytes, size_t valid_bytes,
                                 leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    return leon_pipeline_create_tensor(cfg, nullptr, stream, bytes, valid_bytes, cb, user, out);
}

int leon_pipeline_tensor_table(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, void* out768)
{
    if (!cfg || !out768) return fail(LEON_ERR_INVALID, "null argument");
    return tensor_table_build(cfg, tensor, nullptr, out768);
}

int leon_pipeline_feed(leon_pipeline* p, size_t valid_bytes)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    if (valid_bytes > p->bytes) return fail(LEON_ERR_INVALID, "%zu bytes fed, the stream has %zu", valid_bytes, p->bytes);
    p->flow.feed(valid_bytes);
    return LEON_OK;
}

int leon_pipeline_create_tensor(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const uint8_t* stream, size_t bytes,
                                size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    return leon_pipeline_create_tensor_resized(cfg, tensor, nullptr, stream, bytes, valid_bytes, cb, user, out);
}

int leon_pipeline_resize_weights(int32_t in_size, int32_t crop_start, int32_t crop_size, int32_t out_size, int32_t filter,
                                 int32_t* first, int32_t* count, int32_t* weights, int32_t max_taps)
{
    if (!first || !count || !weights) return fail(LEON_ERR_INVALID, "null argument");
    return resize_axis_build("axis", in_size, crop_start, crop_size, out_size, filter, first, count, weights, max_taps, nullptr);
}

int leon_pipeline_get_tensor_geometry(leon_pipeline* p, leon_pipeline_tensor_geometry* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!(p->output & LEON_PIPELINE_OUTPUT_TENSOR)) return no_output("tensor", "TENSOR");
    *out = p->tensor_geom;
    return LEON_OK;
}

int leon_pipeline_create_tensor_resized(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                        const uint8_t* stream, size_t bytes, size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    return leon_pipeline_create_tensor_format(cfg, tensor, resize, nullptr, stream, bytes, valid_bytes, cb, user, out);
}

int leon_pipeline_get_tensor_shape(leon_pipeline* p, leon_pipeline_tensor_shape* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!(p->output & LEON_PIPELINE_OUTPUT_TENSOR)) return no_output("tensor", "TENSOR");
    const int64_t h = p->tensor_geom.height, w = p->tensor_geom.width;
    const bool hwc = p->tensor_layout == LEON_TENSOR_LAYOUT_HWC;
    *out = leon_pipeline_tensor_shape{p->tensor_dtype, (int32_t)p->tensor_elem, p->tensor_layout, 3, (int32_t)h, (int32_t)w, hwc ? 1 : h * w, hwc ? 3 * w : w, hwc ? 3 : 1};
    return LEON_OK;
}

int leon_pipeline_create_tensor_format(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                       const leon_pipeline_tensor_format* format, const uint8_t* stream, size_t bytes, size_t valid_bytes,
                                       leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    return leon_pipeline_create_tensor_canvas(cfg, tensor, resize, format, nullptr, stream, bytes, valid_bytes, cb, user, out);
}

int leon_pipeline_get_tensor_canvas(leon_pipeline* p, leon_pipeline_tensor_canvas* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!(p->output & LEON_PIPELINE_OUTPUT_TENSOR)) return no_output("tensor", "TENSOR");
    *out = p->tensor_canvas;
    return LEON_OK;
}

int leon_pipeline_letterbox(int32_t src_width, int32_t src_height, int32_t canvas_width, int32_t canvas_height,
                            leon_pipeline_tensor_resize* resize, leon_pipeline_tensor_canvas* canvas)
{
    if (!resize || !canvas) return fail(LEON_ERR_INVALID, "null argument");
    if (src_width < 1 || src_height < 1) return fail(LEON_ERR_INVALID, "letterbox: source %d x %d", src_width, src_height);
    if (canvas_width < 1 || canvas_height < 1) return fail(LEON_ERR_INVALID, "letterbox: canvas %d x %d", canvas_width, canvas_height);
    const leon::FitRect r = leon::letterbox_rect(src_width, src_height, canvas_width, canvas_height);          // (leon_resize_row.h: the device's text too)
    resize->out_width = r.ow; resize->out_height = r.oh;
    canvas->width = canvas_width; canvas->height = canvas_height;
    canvas->x = r.x; canvas->y = r.y;
    return LEON_OK;
}

int leon_pipeline_create_tensor_canvas(const leon_pipeline_config* cfg, const leon_pipeline_tensor_config* tensor, const leon_pipeline_tensor_resize* resize,
                                       const leon_pipeline_tensor_format* format, const leon_pipeline_tensor_canvas* canvas, const uint8_t* stream,
                                       size_t bytes, size_t valid_bytes, leon_pipeline_callback cb, void* user, leon_pipeline** out)
{
    if (!cfg || !stream || bytes < 16 || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (valid_bytes > bytes) return fail(LEON_ERR_INVALID, "%zu valid bytes of a stream of %zu", valid_bytes, bytes);
    *out = nullptr;
    leon_pipeline* p = new (std::nothrow) leon_pipeline();
    if (!p) return fail(LEON_ERR_NOMEM, "out of host memory");
    int rc = plan_pipeline(p, cfg, tensor, resize, format, canvas, stream, bytes, valid_bytes);
    if (rc != LEON_OK) { delete p; return rc; }
    p->cb = cb;
    p->user = user;
    rc = allocate_pipeline(p);
    if (rc != LEON_OK) {          // (the message survives the teardown)
        const std::string msg = g_err;
        leon_pipeline_destroy(p);
        return fail(rc, "%s", msg.c_str());
    }
    // stage 3: the threads
    p->t0 = Clock::now();
    for (int i = 0; i < p->K; i++) p->parsers.emplace_back(parser_main, p);
    p->submitter = std::thread(submit_main, p);
    p->notifier = std::thread(notify_main, p);
    *out = p;
    return LEON_OK;
}

int leon_pipeline_get_info(leon_pipeline* p, leon_pipeline_info* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    *out = p->info;
    const std::shared_ptr<const PipeRun> run = p->flow.run();       // these two change with the run (leon_pipeline_seek)
    out->first_gop = run->first_key;
    out->shard_gops = (uint32_t)run->mine.size();
    return LEON_OK;
}

int leon_pipeline_release_window(leon_pipeline* p, int64_t window)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    if (!p->flow.release(window)) return fail(LEON_ERR_INVALID, "window %lld is not out for delivery", (long long)window);
    return LEON_OK;
}

int leon_pipeline_wait(leon_pipeline* p)
{
    if (!p) return fail(LEON_ERR_INVALID, "null pipeline");
    const int status = p->flow.wait_run();
    if (status != LEON_OK) return fail(status, "%s", p->flow.error());
    return LEON_OK;
}

int leon_pipeline_seek(leon_pipeline* p, double seconds, int32_t mode, int64_t* first_window)
{
    if (!p || !first_window) return fail(LEON_ERR_INVALID, "null argument");
    if (mode != LEON_PIPELINE_SEEK_KEY && mode != LEON_PIPELINE_SEEK_EXACT) return fail(LEON_ERR_INVALID, "seek mode %d", mode);
    if (!std::isfinite(seconds)) return fail(LEON_ERR_INVALID, "seek to a time that is not finite");
    if (p->cfg.loop > 1) return fail(LEON_ERR_INVALID, "a pipeline that loops over the stream (loop = %d, benchmarking) does not seek", p->cfg.loop);
    if (std::this_thread::get_id() == p->notifier.get_id()) return fail(LEON_ERR_INVALID, "leon_pipeline_seek from inside the pipeline's callback");
    if (p->flow.status() != LEON_OK) return fail(LEON_ERR_INVALID, "the pipeline has failed: %s", p->flow.error());
    // the key map through a view of the pipeline's own bytes: nothing is copied, and a partial stream may be seeked
    // past what has arrived (the parser threads wait for leon_pipeline_feed, as after create)
    leon_vlc_stream* st = nullptr;
    if (p->has_keymap && seconds > 0 && leon_vlc_open_scan(p->stream, p->bytes - 16, p->bytes, p->vinfo.has_alpha, &st) != LEON_VLC_OK)
        return fail(LEON_ERR_INVALID, "stream: %s", leon_vlc_last_error());
    const std::shared_ptr<PipeRun> run = make_run(p, st, seconds, 1);
    if (st) leon_vlc_close(st);
    // EXACT: the shard that owns the entry trims its first GOP (trim_to_target); the others decode from their next GOP on
    if (mode == LEON_PIPELINE_SEEK_EXACT && !run->mine.empty() && run->mine[0] == run->first_key) run->exact_ms = std::max(seconds, 0.0) * 1000.0;
    if (!p->flow.seek(run, first_window)) return fail(LEON_ERR_INVALID, "the pipeline has failed: %s", p->flow.error());
    return LEON_OK;
}

int leon_pipeline_get_stats(leon_pipeline* p, leon_pipeline_stats* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    const PipeFlow::Counts c = p->flow.counts();
    out->pictures = p->st_pictures;
    out->gops = p->st_gops;
    out->windows = (uint64_t)c.windows_done;
    out->stream_bytes = p->bytes;
    out->seconds = c.seconds;
    out->parse_seconds_sum = (double)p->st_parse_ns.load() * 1e-9;
    out->upload_bytes = (double)p->st_upload.load();
    out->entries = p->st_entries;
    return LEON_OK;
}

int leon_pipeline_read_frame(leon_pipeline* p, const leon_pipeline_frame* f, uint8_t* rgba_host)
{
    if (!p || !f || !rgba_host) return fail(LEON_ERR_INVALID, "null argument");
    if (!f->rgba) return fail(LEON_ERR_INVALID, "the frame has no RGBA (leon_pipeline_config.output without LEON_PIPELINE_OUTPUT_RGBA)");
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    HIP_TRY(hipMemcpy(rgba_host, f->rgba, p->frame_bytes, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_read_frame_planes(leon_pipeline* p, const leon_pipeline_frame* f, uint8_t* y, uint8_t* cb, uint8_t* cr, uint8_t* a)
{
    if (!p || !f || !y || !cb || !cr) return fail(LEON_ERR_INVALID, "null argument");
    if (!f->y || !f->cb || !f->cr) return fail(LEON_ERR_INVALID, "the frame has no planes (leon_pipeline_config.output without LEON_PIPELINE_OUTPUT_YCBCR)");
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    const size_t fw = (size_t)p->info.frame_width, fh = (size_t)p->info.frame_height;
    const size_t cw = (size_t)p->info.chroma_width, chh = (size_t)p->info.chroma_height;
    const size_t ls = p->planes_geom.luma_stride, cs = p->planes_geom.chroma_stride;
    HIP_TRY(hipMemcpy2D(y, fw, f->y, ls, fw, fh, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(cb, cw, f->cb, cs, cw, chh, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(cr, cw, f->cr, cs, cw, chh, hipMemcpyDeviceToHost));
    if (a && f->a) HIP_TRY(hipMemcpy2D(a, fw, f->a, ls, fw, fh, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_window_tensors(leon_pipeline* p, int64_t window, void** out, int32_t n)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->d_tensor) return no_output("tensor", "TENSOR");
    return window_items(p, window, &PipeWindow::tensors, "tensors", out, n);
}

int leon_pipeline_read_tensor(leon_pipeline* p, int64_t window, int32_t index, void* host)
{
    if (!p || !host) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->d_tensor) return no_output("tensor", "TENSOR");
    uint8_t* src = nullptr;
    if (const int rc = window_item(p, window, index, &PipeWindow::tensors, &src); rc != LEON_OK) return rc;
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    HIP_TRY(hipMemcpy(host, src, p->tensor_bytes, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_motion_layout(int32_t mb_width, int32_t mb_height, struct leon_pipeline_motion_layout* out)
{
    return motion_layout_host(mb_width, mb_height, out);
}

int leon_pipeline_motion_record(int32_t type, int32_t mb_width, int32_t mb_height, const uint8_t* repadd, const uint8_t* mb_dir,
                                const int16_t* mv_fwd, const int16_t* mv_bwd, void* record)
{
    return motion_record_host(type, mb_width, mb_height, repadd, mb_dir, mv_fwd, mv_bwd, record);
}

int leon_pipeline_motion_kernel(int32_t device_id, int32_t mb_width, int32_t mb_height, const leon_pipeline_motion_picture* pictures, int32_t n_pictures,
                                const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring)
{
    return motion_kernel(device_id, mb_width, mb_height, pictures, n_pictures, frames, n_frames, ring_frames, pad_byte, ring);
}

int leon_pipeline_get_motion_layout(leon_pipeline* p, struct leon_pipeline_motion_layout* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->motion.ring) return no_output("motion", "MOTION");
    return motion_layout_host(p->vinfo.mb_width, p->vinfo.mb_height, out);
}

int leon_pipeline_window_motion(leon_pipeline* p, int64_t window, leon_pipeline_motion_frame* out, int32_t n)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->motion.ring) return no_output("motion", "MOTION");
    return window_items(p, window, &PipeWindow::motion, "motion records", out, n);
}

int leon_pipeline_read_motion(leon_pipeline* p, int64_t window, int32_t index, int16_t* mv, uint8_t* info, uint32_t* summary)
{
    if (!p) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->motion.ring) return no_output("motion", "MOTION");
    leon_pipeline_motion_frame f{};
    if (const int rc = window_item(p, window, index, &PipeWindow::motion, &f); rc != LEON_OK) return rc;
    const uint8_t* src = static_cast<const uint8_t*>(f.record);
    const leon::MotionLayout& L = p->motion_lay;
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    if (mv) HIP_TRY(hipMemcpy(mv, src, (size_t)L.mbs * 8, hipMemcpyDeviceToHost));
    if (info) HIP_TRY(hipMemcpy(info, src + L.info_offset, L.mbs, hipMemcpyDeviceToHost));
    if (summary) HIP_TRY(hipMemcpy(summary, src + L.summary_offset, 32, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_activity_layout(int32_t mb_width, int32_t mb_height, struct leon_pipeline_activity_layout* out)
{
    return activity_layout_host(mb_width, mb_height, out);
}

int leon_pipeline_activity_record(int32_t mb_width, int32_t mb_height, const uint32_t* grp_off, const uint32_t* entries, uint32_t n_entries,
                                  const uint8_t* qscale, void* record)
{
    return activity_record_host(mb_width, mb_height, grp_off, entries, n_entries, qscale, record);
}

int leon_pipeline_activity_kernel(int32_t device_id, int32_t mb_width, int32_t mb_height, const leon_pipeline_activity_picture* pictures, int32_t n_pictures,
                                  const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames, int32_t pad_byte, void* ring)
{
    return activity_kernel(device_id, mb_width, mb_height, pictures, n_pictures, frames, n_frames, ring_frames, pad_byte, ring);
}

int leon_pipeline_get_activity_layout(leon_pipeline* p, struct leon_pipeline_activity_layout* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->activity.ring) return no_output("activity", "ACTIVITY");
    return activity_layout_host(p->vinfo.mb_width, p->vinfo.mb_height, out);
}

int leon_pipeline_window_activity(leon_pipeline* p, int64_t window, void** out, int32_t n)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->activity.ring) return no_output("activity", "ACTIVITY");
    return window_items(p, window, &PipeWindow::activity, "activity records", out, n);
}

int leon_pipeline_read_activity(leon_pipeline* p, int64_t window, int32_t index, void* cells, uint32_t* summary)
{
    if (!p) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->activity.ring) return no_output("activity", "ACTIVITY");
    uint8_t* src = nullptr;
    if (const int rc = window_item(p, window, index, &PipeWindow::activity, &src); rc != LEON_OK) return rc;
    const leon::ActivityLayout& L = p->activity_lay;
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    if (cells) HIP_TRY(hipMemcpy(cells, src, (size_t)L.mbs * 8, hipMemcpyDeviceToHost));
    if (summary) HIP_TRY(hipMemcpy(summary, src + L.summary_offset, 32, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_residual_layout(int32_t coded_width, int32_t coded_height, struct leon_pipeline_residual_layout* out)
{
    return residual_layout_host(coded_width, coded_height, out);
}

int leon_pipeline_residual_kernel(int32_t device_id, int32_t coded_width, int32_t coded_height, const leon_pipeline_residual_picture* pictures,
                                  int32_t n_pictures, const leon_pipeline_motion_kernel_frame* frames, int32_t n_frames, int32_t ring_frames,
                                  int32_t pad_byte, void* ring)
{
    return residual_kernel(device_id, coded_width, coded_height, pictures, n_pictures, frames, n_frames, ring_frames, pad_byte, ring);
}

int leon_pipeline_get_residual_layout(leon_pipeline* p, struct leon_pipeline_residual_layout* out)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->residual.ring) return no_output("residual", "RESIDUAL");
    return residual_layout_host(p->vinfo.coded_width, p->vinfo.coded_height, out);
}

int leon_pipeline_window_residual(leon_pipeline* p, int64_t window, void** out, int32_t n)
{
    if (!p || !out) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->residual.ring) return no_output("residual", "RESIDUAL");
    return window_items(p, window, &PipeWindow::residual, "residual records", out, n);
}

int leon_pipeline_read_residual(leon_pipeline* p, int64_t window, int32_t index, int16_t* y, int16_t* cb, int16_t* cr)
{
    if (!p) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->residual.ring) return no_output("residual", "RESIDUAL");
    uint8_t* src = nullptr;
    if (const int rc = window_item(p, window, index, &PipeWindow::residual, &src); rc != LEON_OK) return rc;
    const leon::ResidualLayout& L = p->residual_lay;
    HIP_TRY(hipSetDevice(p->cfg.device_id));
    const size_t w = L.cw, h = L.ch;
    if (y) HIP_TRY(hipMemcpy2D(y, 2 * w, src, 2 * (size_t)L.luma_stride, 2 * w, h, hipMemcpyDeviceToHost));
    if (cb) HIP_TRY(hipMemcpy2D(cb, w, src + L.cb_offset, 2 * (size_t)L.chroma_stride, w, h / 2, hipMemcpyDeviceToHost));
    if (cr) HIP_TRY(hipMemcpy2D(cr, w, src + L.cr_offset, 2 * (size_t)L.chroma_stride, w, h / 2, hipMemcpyDeviceToHost));
    return LEON_OK;
}

int leon_pipeline_regions_check(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* regions, int32_t n,
                                const leon_pipeline_regions_config* cfg, int32_t* bad)
{
    return regions_check(frame_width, frame_height, n_frames, regions, n, cfg, RegionsFit{}, bad, nullptr);
}

int leon_pipeline_resample_regions(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                                   const leon_pipeline_regions_config* cfg, void* device_out, uint64_t out_pitch_bytes)
{
    return resample_regions(p, window, regions, n, cfg, nullptr, device_out, out_pitch_bytes, nullptr);
}

int leon_pipeline_read_regions(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n,
                               const leon_pipeline_regions_config* cfg, void* host)
{
    if (!host) return fail(LEON_ERR_INVALID, "null argument");
    return resample_regions(p, window, regions, n, cfg, nullptr, nullptr, 0, host);
}

int leon_pipeline_resample_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_device* call)
{
    return resample_regions_device(p, window, cfg, nullptr, call, nullptr);
}

int32_t leon_pipeline_region_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* region,
                                    const leon_pipeline_regions_config* cfg)
{
    if (!region || !cfg) return fail(LEON_ERR_INVALID, "null argument");
    const int rc = regions_config_check(frame_width, frame_height, n_frames, 1, cfg);
    return rc != LEON_OK ? rc : region_status(frame_width, frame_height, n_frames, *region, *cfg, RegionsFit{});
}

int leon_pipeline_region_fit_rect(int32_t box_width, int32_t box_height, const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit_settings,
                                  int32_t rect[4])
{
    if (!cfg || !rect) return fail(LEON_ERR_INVALID, "null argument");
    int rc = regions_config_check(1, 1, 0, 1, cfg);
    RegionsFit fit;
    if (rc != LEON_OK || (rc = regions_fit_check(fit_settings, &fit)) != LEON_OK) return rc;
    if (box_width < 1 || box_height < 1) return fail(LEON_ERR_INVALID, "regions fit: a box of %d x %d", box_width, box_height);
    leon_pipeline_region r{};
    r.width = box_width; r.height = box_height;
    const leon::FitRect image = region_image(r, *cfg, fit);
    rect[0] = image.x; rect[1] = image.y; rect[2] = image.ow; rect[3] = image.oh;
    return LEON_OK;
}

int leon_pipeline_regions_fit_check(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* regions, int32_t n,
                                    const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit_settings, int32_t* bad)
{
    if (bad) *bad = -1;
    RegionsFit fit;
    const int rc = regions_fit_check(fit_settings, &fit);
    return rc != LEON_OK ? rc : regions_check(frame_width, frame_height, n_frames, regions, n, cfg, fit, bad, nullptr);
}

int32_t leon_pipeline_region_fit_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_region* region,
                                        const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit_settings)
{
    if (!region || !cfg) return fail(LEON_ERR_INVALID, "null argument");
    RegionsFit fit;
    int rc = regions_config_check(frame_width, frame_height, n_frames, 1, cfg);
    if (rc == LEON_OK) rc = regions_fit_check(fit_settings, &fit);
    return rc != LEON_OK ? rc : region_status(frame_width, frame_height, n_frames, *region, *cfg, fit);
}

int leon_pipeline_resample_regions_fit(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n, const leon_pipeline_regions_config* cfg,
                                       const leon_pipeline_regions_fit* fit, void* device_out, uint64_t out_pitch_bytes)
{
    return resample_regions(p, window, regions, n, cfg, fit, device_out, out_pitch_bytes, nullptr);
}

int leon_pipeline_read_regions_fit(leon_pipeline* p, int64_t window, const leon_pipeline_region* regions, int32_t n, const leon_pipeline_regions_config* cfg,
                                   const leon_pipeline_regions_fit* fit, void* host)
{
    if (!host) return fail(LEON_ERR_INVALID, "null argument");
    return resample_regions(p, window, regions, n, cfg, fit, nullptr, 0, host);
}

int leon_pipeline_resample_regions_device_fit(leon_pipeline* p, int64_t window, const leon_pipeline_regions_config* cfg, const leon_pipeline_regions_fit* fit,
                                              const leon_pipeline_regions_device* call, int32_t* device_rects)
{
    return resample_regions_device(p, window, cfg, fit, call, device_rects);
}

int leon_pipeline_warp_regions_check(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_warp_region* regions, int32_t n,
                                     const leon_pipeline_warp_config* cfg, int32_t* bad)
{
    return warp_regions_check(frame_width, frame_height, n_frames, regions, n, cfg, bad, nullptr);
}

int32_t leon_pipeline_warp_region_status(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_warp_region* region,
                                         const leon_pipeline_warp_config* cfg)
{
    if (!region || !cfg) return fail(LEON_ERR_INVALID, "null argument");
    const int rc = warp_config_check(frame_width, frame_height, n_frames, 1, cfg, nullptr);
    int32_t g;
    return rc != LEON_OK ? rc : leon::warp_record_status(warp_record(*region), n_frames, &g);
}

int leon_pipeline_warp_from_matrix(const double A[6], int32_t m[6])
{
    return warp_quantise(A, m);
}

int leon_pipeline_warp_from_rotated_box(double cx, double cy, double w, double h, double angle_degrees, int32_t out_width, int32_t out_height, int32_t m[6])
{
    if (out_width < 1 || out_height < 1) return fail(LEON_ERR_INVALID, "warp: an out size of %d x %d", out_width, out_height);
    if (!std::isfinite(angle_degrees)) return fail(LEON_ERR_INVALID, "warp: the angle is not finite");
    const double rad = angle_degrees * (3.14159265358979323846 / 180.0), cs = std::cos(rad), sn = std::sin(rad);
    const double ow = out_width, oh = out_height;
    double A[6];
    A[0] = w / ow * cs; A[1] = -h / oh * sn;
    A[3] = w / ow * sn; A[4] = h / oh * cs;
    A[2] = cx - (A[0] * (ow / 2) + A[1] * (oh / 2));
    A[5] = cy - (A[3] * (ow / 2) + A[4] * (oh / 2));
    return warp_quantise(A, m);
}

int leon_pipeline_warp_regions(leon_pipeline* p, int64_t window, const leon_pipeline_warp_region* regions, int32_t n, const leon_pipeline_warp_config* cfg,
                               void* device_out, uint64_t out_pitch_bytes)
{
    return warp_regions(p, window, regions, n, cfg, device_out, out_pitch_bytes, nullptr);
}

int leon_pipeline_read_warp_regions(leon_pipeline* p, int64_t window, const leon_pipeline_warp_region* regions, int32_t n, const leon_pipeline_warp_config* cfg,
                                    void* host)
{
    if (!host) return fail(LEON_ERR_INVALID, "null argument");
    return warp_regions(p, window, regions, n, cfg, nullptr, 0, host);
}

int leon_pipeline_warp_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_warp_config* cfg, const leon_pipeline_warp_regions_call* call)
{
    return warp_regions_device(p, window, cfg, call);
}

int leon_pipeline_carry_refs(const leon_pipeline_frame* frames, const leon_pipeline_motion_frame* motion, int32_t n_frames, int32_t* fwd, int32_t* bwd)
{
    if (n_frames < 0 || (n_frames && (!frames || !motion || !fwd || !bwd))) return fail(LEON_ERR_INVALID, n_frames < 0 ? "carry refs: a negative frame count" : "null argument");
    carry_refs_host(frames, motion, n_frames, fwd, bwd);
    return LEON_OK;
}

int32_t leon_pipeline_carry_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames, const int32_t* fwd, const int32_t* bwd,
                                   const void* const* records, const leon_pipeline_carry_region* rec, leon_pipeline_region* out, int32_t* votes)
{
    return carry_record_host(frame_width, frame_height, mb_width, mb_height, n_frames, fwd, bwd, records, rec, out, votes, false);
}

int leon_pipeline_get_carry_refs(leon_pipeline* p, int64_t window, int32_t* fwd, int32_t* bwd, int32_t n)
{
    if (!p || !fwd || !bwd) return fail(LEON_ERR_INVALID, "null argument");
    if (!p->motion.ring) return no_output("motion", "MOTION");
    size_t has = 0;
    const bool delivered = p->flow.with_delivered(window, [&](const PipeWindow& w) {
        has = w.carry_table.size() / 4;
        if (n >= 0 && (size_t)n == has)
            for (size_t i = 0; i < has; i++) {
                fwd[i] = (int32_t)w.carry_table[4 * i + 1];
                bwd[i] = (int32_t)w.carry_table[4 * i + 2];
            }
    });
    if (!delivered) return fail(LEON_ERR_INVALID, "window %lld is not out for delivery", (long long)window);
    if (n < 0 || (size_t)n != has) return fail(LEON_ERR_INVALID, "window %lld has %zu frames, not %d", (long long)window, has, n);
    return LEON_OK;
}

int leon_pipeline_carry_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_carry_regions_call* call)
{
    return carry_regions_device(p, window, call);
}

int leon_pipeline_carry_regions(leon_pipeline* p, int64_t window, const leon_pipeline_carry_region* regions, int32_t n, leon_pipeline_region* out, int32_t* votes,
                                int32_t* status)
{
    return carry_regions(p, window, regions, n, out, votes, status);
}

int leon_pipeline_carry_device(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames, const int32_t* fwd,
                               const int32_t* bwd, const void* const* records_host, const leon_pipeline_carry_region* regions, int32_t n, leon_pipeline_region* out,
                               int32_t* votes, int32_t* status)
{
    return carry_device(device_id, frame_width, frame_height, mb_width, mb_height, n_frames, fwd, bwd, records_host, regions, n, out, votes, status);
}

int32_t leon_pipeline_gauge_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames, const void* const* motion_records,
                                   const void* const* activity_records, const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* rec, int64_t* stats)
{
    return gauge_record_host(frame_width, frame_height, mb_width, mb_height, n_frames, motion_records, activity_records, cfg, rec, stats, false);
}

int leon_pipeline_gauge_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg, const leon_pipeline_gauge_regions_call* call)
{
    return gauge_regions_device(p, window, cfg, call);
}

int leon_pipeline_gauge_regions(leon_pipeline* p, int64_t window, const leon_pipeline_gauge_config* cfg, const leon_pipeline_region* regions, int32_t n, int64_t* stats,
                                int32_t* status)
{
    return gauge_regions(p, window, cfg, regions, n, stats, status);
}

int leon_pipeline_gauge_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                               const void* const* motion_records_host, const void* const* activity_records_host, const leon_pipeline_gauge_config* cfg,
                               const leon_pipeline_region* regions, int32_t n, int64_t* stats, int32_t* status)
{
    return gauge_kernel(device_id, frame_width, frame_height, mb_width, mb_height, n_frames, motion_records_host, activity_records_host, cfg, regions, n, stats, status);
}

int32_t leon_pipeline_propose_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames, const void* const* motion_records,
                                     const void* const* activity_records, const leon_pipeline_propose_config* cfg, int32_t frame, leon_pipeline_region* regions, int32_t* info,
                                     int32_t* count)
{
    return propose_record_host(frame_width, frame_height, mb_width, mb_height, n_frames, motion_records, activity_records, cfg, frame, regions, info, count, false);
}

int leon_pipeline_propose_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg, const leon_pipeline_propose_regions_call* call)
{
    return propose_regions_device(p, window, cfg, call);
}

int leon_pipeline_propose_regions(leon_pipeline* p, int64_t window, const leon_pipeline_propose_config* cfg, const int32_t* frames, int32_t n, leon_pipeline_region* regions,
                                  int32_t* info, int32_t* count, int32_t* status)
{
    return propose_regions(p, window, cfg, frames, n, regions, info, count, status);
}

int leon_pipeline_propose_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                 const void* const* motion_records_host, const void* const* activity_records_host, const leon_pipeline_propose_config* cfg,
                                 const int32_t* frames, int32_t n, leon_pipeline_region* regions, int32_t* info, int32_t* count, int32_t* status)
{
    return propose_kernel(device_id, frame_width, frame_height, mb_width, mb_height, n_frames, motion_records_host, activity_records_host, cfg, frames, n, regions, info, count,
                          status);
}

int32_t leon_pipeline_suppress_record(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                                      const leon_pipeline_region* regions, int32_t k, const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order,
                                      int32_t* by, int32_t* count, int32_t* status)
{
    return suppress_record_host(frame_width, frame_height, n_frames, cfg, regions, k, scores, score_stride, out, order, by, count, status);
}

int32_t leon_pipeline_match_record(int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a,
                                   int32_t ka, const leon_pipeline_region* b, int32_t kb, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count,
                                   int32_t* status_a, int32_t* status_b)
{
    return match_record_host(frame_width, frame_height, n_frames, cfg, a, ka, b, kb, match_a, match_b, overlap, count, status_a, status_b);
}

int leon_pipeline_suppress_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_suppress_regions_call* call)
{
    return suppress_regions_device(p, window, cfg, call);
}

int leon_pipeline_match_regions_device(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_match_regions_call* call)
{
    return match_regions_device(p, window, cfg, call);
}

int leon_pipeline_suppress_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* regions, int32_t n, int32_t k,
                                   const int32_t* scores, int32_t score_stride, leon_pipeline_region* out, int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    return suppress_regions(p, window, cfg, regions, n, k, scores, score_stride, out, order, by, count, status);
}

int leon_pipeline_match_regions(leon_pipeline* p, int64_t window, const leon_pipeline_overlap_config* cfg, const leon_pipeline_region* a, int32_t ka,
                                const leon_pipeline_region* b, int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b, int32_t* overlap, int32_t* count,
                                int32_t* status_a, int32_t* status_b)
{
    return match_regions(p, window, cfg, a, ka, b, kb, n, match_a, match_b, overlap, count, status_a, status_b);
}

int leon_pipeline_suppress_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                                  const leon_pipeline_region* regions, int32_t n, int32_t k, const int32_t* scores, int32_t score_stride, leon_pipeline_region* out,
                                  int32_t* order, int32_t* by, int32_t* count, int32_t* status)
{
    return suppress_kernel(device_id, frame_width, frame_height, n_frames, cfg, regions, n, k, scores, score_stride, out, order, by, count, status);
}

int leon_pipeline_match_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t n_frames, const leon_pipeline_overlap_config* cfg,
                               const leon_pipeline_region* a, int32_t ka, const leon_pipeline_region* b, int32_t kb, int32_t n, int32_t* match_a, int32_t* match_b,
                               int32_t* overlap, int32_t* count, int32_t* status_a, int32_t* status_b)
{
    return match_kernel(device_id, frame_width, frame_height, n_frames, cfg, a, ka, b, kb, n, match_a, match_b, overlap, count, status_a, status_b);
}

int leon_pipeline_propagate_layout(int32_t frame_width, int32_t frame_height, int32_t stride, int32_t planes, int32_t elem_bytes, struct leon_pipeline_propagate_layout* out)
{
    if (!out) return fail(LEON_ERR_INVALID, "null argument");
    if (frame_width < 1 || frame_width > 16 * leon::kMotionMaxMb || frame_height < 1 || frame_height > 16 * leon::kMotionMaxMb)
        return fail(LEON_ERR_INVALID, "propagate: a frame of %d x %d (1 .. %d each)", frame_width, frame_height, 16 * leon::kMotionMaxMb);
    leon::PropagateGeom g;
    if (!leon::propagate_geometry(frame_width, frame_height, (frame_width + 15) / 16, stride, planes, elem_bytes, &g))
        return fail(LEON_ERR_INVALID, "propagate: stride %d (1, 2, 4, 8, 16), %d planes (1 .. %d), elem_bytes %d (1, 2, 4)", stride, planes, leon::kPropagateMaxPlanes, elem_bytes);
    out->mw = g.mw; out->mh = g.mh;
    out->planes_per_group = g.group; out->fast_path = g.fast;
    out->plane_bytes = g.plane_bytes; out->slot_bytes = (uint64_t)g.planes * g.plane_bytes;
    return LEON_OK;
}

int32_t leon_pipeline_propagate_record(int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames, const void* const* records,
                                       const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hop, void* maps, uint8_t* via)
{
    return propagate_record_host(frame_width, frame_height, mb_width, mb_height, n_frames, records, cfg, hop, maps, via);
}

int leon_pipeline_propagate_maps_device(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_maps_call* call)
{
    return propagate_maps_device(p, window, cfg, call);
}

int leon_pipeline_propagate_maps(leon_pipeline* p, int64_t window, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* maps,
                                 uint8_t* via, int32_t* status)
{
    return propagate_maps(p, window, cfg, hops, n, maps, via, status);
}

int leon_pipeline_propagate_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t mb_width, int32_t mb_height, int32_t n_frames,
                                   const void* const* records_host, const leon_pipeline_propagate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* maps,
                                   uint8_t* via, int32_t* status)
{
    return propagate_kernel(device_id, frame_width, frame_height, mb_width, mb_height, n_frames, records_host, cfg, hops, n, maps, via, status);
}

int leon_pipeline_accumulate_layout(int32_t coded_width, int32_t coded_height, int32_t parts, struct leon_pipeline_accumulate_layout* out)
{
    return accumulate_layout_host(coded_width, coded_height, parts, out);
}

int32_t leon_pipeline_accumulate_record(int32_t coded_width, int32_t coded_height, int32_t n_frames, const void* const* motion_records, const void* const* residual_records,
                                        const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hop, void* slots, uint8_t* via)
{
    return accumulate_record_host(coded_width, coded_height, n_frames, motion_records, residual_records, cfg, hop, slots, via);
}

int leon_pipeline_accumulate_device(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_accumulate_call* call)
{
    return accumulate_device(p, window, cfg, call);
}

int leon_pipeline_accumulate(leon_pipeline* p, int64_t window, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n, void* slots,
                             uint8_t* via, int32_t* status)
{
    return accumulate(p, window, cfg, hops, n, slots, via, status);
}

int leon_pipeline_accumulate_kernel(int32_t device_id, int32_t coded_width, int32_t coded_height, int32_t n_frames, const void* const* motion_records_host,
                                    const void* const* residual_records_host, const leon_pipeline_accumulate_config* cfg, const leon_pipeline_propagate_hop* hops, int32_t n,
                                    void* slots, uint8_t* via, int32_t* status)
{
    return accumulate_kernel(device_id, coded_width, coded_height, n_frames, motion_records_host, residual_records_host, cfg, hops, n, slots, via, status);
}

int32_t leon_pipeline_field_tensor_record(int32_t frame_width, int32_t frame_height, int32_t coded_width, int32_t coded_height, const leon_pipeline_field_config* cfg,
                                          const void* items, const leon_pipeline_region* record, void* out)
{
    return field_tensor_record_host(frame_width, frame_height, coded_width, coded_height, cfg, items, record, out);
}

int leon_pipeline_field_tensors_device(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_field_tensors_call* call)
{
    return field_tensors_device(p, window, cfg, call);
}

int leon_pipeline_field_tensors(leon_pipeline* p, int64_t window, const leon_pipeline_field_config* cfg, const leon_pipeline_region* records, int32_t n, const void* source,
                                void* out, uint64_t out_pitch_bytes, int32_t* status)
{
    return field_tensors(p, window, cfg, records, n, source, out, out_pitch_bytes, status);
}

int leon_pipeline_field_tensors_kernel(int32_t device_id, int32_t frame_width, int32_t frame_height, int32_t coded_width, int32_t coded_height,
                                       const leon_pipeline_field_config* cfg, const void* items, const leon_pipeline_region* records, int32_t n, void* out,
                                       uint64_t out_pitch_bytes, int32_t* status, uint64_t scratch_limit_bytes)
{
    return field_tensors_kernel(device_id, frame_width, frame_height, coded_width, coded_height, cfg, items, records, n, out, out_pitch_bytes, status, scratch_limit_bytes);
}

int leon_pipeline_resize_weights_device(int32_t device_id, int32_t n_axes, const int32_t* axes, int32_t filter, int32_t max_taps, int32_t* first, int32_t* count,
                                        int32_t* weights, int32_t* status)
{
    return resize_weights_device(device_id, n_axes, axes, filter, max_taps, first, count, weights, status);
}

const char* leon_pipeline_error(leon_pipeline* p)
{
    if (!p) return "";
    return p->flow.error();
}

void leon_pipeline_destroy(leon_pipeline* p)
{
    if (!p) return;
    p->flow.stop_quiet();      // no callbacks while tearing down
    for (auto& t : p->parsers) if (t.joinable()) t.join();
    if (p->submitter.joinable()) p->submitter.join();
    if (p->notifier.joinable()) p->notifier.join();      // drains what was submitted, releasing instead of delivering
    hipSetDevice(p->cfg.device_id);
    // every stream of the pipeline is idle before any of its memory is freed (a submit interrupted by `stop` may have
    // left uploads or parser kernels behind that no window's event covers)
    if (p->copy_stream) hipStreamSynchronize(p->copy_stream);
    if (p->regions_stream) hipStreamSynchronize(p->regions_stream);
    if (p->boxes_busy) hipEventSynchronize(p->boxes_done);          // (a caller's stream may still run the last call's launches)
    for (hipStream_t vs : p->vlc_stream)
        if (vs) hipStreamSynchronize(vs);
    if (p->dec) leon_sync(p->dec);
    p->flow.tear_down();       // delivered windows released, their events destroyed in front of the streams
    const int64_t submitted = p->flow.counts().windows_submitted;
    if (getenv("LEON_DEBUG_PIPE_TIMING"))      // where the submit thread's time went (LEON_DEBUG_PIPE_TIMING=1)
        fprintf(stderr, "leon pipeline: %llu windows; per window on the submit thread: %.2f ms waiting for a ring entry, %.2f ms waiting for the window's GOPs "
                        "(parser threads), %.2f ms in submit_window\n", (unsigned long long)submitted,
                submitted ? (double)p->st_wait_ring_ns / 1e6 / (double)submitted : 0.0,
                submitted ? (double)p->st_wait_scan_ns / 1e6 / (double)submitted : 0.0,
                submitted ? (double)p->st_submit_ns.load() / 1e6 / (double)submitted : 0.0);
    const std::vector<double> window_done = p->flow.window_done();
    if (getenv("LEON_DEBUG_PIPE_TIMING") && !window_done.empty()) {
        fprintf(stderr, "leon pipeline: windows completed at (ms):");
        for (size_t i = 0; i < window_done.size() && i < 64; i++) fprintf(stderr, " %.1f", window_done[i] * 1e3);
        fprintf(stderr, "\n");
    }
    leon_decoder* const dec = p->dec;
    delete p;      // the members give back what the pipeline owns: buffers and events first, the streams last (the order of declaration, reversed)
    if (dec) leon_destroy(dec);
}

}  // extern "C"
