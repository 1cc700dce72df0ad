// leon_napi.cc -- thin N-API addon: JavaScript (Node) -> the C ABI of include/leon.h.
// Nothing is computed here; every function forwards to libleon_hip.so and throws a
// JavaScript Error carrying leon_last_error() on failure (the reference throws from
// its GL layer the same way: decoders/jsv.js:120-122, :231-233, :1175).
//
//   const leon = require('./leon_napi.node');
//   const h = leon.create({codedWidth, codedHeight, frameWidth, frameHeight, nSlots, deviceId});
//   h.setQuantMatrices(u8[64], u8[64]); h.acquireSlot(); h.releaseSlot(s); h.freeDecodedSlots();
//   h.submitPicture({type, outSlot, refFwdSlot, refBwdSlot, coefY, coefCb, coefCr, qscale, intra,
//                    repadd, mvFwd, mvBwd, mbDir});            // = jsv.prototype.IDCT_GL
//   h.submitSparse({type, outSlot, refFwdSlot, refBwdSlot, grpOff, entries, nEntries, qscale, intra,
//                   repadd, mvFwd, mvBwd, mbDir});             // the same through the sparse boundary
//   h.convertRGBA(slot, flavour) -> Uint8Array; h.readPlanes(slot) -> {y, cb, cr}; h.sync(); h.destroy();
#include <node_api.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/leon.h"
#include "../../include/leon_pipeline.h"
#include "../../include/leon_vlc.h"
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

namespace {

struct Handle {
    leon_decoder* d;
    leon_config cfg;
};

#define NAPI_OK(call)                                                      \
    do {                                                                   \
        if ((call) != napi_ok) {                                           \
            napi_throw_error(env, nullptr, "N-API call failed: " #call);   \
            return nullptr;                                                \
        }                                                                  \
    } while (0)

napi_value throw_leon(napi_env env, int rc)
{
    char msg[600];
    snprintf(msg, sizeof msg, "leon error %d: %s", rc, leon_last_error());
    napi_throw_error(env, nullptr, msg);
    return nullptr;
}

bool get_i32(napi_env env, napi_value obj, const char* key, int32_t* out, int32_t dflt)
{
    napi_value v;
    bool has = false;
    *out = dflt;
    if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return true;
    if (napi_get_named_property(env, obj, key, &v) != napi_ok) return false;
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t == napi_undefined || t == napi_null) return true;
    return napi_get_value_int32(env, v, out) == napi_ok;
}

// typed array property -> pointer (nullptr when absent/null); checks the element count
bool get_array(napi_env env, napi_value obj, const char* key, napi_typedarray_type want, size_t min_len, const void** out)
{
    *out = nullptr;
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return true;
    if (napi_get_named_property(env, obj, key, &v) != napi_ok) return false;
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t == napi_undefined || t == napi_null) return true;
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) return false;
    napi_typedarray_type type;
    size_t len;
    void* data;
    if (napi_get_typedarray_info(env, v, &type, &len, &data, nullptr, nullptr) != napi_ok) return false;
    if (type != want || len < min_len) return false;
    *out = data;
    return true;
}

Handle* unwrap(napi_env env, napi_callback_info info, size_t* argc, napi_value* argv)
{
    napi_value self;
    if (napi_get_cb_info(env, info, argc, argv, &self, nullptr) != napi_ok) return nullptr;
    Handle* h = nullptr;
    if (napi_unwrap(env, self, (void**)&h) != napi_ok || !h || !h->d) {
        napi_throw_error(env, nullptr, "leon: decoder handle is destroyed or invalid");
        return nullptr;
    }
    return h;
}

void finalize(napi_env, void* data, void*)
{
    Handle* h = (Handle*)data;
    if (h->d) leon_destroy(h->d);
    delete h;
}

napi_value SetQuantMatrices(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    const uint8_t* m[2] = {nullptr, nullptr};
    for (size_t i = 0; i < argc && i < 2; i++) {
        napi_valuetype t;
        napi_typeof(env, argv[i], &t);
        if (t == napi_undefined || t == napi_null) continue;
        napi_typedarray_type type;
        size_t len;
        void* data;
        if (napi_get_typedarray_info(env, argv[i], &type, &len, &data, nullptr, nullptr) != napi_ok || type != napi_uint8_array || len < 64) {
            napi_throw_type_error(env, nullptr, "setQuantMatrices: Uint8Array(64) expected");
            return nullptr;
        }
        m[i] = (const uint8_t*)data;
    }
    int rc = leon_set_quant_matrices(h->d, m[0], m[1]);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value AcquireSlot(napi_env env, napi_callback_info info)
{
    size_t argc = 0;
    Handle* h = unwrap(env, info, &argc, nullptr);
    if (!h) return nullptr;
    int32_t slot = -1;
    int rc = leon_acquire_slot(h->d, &slot);
    if (rc != LEON_OK) return throw_leon(env, rc);          // "no free render buffers"
    napi_value v;
    NAPI_OK(napi_create_int32(env, slot, &v));
    return v;
}

napi_value ReleaseSlot(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int32_t slot = -1;
    if (argc < 1 || napi_get_value_int32(env, argv[0], &slot) != napi_ok) {
        napi_throw_type_error(env, nullptr, "releaseSlot(slot)");
        return nullptr;
    }
    int rc = leon_release_slot(h->d, slot);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value FreeDecodedSlots(napi_env env, napi_callback_info info)
{
    size_t argc = 0;
    Handle* h = unwrap(env, info, &argc, nullptr);
    if (!h) return nullptr;
    int rc = leon_free_decoded_slots(h->d);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value SubmitPicture(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    if (argc < 1) {
        napi_throw_type_error(env, nullptr, "submitPicture(picture)");
        return nullptr;
    }
    napi_value p = argv[0];
    leon_picture pic;
    memset(&pic, 0, sizeof pic);
    size_t ny = (size_t)h->cfg.coded_width * h->cfg.coded_height, nc = ny / 4;
    size_t mbs = (size_t)(h->cfg.coded_width / 16) * (h->cfg.coded_height / 16);
    bool ok = get_i32(env, p, "type", &pic.type, 0) && get_i32(env, p, "outSlot", &pic.out_slot, -1) &&
              get_i32(env, p, "refFwdSlot", &pic.ref_fwd_slot, -1) && get_i32(env, p, "refBwdSlot", &pic.ref_bwd_slot, -1) &&
              get_array(env, p, "coefY", napi_int16_array, ny, (const void**)&pic.coef_y) &&
              get_array(env, p, "coefCb", napi_int16_array, nc, (const void**)&pic.coef_cb) &&
              get_array(env, p, "coefCr", napi_int16_array, nc, (const void**)&pic.coef_cr) &&
              get_array(env, p, "coefA", napi_int16_array, ny, (const void**)&pic.coef_a) &&
              get_array(env, p, "qscale", napi_uint8_array, mbs, (const void**)&pic.qscale) &&
              get_array(env, p, "intra", napi_uint8_array, mbs, (const void**)&pic.intra) &&
              get_array(env, p, "repadd", napi_uint8_array, mbs, (const void**)&pic.repadd) &&
              get_array(env, p, "mvFwd", napi_int16_array, mbs * 2, (const void**)&pic.mv_fwd) &&
              get_array(env, p, "mvBwd", napi_int16_array, mbs * 2, (const void**)&pic.mv_bwd) &&
              get_array(env, p, "mbDir", napi_uint8_array, mbs, (const void**)&pic.mb_dir);
    if (!ok) {
        napi_throw_type_error(env, nullptr, "submitPicture: a boundary tensor has the wrong type or is too short");
        return nullptr;
    }
    int rc = leon_submit_picture(h->d, &pic);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

// = IDCT_GL with the coefficients as sparse group lists (include/leon_vlc.h): what
// leon_vlc_napi's nextPicture() returns goes in unchanged
napi_value SubmitSparse(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    if (argc < 1) {
        napi_throw_type_error(env, nullptr, "submitSparse(picture)");
        return nullptr;
    }
    napi_value p = argv[0];
    leon_sparse_picture pic;
    memset(&pic, 0, sizeof pic);
    const int mbw = h->cfg.coded_width / 16, mbh = h->cfg.coded_height / 16;
    const size_t mbs = (size_t)mbw * mbh;
    const size_t n_groups = (size_t)2 * mbh * ((2 * mbw + 7) / 8) * (h->cfg.alpha ? 2 : 1) + (size_t)2 * mbh * ((mbw + 7) / 8);
    int32_t n_entries = 0;
    bool ok = get_i32(env, p, "type", &pic.type, 0) && get_i32(env, p, "outSlot", &pic.out_slot, -1) &&
              get_i32(env, p, "refFwdSlot", &pic.ref_fwd_slot, -1) && get_i32(env, p, "refBwdSlot", &pic.ref_bwd_slot, -1) &&
              get_i32(env, p, "nEntries", &n_entries, 0) && n_entries >= 0 &&
              get_array(env, p, "grpOff", napi_uint32_array, n_groups + 1, (const void**)&pic.grp_off) &&
              get_array(env, p, "entries", napi_uint32_array, (size_t)n_entries, (const void**)&pic.entries) &&
              get_array(env, p, "qscale", napi_uint8_array, mbs, (const void**)&pic.qscale) &&
              get_array(env, p, "intra", napi_uint8_array, mbs, (const void**)&pic.intra) &&
              get_array(env, p, "repadd", napi_uint8_array, mbs, (const void**)&pic.repadd) &&
              get_array(env, p, "mvFwd", napi_int16_array, mbs * 2, (const void**)&pic.mv_fwd) &&
              get_array(env, p, "mvBwd", napi_int16_array, mbs * 2, (const void**)&pic.mv_bwd) &&
              get_array(env, p, "mbDir", napi_uint8_array, mbs, (const void**)&pic.mb_dir);
    if (!ok) {
        napi_throw_type_error(env, nullptr, "submitSparse: a boundary tensor has the wrong type or is too short");
        return nullptr;
    }
    pic.n_entries = (uint32_t)n_entries;
    int rc = leon_submit_sparse(h->d, &pic, 1, LEON_MEM_HOST);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value make_u8(napi_env env, size_t bytes, uint8_t** data)
{
    napi_value ab, ta;
    if (napi_create_arraybuffer(env, bytes, (void**)data, &ab) != napi_ok) return nullptr;
    if (napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

napi_value ConvertRGBA(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int32_t slot = -1, flavour = 0;
    if (argc < 1 || napi_get_value_int32(env, argv[0], &slot) != napi_ok) {
        napi_throw_type_error(env, nullptr, "convertRGBA(slot[, flavour])");
        return nullptr;
    }
    if (argc > 1) napi_get_value_int32(env, argv[1], &flavour);
    uint8_t* data = nullptr;
    napi_value ta = make_u8(env, (size_t)h->cfg.frame_width * h->cfg.frame_height * 4, &data);
    if (!ta) return nullptr;
    int rc = leon_convert_rgba(h->d, slot, data, LEON_MEM_HOST, flavour);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

napi_value ReadPlanes(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    Handle* h = unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int32_t slot = -1;
    if (argc < 1 || napi_get_value_int32(env, argv[0], &slot) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readPlanes(slot)");
        return nullptr;
    }
    size_t ny = (size_t)h->cfg.coded_width * h->cfg.coded_height, nc = ny / 4;
    uint8_t *y, *cb, *cr;
    napi_value ty = make_u8(env, ny, &y), tcb = make_u8(env, nc, &cb), tcr = make_u8(env, nc, &cr);
    if (!ty || !tcb || !tcr) return nullptr;
    int rc = leon_read_planes(h->d, slot, y, cb, cr);
    if (rc != LEON_OK) return throw_leon(env, rc);
    napi_value o;
    NAPI_OK(napi_create_object(env, &o));
    napi_set_named_property(env, o, "y", ty);
    napi_set_named_property(env, o, "cb", tcb);
    napi_set_named_property(env, o, "cr", tcr);
    if (h->cfg.alpha) {                       // yuva: the fourth plane of the slot
        uint8_t* a;
        napi_value ta = make_u8(env, ny, &a);
        if (!ta) return nullptr;
        rc = leon_read_alpha_plane(h->d, slot, a);
        if (rc != LEON_OK) return throw_leon(env, rc);
        napi_set_named_property(env, o, "a", ta);
    }
    return o;
}

napi_value Sync(napi_env env, napi_callback_info info)
{
    size_t argc = 0;
    Handle* h = unwrap(env, info, &argc, nullptr);
    if (!h) return nullptr;
    int rc = leon_sync(h->d);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value Destroy(napi_env env, napi_callback_info info)
{
    size_t argc = 0;
    napi_value self;
    napi_get_cb_info(env, info, &argc, nullptr, &self, nullptr);
    Handle* h = nullptr;
    if (napi_unwrap(env, self, (void**)&h) == napi_ok && h && h->d) {
        leon_destroy(h->d);
        h->d = nullptr;
    }
    return nullptr;
}

napi_value Create(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    if (argc < 1) {
        napi_throw_type_error(env, nullptr, "create({codedWidth, codedHeight, ...})");
        return nullptr;
    }
    Handle* h = new Handle();
    memset(&h->cfg, 0, sizeof h->cfg);
    h->d = nullptr;
    bool ok = get_i32(env, argv[0], "codedWidth", &h->cfg.coded_width, 0) && get_i32(env, argv[0], "codedHeight", &h->cfg.coded_height, 0) &&
              get_i32(env, argv[0], "frameWidth", &h->cfg.frame_width, 0) && get_i32(env, argv[0], "frameHeight", &h->cfg.frame_height, 0) &&
              get_i32(env, argv[0], "nSlots", &h->cfg.n_slots, 13) && get_i32(env, argv[0], "deviceId", &h->cfg.device_id, 0) &&
              get_i32(env, argv[0], "alpha", &h->cfg.alpha, 0);
    if (!ok) {
        delete h;
        napi_throw_type_error(env, nullptr, "create: integer fields expected");
        return nullptr;
    }
    if (!h->cfg.frame_width) h->cfg.frame_width = h->cfg.coded_width;
    if (!h->cfg.frame_height) h->cfg.frame_height = h->cfg.coded_height;
    int rc = leon_create(&h->cfg, &h->d);
    if (rc != LEON_OK) {
        delete h;
        return throw_leon(env, rc);
    }
    napi_value obj;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_wrap(env, obj, h, finalize, nullptr, nullptr));
    const struct { const char* name; napi_callback fn; } methods[] = {
        {"setQuantMatrices", SetQuantMatrices}, {"acquireSlot", AcquireSlot}, {"releaseSlot", ReleaseSlot},
        {"freeDecodedSlots", FreeDecodedSlots}, {"submitPicture", SubmitPicture}, {"submitSparse", SubmitSparse}, {"convertRGBA", ConvertRGBA},
        {"readPlanes", ReadPlanes}, {"sync", Sync}, {"destroy", Destroy}};
    for (auto& m : methods) {
        napi_value fn;
        NAPI_OK(napi_create_function(env, m.name, NAPI_AUTO_LENGTH, m.fn, nullptr, &fn));
        NAPI_OK(napi_set_named_property(env, obj, m.name, fn));
    }
    return obj;
}

// ---- the native pipeline (include/leon_pipeline.h) -----------------------------------------------------
//   const p = leon.createPipeline(streamBuffer, {deviceId, parserThreads, gopsPerWindow, windowsInFlight,
//                                                maxGopPictures, loop, shardIndex, shardCount}, (window, frames, status) => {...});
//   shardIndex / shardCount: this pipeline decodes the key-map GOPs g = shardIndex (mod shardCount) on deviceId --
//   one Node process per GPU is the JavaScript host's form of the frame-parallel partition.
//   frames: [{gop, displayIndex, type, ts}] in display order; window < 0 = 'ended' (decoders/jsv.js:437).  An open GOP
//   (closed_gop = 0) without its predecessor -- first of a run, seek target, broken_link -- comes without its leading B
//   pictures: its first displayIndex is its I picture's (include/leon_pipeline.h "Open GOPs"; no option).
//   p.readFrame(window, i) -> Uint8Array (copies one frame to the host: tests, thumbnails),
//   p.readPlanes(window, i) -> {y, cb, cr[, a]} packed Uint8Arrays (options.output 2 / 3: the frames' YCbCr planes),
//   p.releaseWindow(window), p.stats(), p.info(), p.destroy().
//   p.seek(seconds, exact) -> firstWindow (leon_pipeline_seek): windows the notify thread queued for the old position and
//   its 'ended' reach no JavaScript callback -- they are released here; a seek after 'ended' starts a new run.
// The callback arrives on the JavaScript thread through a napi_threadsafe_function: the pipeline's notify
// thread waits on the HIP event, nothing ever blocks the event loop (SURVEY.md 8b "Threading").
struct PipeMsg {
    int64_t window;
    int64_t last_window;        // 'ended': the last window delivered before it (which position it ends)
    int32_t status;
    std::vector<leon_pipeline_frame> frames;
};

struct PipeHandle {
    leon_pipeline* p = nullptr;
    napi_threadsafe_function tsfn = nullptr;
    napi_ref stream_ref = nullptr;          // keeps the stream's Buffer alive: the pipeline reads it in place
    std::mutex mu;
    std::map<int64_t, std::vector<leon_pipeline_frame>> out;   // delivered, not yet released
    leon_pipeline_info info{};
    leon_pipeline_tensor_geometry tensor_geom{};      // all 0 without tensor output
    leon_pipeline_tensor_shape tensor_shape{};        // the same
    leon_pipeline_tensor_canvas tensor_canvas{};      // the same
    int64_t last_window = -1;               // notify thread, under mu
    int64_t floor = 0;                      // JavaScript thread: the first window of the latest seek
    bool seeked = false;
};

void pipe_native_cb(void* user, int64_t window, const leon_pipeline_frame* frames, int32_t n, int32_t status)
{
    PipeHandle* h = (PipeHandle*)user;
    PipeMsg* m = new PipeMsg();
    m->window = window;
    m->status = status;
    if (frames && n > 0) m->frames.assign(frames, frames + n);
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (window >= 0) {
            h->out[window] = m->frames;
            h->last_window = std::max(h->last_window, window);
        }
        m->last_window = h->last_window;
    }
    napi_call_threadsafe_function(h->tsfn, m, napi_tsfn_blocking);
}

void pipe_call_js(napi_env env, napi_value js_cb, void* ctx, void* data)
{
    PipeHandle* h = (PipeHandle*)ctx;
    PipeMsg* m = (PipeMsg*)data;
    // queued for a position seeked away from (the seek ran on this thread in between): a window is given back, an 'ended'
    // dropped.  (Window ids count on across seeks; the windows of the new position start at `floor`.)
    const bool stale = h->seeked && (m->window >= 0 ? m->window < h->floor : m->last_window < h->floor);
    if (stale) {
        if (m->window >= 0 && h->p) {
            {
                std::lock_guard<std::mutex> lk(h->mu);
                h->out.erase(m->window);
            }
            leon_pipeline_release_window(h->p, m->window);
        }
        delete m;
        return;
    }
    // 'ended': nothing more will come unless a seek restarts the run -- let the event loop end.  Before the call: a seek
    // from the handler refs it again (PipeSeek).
    if (m->window < 0 && h->tsfn && env) napi_unref_threadsafe_function(env, h->tsfn);
    if (env && js_cb) {
        napi_value argv[3], undef, ret;
        napi_create_int64(env, m->window, &argv[0]);
        napi_create_array_with_length(env, m->frames.size(), &argv[1]);
        for (size_t i = 0; i < m->frames.size(); i++) {
            napi_value o, v;
            napi_create_object(env, &o);
            napi_create_double(env, (double)m->frames[i].gop, &v); napi_set_named_property(env, o, "gop", v);
            napi_create_int32(env, m->frames[i].display_index, &v); napi_set_named_property(env, o, "displayIndex", v);
            napi_create_int32(env, m->frames[i].type, &v); napi_set_named_property(env, o, "type", v);
            napi_create_double(env, m->frames[i].ts_ms, &v); napi_set_named_property(env, o, "ts", v);
            napi_set_element(env, argv[1], (uint32_t)i, o);
        }
        napi_create_int32(env, m->status, &argv[2]);
        napi_get_undefined(env, &undef);
        napi_call_function(env, undef, js_cb, 3, argv, &ret);
    }
    delete m;
}

void pipe_finalize(napi_env env, void* data, void*)
{
    PipeHandle* h = (PipeHandle*)data;
    if (h->p) leon_pipeline_destroy(h->p);
    if (h->tsfn) napi_release_threadsafe_function(h->tsfn, napi_tsfn_abort);
    if (h->stream_ref) napi_delete_reference(env, h->stream_ref);
    delete h;
}

PipeHandle* pipe_unwrap(napi_env env, napi_callback_info info, size_t* argc, napi_value* argv)
{
    napi_value self;
    if (napi_get_cb_info(env, info, argc, argv, &self, nullptr) != napi_ok) return nullptr;
    PipeHandle* h = nullptr;
    if (napi_unwrap(env, self, (void**)&h) != napi_ok || !h || !h->p) {
        napi_throw_error(env, nullptr, "pipeline is destroyed");
        return nullptr;
    }
    return h;
}

napi_value PipeRelease(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    if (argc < 1 || napi_get_value_int64(env, argv[0], &w) != napi_ok) {
        napi_throw_type_error(env, nullptr, "releaseWindow(window)");
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(h->mu);
        h->out.erase(w);
    }
    int rc = leon_pipeline_release_window(h->p, w);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value PipeReadFrame(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readFrame(window, index)");
        return nullptr;
    }
    leon_pipeline_frame f{};
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto it = h->out.find(w);
        if (it == h->out.end() || i < 0 || (size_t)i >= it->second.size()) {
            napi_throw_range_error(env, nullptr, "readFrame: no such frame (window released?)");
            return nullptr;
        }
        f = it->second[(size_t)i];
    }
    const size_t bytes = (size_t)h->info.frame_width * h->info.frame_height * 4;
    napi_value ab, ta;
    void* data = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, bytes, &data, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta));
    int rc = leon_pipeline_read_frame(h->p, &f, (uint8_t*)data);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

// p.readPlanes(window, i) -> {y, cb, cr[, a]}: packed Uint8Arrays of one frame's YCbCr planes (output 'ycbcr' / 'both')
napi_value PipeReadPlanes(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readPlanes(window, index)");
        return nullptr;
    }
    leon_pipeline_frame f{};
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto it = h->out.find(w);
        if (it == h->out.end() || i < 0 || (size_t)i >= it->second.size()) {
            napi_throw_range_error(env, nullptr, "readPlanes: no such frame (window released?)");
            return nullptr;
        }
        f = it->second[(size_t)i];
    }
    const size_t ybytes = (size_t)h->info.frame_width * h->info.frame_height, cbytes = (size_t)h->info.chroma_width * h->info.chroma_height;
    const char* names[4] = {"y", "cb", "cr", "a"};
    const size_t sizes[4] = {ybytes, cbytes, cbytes, ybytes};
    void* data[4] = {nullptr, nullptr, nullptr, nullptr};
    napi_value o, ab, ta;
    NAPI_OK(napi_create_object(env, &o));
    for (int k = 0; k < (f.a ? 4 : 3); k++) {
        NAPI_OK(napi_create_arraybuffer(env, sizes[k], &data[k], &ab));
        NAPI_OK(napi_create_typedarray(env, napi_uint8_array, sizes[k], ab, 0, &ta));
        NAPI_OK(napi_set_named_property(env, o, names[k], ta));
    }
    int rc = leon_pipeline_read_frame_planes(h->p, &f, (uint8_t*)data[0], (uint8_t*)data[1], (uint8_t*)data[2], (uint8_t*)data[3]);
    return rc == LEON_OK ? o : throw_leon(env, rc);
}

// p.readTensor(window, i) -> Uint16Array (fp16 / bf16 bit patterns), Float32Array or Uint8Array (tensorDtype 'uint8'),
// [3][tensorHeight][tensorWidth] packed (the frame's size, or opts.tensorSize; [tensorHeight][tensorWidth][3] with tensorLayout 'hwc'):
// one frame's tensor (output 'tensor' ...)
napi_value PipeReadTensor(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readTensor(window, index)");
        return nullptr;
    }
    if (!h->info.tensor_dtype) {
        napi_throw_error(env, nullptr, "readTensor: the pipeline has no tensor output (opts.output)");
        return nullptr;
    }
    const size_t bytes = (size_t)h->info.tensor_frame_bytes, eb = (size_t)h->info.tensor_element_bytes;
    napi_value ab, ta;
    void* data = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, bytes, &data, &ab));
    NAPI_OK(napi_create_typedarray(env, eb == 4 ? napi_float32_array : (eb == 1 ? napi_uint8_array : napi_uint16_array), bytes / eb, ab, 0, &ta));
    int rc = leon_pipeline_read_tensor(h->p, w, i, data);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

// p.readMotion(window, i) -> {mv: Int16Array [mbs][4], info: Uint8Array [mbs], summary: Uint32Array [8], fwdGop, fwdDisplay, bwdDisplay,
// mbWidth, mbHeight}: one frame's motion record (opts.motion; include/leon_pipeline.h LEON_PIPELINE_OUTPUT_MOTION), copied to the host
napi_value PipeReadMotion(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readMotion(window, index)");
        return nullptr;
    }
    struct leon_pipeline_motion_layout lay;
    int rc = leon_pipeline_get_motion_layout(h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    size_t n = 0;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto it = h->out.find(w);
        if (it != h->out.end()) n = it->second.size();
    }
    if (i < 0 || (size_t)i >= n) {
        napi_throw_error(env, nullptr, "readMotion: no such frame in a delivered window");
        return nullptr;
    }
    std::vector<leon_pipeline_motion_frame> refs(n);
    if ((rc = leon_pipeline_window_motion(h->p, w, refs.data(), (int32_t)n)) != LEON_OK) return throw_leon(env, rc);
    napi_value o, ab[3], ta[3];
    void* data[3] = {nullptr, nullptr, nullptr};
    const size_t mbs = (size_t)lay.mbs;
    NAPI_OK(napi_create_object(env, &o));
    NAPI_OK(napi_create_arraybuffer(env, mbs * 8, &data[0], &ab[0]));
    NAPI_OK(napi_create_typedarray(env, napi_int16_array, mbs * 4, ab[0], 0, &ta[0]));
    NAPI_OK(napi_create_arraybuffer(env, mbs, &data[1], &ab[1]));
    NAPI_OK(napi_create_typedarray(env, napi_uint8_array, mbs, ab[1], 0, &ta[1]));
    NAPI_OK(napi_create_arraybuffer(env, 32, &data[2], &ab[2]));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, 8, ab[2], 0, &ta[2]));
    if ((rc = leon_pipeline_read_motion(h->p, w, i, (int16_t*)data[0], (uint8_t*)data[1], (uint32_t*)data[2])) != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_set_named_property(env, o, "mv", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "info", ta[1]));
    NAPI_OK(napi_set_named_property(env, o, "summary", ta[2]));
    const leon_pipeline_motion_frame& m = refs[(size_t)i];
    const struct { const char* name; double v; } nums[] = {{"fwdGop", (double)m.fwd_gop}, {"fwdDisplay", (double)m.fwd_display}, {"bwdDisplay", (double)m.bwd_display},
                                                           {"mbWidth", (double)lay.mb_width}, {"mbHeight", (double)lay.mb_height}};
    for (const auto& kv : nums) {
        napi_value v;
        NAPI_OK(napi_create_double(env, kv.v, &v));
        NAPI_OK(napi_set_named_property(env, o, kv.name, v));
    }
    return o;
}

// p.readActivity(window, i) -> {cells: Uint8Array [mbs][8] (per macroblock uint16 ac_count, ac_mag, dc_mag little endian, uint8 blocks, qscale),
// summary: Uint32Array [8], mbWidth, mbHeight}: one frame's activity record (opts.activity; include/leon_pipeline.h
// LEON_PIPELINE_OUTPUT_ACTIVITY), copied to the host; js/leon_pipeline.js splits the cells into typed arrays
napi_value PipeReadActivity(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readActivity(window, index)");
        return nullptr;
    }
    struct leon_pipeline_activity_layout lay;
    int rc = leon_pipeline_get_activity_layout(h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    napi_value o, ab[2], ta[2];
    void* data[2] = {nullptr, nullptr};
    const size_t mbs = (size_t)lay.mbs;
    NAPI_OK(napi_create_object(env, &o));
    NAPI_OK(napi_create_arraybuffer(env, mbs * 8, &data[0], &ab[0]));
    NAPI_OK(napi_create_typedarray(env, napi_uint8_array, mbs * 8, ab[0], 0, &ta[0]));
    NAPI_OK(napi_create_arraybuffer(env, 32, &data[1], &ab[1]));
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, 8, ab[1], 0, &ta[1]));
    if ((rc = leon_pipeline_read_activity(h->p, w, i, data[0], (uint32_t*)data[1])) != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_set_named_property(env, o, "cells", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "summary", ta[1]));
    const struct { const char* name; double v; } nums[] = {{"mbWidth", (double)lay.mb_width}, {"mbHeight", (double)lay.mb_height}};
    for (const auto& kv : nums) {
        napi_value v;
        NAPI_OK(napi_create_double(env, kv.v, &v));
        NAPI_OK(napi_set_named_property(env, o, kv.name, v));
    }
    return o;
}

// p.readResidual(window, i) -> {y: Int16Array [codedHeight][codedWidth], cb, cr: Int16Array [codedHeight / 2][codedWidth / 2], codedWidth,
// codedHeight}: one frame's residual record (opts.residual; include/leon_pipeline.h LEON_PIPELINE_OUTPUT_RESIDUAL), copied to the host, packed
napi_value PipeReadResidual(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t i = -1;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_get_value_int32(env, argv[1], &i) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readResidual(window, index)");
        return nullptr;
    }
    struct leon_pipeline_residual_layout lay;
    int rc = leon_pipeline_get_residual_layout(h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    napi_value o, ab[3], ta[3];
    void* data[3] = {nullptr, nullptr, nullptr};
    const size_t luma = (size_t)lay.coded_width * (size_t)lay.coded_height;
    NAPI_OK(napi_create_object(env, &o));
    for (int k = 0; k < 3; k++) {
        const size_t n = k == 0 ? luma : luma / 4;
        NAPI_OK(napi_create_arraybuffer(env, n * 2, &data[k], &ab[k]));
        NAPI_OK(napi_create_typedarray(env, napi_int16_array, n, ab[k], 0, &ta[k]));
    }
    if ((rc = leon_pipeline_read_residual(h->p, w, i, (int16_t*)data[0], (int16_t*)data[1], (int16_t*)data[2])) != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_set_named_property(env, o, "y", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "cb", ta[1]));
    NAPI_OK(napi_set_named_property(env, o, "cr", ta[2]));
    const struct { const char* name; double v; } nums[] = {{"codedWidth", (double)lay.coded_width}, {"codedHeight", (double)lay.coded_height}};
    for (const auto& kv : nums) {
        napi_value v;
        NAPI_OK(napi_create_double(env, kv.v, &v));
        NAPI_OK(napi_set_named_property(env, o, kv.name, v));
    }
    return o;
}

// p.readRegions(window, boxes, outHeight, outWidth, filter) -> Buffer of n * region bytes (3 * outHeight * outWidth elements of the
// pipeline's element type and layout each, packed): leon_pipeline_read_regions.  boxes: an Int32Array of n x [frame index, x, y, width, height].
// Five numbers more -- fit mode, anchor, pad r, g, b (leon_pipeline_regions_fit) -- make it leon_pipeline_read_regions_fit.
napi_value PipeReadRegions(napi_env env, napi_callback_info info)
{
    size_t argc = 10;
    napi_value argv[10];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t oh = 0, ow = 0, filter = 0;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void* boxes = nullptr;
    napi_value ab;
    bool is_ta = false;
    if (argc < 5 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[1], &tt, &len, &boxes, &ab, &off) != napi_ok || tt != napi_int32_array || len % 5 != 0 ||
        napi_get_value_int32(env, argv[2], &oh) != napi_ok || napi_get_value_int32(env, argv[3], &ow) != napi_ok || napi_get_value_int32(env, argv[4], &filter) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readRegions(window, Int32Array of [frame, x, y, width, height] per region, outHeight, outWidth, filter)");
        return nullptr;
    }
    const bool fitted = argc > 5;
    leon_pipeline_regions_fit fit{};
    if (fitted && (argc < 10 || napi_get_value_int32(env, argv[5], &fit.mode) != napi_ok || napi_get_value_int32(env, argv[6], &fit.anchor) != napi_ok ||
                   napi_get_value_int32(env, argv[7], &fit.pad[0]) != napi_ok || napi_get_value_int32(env, argv[8], &fit.pad[1]) != napi_ok ||
                   napi_get_value_int32(env, argv[9], &fit.pad[2]) != napi_ok)) {
        napi_throw_type_error(env, nullptr, "readRegions(..., filter, fitMode, anchor, padR, padG, padB)");
        return nullptr;
    }
    if (!h->info.tensor_dtype) {
        napi_throw_error(env, nullptr, "readRegions: the pipeline has no tensor output (opts.output)");
        return nullptr;
    }
    const size_t n = len / 5;
    std::vector<leon_pipeline_region> regions(n ? n : 1);
    const int32_t* b = static_cast<const int32_t*>(boxes);
    for (size_t i = 0; i < n; i++) regions[i] = leon_pipeline_region{b[5 * i], b[5 * i + 1], b[5 * i + 2], b[5 * i + 3], b[5 * i + 4], {0, 0, 0}};
    const leon_pipeline_regions_config cfg{ow, oh, filter, {0, 0, 0, 0, 0}};
    // (a size the library refuses allocates nothing here)
    const bool sized = oh >= 1 && oh <= 4096 && ow >= 1 && ow <= 4096 && n >= 1 && n <= 65535;
    const size_t bytes = sized ? n * 3 * (size_t)oh * (size_t)ow * (size_t)h->info.tensor_element_bytes : 0;
    napi_value buf;
    void* data = nullptr;
    NAPI_OK(napi_create_buffer(env, bytes ? bytes : 1, &data, &buf));
    const int32_t count = (int32_t)std::min<size_t>(n, 65536);
    int rc = fitted ? leon_pipeline_read_regions_fit(h->p, w, regions.data(), count, &cfg, &fit, data) : leon_pipeline_read_regions(h->p, w, regions.data(), count, &cfg, data);
    return rc == LEON_OK ? buf : throw_leon(env, rc);
}

// p.readWarpRegions(window, records, outHeight, outWidth, padR, padG, padB) -> Buffer of n * region bytes, packed:
// leon_pipeline_read_warp_regions.  records: an Int32Array of n x [frame index, a00, a01, tx, a10, a11, ty] (Q16).
napi_value PipeReadWarpRegions(napi_env env, napi_callback_info info)
{
    size_t argc = 7;
    napi_value argv[7];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    leon_pipeline_warp_config cfg{};
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void* words = nullptr;
    napi_value ab;
    bool is_ta = false;
    if (argc < 7 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[1], &tt, &len, &words, &ab, &off) != napi_ok || tt != napi_int32_array || len % 7 != 0 ||
        napi_get_value_int32(env, argv[2], &cfg.out_height) != napi_ok || napi_get_value_int32(env, argv[3], &cfg.out_width) != napi_ok ||
        napi_get_value_int32(env, argv[4], &cfg.pad[0]) != napi_ok || napi_get_value_int32(env, argv[5], &cfg.pad[1]) != napi_ok ||
        napi_get_value_int32(env, argv[6], &cfg.pad[2]) != napi_ok) {
        napi_throw_type_error(env, nullptr, "readWarpRegions(window, Int32Array of [frame, a00, a01, tx, a10, a11, ty] per region, outHeight, outWidth, padR, padG, padB)");
        return nullptr;
    }
    if (!h->info.tensor_dtype) {
        napi_throw_error(env, nullptr, "readWarpRegions: the pipeline has no tensor output (opts.output)");
        return nullptr;
    }
    const size_t n = len / 7;
    std::vector<leon_pipeline_warp_region> regions(n ? n : 1);
    const int32_t* b = static_cast<const int32_t*>(words);
    for (size_t i = 0; i < n; i++)
        regions[i] = leon_pipeline_warp_region{b[7 * i], {b[7 * i + 1], b[7 * i + 2], b[7 * i + 3], b[7 * i + 4], b[7 * i + 5], b[7 * i + 6]}, 0};
    const int32_t oh = cfg.out_height, ow = cfg.out_width;
    // (a size the library refuses allocates nothing here)
    const bool sized = oh >= 1 && oh <= 4096 && ow >= 1 && ow <= 4096 && n >= 1 && n <= 65535;
    const size_t bytes = sized ? n * 3 * (size_t)oh * (size_t)ow * (size_t)h->info.tensor_element_bytes : 0;
    napi_value buf;
    void* data = nullptr;
    NAPI_OK(napi_create_buffer(env, bytes ? bytes : 1, &data, &buf));
    const int rc = leon_pipeline_read_warp_regions(h->p, w, regions.data(), (int32_t)std::min<size_t>(n, 65536), &cfg, data);
    return rc == LEON_OK ? buf : throw_leon(env, rc);
}

// p.carryRegions(window, records) -> {out: Int32Array [n][8] (leon_pipeline_region records: frame = target, the moved box, three zeros),
// votes: Int32Array [n][4] (A, I, dh, dv), status: Int32Array [n] (LEON_REGION_*; not 0: the record's words of out and votes are 0)}:
// leon_pipeline_carry_regions (opts.motion).  records: an Int32Array of n x [frame index, x, y, width, height, target frame index].
napi_value PipeCarryRegions(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void* words = nullptr;
    napi_value ab;
    bool is_ta = false;
    if (argc < 2 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[1], &tt, &len, &words, &ab, &off) != napi_ok || tt != napi_int32_array || len % 6 != 0) {
        napi_throw_type_error(env, nullptr, "carryRegions(window, Int32Array of [frame, x, y, width, height, target] per record)");
        return nullptr;
    }
    const size_t n = len / 6, m = n >= 1 && n <= 65535 ? n : 1;          // (a count the library refuses allocates nothing to speak of here)
    std::vector<leon_pipeline_carry_region> regions(m);
    const int32_t* b = static_cast<const int32_t*>(words);
    for (size_t i = 0; i < n && i < m; i++)
        regions[i] = leon_pipeline_carry_region{b[6 * i], b[6 * i + 1], b[6 * i + 2], b[6 * i + 3], b[6 * i + 4], b[6 * i + 5], {0, 0}};
    napi_value o, abs[3], ta[3];
    void* data[3] = {nullptr, nullptr, nullptr};
    const size_t per[3] = {8, 4, 1};
    NAPI_OK(napi_create_object(env, &o));
    for (int k = 0; k < 3; k++) {          // (a new ArrayBuffer is zero-filled: what a refused record keeps)
        NAPI_OK(napi_create_arraybuffer(env, m * per[k] * 4, &data[k], &abs[k]));
        NAPI_OK(napi_create_typedarray(env, napi_int32_array, m * per[k], abs[k], 0, &ta[k]));
    }
    const int rc = leon_pipeline_carry_regions(h->p, w, regions.data(), (int32_t)std::min<size_t>(n, 65536), static_cast<leon_pipeline_region*>(data[0]),
                                               static_cast<int32_t*>(data[1]), static_cast<int32_t*>(data[2]));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_set_named_property(env, o, "out", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "votes", ta[1]));
    NAPI_OK(napi_set_named_property(env, o, "status", ta[2]));
    return o;
}

// p.gaugeRegions(window, regions, sources) -> {stats: Float64Array [n][16] (every word is below 2^53, so a double holds it exactly),
// status: Int32Array [n] (LEON_REGION_*; not 0: the record's words of stats are 0)}: leon_pipeline_gauge_regions (opts.motion and / or
// opts.activity).  regions: an Int32Array of n x [frame index, x, y, width, height]; sources: LEON_GAUGE_* bits.
napi_value PipeGaugeRegions(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    int32_t sources = 0;
    napi_typedarray_type tt;
    size_t len = 0, off = 0;
    void* words = nullptr;
    napi_value ab;
    bool is_ta = false;
    if (argc < 3 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, argv[1], &tt, &len, &words, &ab, &off) != napi_ok || tt != napi_int32_array || len % 5 != 0 ||
        napi_get_value_int32(env, argv[2], &sources) != napi_ok) {
        napi_throw_type_error(env, nullptr, "gaugeRegions(window, Int32Array of [frame, x, y, width, height] per record, sources)");
        return nullptr;
    }
    const size_t n = len / 5, m = n >= 1 && n <= 65535 ? n : 1;          // (a count the library refuses allocates nothing to speak of here)
    std::vector<leon_pipeline_region> regions(m);
    const int32_t* b = static_cast<const int32_t*>(words);
    for (size_t i = 0; i < n && i < m; i++) regions[i] = leon_pipeline_region{b[5 * i], b[5 * i + 1], b[5 * i + 2], b[5 * i + 3], b[5 * i + 4], {0, 0, 0}};
    std::vector<int64_t> stats(m * 16, 0);          // (zeros: what a refused record keeps)
    napi_value o, abs[2], ta[2];
    void* data[2] = {nullptr, nullptr};
    NAPI_OK(napi_create_object(env, &o));
    NAPI_OK(napi_create_arraybuffer(env, m * 16 * 8, &data[0], &abs[0]));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, m * 16, abs[0], 0, &ta[0]));
    NAPI_OK(napi_create_arraybuffer(env, m * 4, &data[1], &abs[1]));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, m, abs[1], 0, &ta[1]));
    leon_pipeline_gauge_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.sources = sources;
    const int rc = leon_pipeline_gauge_regions(h->p, w, &cfg, regions.data(), (int32_t)std::min<size_t>(n, 65536), stats.data(), static_cast<int32_t*>(data[1]));
    if (rc != LEON_OK) return throw_leon(env, rc);
    double* d = static_cast<double*>(data[0]);
    for (size_t i = 0; i < m * 16; i++) d[i] = (double)stats[i];
    NAPI_OK(napi_set_named_property(env, o, "stats", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "status", ta[1]));
    return o;
}

// p.proposeRegions(window, frames, config) -> {regions: Int32Array [n][K][8], count: Int32Array [n], info: Int32Array [n][K][2],
// status: Int32Array [n] (LEON_REGION_*; not 0: the request's rows and count are 0)}: leon_pipeline_propose_regions (opts.motion and / or
// opts.activity).  frames: an Int32Array of n window frame indices; config: an Int32Array of the 8 words of leon_pipeline_propose_config.
napi_value PipeProposeRegions(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    napi_typedarray_type tt[2];
    size_t len[2] = {0, 0}, off = 0;
    void* words[2] = {nullptr, nullptr};
    napi_value ab;
    bool is_ta[2] = {false, false};
    if (argc < 3 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_ta[0]) != napi_ok || !is_ta[0] ||
        napi_is_typedarray(env, argv[2], &is_ta[1]) != napi_ok || !is_ta[1] || napi_get_typedarray_info(env, argv[1], &tt[0], &len[0], &words[0], &ab, &off) != napi_ok ||
        napi_get_typedarray_info(env, argv[2], &tt[1], &len[1], &words[1], &ab, &off) != napi_ok || tt[0] != napi_int32_array || tt[1] != napi_int32_array || len[1] != 8) {
        napi_throw_type_error(env, nullptr, "proposeRegions(window, Int32Array of frame indices, Int32Array of the config's 8 words)");
        return nullptr;
    }
    leon_pipeline_propose_config cfg;
    memcpy(&cfg, words[1], sizeof cfg);
    const size_t n = len[0], m = n >= 1 && n <= 65535 ? n : 1;          // (a count or a K the library refuses allocates nothing to speak of here)
    const size_t K = cfg.max_boxes >= 1 && cfg.max_boxes <= 1024 ? (size_t)cfg.max_boxes : 1;
    const size_t elems[4] = {m * K * 8, m, m * K * 2, m};
    const char* names[4] = {"regions", "count", "info", "status"};
    napi_value o, abs[4], ta[4];
    void* data[4] = {nullptr, nullptr, nullptr, nullptr};
    NAPI_OK(napi_create_object(env, &o));
    for (int i = 0; i < 4; i++) {
        NAPI_OK(napi_create_arraybuffer(env, elems[i] * 4, &data[i], &abs[i]));          // (zeros: what a refused request keeps)
        NAPI_OK(napi_create_typedarray(env, napi_int32_array, elems[i], abs[i], 0, &ta[i]));
    }
    const int rc = leon_pipeline_propose_regions(h->p, w, &cfg, static_cast<const int32_t*>(words[0]), (int32_t)std::min<size_t>(n, 65536),
                                                 static_cast<leon_pipeline_region*>(data[0]), static_cast<int32_t*>(data[2]), static_cast<int32_t*>(data[1]),
                                                 static_cast<int32_t*>(data[3]));
    if (rc != LEON_OK) return throw_leon(env, rc);
    for (int i = 0; i < 4; i++) NAPI_OK(napi_set_named_property(env, o, names[i], ta[i]));
    return o;
}

// p.propagateMaps(window, maps, hops, stride, planes, elemBytes, fill) -> {via: Uint8Array [n][mh][mw] (0 fill, 1 forward, 2 backward),
// status: Int32Array [n] (LEON_REGION_*; not 0: the record's slot and via map are left as they were, via zero)}:
// leon_pipeline_propagate_maps (opts.motion).  maps: a Uint8Array over the bytes of [slots][planes][mh][mw], contiguous, WRITTEN IN
// PLACE; hops: an Int32Array of n x [target frame index, dst slot, fwd slot, bwd slot].  The slot pitch is the map's size, so a map
// whose bytes are no multiple of 4 is refused by the library (js/leon_pipeline.js says so).
napi_value PipePropagateMaps(napi_env env, napi_callback_info info)
{
    size_t argc = 7;
    napi_value argv[7];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    int64_t w = -1;
    napi_typedarray_type tm, th;
    size_t mlen = 0, hlen = 0, off = 0;
    void *maps = nullptr, *words = nullptr;
    napi_value ab;
    bool is_m = false, is_h = false;
    int32_t stride = 0, planes = 0, elem = 0;
    uint32_t fill = 0;
    if (argc < 7 || napi_get_value_int64(env, argv[0], &w) != napi_ok || napi_is_typedarray(env, argv[1], &is_m) != napi_ok || !is_m ||
        napi_get_typedarray_info(env, argv[1], &tm, &mlen, &maps, &ab, &off) != napi_ok || tm != napi_uint8_array ||
        napi_is_typedarray(env, argv[2], &is_h) != napi_ok || !is_h || napi_get_typedarray_info(env, argv[2], &th, &hlen, &words, &ab, &off) != napi_ok ||
        th != napi_int32_array || hlen % 4 != 0 || napi_get_value_int32(env, argv[3], &stride) != napi_ok || napi_get_value_int32(env, argv[4], &planes) != napi_ok ||
        napi_get_value_int32(env, argv[5], &elem) != napi_ok || napi_get_value_uint32(env, argv[6], &fill) != napi_ok) {
        napi_throw_type_error(env, nullptr, "propagateMaps(window, Uint8Array maps, Int32Array of [target, dst, fwd, bwd] per hop, stride, planes, elemBytes, fill)");
        return nullptr;
    }
    struct leon_pipeline_propagate_layout lay;
    int rc = leon_pipeline_propagate_layout(h->info.frame_width, h->info.frame_height, stride, planes, elem, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    if (!lay.slot_bytes || mlen % lay.slot_bytes != 0 || mlen / lay.slot_bytes < 1) {
        napi_throw_type_error(env, nullptr, "propagateMaps: maps is not a whole number of maps of planes * mh * mw * elemBytes bytes");
        return nullptr;
    }
    const size_t n = hlen / 4, m = n >= 1 && n <= 65535 ? n : 1;          // (a count the library refuses allocates nothing to speak of here)
    std::vector<leon_pipeline_propagate_hop> hops(m);
    const int32_t* b = static_cast<const int32_t*>(words);
    for (size_t i = 0; i < n && i < m; i++) hops[i] = leon_pipeline_propagate_hop{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3], {0, 0, 0, 0}};
    leon_pipeline_propagate_config cfg{};
    cfg.stride = stride; cfg.planes = planes; cfg.elem_bytes = elem;
    cfg.n_slots = (int32_t)std::min<size_t>(mlen / lay.slot_bytes, 65536);
    cfg.fill = fill;
    cfg.slot_pitch_bytes = lay.slot_bytes; cfg.maps_bytes = mlen;
    napi_value o, abs[2], ta[2];
    void* data[2] = {nullptr, nullptr};
    const size_t cells = (size_t)lay.mh * (size_t)lay.mw;
    NAPI_OK(napi_create_object(env, &o));          // (a new ArrayBuffer is zero-filled: what a refused record keeps)
    NAPI_OK(napi_create_arraybuffer(env, m * cells, &data[0], &abs[0]));
    NAPI_OK(napi_create_typedarray(env, napi_uint8_array, m * cells, abs[0], 0, &ta[0]));
    NAPI_OK(napi_create_arraybuffer(env, m * 4, &data[1], &abs[1]));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, m, abs[1], 0, &ta[1]));
    rc = leon_pipeline_propagate_maps(h->p, w, &cfg, hops.data(), (int32_t)std::min<size_t>(n, 65536), maps, static_cast<uint8_t*>(data[0]), static_cast<int32_t*>(data[1]));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_set_named_property(env, o, "via", ta[0]));
    NAPI_OK(napi_set_named_property(env, o, "status", ta[1]));
    return o;
}

// opts[name] as three floats (an array of numbers); absent: zeros
bool get_f32x3(napi_env env, napi_value opts, const char* name, float* out)
{
    napi_value v, e;
    bool has = false, is_arr = false;
    if (napi_has_named_property(env, opts, name, &has) != napi_ok || !has) return true;
    if (napi_get_named_property(env, opts, name, &v) != napi_ok) return false;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) == napi_ok && (t == napi_undefined || t == napi_null)) return true;
    uint32_t n = 0;
    if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, v, &n) != napi_ok || n != 3) return false;
    for (uint32_t k = 0; k < 3; k++) {
        double d = 0;
        if (napi_get_element(env, v, k, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return false;
        out[k] = (float)d;
    }
    return true;
}

napi_value PipeStats(napi_env env, napi_callback_info info)
{
    size_t argc = 0;
    PipeHandle* h = pipe_unwrap(env, info, &argc, nullptr);
    if (!h) return nullptr;
    leon_pipeline_stats s{};
    leon_pipeline_get_stats(h->p, &s);
    napi_value o, v;
    NAPI_OK(napi_create_object(env, &o));
    const struct { const char* k; double val; } kv[] = {
        {"pictures", (double)s.pictures}, {"gops", (double)s.gops}, {"windows", (double)s.windows}, {"streamBytes", (double)s.stream_bytes},
        {"seconds", s.seconds}, {"parseSecondsSum", s.parse_seconds_sum}, {"uploadBytes", s.upload_bytes}, {"entries", (double)s.entries},
        {"frameWidth", (double)h->info.frame_width}, {"frameHeight", (double)h->info.frame_height},
        {"codedWidth", (double)h->info.coded_width}, {"codedHeight", (double)h->info.coded_height},
        {"pictureRate", h->info.picture_rate}, {"keyMapGops", (double)h->info.gops}, {"shardGops", (double)h->info.shard_gops}, {"firstGop", (double)h->info.first_gop}, {"duration", h->info.duration}, {"parserThreads", (double)h->info.parser_threads},
        {"gopsPerWindow", (double)h->info.gops_per_window}, {"output", (double)h->info.output},
        {"chromaWidth", (double)h->info.chroma_width}, {"chromaHeight", (double)h->info.chroma_height},
        {"tensorDtype", (double)h->info.tensor_dtype}, {"tensorElementBytes", (double)h->info.tensor_element_bytes},
        {"tensorFrameBytes", (double)h->info.tensor_frame_bytes}, {"tensorFramePitch", (double)h->info.tensor_frame_pitch},
        {"tensorGopPitch", (double)h->info.tensor_gop_pitch}, {"tensorWidth", (double)h->tensor_geom.width}, {"tensorHeight", (double)h->tensor_geom.height},
        // where the resampled image lies in the tensor (leon_pipeline_tensor_canvas; without a canvas: all of it)
        {"tensorImageX", (double)h->tensor_canvas.x}, {"tensorImageY", (double)h->tensor_canvas.y},
        {"tensorImageWidth", (double)h->tensor_canvas.image_width}, {"tensorImageHeight", (double)h->tensor_canvas.image_height}};
    for (auto& e : kv) {
        NAPI_OK(napi_create_double(env, e.val, &v));
        NAPI_OK(napi_set_named_property(env, o, e.k, v));
    }
    if (h->info.tensor_dtype) {          // the tensors' layout by its option name
        NAPI_OK(napi_create_string_utf8(env, h->tensor_shape.layout == LEON_TENSOR_LAYOUT_HWC ? "hwc" : "chw", NAPI_AUTO_LENGTH, &v));
        NAPI_OK(napi_set_named_property(env, o, "tensorLayout", v));
    }
    return o;
}

napi_value PipeDestroy(napi_env env, napi_callback_info info)
{
    napi_value self;
    size_t argc = 0;
    NAPI_OK(napi_get_cb_info(env, info, &argc, nullptr, &self, nullptr));
    PipeHandle* h = nullptr;
    if (napi_unwrap(env, self, (void**)&h) == napi_ok && h && h->p) {
        leon_pipeline_destroy(h->p);       // joins the notify thread: no further callbacks are queued
        h->p = nullptr;
        if (h->tsfn) {
            napi_release_threadsafe_function(h->tsfn, napi_tsfn_abort);
            h->tsfn = nullptr;
        }
    }
    return nullptr;
}

// seek(seconds, exact) -> firstWindow
napi_value PipeSeek(napi_env env, napi_callback_info info)
{
    size_t argc = 2;
    napi_value argv[2];
    PipeHandle* h = pipe_unwrap(env, info, &argc, argv);
    if (!h) return nullptr;
    double t = 0;
    bool exact = false;
    if (argc < 1 || napi_get_value_double(env, argv[0], &t) != napi_ok) { napi_throw_type_error(env, nullptr, "seek(seconds, exact)"); return nullptr; }
    if (argc >= 2) napi_get_value_bool(env, argv[1], &exact);
    int64_t first = -1;
    const int rc = leon_pipeline_seek(h->p, t, exact ? LEON_PIPELINE_SEEK_EXACT : LEON_PIPELINE_SEEK_KEY, &first);
    if (rc != LEON_OK) return throw_leon(env, rc);
    h->floor = first;
    h->seeked = true;
    leon_pipeline_get_info(h->p, &h->info);
    if (h->tsfn) napi_ref_threadsafe_function(env, h->tsfn);      // (unref'd by an 'ended' before): the run goes on
    napi_value v;
    NAPI_OK(napi_create_int64(env, first, &v));
    return v;
}

// feed(validBytes): more of the stream has arrived in the Buffer the pipeline was created on
napi_value PipeFeed(napi_env env, napi_callback_info info)
{
    size_t argc = 1;
    napi_value argv[1], self;
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, &self, nullptr));
    PipeHandle* h = nullptr;
    if (napi_unwrap(env, self, (void**)&h) != napi_ok || !h || !h->p) { napi_throw_error(env, nullptr, "pipeline destroyed"); return nullptr; }
    int64_t v = -1;
    if (argc < 1 || napi_get_value_int64(env, argv[0], &v) != napi_ok || v < 0) { napi_throw_type_error(env, nullptr, "feed(validBytes)"); return nullptr; }
    const int rc = leon_pipeline_feed(h->p, (size_t)v);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value CreatePipeline(napi_env env, napi_callback_info info)
{
    size_t argc = 3;
    napi_value argv[3];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    bool is_buf = false;
    if (argc >= 1) napi_is_buffer(env, argv[0], &is_buf);
    napi_valuetype cbt = napi_undefined;
    if (argc >= 3) napi_typeof(env, argv[2], &cbt);
    if (argc < 3 || !is_buf || cbt != napi_function) {
        napi_throw_type_error(env, nullptr, "createPipeline(streamBuffer, options, callback)");
        return nullptr;
    }
    void* data = nullptr;
    size_t len = 0;
    NAPI_OK(napi_get_buffer_info(env, argv[0], &data, &len));
    leon_pipeline_config cfg;
    memset(&cfg, 0, sizeof cfg);
    bool ok = get_i32(env, argv[1], "deviceId", &cfg.device_id, 0) && get_i32(env, argv[1], "parserThreads", &cfg.parser_threads, 0) &&
              get_i32(env, argv[1], "gopsPerWindow", &cfg.gops_per_window, 0) && get_i32(env, argv[1], "windowsInFlight", &cfg.windows_in_flight, 0) &&
              get_i32(env, argv[1], "maxGopPictures", &cfg.max_gop_pictures, 0) && get_i32(env, argv[1], "loop", &cfg.loop, 0) &&
              get_i32(env, argv[1], "shardIndex", &cfg.shard_index, 0) && get_i32(env, argv[1], "shardCount", &cfg.shard_count, 0) &&
              get_i32(env, argv[1], "gpuParser", &cfg.gpu_parser, 0) && get_i32(env, argv[1], "displayFlavour", &cfg.display_flavour, 0) &&
              get_i32(env, argv[1], "output", &cfg.output, 0);      // LEON_PIPELINE_OUTPUT_* bits (js/leon_pipeline.js maps the names)
    {   // startSeconds: begin at the key-map entry at or before this time
        napi_value v;
        bool has = false;
        if (ok && napi_has_named_property(env, argv[1], "startSeconds", &has) == napi_ok && has &&
            napi_get_named_property(env, argv[1], "startSeconds", &v) == napi_ok) {
            napi_valuetype t;
            napi_typeof(env, v, &t);
            if (t == napi_number) napi_get_value_double(env, v, &cfg.start_seconds);
        }
    }
    // the tensor output's settings (leon_pipeline_tensor_config): tensorDtype LEON_TENSOR_* (js/leon_pipeline.js maps the names),
    // tensorScale / tensorBias [r, g, b]
    leon_pipeline_tensor_config tcfg;
    memset(&tcfg, 0, sizeof tcfg);
    ok = ok && get_i32(env, argv[1], "tensorDtype", &tcfg.dtype, 0);
    if (!ok) {
        napi_throw_type_error(env, nullptr, "createPipeline: integer options expected");
        return nullptr;
    }
    if (!get_f32x3(env, argv[1], "tensorScale", tcfg.scale) || !get_f32x3(env, argv[1], "tensorBias", tcfg.bias)) {
        napi_throw_type_error(env, nullptr, "createPipeline: tensorScale / tensorBias must be arrays of three numbers");
        return nullptr;
    }
    // ... resampled to a model's input size (leon_pipeline_tensor_resize; js/leon_pipeline.js spreads tensorSize / tensorCrop into these and maps tensorFilter's names to LEON_RESIZE_*)
    leon_pipeline_tensor_resize rcfg;
    memset(&rcfg, 0, sizeof rcfg);
    if (!(get_i32(env, argv[1], "tensorOutWidth", &rcfg.out_width, 0) && get_i32(env, argv[1], "tensorOutHeight", &rcfg.out_height, 0) &&
          get_i32(env, argv[1], "tensorCropX", &rcfg.crop_x, 0) && get_i32(env, argv[1], "tensorCropY", &rcfg.crop_y, 0) &&
          get_i32(env, argv[1], "tensorCropWidth", &rcfg.crop_width, 0) && get_i32(env, argv[1], "tensorCropHeight", &rcfg.crop_height, 0) &&
          get_i32(env, argv[1], "tensorFilter", &rcfg.filter, 0))) {
        napi_throw_type_error(env, nullptr, "createPipeline: integer options expected");
        return nullptr;
    }
    // ... and their layout (leon_pipeline_tensor_format; js/leon_pipeline.js maps 'chw' / 'hwc' to LEON_TENSOR_LAYOUT_*)
    leon_pipeline_tensor_format fcfg;
    memset(&fcfg, 0, sizeof fcfg);
    if (!get_i32(env, argv[1], "tensorLayout", &fcfg.layout, 0)) {
        napi_throw_type_error(env, nullptr, "createPipeline: integer options expected");
        return nullptr;
    }
    // ... placed in a padded canvas (leon_pipeline_tensor_canvas; js/leon_pipeline.js spreads tensorCanvas / tensorOrigin / tensorPadValue /
    // tensorLetterbox into these).  tensorLetterbox: out size, canvas and origin from leon_pipeline_letterbox of the crop box, or of the
    // frame (the stream's first sequence header)
    leon_pipeline_tensor_canvas ccfg;
    memset(&ccfg, 0, sizeof ccfg);
    int32_t lb_w = 0, lb_h = 0, origin_set = 0;
    if (!(get_i32(env, argv[1], "tensorCanvasWidth", &ccfg.width, 0) && get_i32(env, argv[1], "tensorCanvasHeight", &ccfg.height, 0) &&
          get_i32(env, argv[1], "tensorOriginX", &ccfg.x, 0) && get_i32(env, argv[1], "tensorOriginY", &ccfg.y, 0) && get_i32(env, argv[1], "tensorOriginSet", &origin_set, 0) &&
          get_i32(env, argv[1], "tensorPadR", &ccfg.pad[0], 0) && get_i32(env, argv[1], "tensorPadG", &ccfg.pad[1], 0) && get_i32(env, argv[1], "tensorPadB", &ccfg.pad[2], 0) &&
          get_i32(env, argv[1], "tensorLetterboxWidth", &lb_w, 0) && get_i32(env, argv[1], "tensorLetterboxHeight", &lb_h, 0))) {
        napi_throw_type_error(env, nullptr, "createPipeline: integer options expected");
        return nullptr;
    }
    if (lb_w || lb_h) {
        if (rcfg.out_width || rcfg.out_height || ccfg.width || ccfg.height || origin_set) {
            napi_throw_type_error(env, nullptr, "createPipeline: tensorLetterbox derives tensorSize, tensorCanvas and tensorOrigin: give it alone");
            return nullptr;
        }
        int32_t sw = rcfg.crop_width, sh = rcfg.crop_height;
        if (!(rcfg.crop_x | rcfg.crop_y | rcfg.crop_width | rcfg.crop_height)) {
            leon_vlc_stream* st = nullptr;
            leon_vlc_info vi;
            if (leon_vlc_open((const uint8_t*)data, len, 1, &st) != LEON_VLC_OK) {
                napi_throw_error(env, nullptr, leon_vlc_last_error());
                return nullptr;
            }
            leon_vlc_get_info(st, &vi);
            leon_vlc_close(st);
            sw = vi.frame_width; sh = vi.frame_height;
        }
        const int lrc = leon_pipeline_letterbox(sw, sh, lb_w, lb_h, &rcfg, &ccfg);
        if (lrc != LEON_OK) return throw_leon(env, lrc);
    } else if ((ccfg.width || ccfg.height) && !origin_set) {          // centred, as leon_pipeline_letterbox centres (what does not fit is create's to refuse)
        ccfg.x = ccfg.width >= rcfg.out_width ? (ccfg.width - rcfg.out_width) / 2 : 0;
        ccfg.y = ccfg.height >= rcfg.out_height ? (ccfg.height - rcfg.out_height) / 2 : 0;
    }
    const bool canvas = (ccfg.width | ccfg.height | ccfg.x | ccfg.y | ccfg.pad[0] | ccfg.pad[1] | ccfg.pad[2]) != 0;
    const bool resized = (rcfg.out_width | rcfg.out_height | rcfg.crop_x | rcfg.crop_y | rcfg.crop_width | rcfg.crop_height | rcfg.filter) != 0;
    const bool tensor = (cfg.output & LEON_PIPELINE_OUTPUT_TENSOR) != 0 || tcfg.dtype != 0 || resized || fcfg.layout != 0 || canvas;
    PipeHandle* h = new PipeHandle();
    napi_value name;
    NAPI_OK(napi_create_string_utf8(env, "leon pipeline frames", NAPI_AUTO_LENGTH, &name));
    if (napi_create_threadsafe_function(env, argv[2], nullptr, name, 0, 1, nullptr, nullptr, h, pipe_call_js, &h->tsfn) != napi_ok) {
        delete h;
        napi_throw_error(env, nullptr, "napi_create_threadsafe_function failed");
        return nullptr;
    }
    napi_create_reference(env, argv[0], 1, &h->stream_ref);
    // validBytes: the stream is still arriving (leon_pipeline_create_partial) -- the loader writes on into the same
    // Buffer and calls feed(validBytesNow), as addBuffer does in the reference (features/bitreader.js:332-430)
    // (a presence test and a double, not an int32 with -1 for "absent": 2 GiB and more of a stream may have arrived)
    bool partial = false;
    double valid = 0;
    {
        napi_value v;
        bool has = false;
        if (napi_has_named_property(env, argv[1], "validBytes", &has) == napi_ok && has && napi_get_named_property(env, argv[1], "validBytes", &v) == napi_ok) {
            napi_valuetype t;
            if (napi_typeof(env, v, &t) == napi_ok && t != napi_undefined && t != napi_null) {
                if (t != napi_number || napi_get_value_double(env, v, &valid) != napi_ok || !(valid >= 0) || valid > (double)len || valid != (double)(size_t)valid) {
                    napi_release_threadsafe_function(h->tsfn, napi_tsfn_abort);
                    napi_delete_reference(env, h->stream_ref);
                    delete h;
                    napi_throw_range_error(env, nullptr, "createPipeline: validBytes must be an integer between 0 and the stream's length");
                    return nullptr;
                }
                partial = true;
            }
        }
    }
    int rc = tensor ? leon_pipeline_create_tensor_canvas(&cfg, &tcfg, resized ? &rcfg : nullptr, fcfg.layout ? &fcfg : nullptr, canvas ? &ccfg : nullptr, (const uint8_t*)data, len, partial ? (size_t)valid : len, pipe_native_cb, h, &h->p)
           : partial ? leon_pipeline_create_partial(&cfg, (const uint8_t*)data, len, (size_t)valid, pipe_native_cb, h, &h->p)
                     : leon_pipeline_create(&cfg, (const uint8_t*)data, len, pipe_native_cb, h, &h->p);
    if (rc != LEON_OK) {
        napi_release_threadsafe_function(h->tsfn, napi_tsfn_abort);
        napi_delete_reference(env, h->stream_ref);
        delete h;
        return throw_leon(env, rc);
    }
    leon_pipeline_get_info(h->p, &h->info);
    if (h->info.tensor_dtype) {
        leon_pipeline_get_tensor_geometry(h->p, &h->tensor_geom);
        leon_pipeline_get_tensor_shape(h->p, &h->tensor_shape);
        leon_pipeline_get_tensor_canvas(h->p, &h->tensor_canvas);
    }
    napi_value obj;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_wrap(env, obj, h, pipe_finalize, nullptr, nullptr));
    const struct { const char* name; napi_callback fn; } methods[] = {
        {"releaseWindow", PipeRelease}, {"readFrame", PipeReadFrame}, {"readPlanes", PipeReadPlanes}, {"readTensor", PipeReadTensor}, {"readMotion", PipeReadMotion}, {"readActivity", PipeReadActivity}, {"readResidual", PipeReadResidual},{"readRegions", PipeReadRegions}, {"readWarpRegions", PipeReadWarpRegions}, {"carryRegions", PipeCarryRegions}, {"gaugeRegions", PipeGaugeRegions}, {"proposeRegions", PipeProposeRegions}, {"propagateMaps", PipePropagateMaps}, {"stats", PipeStats}, {"destroy", PipeDestroy}, {"feed", PipeFeed}, {"seek", PipeSeek}};
    for (auto& m : methods) {
        napi_value fn;
        NAPI_OK(napi_create_function(env, m.name, NAPI_AUTO_LENGTH, m.fn, nullptr, &fn));
        NAPI_OK(napi_set_named_property(env, obj, m.name, fn));
    }
    return obj;
}

// letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight) -> [outWidth, outHeight, x, y]: leon_pipeline_letterbox, no device
napi_value Letterbox(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    int32_t a[4] = {0, 0, 0, 0};
    for (size_t k = 0; k < 4; k++)
        if (argc < 4 || napi_get_value_int32(env, argv[k], &a[k]) != napi_ok) {
            napi_throw_type_error(env, nullptr, "letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight)");
            return nullptr;
        }
    leon_pipeline_tensor_resize rz;
    leon_pipeline_tensor_canvas cv;
    memset(&rz, 0, sizeof rz);
    memset(&cv, 0, sizeof cv);
    const int rc = leon_pipeline_letterbox(a[0], a[1], a[2], a[3], &rz, &cv);
    if (rc != LEON_OK) return throw_leon(env, rc);
    const int32_t r[4] = {rz.out_width, rz.out_height, cv.x, cv.y};
    napi_value arr, v;
    NAPI_OK(napi_create_array_with_length(env, 4, &arr));
    for (uint32_t k = 0; k < 4; k++) {
        NAPI_OK(napi_create_int32(env, r[k], &v));
        NAPI_OK(napi_set_element(env, arr, k, v));
    }
    return arr;
}

napi_value AbiVersion(napi_env env, napi_callback_info)
{
    napi_value v;
    NAPI_OK(napi_create_int32(env, leon_abi_version(), &v));
    return v;
}

napi_value Init(napi_env env, napi_value exports)
{
    if (leon_abi_version() != LEON_ABI_VERSION) {      // the addon was compiled against another include/leon.h than the library it found
        napi_throw_error(env, nullptr, "leon_napi: libleon_hip.so speaks another ABI version than this addon was built for; rebuild both");
        return exports;
    }
    napi_value fn;
    NAPI_OK(napi_create_function(env, "create", NAPI_AUTO_LENGTH, Create, nullptr, &fn));
    NAPI_OK(napi_set_named_property(env, exports, "create", fn));
    NAPI_OK(napi_create_function(env, "createPipeline", NAPI_AUTO_LENGTH, CreatePipeline, nullptr, &fn));
    NAPI_OK(napi_set_named_property(env, exports, "createPipeline", fn));
    NAPI_OK(napi_create_function(env, "letterbox", NAPI_AUTO_LENGTH, Letterbox, nullptr, &fn));
    NAPI_OK(napi_set_named_property(env, exports, "letterbox", fn));
    NAPI_OK(napi_create_function(env, "abiVersion", NAPI_AUTO_LENGTH, AbiVersion, nullptr, &fn));
    NAPI_OK(napi_set_named_property(env, exports, "abiVersion", fn));
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
