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
//
// Every method is the same few steps, and each step is written once below: the argument reader (Args / Call<H>: the receiver's
// handle, typed getters, one usage text thrown as a TypeError), the makers of what goes back (make_array, make_object, set_numbers)
// and, for a pipeline, the delivered-frame lookup, the record-count rule, the region batch's size and the tensor-output requirement.
// DESIGN.md ("The Node addon") adds a method in five lines; tests/node_*_pins*.js pin every refusal's class and text.
#include <node_api.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/leon.h"
#include "../../include/leon_pipeline.h"
#include "../../include/leon_vlc.h"
#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <vector>

namespace {

// the decoder handle of create()
struct Handle {
    leon_decoder* d;
    leon_config cfg;
};

// the pipeline handle of createPipeline() ("the native pipeline" below)
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

// a handle lives until its destroy(); what a method of a dead one throws unless it says otherwise
bool live(const Handle* h) { return h->d != nullptr; }
bool live(const PipeHandle* h) { return h->p != nullptr; }
const char* dead_text(const Handle*) { return "leon: decoder handle is destroyed or invalid"; }
const char* dead_text(const PipeHandle*) { return "pipeline is destroyed"; }

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

// ---- the argument reader ---------------------------------------------------------------------------------
// The arguments of one call.  A getter that does not find what it asks for notes it; bad() then throws the call's usage text as a
// TypeError, once, whichever getter it was.  Arguments that were not passed are undefined, which no getter takes, so "too few
// arguments" needs no test of its own.
struct Args {
    napi_env env;
    const char* usage;
    size_t argc = 10;
    napi_value argv[10] = {};
    napi_value self = nullptr;
    bool failed = false, thrown = false;

    Args(napi_env env, napi_callback_info info, const char* usage) : env(env), usage(usage)
    {
        if (napi_get_cb_info(env, info, &argc, argv, &self, nullptr) != napi_ok) {
            napi_throw_error(env, nullptr, "N-API call failed: napi_get_cb_info");
            thrown = true;
        }
    }
    // true: the call is refused -- something has been thrown already, or a getter failed or `also` holds and the usage text is thrown now
    bool bad(bool also = false)
    {
        if (!thrown && (failed || also)) {
            napi_throw_type_error(env, nullptr, usage);
            thrown = true;
        }
        return thrown;
    }
    bool absent(size_t k) const          // undefined or null
    {
        napi_valuetype t = napi_undefined;
        napi_typeof(env, argv[k], &t);
        return t == napi_undefined || t == napi_null;
    }
    int64_t i64(size_t k) { int64_t v = -1; failed |= napi_get_value_int64(env, argv[k], &v) != napi_ok; return v; }
    int32_t i32(size_t k) { int32_t v = -1; failed |= napi_get_value_int32(env, argv[k], &v) != napi_ok; return v; }
    uint32_t u32(size_t k) { uint32_t v = 0; failed |= napi_get_value_uint32(env, argv[k], &v) != napi_ok; return v; }
    double f64(size_t k) { double v = 0; failed |= napi_get_value_double(env, argv[k], &v) != napi_ok; return v; }
    // (with a default: whatever is no number, or no boolean, counts as not given)
    int32_t i32(size_t k, int32_t dflt) { napi_get_value_int32(env, argv[k], &dflt); return dflt; }
    bool flag(size_t k, bool dflt) { napi_get_value_bool(env, argv[k], &dflt); return dflt; }
    // v as a typed array of `kind`: its storage and its element count
    static bool typed(napi_env env, napi_value v, napi_typedarray_type kind, void** data, size_t* len)
    {
        bool is_ta = false;
        napi_typedarray_type t;
        return napi_is_typedarray(env, v, &is_ta) == napi_ok && is_ta && napi_get_typedarray_info(env, v, &t, len, data, nullptr, nullptr) == napi_ok && t == kind;
    }
    void* array(size_t k, napi_typedarray_type kind, size_t* len)
    {
        void* data = nullptr;
        if (typed(env, argv[k], kind, &data, len)) return data;
        failed = true;
        *len = 0;
        return nullptr;
    }
    // an Int32Array of rows of `words` words: the words and the number of rows
    const int32_t* rows(size_t k, size_t words, size_t* n)
    {
        size_t len = 0;
        const int32_t* b = static_cast<const int32_t*>(array(k, napi_int32_array, &len));
        failed |= len % words != 0;
        *n = len / words;
        return b;
    }
};

// ... of a method: h is the receiver's live handle.  A dead or missing handle throws `dead` before any argument is looked at; with
// dead == nullptr an absent handle is fine and h is nullptr (destroy).
template <class H>
struct Call : Args {
    H* h = nullptr;

    Call(napi_env env, napi_callback_info info, const char* usage, const char* dead = dead_text(static_cast<const H*>(nullptr))) : Args(env, info, usage)
    {
        H* got = nullptr;
        if (thrown) return;
        if (napi_unwrap(env, self, (void**)&got) == napi_ok && got && live(got)) {
            h = got;
        } else if (dead) {
            napi_throw_error(env, nullptr, dead);
            thrown = true;
        }
    }
};

// ---- what goes back ---------------------------------------------------------------------------------------
// a new typed array of n elements of `kind` (a new ArrayBuffer is zero-filled: what a refused record keeps); *data: its storage
napi_status make_array(napi_env env, napi_typedarray_type kind, size_t n, void** data, napi_value* out)
{
    static const size_t bytes[] = {1, 1, 1, 2, 2, 4, 4, 4, 8};          // napi_int8_array .. napi_float64_array
    napi_value ab;
    const napi_status s = napi_create_arraybuffer(env, n * bytes[kind], data, &ab);
    return s != napi_ok ? s : napi_create_typedarray(env, kind, n, ab, 0, out);
}

struct Prop { const char* name; napi_value v; };
struct Num { const char* name; double v; };

napi_status set_props(napi_env env, napi_value o, std::initializer_list<Prop> props)
{
    for (const Prop& p : props) {
        const napi_status s = napi_set_named_property(env, o, p.name, p.v);
        if (s != napi_ok) return s;
    }
    return napi_ok;
}

napi_status make_object(napi_env env, std::initializer_list<Prop> props, napi_value* o)
{
    const napi_status s = napi_create_object(env, o);
    return s != napi_ok ? s : set_props(env, *o, props);
}

napi_status set_numbers(napi_env env, napi_value o, std::initializer_list<Num> nums)
{
    for (const Num& n : nums) {
        napi_value v;
        napi_status s = napi_create_double(env, n.v, &v);
        if (s == napi_ok) s = napi_set_named_property(env, o, n.name, v);
        if (s != napi_ok) return s;
    }
    return napi_ok;
}

struct Method { const char* name; napi_callback fn; };

napi_status define_methods(napi_env env, napi_value obj, std::initializer_list<Method> table)
{
    for (const Method& m : table) {
        napi_value fn;
        napi_status s = napi_create_function(env, m.name, NAPI_AUTO_LENGTH, m.fn, nullptr, &fn);
        if (s == napi_ok) s = napi_set_named_property(env, obj, m.name, fn);
        if (s != napi_ok) return s;
    }
    return napi_ok;
}

// ---- options: properties of an object ------------------------------------------------------------------------
// obj[key]: 1 and the value in *v; 0 absent (no such property, undefined or null); -1 it cannot be read
int get_prop(napi_env env, napi_value obj, const char* key, napi_value* v)
{
    bool has = false;
    napi_valuetype t = napi_undefined;
    if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return 0;
    if (napi_get_named_property(env, obj, key, v) != napi_ok) return -1;
    napi_typeof(env, *v, &t);
    return t == napi_undefined || t == napi_null ? 0 : 1;
}

bool get_i32(napi_env env, napi_value obj, const char* key, int32_t* out, int32_t dflt)
{
    napi_value v;
    *out = dflt;
    const int got = get_prop(env, obj, key, &v);
    return got == 0 || (got > 0 && napi_get_value_int32(env, v, out) == napi_ok);
}

// typed array property -> pointer (nullptr when absent/null); checks the element count
bool get_array(napi_env env, napi_value obj, const char* key, napi_typedarray_type want, size_t min_len, const void** out)
{
    napi_value v;
    void* data = nullptr;
    size_t len = 0;
    *out = nullptr;
    const int got = get_prop(env, obj, key, &v);
    if (got == 0) return true;
    if (got < 0 || !Args::typed(env, v, want, &data, &len) || len < min_len) return false;
    *out = data;
    return true;
}

// opts[name] as a double: 1 a number, in *out; 0 absent (or not to be read); -1 something else
int get_f64(napi_env env, napi_value opts, const char* name, double* out)
{
    napi_value v;
    if (get_prop(env, opts, name, &v) <= 0) return 0;
    return napi_get_value_double(env, v, out) == napi_ok ? 1 : -1;
}

// opts[name] as three floats (an array of numbers); absent: zeros
bool get_f32x3(napi_env env, napi_value opts, const char* name, float* out)
{
    napi_value v, e;
    bool is_arr = false;
    uint32_t n = 0;
    const int got = get_prop(env, opts, name, &v);
    if (got <= 0) return got == 0;
    if (napi_is_array(env, v, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, v, &n) != napi_ok || n != 3) return false;
    for (uint32_t k = 0; k < 3; k++) {
        double d = 0;
        if (napi_get_element(env, v, k, &e) != napi_ok || napi_get_value_double(env, e, &d) != napi_ok) return false;
        out[k] = (float)d;
    }
    return true;
}

struct IntOpt { const char* name; int32_t* field; int32_t dflt; };

// ---- the decoder handle -------------------------------------------------------------------------------------
void finalize(napi_env, void* data, void*)
{
    Handle* h = (Handle*)data;
    if (h->d) leon_destroy(h->d);
    delete h;
}

napi_value SetQuantMatrices(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, "setQuantMatrices: Uint8Array(64) expected");
    if (a.bad()) return nullptr;
    const uint8_t* m[2] = {nullptr, nullptr};
    for (size_t i = 0; i < 2; i++) {
        size_t len = 0;
        if (a.absent(i)) continue;
        m[i] = static_cast<const uint8_t*>(a.array(i, napi_uint8_array, &len));
        if (a.bad(len < 64)) return nullptr;
    }
    int rc = leon_set_quant_matrices(a.h->d, m[0], m[1]);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value AcquireSlot(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, nullptr);
    if (a.bad()) return nullptr;
    int32_t slot = -1;
    int rc = leon_acquire_slot(a.h->d, &slot);
    if (rc != LEON_OK) return throw_leon(env, rc);          // "no free render buffers"
    napi_value v;
    NAPI_OK(napi_create_int32(env, slot, &v));
    return v;
}

napi_value ReleaseSlot(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, "releaseSlot(slot)");
    const int32_t slot = a.i32(0);
    if (a.bad()) return nullptr;
    int rc = leon_release_slot(a.h->d, slot);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value FreeDecodedSlots(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, nullptr);
    if (a.bad()) return nullptr;
    int rc = leon_free_decoded_slots(a.h->d);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value SubmitPicture(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, "submitPicture(picture)");
    if (a.bad(a.argc < 1)) return nullptr;
    Handle* h = a.h;
    napi_value p = a.argv[0];
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
    Call<Handle> a(env, info, "submitSparse(picture)");
    if (a.bad(a.argc < 1)) return nullptr;
    Handle* h = a.h;
    napi_value p = a.argv[0];
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

napi_value ConvertRGBA(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, "convertRGBA(slot[, flavour])");
    const int32_t slot = a.i32(0), flavour = a.i32(1, 0);
    if (a.bad()) return nullptr;
    void* data = nullptr;
    napi_value ta;
    NAPI_OK(make_array(env, napi_uint8_array, (size_t)a.h->cfg.frame_width * a.h->cfg.frame_height * 4, &data, &ta));
    int rc = leon_convert_rgba(a.h->d, slot, data, LEON_MEM_HOST, flavour);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

napi_value ReadPlanes(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, "readPlanes(slot)");
    const int32_t slot = a.i32(0);
    if (a.bad()) return nullptr;
    Handle* h = a.h;
    size_t ny = (size_t)h->cfg.coded_width * h->cfg.coded_height, nc = ny / 4;
    void *y, *cb, *cr;
    napi_value ty, tcb, tcr, o;
    NAPI_OK(make_array(env, napi_uint8_array, ny, &y, &ty));
    NAPI_OK(make_array(env, napi_uint8_array, nc, &cb, &tcb));
    NAPI_OK(make_array(env, napi_uint8_array, nc, &cr, &tcr));
    int rc = leon_read_planes(h->d, slot, (uint8_t*)y, (uint8_t*)cb, (uint8_t*)cr);
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"y", ty}, {"cb", tcb}, {"cr", tcr}}, &o));
    if (h->cfg.alpha) {                       // yuva: the fourth plane of the slot
        void* al;
        napi_value ta;
        NAPI_OK(make_array(env, napi_uint8_array, ny, &al, &ta));
        rc = leon_read_alpha_plane(h->d, slot, (uint8_t*)al);
        if (rc != LEON_OK) return throw_leon(env, rc);
        NAPI_OK(set_props(env, o, {{"a", ta}}));
    }
    return o;
}

napi_value Sync(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, nullptr);
    if (a.bad()) return nullptr;
    int rc = leon_sync(a.h->d);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value Destroy(napi_env env, napi_callback_info info)
{
    Call<Handle> a(env, info, nullptr, nullptr);
    if (a.h) {
        leon_destroy(a.h->d);
        a.h->d = nullptr;
    }
    return nullptr;
}

napi_value Create(napi_env env, napi_callback_info info)
{
    Args a(env, info, "create({codedWidth, codedHeight, ...})");
    if (a.bad(a.argc < 1)) return nullptr;
    Handle* h = new Handle();
    memset(&h->cfg, 0, sizeof h->cfg);
    h->d = nullptr;
    bool ok = true;
    for (const IntOpt& o : {IntOpt{"codedWidth", &h->cfg.coded_width, 0}, {"codedHeight", &h->cfg.coded_height, 0}, {"frameWidth", &h->cfg.frame_width, 0},
                            {"frameHeight", &h->cfg.frame_height, 0}, {"nSlots", &h->cfg.n_slots, 13}, {"deviceId", &h->cfg.device_id, 0}, {"alpha", &h->cfg.alpha, 0}})
        ok = ok && get_i32(env, a.argv[0], o.name, o.field, o.dflt);
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
    NAPI_OK(define_methods(env, obj, {{"setQuantMatrices", SetQuantMatrices}, {"acquireSlot", AcquireSlot}, {"releaseSlot", ReleaseSlot}, {"freeDecodedSlots", FreeDecodedSlots},
                                      {"submitPicture", SubmitPicture}, {"submitSparse", SubmitSparse}, {"convertRGBA", ConvertRGBA}, {"readPlanes", ReadPlanes}, {"sync", Sync},
                                      {"destroy", Destroy}}));
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
            const leon_pipeline_frame& f = m->frames[i];
            napi_value o;
            napi_create_object(env, &o);
            set_numbers(env, o, {{"gop", (double)f.gop}, {"displayIndex", (double)f.display_index}, {"type", (double)f.type}, {"ts", f.ts_ms}});
            napi_set_element(env, argv[1], (uint32_t)i, o);
        }
        napi_create_int32(env, m->status, &argv[2]);
        napi_get_undefined(env, &undef);
        napi_call_function(env, undef, js_cb, 3, argv, &ret);
    }
    delete m;
}

// the end of a PipeHandle that no JavaScript object owns (yet, or any more), in this order: the pipeline, the threadsafe function (a
// live one keeps the event loop alive), the stream's reference, the handle
void pipe_release(napi_env env, PipeHandle* h)
{
    if (h->p) leon_pipeline_destroy(h->p);
    if (h->tsfn) napi_release_threadsafe_function(h->tsfn, napi_tsfn_abort);
    if (h->stream_ref) napi_delete_reference(env, h->stream_ref);
    delete h;
}

void pipe_finalize(napi_env env, void* data, void*) { pipe_release(env, (PipeHandle*)data); }

// owns the handle from `new` until napi_wrap has it: every way out of CreatePipeline before that releases it
struct PipeGuard {
    napi_env env;
    PipeHandle* h;
    ~PipeGuard() { if (h) pipe_release(env, h); }
};

// The delivered window w, under h->mu: its frame count, and its frame i in *f where f is given.  No such window, or no frame i in
// it: `text` is thrown (as a RangeError where `range`) and false comes back.
bool delivered(napi_env env, PipeHandle* h, int64_t w, int32_t i, leon_pipeline_frame* f, size_t* n, bool range, const char* text)
{
    std::lock_guard<std::mutex> lk(h->mu);
    auto it = h->out.find(w);
    *n = it == h->out.end() ? 0 : it->second.size();
    if (i < 0 || (size_t)i >= *n) {
        if (range) napi_throw_range_error(env, nullptr, text);
        else napi_throw_error(env, nullptr, text);
        return false;
    }
    if (f) *f = it->second[(size_t)i];
    return true;
}

// The record-count rule of the calls that take n records.  The library takes 1 .. 65535 (`ok`) and refuses the rest by its own
// text, so that n is handed on: as `count`, clamped to a value an int32 holds and the library still refuses.  `rows` is what the
// result arrays and the record vector are sized for: n where the library takes it, else one row -- a count it refuses allocates
// nothing to speak of here.
struct Count { bool ok; size_t rows; int32_t count; };

Count record_count(size_t n)
{
    const bool ok = n >= 1 && n <= 65535;
    return Count{ok, ok ? n : 1, (int32_t)std::min<size_t>(n, 65536)};
}

// a Buffer for a batch of n regions of oh x ow in the pipeline's element type (one byte where the library refuses the size or
// the count: that allocates nothing here)
napi_status region_batch(napi_env env, const PipeHandle* h, size_t n, int32_t oh, int32_t ow, void** data, napi_value* buf)
{
    const bool sized = oh >= 1 && oh <= 4096 && ow >= 1 && ow <= 4096 && record_count(n).ok;
    const size_t bytes = sized ? n * 3 * (size_t)oh * (size_t)ow * (size_t)h->info.tensor_element_bytes : 0;
    return napi_create_buffer(env, bytes ? bytes : 1, data, buf);
}

bool has_tensor_output(napi_env env, const PipeHandle* h, const char* method)
{
    if (h->info.tensor_dtype) return true;
    char msg[120];
    snprintf(msg, sizeof msg, "%s: the pipeline has no tensor output (opts.output)", method);
    napi_throw_error(env, nullptr, msg);
    return false;
}

napi_value PipeRelease(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "releaseWindow(window)");
    const int64_t w = a.i64(0);
    if (a.bad()) return nullptr;
    {
        std::lock_guard<std::mutex> lk(a.h->mu);
        a.h->out.erase(w);
    }
    int rc = leon_pipeline_release_window(a.h->p, w);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value PipeReadFrame(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readFrame(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad()) return nullptr;
    PipeHandle* h = a.h;
    leon_pipeline_frame f{};
    size_t n;
    if (!delivered(env, h, w, i, &f, &n, true, "readFrame: no such frame (window released?)")) return nullptr;
    napi_value ta;
    void* data = nullptr;
    NAPI_OK(make_array(env, napi_uint8_array, (size_t)h->info.frame_width * h->info.frame_height * 4, &data, &ta));
    int rc = leon_pipeline_read_frame(h->p, &f, (uint8_t*)data);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

// p.readPlanes(window, i) -> {y, cb, cr[, a]}: packed Uint8Arrays of one frame's YCbCr planes (output 'ycbcr' / 'both')
napi_value PipeReadPlanes(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readPlanes(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad()) return nullptr;
    PipeHandle* h = a.h;
    leon_pipeline_frame f{};
    size_t n;
    if (!delivered(env, h, w, i, &f, &n, true, "readPlanes: no such frame (window released?)")) return nullptr;
    const size_t ybytes = (size_t)h->info.frame_width * h->info.frame_height, cbytes = (size_t)h->info.chroma_width * h->info.chroma_height;
    const char* names[4] = {"y", "cb", "cr", "a"};
    const size_t sizes[4] = {ybytes, cbytes, cbytes, ybytes};
    void* data[4] = {nullptr, nullptr, nullptr, nullptr};
    napi_value o, ta;
    NAPI_OK(napi_create_object(env, &o));
    for (int k = 0; k < (f.a ? 4 : 3); k++) {
        NAPI_OK(make_array(env, napi_uint8_array, sizes[k], &data[k], &ta));
        NAPI_OK(set_props(env, o, {{names[k], ta}}));
    }
    int rc = leon_pipeline_read_frame_planes(h->p, &f, (uint8_t*)data[0], (uint8_t*)data[1], (uint8_t*)data[2], (uint8_t*)data[3]);
    return rc == LEON_OK ? o : throw_leon(env, rc);
}

// p.readTensor(window, i) -> Uint16Array (fp16 / bf16 bit patterns), Float32Array or Uint8Array (tensorDtype 'uint8'),
// [3][tensorHeight][tensorWidth] packed (the frame's size, or opts.tensorSize; [tensorHeight][tensorWidth][3] with tensorLayout 'hwc'):
// one frame's tensor (output 'tensor' ...)
napi_value PipeReadTensor(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readTensor(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad() || !has_tensor_output(env, a.h, "readTensor")) return nullptr;
    const size_t bytes = (size_t)a.h->info.tensor_frame_bytes, eb = (size_t)a.h->info.tensor_element_bytes;
    napi_value ta;
    void* data = nullptr;
    NAPI_OK(make_array(env, eb == 4 ? napi_float32_array : (eb == 1 ? napi_uint8_array : napi_uint16_array), bytes / eb, &data, &ta));
    int rc = leon_pipeline_read_tensor(a.h->p, w, i, data);
    return rc == LEON_OK ? ta : throw_leon(env, rc);
}

// p.readMotion(window, i) -> {mv: Int16Array [mbs][4], info: Uint8Array [mbs], summary: Uint32Array [8], fwdGop, fwdDisplay, bwdDisplay,
// mbWidth, mbHeight}: one frame's motion record (opts.motion; include/leon_pipeline.h LEON_PIPELINE_OUTPUT_MOTION), copied to the host
napi_value PipeReadMotion(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readMotion(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad()) return nullptr;
    PipeHandle* h = a.h;
    struct leon_pipeline_motion_layout lay;
    int rc = leon_pipeline_get_motion_layout(h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    size_t n = 0;
    if (!delivered(env, h, w, i, nullptr, &n, false, "readMotion: no such frame in a delivered window")) return nullptr;
    std::vector<leon_pipeline_motion_frame> refs(n);
    if ((rc = leon_pipeline_window_motion(h->p, w, refs.data(), (int32_t)n)) != LEON_OK) return throw_leon(env, rc);
    napi_value o, mv, mbinfo, summary;
    void *mv_data, *info_data, *summary_data;
    const size_t mbs = (size_t)lay.mbs;
    NAPI_OK(make_array(env, napi_int16_array, mbs * 4, &mv_data, &mv));
    NAPI_OK(make_array(env, napi_uint8_array, mbs, &info_data, &mbinfo));
    NAPI_OK(make_array(env, napi_uint32_array, 8, &summary_data, &summary));
    if ((rc = leon_pipeline_read_motion(h->p, w, i, (int16_t*)mv_data, (uint8_t*)info_data, (uint32_t*)summary_data)) != LEON_OK) return throw_leon(env, rc);
    const leon_pipeline_motion_frame& m = refs[(size_t)i];
    NAPI_OK(make_object(env, {{"mv", mv}, {"info", mbinfo}, {"summary", summary}}, &o));
    NAPI_OK(set_numbers(env, o, {{"fwdGop", (double)m.fwd_gop}, {"fwdDisplay", (double)m.fwd_display}, {"bwdDisplay", (double)m.bwd_display},
                                 {"mbWidth", (double)lay.mb_width}, {"mbHeight", (double)lay.mb_height}}));
    return o;
}

// p.readActivity(window, i) -> {cells: Uint8Array [mbs][8] (per macroblock uint16 ac_count, ac_mag, dc_mag little endian, uint8 blocks, qscale),
// summary: Uint32Array [8], mbWidth, mbHeight}: one frame's activity record (opts.activity; include/leon_pipeline.h
// LEON_PIPELINE_OUTPUT_ACTIVITY), copied to the host; js/leon_pipeline.js splits the cells into typed arrays
napi_value PipeReadActivity(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readActivity(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad()) return nullptr;
    struct leon_pipeline_activity_layout lay;
    int rc = leon_pipeline_get_activity_layout(a.h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    napi_value o, cells, summary;
    void *cells_data, *summary_data;
    NAPI_OK(make_array(env, napi_uint8_array, (size_t)lay.mbs * 8, &cells_data, &cells));
    NAPI_OK(make_array(env, napi_uint32_array, 8, &summary_data, &summary));
    if ((rc = leon_pipeline_read_activity(a.h->p, w, i, cells_data, (uint32_t*)summary_data)) != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"cells", cells}, {"summary", summary}}, &o));
    NAPI_OK(set_numbers(env, o, {{"mbWidth", (double)lay.mb_width}, {"mbHeight", (double)lay.mb_height}}));
    return o;
}

// p.readResidual(window, i) -> {y: Int16Array [codedHeight][codedWidth], cb, cr: Int16Array [codedHeight / 2][codedWidth / 2], codedWidth,
// codedHeight}: one frame's residual record (opts.residual; include/leon_pipeline.h LEON_PIPELINE_OUTPUT_RESIDUAL), copied to the host, packed
napi_value PipeReadResidual(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readResidual(window, index)");
    const int64_t w = a.i64(0);
    const int32_t i = a.i32(1);
    if (a.bad()) return nullptr;
    struct leon_pipeline_residual_layout lay;
    int rc = leon_pipeline_get_residual_layout(a.h->p, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    napi_value o, ta[3];
    void* data[3] = {nullptr, nullptr, nullptr};
    const size_t luma = (size_t)lay.coded_width * (size_t)lay.coded_height;
    for (int k = 0; k < 3; k++) NAPI_OK(make_array(env, napi_int16_array, k == 0 ? luma : luma / 4, &data[k], &ta[k]));
    if ((rc = leon_pipeline_read_residual(a.h->p, w, i, (int16_t*)data[0], (int16_t*)data[1], (int16_t*)data[2])) != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"y", ta[0]}, {"cb", ta[1]}, {"cr", ta[2]}}, &o));
    NAPI_OK(set_numbers(env, o, {{"codedWidth", (double)lay.coded_width}, {"codedHeight", (double)lay.coded_height}}));
    return o;
}

// p.readRegions(window, boxes, outHeight, outWidth, filter) -> Buffer of n * region bytes (3 * outHeight * outWidth elements of the
// pipeline's element type and layout each, packed): leon_pipeline_read_regions.  boxes: an Int32Array of n x [frame index, x, y, width, height].
// Five numbers more -- fit mode, anchor, pad r, g, b (leon_pipeline_regions_fit) -- make it leon_pipeline_read_regions_fit.
napi_value PipeReadRegions(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readRegions(window, Int32Array of [frame, x, y, width, height] per region, outHeight, outWidth, filter)");
    size_t n = 0;
    const int64_t w = a.i64(0);
    const int32_t* b = a.rows(1, 5, &n);
    const int32_t oh = a.i32(2), ow = a.i32(3), filter = a.i32(4);
    if (a.bad()) return nullptr;
    const bool fitted = a.argc > 5;
    leon_pipeline_regions_fit fit{};
    if (fitted) {
        a.usage = "readRegions(..., filter, fitMode, anchor, padR, padG, padB)";
        fit.mode = a.i32(5);
        fit.anchor = a.i32(6);
        for (size_t k = 0; k < 3; k++) fit.pad[k] = a.i32(7 + k);
    }
    if (a.bad() || !has_tensor_output(env, a.h, "readRegions")) return nullptr;
    std::vector<leon_pipeline_region> regions(n ? n : 1);
    for (size_t i = 0; i < n; i++) regions[i] = leon_pipeline_region{b[5 * i], b[5 * i + 1], b[5 * i + 2], b[5 * i + 3], b[5 * i + 4], {0, 0, 0}};
    const leon_pipeline_regions_config cfg{ow, oh, filter, {0, 0, 0, 0, 0}};
    napi_value buf;
    void* data = nullptr;
    NAPI_OK(region_batch(env, a.h, n, oh, ow, &data, &buf));
    const int32_t count = record_count(n).count;
    int rc = fitted ? leon_pipeline_read_regions_fit(a.h->p, w, regions.data(), count, &cfg, &fit, data) : leon_pipeline_read_regions(a.h->p, w, regions.data(), count, &cfg, data);
    return rc == LEON_OK ? buf : throw_leon(env, rc);
}

// p.readWarpRegions(window, records, outHeight, outWidth, padR, padG, padB) -> Buffer of n * region bytes, packed:
// leon_pipeline_read_warp_regions.  records: an Int32Array of n x [frame index, a00, a01, tx, a10, a11, ty] (Q16).
napi_value PipeReadWarpRegions(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "readWarpRegions(window, Int32Array of [frame, a00, a01, tx, a10, a11, ty] per region, outHeight, outWidth, padR, padG, padB)");
    size_t n = 0;
    leon_pipeline_warp_config cfg{};
    const int64_t w = a.i64(0);
    const int32_t* b = a.rows(1, 7, &n);
    cfg.out_height = a.i32(2);
    cfg.out_width = a.i32(3);
    for (size_t k = 0; k < 3; k++) cfg.pad[k] = a.i32(4 + k);
    if (a.bad() || !has_tensor_output(env, a.h, "readWarpRegions")) return nullptr;
    std::vector<leon_pipeline_warp_region> regions(n ? n : 1);
    for (size_t i = 0; i < n; i++)
        regions[i] = leon_pipeline_warp_region{b[7 * i], {b[7 * i + 1], b[7 * i + 2], b[7 * i + 3], b[7 * i + 4], b[7 * i + 5], b[7 * i + 6]}, 0};
    napi_value buf;
    void* data = nullptr;
    NAPI_OK(region_batch(env, a.h, n, cfg.out_height, cfg.out_width, &data, &buf));
    const int rc = leon_pipeline_read_warp_regions(a.h->p, w, regions.data(), record_count(n).count, &cfg, data);
    return rc == LEON_OK ? buf : throw_leon(env, rc);
}

// p.carryRegions(window, records) -> {out: Int32Array [n][8] (leon_pipeline_region records: frame = target, the moved box, three zeros),
// votes: Int32Array [n][4] (A, I, dh, dv), status: Int32Array [n] (LEON_REGION_*; not 0: the record's words of out and votes are 0)}:
// leon_pipeline_carry_regions (opts.motion).  records: an Int32Array of n x [frame index, x, y, width, height, target frame index].
napi_value PipeCarryRegions(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "carryRegions(window, Int32Array of [frame, x, y, width, height, target] per record)");
    size_t n = 0;
    const int64_t w = a.i64(0);
    const int32_t* b = a.rows(1, 6, &n);
    if (a.bad()) return nullptr;
    const Count c = record_count(n);
    std::vector<leon_pipeline_carry_region> regions(c.rows);
    for (size_t i = 0; i < n && i < c.rows; i++)
        regions[i] = leon_pipeline_carry_region{b[6 * i], b[6 * i + 1], b[6 * i + 2], b[6 * i + 3], b[6 * i + 4], b[6 * i + 5], {0, 0}};
    napi_value o, out, votes, status;
    void *out_data, *votes_data, *status_data;
    NAPI_OK(make_array(env, napi_int32_array, c.rows * 8, &out_data, &out));
    NAPI_OK(make_array(env, napi_int32_array, c.rows * 4, &votes_data, &votes));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &status_data, &status));
    const int rc = leon_pipeline_carry_regions(a.h->p, w, regions.data(), c.count, static_cast<leon_pipeline_region*>(out_data), static_cast<int32_t*>(votes_data),
                                               static_cast<int32_t*>(status_data));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"out", out}, {"votes", votes}, {"status", status}}, &o));
    return o;
}

// p.gaugeRegions(window, regions, sources) -> {stats: Float64Array [n][16] (every word is below 2^53, so a double holds it exactly),
// status: Int32Array [n] (LEON_REGION_*; not 0: the record's words of stats are 0)}: leon_pipeline_gauge_regions (opts.motion and / or
// opts.activity).  regions: an Int32Array of n x [frame index, x, y, width, height]; sources: LEON_GAUGE_* bits.
napi_value PipeGaugeRegions(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "gaugeRegions(window, Int32Array of [frame, x, y, width, height] per record, sources)");
    size_t n = 0;
    const int64_t w = a.i64(0);
    const int32_t* b = a.rows(1, 5, &n);
    const int32_t sources = a.i32(2);
    if (a.bad()) return nullptr;
    const Count c = record_count(n);
    std::vector<leon_pipeline_region> regions(c.rows);
    for (size_t i = 0; i < n && i < c.rows; i++) regions[i] = leon_pipeline_region{b[5 * i], b[5 * i + 1], b[5 * i + 2], b[5 * i + 3], b[5 * i + 4], {0, 0, 0}};
    std::vector<int64_t> words(c.rows * 16, 0);          // (zeros: what a refused record keeps)
    napi_value o, stats, status;
    void *stats_data, *status_data;
    NAPI_OK(make_array(env, napi_float64_array, c.rows * 16, &stats_data, &stats));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &status_data, &status));
    leon_pipeline_gauge_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.sources = sources;
    const int rc = leon_pipeline_gauge_regions(a.h->p, w, &cfg, regions.data(), c.count, words.data(), static_cast<int32_t*>(status_data));
    if (rc != LEON_OK) return throw_leon(env, rc);
    double* d = static_cast<double*>(stats_data);
    for (size_t i = 0; i < c.rows * 16; i++) d[i] = (double)words[i];
    NAPI_OK(make_object(env, {{"stats", stats}, {"status", status}}, &o));
    return o;
}

// p.proposeRegions(window, frames, config) -> {regions: Int32Array [n][K][8], count: Int32Array [n], info: Int32Array [n][K][2],
// status: Int32Array [n] (LEON_REGION_*; not 0: the request's rows and count are 0)}: leon_pipeline_propose_regions (opts.motion and / or
// opts.activity).  frames: an Int32Array of n window frame indices; config: an Int32Array of the 8 words of leon_pipeline_propose_config.
napi_value PipeProposeRegions(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "proposeRegions(window, Int32Array of frame indices, Int32Array of the config's 8 words)");
    size_t n = 0, config_words = 0;
    const int64_t w = a.i64(0);
    const int32_t* frames = a.rows(1, 1, &n);
    const void* config = a.array(2, napi_int32_array, &config_words);
    if (a.bad(config_words != 8)) return nullptr;
    leon_pipeline_propose_config cfg;
    memcpy(&cfg, config, sizeof cfg);
    const Count c = record_count(n);          // (a K the library refuses allocates nothing to speak of either)
    const size_t K = cfg.max_boxes >= 1 && cfg.max_boxes <= 1024 ? (size_t)cfg.max_boxes : 1;
    napi_value o, regions, count, boxinfo, status;
    void *regions_data, *count_data, *info_data, *status_data;
    NAPI_OK(make_array(env, napi_int32_array, c.rows * K * 8, &regions_data, &regions));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &count_data, &count));
    NAPI_OK(make_array(env, napi_int32_array, c.rows * K * 2, &info_data, &boxinfo));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &status_data, &status));
    const int rc = leon_pipeline_propose_regions(a.h->p, w, &cfg, frames, c.count, static_cast<leon_pipeline_region*>(regions_data), static_cast<int32_t*>(info_data),
                                                 static_cast<int32_t*>(count_data), static_cast<int32_t*>(status_data));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"regions", regions}, {"count", count}, {"info", boxinfo}, {"status", status}}, &o));
    return o;
}

// p.propagateMaps(window, maps, hops, stride, planes, elemBytes, fill) -> {via: Uint8Array [n][mh][mw] (0 fill, 1 forward, 2 backward),
// status: Int32Array [n] (LEON_REGION_*; not 0: the record's slot and via map are left as they were, via zero)}:
// leon_pipeline_propagate_maps (opts.motion).  maps: a Uint8Array over the bytes of [slots][planes][mh][mw], contiguous, WRITTEN IN
// PLACE; hops: an Int32Array of n x [target frame index, dst slot, fwd slot, bwd slot].  The slot pitch is the map's size, so a map
// whose bytes are no multiple of 4 is refused by the library (js/leon_pipeline.js says so).
napi_value PipePropagateMaps(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "propagateMaps(window, Uint8Array maps, Int32Array of [target, dst, fwd, bwd] per hop, stride, planes, elemBytes, fill)");
    size_t mlen = 0, n = 0;
    const int64_t w = a.i64(0);
    void* maps = a.array(1, napi_uint8_array, &mlen);
    const int32_t* b = a.rows(2, 4, &n);
    const int32_t stride = a.i32(3), planes = a.i32(4), elem = a.i32(5);
    const uint32_t fill = a.u32(6);
    if (a.bad()) return nullptr;
    struct leon_pipeline_propagate_layout lay;
    int rc = leon_pipeline_propagate_layout(a.h->info.frame_width, a.h->info.frame_height, stride, planes, elem, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    if (!lay.slot_bytes || mlen % lay.slot_bytes != 0 || mlen / lay.slot_bytes < 1) {
        napi_throw_type_error(env, nullptr, "propagateMaps: maps is not a whole number of maps of planes * mh * mw * elemBytes bytes");
        return nullptr;
    }
    const Count c = record_count(n);
    std::vector<leon_pipeline_propagate_hop> hops(c.rows);
    for (size_t i = 0; i < n && i < c.rows; i++) hops[i] = leon_pipeline_propagate_hop{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3], {0, 0, 0, 0}};
    leon_pipeline_propagate_config cfg{};
    cfg.stride = stride; cfg.planes = planes; cfg.elem_bytes = elem;
    cfg.n_slots = record_count(mlen / lay.slot_bytes).count;
    cfg.fill = fill;
    cfg.slot_pitch_bytes = lay.slot_bytes; cfg.maps_bytes = mlen;
    napi_value o, via, status;
    void *via_data, *status_data;
    NAPI_OK(make_array(env, napi_uint8_array, c.rows * (size_t)lay.mh * (size_t)lay.mw, &via_data, &via));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &status_data, &status));
    rc = leon_pipeline_propagate_maps(a.h->p, w, &cfg, hops.data(), c.count, maps, static_cast<uint8_t*>(via_data), static_cast<int32_t*>(status_data));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(make_object(env, {{"via", via}, {"status", status}}, &o));
    return o;
}

// p.accumulate(window, hops, parts, slots) -> {slots (the array handed in, WRITTEN IN PLACE), via: Uint8Array [n][mbh][mbw] (0 restart,
// 1 forward, 2 backward), status: Int32Array [n] (LEON_REGION_*; not 0: the hop's slot is left as it was, its via zero), layout: the
// numbers of leon_pipeline_accumulate_layout}: leon_pipeline_accumulate (opts.motion, and opts.residual for parts & 2).  hops: an
// Int32Array of n x [target frame index, dst slot, fwd slot, bwd slot]; slots: an Int16Array over a whole number of accumulators, each
// the layout's slotBytes (always a multiple of 256) long, or a number: that many accumulators made here, all zero.
napi_value PipeAccumulate(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "accumulate(window, Int32Array of [target, dst, fwd, bwd] per hop, parts, Int16Array slots or their number 1 .. 65535)");
    size_t slen = 0, n = 0;
    const int64_t w = a.i64(0);
    const int32_t* b = a.rows(1, 4, &n);
    const int32_t parts = a.i32(2);
    napi_valuetype kind = napi_undefined;
    napi_typeof(env, a.argv[3], &kind);
    const int32_t fresh = kind == napi_number ? a.i32(3) : 0;          // a number: that many accumulators, made here, all zero
    napi_value held = a.argv[3];
    void* slots = kind == napi_number ? nullptr : a.array(3, napi_int16_array, &slen);
    if (a.bad(kind == napi_number && !record_count((size_t)(fresh < 0 ? 0 : fresh)).ok)) return nullptr;
    struct leon_pipeline_accumulate_layout lay;
    int rc = leon_pipeline_accumulate_layout(a.h->info.coded_width, a.h->info.coded_height, parts, &lay);
    if (rc != LEON_OK) return throw_leon(env, rc);
    if (kind == napi_number) {
        slen = (size_t)fresh * (lay.slot_bytes / 2);
        NAPI_OK(make_array(env, napi_int16_array, slen, &slots, &held));
    }
    const size_t bytes = slen * 2;
    if (!lay.slot_bytes || bytes % lay.slot_bytes != 0 || bytes / lay.slot_bytes < 1) {
        napi_throw_type_error(env, nullptr, "accumulate: slots is not a whole number of accumulators of the layout's slotBytes");
        return nullptr;
    }
    const Count c = record_count(n);
    std::vector<leon_pipeline_propagate_hop> hops(c.rows);
    for (size_t i = 0; i < n && i < c.rows; i++) hops[i] = leon_pipeline_propagate_hop{b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3], {0, 0, 0, 0}};
    leon_pipeline_accumulate_config cfg{};
    cfg.parts = parts;
    cfg.n_slots = record_count(bytes / lay.slot_bytes).count;
    cfg.slot_pitch_bytes = lay.slot_bytes; cfg.slots_bytes = bytes;
    const size_t mbs = (size_t)(lay.coded_width / 16) * (size_t)(lay.coded_height / 16);
    napi_value o, layout, via, status;
    void *via_data, *status_data;
    NAPI_OK(make_array(env, napi_uint8_array, c.rows * mbs, &via_data, &via));
    NAPI_OK(make_array(env, napi_int32_array, c.rows, &status_data, &status));
    rc = leon_pipeline_accumulate(a.h->p, w, &cfg, hops.data(), c.count, slots, static_cast<uint8_t*>(via_data), static_cast<int32_t*>(status_data));
    if (rc != LEON_OK) return throw_leon(env, rc);
    NAPI_OK(napi_create_object(env, &layout));
    NAPI_OK(set_numbers(env, layout, {{"codedWidth", (double)lay.coded_width}, {"codedHeight", (double)lay.coded_height}, {"parts", (double)lay.parts},
                                      {"planes", (double)lay.planes}, {"lumaStride", (double)lay.luma_stride}, {"chromaStride", (double)lay.chroma_stride},
                                      {"axOffset", (double)lay.ax_offset}, {"ayOffset", (double)lay.ay_offset}, {"ageOffset", (double)lay.age_offset},
                                      {"ryOffset", (double)lay.ry_offset}, {"rcbOffset", (double)lay.rcb_offset}, {"rcrOffset", (double)lay.rcr_offset},
                                      {"slotBytes", (double)lay.slot_bytes}, {"slotPitch", (double)lay.slot_pitch}}));
    NAPI_OK(make_object(env, {{"slots", held}, {"via", via}, {"status", status}, {"layout", layout}}, &o));
    return o;
}

napi_value PipeStats(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, nullptr);
    if (a.bad()) return nullptr;
    PipeHandle* h = a.h;
    leon_pipeline_stats s{};
    leon_pipeline_get_stats(h->p, &s);
    napi_value o, v;
    NAPI_OK(napi_create_object(env, &o));
    NAPI_OK(set_numbers(env, o, {
        {"pictures", (double)s.pictures}, {"gops", (double)s.gops}, {"windows", (double)s.windows}, {"streamBytes", (double)s.stream_bytes},
        {"seconds", s.seconds}, {"parseSecondsSum", s.parse_seconds_sum}, {"uploadBytes", s.upload_bytes}, {"entries", (double)s.entries},
        {"frameWidth", (double)h->info.frame_width}, {"frameHeight", (double)h->info.frame_height},
        {"codedWidth", (double)h->info.coded_width}, {"codedHeight", (double)h->info.coded_height},
        {"pictureRate", h->info.picture_rate}, {"keyMapGops", (double)h->info.gops}, {"shardGops", (double)h->info.shard_gops}, {"firstGop", (double)h->info.first_gop},
        {"duration", h->info.duration}, {"parserThreads", (double)h->info.parser_threads},
        {"gopsPerWindow", (double)h->info.gops_per_window}, {"output", (double)h->info.output},
        {"chromaWidth", (double)h->info.chroma_width}, {"chromaHeight", (double)h->info.chroma_height},
        {"tensorDtype", (double)h->info.tensor_dtype}, {"tensorElementBytes", (double)h->info.tensor_element_bytes},
        {"tensorFrameBytes", (double)h->info.tensor_frame_bytes}, {"tensorFramePitch", (double)h->info.tensor_frame_pitch},
        {"tensorGopPitch", (double)h->info.tensor_gop_pitch}, {"tensorWidth", (double)h->tensor_geom.width}, {"tensorHeight", (double)h->tensor_geom.height},
        // where the resampled image lies in the tensor (leon_pipeline_tensor_canvas; without a canvas: all of it)
        {"tensorImageX", (double)h->tensor_canvas.x}, {"tensorImageY", (double)h->tensor_canvas.y},
        {"tensorImageWidth", (double)h->tensor_canvas.image_width}, {"tensorImageHeight", (double)h->tensor_canvas.image_height}}));
    if (h->info.tensor_dtype) {          // the tensors' layout by its option name
        NAPI_OK(napi_create_string_utf8(env, h->tensor_shape.layout == LEON_TENSOR_LAYOUT_HWC ? "hwc" : "chw", NAPI_AUTO_LENGTH, &v));
        NAPI_OK(set_props(env, o, {{"tensorLayout", v}}));
    }
    return o;
}

napi_value PipeDestroy(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, nullptr, nullptr);
    if (a.h) {
        leon_pipeline_destroy(a.h->p);       // joins the notify thread: no further callbacks are queued
        a.h->p = nullptr;
        if (a.h->tsfn) {
            napi_release_threadsafe_function(a.h->tsfn, napi_tsfn_abort);
            a.h->tsfn = nullptr;
        }
    }
    return nullptr;
}

// seek(seconds, exact) -> firstWindow
napi_value PipeSeek(napi_env env, napi_callback_info info)
{
    Call<PipeHandle> a(env, info, "seek(seconds, exact)");
    const double t = a.f64(0);
    const bool exact = a.flag(1, false);
    if (a.bad()) return nullptr;
    PipeHandle* h = a.h;
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
    Call<PipeHandle> a(env, info, "feed(validBytes)", "pipeline destroyed");
    const int64_t v = a.i64(0);
    if (a.bad(v < 0)) return nullptr;
    const int rc = leon_pipeline_feed(a.h->p, (size_t)v);
    return rc == LEON_OK ? nullptr : throw_leon(env, rc);
}

napi_value CreatePipeline(napi_env env, napi_callback_info info)
{
    Args a(env, info, "createPipeline(streamBuffer, options, callback)");
    bool is_buf = false;
    napi_valuetype cbt = napi_undefined;
    napi_is_buffer(env, a.argv[0], &is_buf);
    napi_typeof(env, a.argv[2], &cbt);
    if (a.bad(!is_buf || cbt != napi_function)) return nullptr;
    napi_value opts = a.argv[1];
    void* data = nullptr;
    size_t len = 0;
    NAPI_OK(napi_get_buffer_info(env, a.argv[0], &data, &len));
    // The integer options, one table per struct of include/leon_pipeline.h (js/leon_pipeline.js maps the names of output, tensorDtype,
    // tensorFilter and tensorLayout to LEON_PIPELINE_OUTPUT_* bits, LEON_TENSOR_*, LEON_RESIZE_* and LEON_TENSOR_LAYOUT_*, and spreads
    // tensorSize / tensorCrop / tensorCanvas / tensorOrigin / tensorPadValue / tensorLetterbox into these): the decode itself; the
    // tensor output's element type; the tensors resampled to a model's input size; their layout; the image placed in a padded canvas.
    // tensorLetterbox: out size, canvas and origin from leon_pipeline_letterbox of the crop box, or of the frame (the stream's first
    // sequence header).
    leon_pipeline_config cfg;
    leon_pipeline_tensor_config tcfg;
    leon_pipeline_tensor_resize rcfg;
    leon_pipeline_tensor_format fcfg;
    leon_pipeline_tensor_canvas ccfg;
    memset(&cfg, 0, sizeof cfg);
    memset(&tcfg, 0, sizeof tcfg);
    memset(&rcfg, 0, sizeof rcfg);
    memset(&fcfg, 0, sizeof fcfg);
    memset(&ccfg, 0, sizeof ccfg);
    int32_t lb_w = 0, lb_h = 0, origin_set = 0;
    const std::vector<IntOpt> tables[5] = {
        {{"deviceId", &cfg.device_id, 0}, {"parserThreads", &cfg.parser_threads, 0}, {"gopsPerWindow", &cfg.gops_per_window, 0}, {"windowsInFlight", &cfg.windows_in_flight, 0},
         {"maxGopPictures", &cfg.max_gop_pictures, 0}, {"loop", &cfg.loop, 0}, {"shardIndex", &cfg.shard_index, 0}, {"shardCount", &cfg.shard_count, 0},
         {"gpuParser", &cfg.gpu_parser, 0}, {"displayFlavour", &cfg.display_flavour, 0}, {"output", &cfg.output, 0}},
        {{"tensorDtype", &tcfg.dtype, 0}},
        {{"tensorOutWidth", &rcfg.out_width, 0}, {"tensorOutHeight", &rcfg.out_height, 0}, {"tensorCropX", &rcfg.crop_x, 0}, {"tensorCropY", &rcfg.crop_y, 0},
         {"tensorCropWidth", &rcfg.crop_width, 0}, {"tensorCropHeight", &rcfg.crop_height, 0}, {"tensorFilter", &rcfg.filter, 0}},
        {{"tensorLayout", &fcfg.layout, 0}},
        {{"tensorCanvasWidth", &ccfg.width, 0}, {"tensorCanvasHeight", &ccfg.height, 0}, {"tensorOriginX", &ccfg.x, 0}, {"tensorOriginY", &ccfg.y, 0},
         {"tensorOriginSet", &origin_set, 0}, {"tensorPadR", &ccfg.pad[0], 0}, {"tensorPadG", &ccfg.pad[1], 0}, {"tensorPadB", &ccfg.pad[2], 0},
         {"tensorLetterboxWidth", &lb_w, 0}, {"tensorLetterboxHeight", &lb_h, 0}}};
    size_t bad_table = 5;          // the first table with an option that is no integer
    for (size_t t = 0; t < 5; t++)
        for (const IntOpt& o : tables[t])
            if (!get_i32(env, opts, o.name, o.field, o.dflt) && bad_table == 5) bad_table = t;
    // tensorScale / tensorBias [r, g, b] stand between the element type and the resize options, and so does their fault
    const bool bad_scale = !get_f32x3(env, opts, "tensorScale", tcfg.scale) || !get_f32x3(env, opts, "tensorBias", tcfg.bias);
    if (bad_table < 2 || (bad_table < 5 && !bad_scale)) {
        napi_throw_type_error(env, nullptr, "createPipeline: integer options expected");
        return nullptr;
    }
    if (bad_scale) {
        napi_throw_type_error(env, nullptr, "createPipeline: tensorScale / tensorBias must be arrays of three numbers");
        return nullptr;
    }
    get_f64(env, opts, "startSeconds", &cfg.start_seconds);          // begin at the key-map entry at or before this time (no number: 0)
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
    PipeGuard guard{env, new PipeHandle()};
    PipeHandle* h = guard.h;
    napi_value name;
    NAPI_OK(napi_create_string_utf8(env, "leon pipeline frames", NAPI_AUTO_LENGTH, &name));
    if (napi_create_threadsafe_function(env, a.argv[2], nullptr, name, 0, 1, nullptr, nullptr, h, pipe_call_js, &h->tsfn) != napi_ok) {
        napi_throw_error(env, nullptr, "napi_create_threadsafe_function failed");
        return nullptr;
    }
    napi_create_reference(env, a.argv[0], 1, &h->stream_ref);
    // validBytes: the stream is still arriving (leon_pipeline_create_partial) -- the loader writes on into the same
    // Buffer and calls feed(validBytesNow), as addBuffer does in the reference (features/bitreader.js:332-430)
    // (a presence test and a double, not an int32 with -1 for "absent": 2 GiB and more of a stream may have arrived)
    double valid = 0;
    const int given = get_f64(env, opts, "validBytes", &valid);
    if (given < 0 || (given > 0 && (!(valid >= 0) || valid > (double)len || valid != (double)(size_t)valid))) {
        napi_throw_range_error(env, nullptr, "createPipeline: validBytes must be an integer between 0 and the stream's length");
        return nullptr;
    }
    const bool partial = given > 0;
    int rc = tensor ? leon_pipeline_create_tensor_canvas(&cfg, &tcfg, resized ? &rcfg : nullptr, fcfg.layout ? &fcfg : nullptr, canvas ? &ccfg : nullptr, (const uint8_t*)data, len, partial ? (size_t)valid : len, pipe_native_cb, h, &h->p)
           : partial ? leon_pipeline_create_partial(&cfg, (const uint8_t*)data, len, (size_t)valid, pipe_native_cb, h, &h->p)
                     : leon_pipeline_create(&cfg, (const uint8_t*)data, len, pipe_native_cb, h, &h->p);
    if (rc != LEON_OK) return throw_leon(env, rc);
    leon_pipeline_get_info(h->p, &h->info);
    if (h->info.tensor_dtype) {
        leon_pipeline_get_tensor_geometry(h->p, &h->tensor_geom);
        leon_pipeline_get_tensor_shape(h->p, &h->tensor_shape);
        leon_pipeline_get_tensor_canvas(h->p, &h->tensor_canvas);
    }
    napi_value obj;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_wrap(env, obj, h, pipe_finalize, nullptr, nullptr));
    guard.h = nullptr;          // the object owns it now (pipe_finalize)
    NAPI_OK(define_methods(env, obj, {{"releaseWindow", PipeRelease}, {"readFrame", PipeReadFrame}, {"readPlanes", PipeReadPlanes}, {"readTensor", PipeReadTensor},
                                      {"readMotion", PipeReadMotion}, {"readActivity", PipeReadActivity}, {"readResidual", PipeReadResidual}, {"readRegions", PipeReadRegions},
                                      {"readWarpRegions", PipeReadWarpRegions}, {"carryRegions", PipeCarryRegions}, {"gaugeRegions", PipeGaugeRegions},
                                      {"proposeRegions", PipeProposeRegions}, {"propagateMaps", PipePropagateMaps}, {"stats", PipeStats}, {"destroy", PipeDestroy}, {"feed", PipeFeed},
                                      {"seek", PipeSeek}}));
    // accumulate: callable like the rest, not enumerable (as a class's methods are not): Object.keys(handle) is a list callers iterate,
    // "every method after destroy" among them, and stays what it was
    const napi_property_descriptor accumulate = {"accumulate", nullptr, PipeAccumulate, nullptr, nullptr, nullptr, (napi_property_attributes)(napi_writable | napi_configurable), nullptr};
    NAPI_OK(napi_define_properties(env, obj, 1, &accumulate));
    return obj;
}

// letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight) -> [outWidth, outHeight, x, y]: leon_pipeline_letterbox, no device
napi_value Letterbox(napi_env env, napi_callback_info info)
{
    Args a(env, info, "letterbox(srcWidth, srcHeight, canvasWidth, canvasHeight)");
    int32_t s[4];
    for (size_t k = 0; k < 4; k++) s[k] = a.i32(k);
    if (a.bad()) return nullptr;
    leon_pipeline_tensor_resize rz;
    leon_pipeline_tensor_canvas cv;
    memset(&rz, 0, sizeof rz);
    memset(&cv, 0, sizeof cv);
    const int rc = leon_pipeline_letterbox(s[0], s[1], s[2], s[3], &rz, &cv);
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
    NAPI_OK(define_methods(env, exports, {{"create", Create}, {"createPipeline", CreatePipeline}, {"letterbox", Letterbox}, {"abiVersion", AbiVersion}}));
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
