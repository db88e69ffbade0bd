// Node N-API addon: the thin FFI between the reference's TypeScript surface
// (compute_msm, src/submission/submission.ts:25-157) and libmsm's C ABI (include/msm.h).
//
// Exports (all compute is asynchronous through napi_async_work, resolving a Promise, because
// compute_msm is async in the reference):
//   computeMsmU32(points: Uint32Array(32n), scalars: Uint32Array(8n), windowSize, devices?)
//       -> Promise<Uint32Array(16)>
//   computeMsmBigInt(points: {x,y,t,z: bigint}[], scalars: bigint[], windowSize, devices?)
//       -> Promise<Uint32Array(16)>
//       BigInt -> big-endian u32 marshalling happens natively (napi_get_value_bigint_words),
//       replacing convert_worker.ts:8-57 and the 8-worker fan-out of submission.ts:47-74.
//   `devices` (an array of HIP ordinals) shards the MSM over those gfx950 devices in this one call
//   (msm_opts MSM_FLAG_DEVICES: one host thread and PCIe link per device, partials joined with one
//   EC add each -- the reference's CPU/GPU split of submission.ts:116-154 generalised).
//
// Input ownership while the promise is pending (the worker thread reads the inputs): typed arrays
// over a SharedArrayBuffer -- what the reference's own compute_msm allocates
// (submission.ts:35-39) and what submission.mjs's flattenU32 builds -- cannot be detached, so they
// are read in place (a reference keeps them alive; writing them before the promise settles races
// with the upload).  Typed arrays over a plain ArrayBuffer could be detached (transferred) by the
// caller while the job runs, freeing the memory under the worker, so they are copied first.
//   pointAddAffine(a: Uint32Array(16), b: Uint32Array(16)) -> Uint32Array(16)      (lib.rs:240-253)
//   split(windowSize, scalars: Uint32Array(8n)) -> Uint32Array(W*n)                 (lib.rs:196-202)
//   bestWindowSize(n) -> number                                                     (submission.ts:18-23)
//   init() -> number (0 ok), deviceCount() -> number, deviceOrdinals() -> number[],
//   strerror(code) -> string
// Resident prepared bases (msm_bases_*; these three are not enumerable, the list above is the
// addon's enumerable surface):
//   prepareBases(points: Uint32Array(32n), levels?, windowSize?) -> { id, n, levels, windowSize, bytes }
//   computeMsmPrepared(id, scalars: Uint32Array(8n)) -> Promise<Uint32Array(16)>
//   computeMsmPrepared(id, scalars: Uint32Array(8m), first?: number, indices?: Uint32Array(m),
//                      scalarBits?: number)   (scalarBits = b: ceil(b / 32) words per scalar)
//       over a subset of the bases: the range [first, first + m), or bases indices[0..m)
//   scaleBases(id, scalars: Uint32Array(8m), first?, indices?, scalarBits?, asBases?, levels?, windowSize?)
//       -> Uint32Array(32m), the wire points s_i * P_i, or with asBases the object of a new handle
//   combineBases(id, otherId?, a?: Uint32Array, b?: Uint32Array, aFirst, bFirst, aIndices?, bIndices?, m, flags,
//                scalarBits?, keep?, levels?, windowSize?)
//       -> Uint32Array(32m), the wire points a_i * A_i +- b_i * B_i (flags: MSM_COMBINE_*), or with keep the
//          object of a new handle
//   releaseBases(id) -> number (0 ok, -1 for a handle already released)
// Fixed-base tables (msm_fixed_*; not enumerable either):
//   prepareFixedBase(id, first?, count?, indices?, windowBits?, scalarBits?)
//       -> { id, bases, windowBits, scalarBits, windows, records, bytes }
//   fixedBaseMul(id, scalars: Uint32Array(8 m bases), scalarBits?, asBases?, levels?, windowSize?)
//       -> Uint32Array(32m), the wire points sum_j s_ij * B_j, or with asBases the object of a new handle
//   releaseFixedBase(id) -> number (0 ok, -1 for a table already released)
//   Handles and tables left open are freed by the cleanup hook's msm_shutdown.
#include <node_api.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "msm.h"

namespace {

#define NAPI_OK(call)                                              \
  do {                                                             \
    if ((call) != napi_ok) {                                       \
      napi_throw_error(env, nullptr, "N-API call failed: " #call); \
      return nullptr;                                              \
    }                                                              \
  } while (0)

// Staging for the copies of plain-ArrayBuffer inputs: one buffer pair kept between calls (its pages
// stay mapped: a fresh 160 MB allocation per 2^20 call spent ~60 ms in first-touch page faults),
// lent to one job at a time; a concurrent job gets its own and frees it when done.  The cached pair
// is kept only up to MSM_NODE_STAGING_CACHE_MB (default 256 MiB: a 2^20 MSM's 160 MiB); a larger
// one is freed after its job.  SharedArrayBuffer inputs need no staging at all.
struct Staging {
  std::vector<uint32_t> points, scalars;
  size_t bytes() const { return (points.capacity() + scalars.capacity()) * 4; }
};
std::mutex g_stage_mu;
Staging* g_stage = nullptr;  // the idle cached pair, or null while lent out

size_t staging_cache_cap() {
  static const size_t cap = (getenv("MSM_NODE_STAGING_CACHE_MB") ? (size_t)atol(getenv("MSM_NODE_STAGING_CACHE_MB"))
                                                                  : (size_t)256) << 20;
  return cap;
}

Staging* take_staging() {
  std::lock_guard<std::mutex> lk(g_stage_mu);
  Staging* s = g_stage ? g_stage : new Staging();
  g_stage = nullptr;
  return s;
}
void give_staging(Staging* s) {
  std::lock_guard<std::mutex> lk(g_stage_mu);
  if (!g_stage && s->bytes() <= staging_cache_cap()) {
    g_stage = s;
  } else {
    delete s;
  }
}

// dst[0..n) = src[0..n) over a few threads (one thread copies ~10 GB/s)
void copy_words(uint32_t* dst, const uint32_t* src, size_t n) {
  const size_t parts = n >= (1u << 20) ? 8 : 1;
  std::vector<std::thread> th;
  const size_t per = (n + parts - 1) / parts;
  for (size_t k = 1; k < parts; k++) {
    const size_t lo = std::min(n, k * per), hi = std::min(n, lo + per);
    th.emplace_back([=] { memcpy(dst + lo, src + lo, (hi - lo) * 4); });
  }
  memcpy(dst, src, std::min(n, per) * 4);
  for (auto& t : th) t.join();
}

struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  // marshalled BigInt inputs (computeMsmBigInt)
  std::vector<uint32_t> points, scalars;
  // the copy of plain-ArrayBuffer typed arrays (computeMsmU32), returned to the cache when done
  Staging* stage = nullptr;
  // computeMsmU32 over SharedArrayBuffers: the caller's arrays, held by references until the job
  // completes and read in place by msm_compute
  napi_ref ref_points = nullptr, ref_scalars = nullptr;
  const uint32_t* p_points = nullptr;
  const uint32_t* p_scalars = nullptr;
  size_t n = 0;
  uint32_t window = 0;
  std::vector<int32_t> devices;  // empty: the current device
  double cpu_work_ratio = 0;     // > 0: CPU/GPU co-compute (msm_compute_cocompute)
  const msm_bases* bases = nullptr;  // computeMsmPrepared: the handle whose records the MSM reads
  // computeMsmPrepared over a subset of the handle's bases (msm_bases_compute_subset): n terms over
  // bases [first, first + n), or over bases indices[0..n) (a copy of the caller's array)
  bool subset = false, indexed = false;
  uint64_t first = 0;
  std::vector<uint32_t> indices;
  uint32_t scalar_bits = 0;  // computeMsmPrepared: narrow scalars (MSM_FLAG_SCALAR_BITS); 0 = the 8-word format
  uint32_t scalar_type = 0;  // computeMsmPrepared: a native integer array (MSM_FLAG_SCALAR_TYPE); 0 = a word format
  uint32_t scalar_field = 0; // computeMsmPrepared: wide scalars (MSM_FLAG_SCALAR_FIELD, MSM_FIELD_*); 0 = none
  uint32_t out[16] = {0};
  int rc = 0;
};

void execute(napi_env, void* data) {
  Job* j = static_cast<Job*>(data);
  msm_opts o;
  memset(&o, 0, sizeof(o));
  o.window_bits = j->window;
  o.device = -1;
  if (!j->devices.empty()) {
    o.flags |= MSM_FLAG_DEVICES;
    o.devices = j->devices.data();
    o.n_devices = (uint32_t)j->devices.size();
  }
  const uint32_t* pts = j->p_points ? j->p_points : j->stage ? j->stage->points.data() : j->points.data();
  const uint32_t* sc = j->p_scalars ? j->p_scalars : j->stage ? j->stage->scalars.data() : j->scalars.data();
  msm_opts_typed obt;  // the handle entries' options: the scalars' width and type only
  memset(&obt, 0, sizeof(obt));
  msm_opts& ob = obt.opts;
  ob.device = -1;
  if (j->scalar_bits) {
    ob.flags = MSM_FLAG_SCALAR_BITS;
    ob.scalar_bits = j->scalar_bits;
  }
  if (j->scalar_type) {
    ob.flags |= MSM_FLAG_SCALAR_TYPE;
    obt.scalar_type = j->scalar_type;
  }
  if (j->scalar_field) {
    ob.flags |= MSM_FLAG_SCALAR_FIELD;
    obt.scalar_field = j->scalar_field;
  }
  if (j->bases && j->subset) {
    const uint32_t* ix = j->indices.data();
    msm_subset_t sub;
    sub.first = j->first;
    sub.m = j->n;
    sub.indices = j->indexed ? &ix : nullptr;
    j->rc = msm_bases_compute_subset(j->bases, &sub, sc, &ob, j->out);
    return;
  }
  if (j->bases) {
    j->rc = msm_bases_compute(j->bases, sc, &ob, j->out);
    return;
  }
  j->rc = j->cpu_work_ratio != 0 ? msm_compute_cocompute(pts, sc, j->n, &o, j->cpu_work_ratio, 0, j->out)
                                  : msm_compute(pts, sc, j->n, &o, j->out);
}

void complete(napi_env env, napi_status, void* data) {
  Job* j = static_cast<Job*>(data);
  if (j->rc == MSM_OK) {
    napi_value ab, arr;
    void* buf;
    napi_create_arraybuffer(env, 64, &buf, &ab);
    memcpy(buf, j->out, 64);
    napi_create_typedarray(env, napi_uint32_array, 16, ab, 0, &arr);
    napi_resolve_deferred(env, j->deferred, arr);
  } else {
    napi_value msg, code, err;
    std::string m = std::string("libmsm: ") + msm_strerror(j->rc);
    napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
    napi_create_int32(env, j->rc, &code);
    napi_create_error(env, nullptr, msg, &err);
    napi_set_named_property(env, err, "code", code);
    napi_reject_deferred(env, j->deferred, err);
  }
  if (j->ref_points) napi_delete_reference(env, j->ref_points);
  if (j->ref_scalars) napi_delete_reference(env, j->ref_scalars);
  if (j->stage) give_staging(j->stage);
  napi_delete_async_work(env, j->work);
  delete j;
}

napi_value start_job(napi_env env, Job* j) {
  napi_value promise, name;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "msm_compute", NAPI_AUTO_LENGTH, &name));
  NAPI_OK(napi_create_async_work(env, nullptr, name, execute, complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

bool get_u32_array(napi_env env, napi_value v, const uint32_t** data, size_t* len, bool* shared = nullptr) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type t;
  void* d;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &t, len, &d, &ab, &off) != napi_ok || t != napi_uint32_array) return false;
  *data = static_cast<const uint32_t*>(d);
  if (shared) {  // napi_is_arraybuffer is false for a SharedArrayBuffer
    bool plain = true;
    if (napi_is_arraybuffer(env, ab, &plain) != napi_ok) return false;
    *shared = !plain;
  }
  return true;
}

// computeMsmPrepared's `scalarType`: the MSM_SCALAR_* value of a name, the typed-array class that
// holds such a vector and its element bits.
struct NativeType {
  const char* name;
  uint32_t type;
  napi_typedarray_type cls;
  uint32_t bits;
};
const NativeType NATIVE_TYPES[] = {
    {"bit", MSM_SCALAR_BIT, napi_uint8_array, 1},        {"u8", MSM_SCALAR_U8, napi_uint8_array, 8},
    {"i8", MSM_SCALAR_I8, napi_int8_array, 8},           {"u16", MSM_SCALAR_U16, napi_uint16_array, 16},
    {"i16", MSM_SCALAR_I16, napi_int16_array, 16},       {"u32", MSM_SCALAR_U32, napi_uint32_array, 32},
    {"i32", MSM_SCALAR_I32, napi_int32_array, 32},       {"u64", MSM_SCALAR_U64, napi_biguint64_array, 64},
    {"i64", MSM_SCALAR_I64, napi_bigint64_array, 64}};
const NativeType* native_type(napi_env env, napi_value v) {
  char name[8] = {0};
  size_t len = 0;
  if (napi_get_value_string_utf8(env, v, name, sizeof(name), &len) != napi_ok) return nullptr;
  for (const NativeType& t : NATIVE_TYPES)
    if (!strcmp(name, t.name)) return &t;
  return nullptr;
}
// computeMsmPrepared's wide `scalarType` names: the MSM_FIELD_* value and the element's bytes.  Such a
// vector comes as a BigUint64Array, Uint32Array or Uint8Array of little-endian limbs, words or bytes.
struct WideType {
  const char* name;
  uint32_t field, bytes;
};
const WideType WIDE_TYPES[] = {{"u128", MSM_FIELD_U128, 16}, {"i128", MSM_FIELD_I128, 16},
                               {"u256", MSM_FIELD_U256, 32}, {"fr_mont", MSM_FIELD_FR_MONT, 32}};
const WideType* wide_type(napi_env env, napi_value v) {
  char name[8] = {0};
  size_t len = 0;
  if (napi_get_value_string_utf8(env, v, name, sizeof(name), &len) != napi_ok) return nullptr;
  for (const WideType& t : WIDE_TYPES)
    if (!strcmp(name, t.name)) return &t;
  return nullptr;
}
// A typed array of exactly the class `cls`: its bytes and element count.
bool get_typed_array(napi_env env, napi_value v, napi_typedarray_type cls, const void** data, size_t* len, bool* shared) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type t;
  void* d;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &t, len, &d, &ab, &off) != napi_ok || t != cls) return false;
  *data = d;
  bool plain = true;  // napi_is_arraybuffer is false for a SharedArrayBuffer
  if (napi_is_arraybuffer(env, ab, &plain) != napi_ok) return false;
  *shared = !plain;
  return true;
}

// Optional device list: an array of HIP ordinals (undefined / null: none).  false on a bad value.
bool get_devices(napi_env env, size_t argc, napi_value* argv, size_t at, std::vector<int32_t>* out) {
  out->clear();
  if (argc <= at) return true;
  napi_valuetype vt;
  if (napi_typeof(env, argv[at], &vt) != napi_ok) return false;
  if (vt == napi_undefined || vt == napi_null) return true;
  bool arr = false;
  if (napi_is_array(env, argv[at], &arr) != napi_ok || !arr) return false;
  uint32_t len = 0;
  if (napi_get_array_length(env, argv[at], &len) != napi_ok) return false;
  for (uint32_t i = 0; i < len; i++) {
    napi_value e;
    int32_t d;
    if (napi_get_element(env, argv[at], i, &e) != napi_ok || napi_get_value_int32(env, e, &d) != napi_ok) return false;
    out->push_back(d);
  }
  return true;  // shape and ordinals are checked by libmsm (msm_opts, MSM_ERR_INVALID_ARG)
}

// Optional cpuWorkRatio (submission.ts:95-98): a number >= 0 (undefined / null: 0).  false on a bad value.
bool get_ratio(napi_env env, size_t argc, napi_value* argv, size_t at, double* out) {
  *out = 0;
  if (argc <= at) return true;
  napi_valuetype vt;
  if (napi_typeof(env, argv[at], &vt) != napi_ok) return false;
  if (vt == napi_undefined || vt == napi_null) return true;
  if (vt != napi_number || napi_get_value_double(env, argv[at], out) != napi_ok) return false;
  return *out >= 0;  // NaN and negatives rejected here (libmsm rejects them too)
}

uint32_t get_window(napi_env env, napi_value v) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return 0;
  uint32_t w = 0;
  napi_get_value_uint32(env, v, &w);
  return w;
}

napi_value ComputeMsmU32(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint32_t *pts, *sc;
  size_t plen, slen;
  bool pshared = false, sshared = false;
  std::vector<int32_t> devs;
  double ratio = 0;
  if (argc < 2 || !get_u32_array(env, argv[0], &pts, &plen, &pshared) ||
      !get_u32_array(env, argv[1], &sc, &slen, &sshared) || !get_devices(env, argc, argv, 3, &devs) ||
      !get_ratio(env, argc, argv, 4, &ratio)) {
    napi_throw_type_error(env, nullptr,
                          "computeMsmU32(points: Uint32Array, scalars: Uint32Array, windowSize?, devices?: number[], "
                          "cpuWorkRatio?: number >= 0)");
    return nullptr;
  }
  Job* j = new Job();
  j->n = std::min(plen / 32, slen / 8);
  j->devices = std::move(devs);
  j->cpu_work_ratio = ratio;
  if (pshared && sshared) {
    j->p_points = pts;
    j->p_scalars = sc;
    if (napi_create_reference(env, argv[0], 1, &j->ref_points) != napi_ok ||
        napi_create_reference(env, argv[1], 1, &j->ref_scalars) != napi_ok) {
      if (j->ref_points) napi_delete_reference(env, j->ref_points);
      delete j;
      napi_throw_error(env, nullptr, "cannot reference the input arrays");
      return nullptr;
    }
  } else {  // detachable memory: the worker reads a copy
    j->stage = take_staging();
    if (j->stage->points.size() < j->n * 32) j->stage->points.resize(j->n * 32);
    if (j->stage->scalars.size() < j->n * 8) j->stage->scalars.resize(j->n * 8);
    copy_words(j->stage->points.data(), pts, j->n * 32);
    copy_words(j->stage->scalars.data(), sc, j->n * 8);
  }
  j->window = argc > 2 ? get_window(env, argv[2]) : 0;
  return start_job(env, j);
}

// bigint -> 8 big-endian u32 words; false if negative or wider than 256 bits
bool bigint_be(napi_env env, napi_value v, uint32_t* out8) {
  int sign = 0;
  size_t wc = 4;
  uint64_t words[4] = {0, 0, 0, 0};
  if (napi_get_value_bigint_words(env, v, &sign, &wc, words) != napi_ok) return false;
  if (sign || wc > 4) return false;
  for (int i = 0; i < 4; i++) {
    out8[7 - 2 * i] = (uint32_t)words[i];
    out8[6 - 2 * i] = (uint32_t)(words[i] >> 32);
  }
  return true;
}

napi_value ComputeMsmBigInt(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  bool ap = false, as = false;
  if (argc < 2 || napi_is_array(env, argv[0], &ap) != napi_ok || !ap || napi_is_array(env, argv[1], &as) != napi_ok ||
      !as) {
    napi_throw_type_error(env, nullptr, "computeMsmBigInt(points: BigIntPoint[], scalars: bigint[], windowSize?)");
    return nullptr;
  }
  uint32_t np_ = 0, ns = 0;
  NAPI_OK(napi_get_array_length(env, argv[0], &np_));
  NAPI_OK(napi_get_array_length(env, argv[1], &ns));
  Job* j = new Job();
  if (!get_devices(env, argc, argv, 3, &j->devices) || !get_ratio(env, argc, argv, 4, &j->cpu_work_ratio)) {
    delete j;
    napi_throw_type_error(env, nullptr, "devices must be an array of device ordinals, cpuWorkRatio a number >= 0");
    return nullptr;
  }
  j->n = std::min(np_, ns);
  j->points.resize(j->n * 32);
  j->scalars.resize(j->n * 8);
  // The four property keys are made once per call (napi_get_named_property would create and
  // intern a string per coordinate: 4 n of them), and the element handles live in one handle
  // scope per block of points, so the handle stack stays small instead of growing by ~6 n handles.
  static const char* names[4] = {"x", "y", "t", "z"};
  napi_value keys[4];
  for (int k = 0; k < 4; k++)
    if (napi_create_string_utf8(env, names[k], 1, &keys[k]) != napi_ok) {
      delete j;
      napi_throw_error(env, nullptr, "cannot create the coordinate keys");
      return nullptr;
    }
  constexpr uint32_t BLOCK = 1024;
  const char* bad = nullptr;  // the error of the first bad element, thrown after its scope closes
  for (uint32_t i0 = 0; i0 < j->n && !bad; i0 += BLOCK) {
    napi_handle_scope scope;
    if (napi_open_handle_scope(env, &scope) != napi_ok) {
      bad = "bad input element";
      break;
    }
    const uint32_t i1 = std::min<uint32_t>(j->n, i0 + BLOCK);
    for (uint32_t i = i0; i < i1 && !bad; i++) {
      napi_value p, s;
      if (napi_get_element(env, argv[0], i, &p) != napi_ok || napi_get_element(env, argv[1], i, &s) != napi_ok) {
        bad = "bad input element";
        break;
      }
      for (int k = 0; k < 4 && !bad; k++) {
        napi_value c;
        if (napi_get_property(env, p, keys[k], &c) != napi_ok || !bigint_be(env, c, &j->points[i * 32 + 8 * k]))
          bad = "point coordinate must be a bigint in [0, 2^256)";
      }
      if (!bad && !bigint_be(env, s, &j->scalars[i * 8])) bad = "scalar must be a bigint in [0, 2^256)";
    }
    napi_close_handle_scope(env, scope);
  }
  if (bad) {
    delete j;
    bool pending = false;
    napi_is_exception_pending(env, &pending);  // a throwing getter: keep its exception
    if (!pending) {
      if (bad[0] == 'b') napi_throw_error(env, nullptr, bad);
      else napi_throw_range_error(env, nullptr, bad);
    }
    return nullptr;
  }
  j->window = argc > 2 ? get_window(env, argv[2]) : 0;
  return start_job(env, j);
}

napi_value make_u32(napi_env env, const uint32_t* src, size_t n) {
  napi_value ab, arr;
  void* buf;
  NAPI_OK(napi_create_arraybuffer(env, n * 4, &buf, &ab));
  if (n) memcpy(buf, src, n * 4);
  NAPI_OK(napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &arr));
  return arr;
}

napi_value throw_rc(napi_env env, int rc) {
  std::string m = std::string("libmsm: ") + msm_strerror(rc);
  napi_throw_error(env, std::to_string(rc).c_str(), m.c_str());
  return nullptr;
}

napi_value PointAddAffine(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint32_t *a, *b;
  size_t la, lb;
  if (argc < 2 || !get_u32_array(env, argv[0], &a, &la) || !get_u32_array(env, argv[1], &b, &lb) || la != 16 ||
      lb != 16) {
    napi_throw_type_error(env, nullptr, "pointAddAffine(a: Uint32Array(16), b: Uint32Array(16))");
    return nullptr;
  }
  uint32_t out[16];
  int rc = msm_point_add_affine(a, b, out);
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out, 16);
}

napi_value Split(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint32_t* sc;
  size_t len;
  uint32_t c = argc > 0 ? get_window(env, argv[0]) : 0;
  if (argc < 2 || !get_u32_array(env, argv[1], &sc, &len)) {
    napi_throw_type_error(env, nullptr, "split(windowSize, scalars: Uint32Array)");
    return nullptr;
  }
  size_t n = len / 8;
  uint32_t nw = msm_split_windows(c);
  std::vector<uint32_t> out((size_t)nw * n + 1);
  int rc = msm_split(c, sc, n, out.data());
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out.data(), (size_t)nw * n);
}

// flattenU32(points, scalars, pointWords, scalarWords): U32ArrayPoint[] / Uint32Array[] into flat
// wire buffers (x|y|t|z BE words per point, submission.ts:75-86), natively: per point one property
// read per coordinate (keys made once) and one typed-array lookup, then a 32-B copy.  The A/B
// against the JS loop (flattenU32 in submission.mjs) is tools/node_flatten_ab.mjs.
napi_value FlattenU32(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  if (argc < 4) {
    napi_throw_type_error(env, nullptr, "flattenU32(points, scalars, pointWords, scalarWords)");
    return nullptr;
  }
  uint32_t np_ = 0, ns = 0;
  NAPI_OK(napi_get_array_length(env, argv[0], &np_));
  NAPI_OK(napi_get_array_length(env, argv[1], &ns));
  const uint32_t n = std::min(np_, ns);
  const uint32_t *pwc = nullptr, *swc = nullptr;
  size_t plen = 0, slen = 0;
  if (!get_u32_array(env, argv[2], &pwc, &plen) || !get_u32_array(env, argv[3], &swc, &slen) ||
      plen < (size_t)n * 32 || slen < (size_t)n * 8) {
    napi_throw_type_error(env, nullptr, "pointWords / scalarWords must be Uint32Arrays of n x 32 / n x 8 words");
    return nullptr;
  }
  uint32_t* pw = const_cast<uint32_t*>(pwc);  // the caller's output buffers
  uint32_t* sw = const_cast<uint32_t*>(swc);
  static const char* names[4] = {"x", "y", "t", "z"};
  napi_value keys[4];
  for (int k = 0; k < 4; k++) NAPI_OK(napi_create_string_utf8(env, names[k], 1, &keys[k]));
  constexpr uint32_t BLOCK = 1024;
  const char* bad = nullptr;
  for (uint32_t i0 = 0; i0 < n && !bad; i0 += BLOCK) {
    napi_handle_scope scope;
    if (napi_open_handle_scope(env, &scope) != napi_ok) {
      bad = "bad input element";
      break;
    }
    const uint32_t i1 = std::min<uint32_t>(n, i0 + BLOCK);
    for (uint32_t i = i0; i < i1 && !bad; i++) {
      napi_value p, s;
      const uint32_t* src;
      size_t len;
      if (napi_get_element(env, argv[0], i, &p) != napi_ok || napi_get_element(env, argv[1], i, &s) != napi_ok) {
        bad = "bad input element";
        break;
      }
      for (int k = 0; k < 4 && !bad; k++) {
        napi_value c;
        if (napi_get_property(env, p, keys[k], &c) != napi_ok || !get_u32_array(env, c, &src, &len) || len < 8)
          bad = "point coordinates must be Uint32Arrays of 8 words";
        else
          memcpy(pw + (size_t)i * 32 + 8 * k, src, 32);
      }
      if (!bad) {
        if (!get_u32_array(env, s, &src, &len) || len < 8)
          bad = "scalars must be Uint32Arrays of 8 words";
        else
          memcpy(sw + (size_t)i * 8, src, 32);
      }
    }
    napi_close_handle_scope(env, scope);
  }
  if (bad) {
    bool pending = false;
    napi_is_exception_pending(env, &pending);
    if (!pending) napi_throw_type_error(env, nullptr, bad);
    return nullptr;
  }
  napi_value r;
  NAPI_OK(napi_create_uint32(env, n, &r));
  return r;
}

// ---- resident prepared bases ---------------------------------------------------------------------
const msm_bases* get_handle(napi_env env, napi_value v) {
  double id = 0;
  if (napi_get_value_double(env, v, &id) != napi_ok || !(id >= 1) || id > 9007199254740992.0) return nullptr;
  return reinterpret_cast<const msm_bases*>((uintptr_t)id);
}

napi_value bases_object(napi_env env, msm_bases* h);

// prepareBases(points, levels?, windowSize?, form?): with `form` (MSM_POINTS_X_*) the array holds
// compressed points, 8 words each, and y is recovered on the device (msm_bases_create_compressed).
napi_value PrepareBases(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint32_t* pts;
  size_t plen;
  if (argc < 1 || !get_u32_array(env, argv[0], &pts, &plen)) {
    napi_throw_type_error(env, nullptr, "prepareBases(points: Uint32Array, levels?, windowSize?, form?)");
    return nullptr;
  }
  const uint32_t form = argc > 3 ? get_window(env, argv[3]) : 0;
  msm_opts o;
  memset(&o, 0, sizeof(o));
  o.device = -1;
  o.window_bits = argc > 2 ? get_window(env, argv[2]) : 0;
  const uint32_t levels = argc > 1 ? get_window(env, argv[1]) : 0;
  msm_bases* h = nullptr;
  // synchronous: the points are read before this returns (upload and preparation, ~3 ms at 2^20)
  int rc = form ? msm_bases_create_compressed(pts, plen / 8, form, &o, levels, &h)
                : msm_bases_create(pts, plen / 32, &o, levels, &h);
  if (rc != MSM_OK) return throw_rc(env, rc);
  return bases_object(env, h);
}

// The object prepareBases and scaleBases hand out for a new handle: its id and what msm_bases_info says.
napi_value bases_object(napi_env env, msm_bases* h) {
  msm_bases_info_t inf;
  int rc = msm_bases_info(h, &inf);
  if (rc != MSM_OK) return throw_rc(env, rc);
  napi_value obj, v;
  NAPI_OK(napi_create_object(env, &obj));
  const struct {
    const char* name;
    double val;
  } fields[] = {{"id", (double)reinterpret_cast<uintptr_t>(h)}, {"n", (double)inf.n},
                {"levels", (double)inf.levels}, {"windowSize", (double)inf.window_bits},
                {"bytes", (double)inf.bytes}};
  for (const auto& f : fields) {
    NAPI_OK(napi_create_double(env, f.val, &v));
    NAPI_OK(napi_set_named_property(env, obj, f.name, v));
  }
  return obj;
}

// decompressPoints(xs: Uint32Array of n x 8 words, form) -> Uint32Array of n x 32 wire words
// (msm_decompress_points; synchronous, as prepareBases is).
napi_value DecompressPoints(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint32_t* xs;
  size_t len;
  if (argc < 2 || !get_u32_array(env, argv[0], &xs, &len)) {
    napi_throw_type_error(env, nullptr, "decompressPoints(xs: Uint32Array, form)");
    return nullptr;
  }
  const size_t n = len / 8;
  std::vector<uint32_t> out(n * 32 + 1);
  int rc = msm_decompress_points(xs, n, get_window(env, argv[1]), nullptr, out.data());
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out.data(), n * 32);
}

// scaleBases(id, scalars, first?, indices?, scalarBits?, asBases?, levels?, windowSize?): the per-point
// multiples s_i * P_i of a handle's bases (msm_bases_scale; synchronous, as prepareBases is) -- all of
// them, the range from `first`, or bases indices[i]; the scalar array gives m.  A Uint32Array of m x 32
// wire words, or with `asBases` the object of a new handle (msm_bases_scale_create).
napi_value ScaleBases(napi_env env, napi_callback_info info) {
  size_t argc = 8;
  napi_value argv[8];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  const bool has_first = given(2), has_idx = given(3), has_bits = given(4);
  const uint32_t* sc;
  const uint32_t* ix = nullptr;
  size_t slen, ilen = 0;
  double first = 0, bits = 0;
  bool as_bases = false;
  if (argc < 2 || !h || !get_u32_array(env, argv[1], &sc, &slen) ||
      (has_first && (napi_get_value_double(env, argv[2], &first) != napi_ok || !(first >= 0) ||
                     first > 9007199254740992.0 || first != (double)(uint64_t)first)) ||
      (has_idx && !get_u32_array(env, argv[3], &ix, &ilen)) ||
      (has_bits && (napi_get_value_double(env, argv[4], &bits) != napi_ok || bits != (double)(uint32_t)bits)) ||
      (given(5) && napi_get_value_bool(env, argv[5], &as_bases) != napi_ok)) {
    napi_throw_type_error(env, nullptr,
                          "scaleBases(id: number, scalars: Uint32Array, first?: number, indices?: Uint32Array, "
                          "scalarBits?: number, asBases?: boolean, levels?: number, windowSize?: number)");
    return nullptr;
  }
  if (has_bits && (bits < 1 || bits > 256)) return throw_rc(env, MSM_ERR_INVALID_ARG);
  const size_t sw = has_bits ? ((size_t)bits + 31) / 32 : 8;  // words per scalar
  const size_t m = slen / sw;
  if (has_idx && ilen != m) {
    napi_throw_range_error(env, nullptr, "one index per scalar");
    return nullptr;
  }
  msm_opts o;
  memset(&o, 0, sizeof(o));
  o.device = -1;
  o.window_bits = given(7) ? get_window(env, argv[7]) : 0;
  if (has_bits) {
    o.flags |= MSM_FLAG_SCALAR_BITS;
    o.scalar_bits = (uint32_t)bits;
  }
  msm_subset_t sub;
  sub.first = (uint64_t)first;
  sub.m = m;
  sub.indices = has_idx ? &ix : nullptr;
  if (as_bases) {
    msm_bases* nh = nullptr;
    int rc = msm_bases_scale_create(h, &sub, sc, &o, given(6) ? get_window(env, argv[6]) : 0, &nh);
    if (rc != MSM_OK) return throw_rc(env, rc);
    return bases_object(env, nh);
  }
  std::vector<uint32_t> out(m * 32 + 1);
  int rc = msm_bases_scale(h, &sub, sc, &o, out.data());
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out.data(), m * 32);
}

// combineBases(id, otherId?, a?, b?, aFirst, bFirst, aIndices?, bIndices?, m, flags, scalarBits?, keep?, levels?,
// windowSize?): the pairwise combinations a_i * A_i +- b_i * B_i of two subsets of one handle's bases or of
// two handles' (msm_bases_combine; synchronous, as prepareBases is).  `a` and `b` hold m scalars, or one with
// the side's broadcast flag, or are absent (the scalar 1).  A Uint32Array of m x 32 wire words, or with
// `keep` the object of a new handle (msm_bases_combine_create).
napi_value CombineBases(napi_env env, napi_callback_info info) {
  size_t argc = 14;
  napi_value argv[14];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  auto index_of = [&](size_t at, double* v) {  // a non-negative integer a double holds exactly
    return napi_get_value_double(env, argv[at], v) == napi_ok && *v >= 0 && *v <= 9007199254740992.0 &&
           *v == (double)(uint64_t)*v;
  };
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  const msm_bases* other = given(1) ? get_handle(env, argv[1]) : nullptr;
  const uint32_t* sc[2] = {nullptr, nullptr};
  const uint32_t* ix[2] = {nullptr, nullptr};
  size_t slen[2] = {0, 0}, ilen[2] = {0, 0};
  double first[2] = {0, 0}, m = 0, flags = 0, bits = 0;
  bool keep = false;
  const bool has_bits = given(10);
  bool ok = argc >= 10 && h && (!given(1) || other) && index_of(8, &m) && index_of(9, &flags) && flags < 8;
  for (int s = 0; ok && s < 2; s++) {
    if (given(2 + s)) ok = get_u32_array(env, argv[2 + s], &sc[s], &slen[s]);
    if (ok && given(4 + s)) ok = index_of(4 + s, &first[s]);
    if (ok && given(6 + s)) ok = get_u32_array(env, argv[6 + s], &ix[s], &ilen[s]);
  }
  if (ok && has_bits) ok = napi_get_value_double(env, argv[10], &bits) == napi_ok && bits == (double)(uint32_t)bits;
  if (ok && given(11)) ok = napi_get_value_bool(env, argv[11], &keep) == napi_ok;
  if (!ok) {
    napi_throw_type_error(env, nullptr,
                          "combineBases(id: number, otherId?: number, a?: Uint32Array, b?: Uint32Array, aFirst: number, "
                          "bFirst: number, aIndices?: Uint32Array, bIndices?: Uint32Array, m: number, flags: number, "
                          "scalarBits?: number, keep?: boolean, levels?: number, windowSize?: number)");
    return nullptr;
  }
  if (has_bits && (bits < 1 || bits > 256)) return throw_rc(env, MSM_ERR_INVALID_ARG);
  const size_t sw = has_bits ? ((size_t)bits + 31) / 32 : 8;  // words per scalar
  const uint32_t fl = (uint32_t)flags;
  for (int s = 0; s < 2; s++) {
    const bool bcast = fl & (s ? MSM_COMBINE_B_BROADCAST : MSM_COMBINE_A_BROADCAST);
    if ((sc[s] && slen[s] != (bcast ? 1 : (size_t)m) * sw) || (ix[s] && ilen[s] != (size_t)m)) {
      napi_throw_range_error(env, nullptr, "m scalars (one for a broadcast side) and m indices per side");
      return nullptr;
    }
  }
  msm_opts o;
  memset(&o, 0, sizeof(o));
  o.device = -1;
  o.window_bits = given(13) ? get_window(env, argv[13]) : 0;
  if (has_bits) {
    o.flags |= MSM_FLAG_SCALAR_BITS;
    o.scalar_bits = (uint32_t)bits;
  }
  msm_combine_t cb;
  memset(&cb, 0, sizeof(cb));
  cb.b_bases = other;
  cb.a.first = (uint64_t)first[0];
  cb.b.first = (uint64_t)first[1];
  cb.a.m = cb.b.m = (uint64_t)m;
  cb.a.indices = ix[0] ? &ix[0] : nullptr;
  cb.b.indices = ix[1] ? &ix[1] : nullptr;
  cb.a_scalars = sc[0];
  cb.b_scalars = sc[1];
  cb.flags = fl;
  if (keep) {
    msm_bases* nh = nullptr;
    int rc = msm_bases_combine_create(h, &cb, &o, given(12) ? get_window(env, argv[12]) : 0, &nh);
    if (rc != MSM_OK) return throw_rc(env, rc);
    return bases_object(env, nh);
  }
  std::vector<uint32_t> out((size_t)m * 32 + 1);
  int rc = msm_bases_combine(h, &cb, &o, out.data());
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out.data(), (size_t)m * 32);
}

// computeMsmPrepared(id, scalars[, first, indices]): with `first` (a number) or `indices` (a
// Uint32Array) the MSM runs over a subset of the handle's bases and the scalar array gives its
// length (msm_bases_compute_subset); with neither (absent or undefined) over all of them.  With
// `scalarBits` = b (1..256) the scalars are narrow: ceil(b / 32) words each (MSM_FLAG_SCALAR_BITS).
// With `scalarType` (a name of NATIVE_TYPES) the scalars are a typed array of that integer type as it is
// (MSM_FLAG_SCALAR_TYPE): its class must be the type's, scalarBits then bounds the magnitude, and a
// bitmap's term count is `count`, else the index list's length, the handle's n, or 8 per byte.
// A name of WIDE_TYPES declares little-endian 128- / 256-bit elements (MSM_FLAG_SCALAR_FIELD): a
// BigUint64Array, Uint32Array or Uint8Array of exactly the call's terms.
napi_value ComputeMsmPreparedTyped(napi_env env, size_t argc, napi_value* argv);
napi_value ComputeMsmPrepared(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  {
    napi_valuetype vt = napi_undefined;
    if (argc > 5 && napi_typeof(env, argv[5], &vt) == napi_ok && vt != napi_undefined && vt != napi_null)
      return ComputeMsmPreparedTyped(env, argc, argv);
  }
  const uint32_t* sc;
  size_t slen;
  bool sshared = false;
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  const bool has_first = given(2), has_idx = given(3), has_bits = given(4);
  double first = 0, bits = 0;
  const uint32_t* ix = nullptr;
  size_t ilen = 0;
  if (argc < 2 || !h || !get_u32_array(env, argv[1], &sc, &slen, &sshared) ||
      (has_first && (napi_get_value_double(env, argv[2], &first) != napi_ok || !(first >= 0) ||
                     first > 9007199254740992.0 || first != (double)(uint64_t)first)) ||
      (has_idx && !get_u32_array(env, argv[3], &ix, &ilen)) ||
      (has_bits && (napi_get_value_double(env, argv[4], &bits) != napi_ok || bits != (double)(uint32_t)bits))) {
    napi_throw_type_error(env, nullptr,
                          "computeMsmPrepared(id: number, scalars: Uint32Array, first?: number, indices?: Uint32Array, "
                          "scalarBits?: number)");
    return nullptr;
  }
  if (has_bits && (bits < 1 || bits > 256)) return throw_rc(env, MSM_ERR_INVALID_ARG);
  const size_t sw = has_bits ? ((size_t)bits + 31) / 32 : 8;  // words per scalar
  msm_bases_info_t inf;
  int rc = msm_bases_info(h, &inf);
  if (rc != MSM_OK) return throw_rc(env, rc);  // released, or never a handle
  const bool subset = has_first || has_idx;
  if (!subset && slen / sw < inf.n) {
    napi_throw_range_error(env, nullptr, "fewer scalars than the handle has points");
    return nullptr;
  }
  if (has_idx && ilen != slen / sw) {
    napi_throw_range_error(env, nullptr, "one index per scalar");
    return nullptr;
  }
  Job* j = new Job();
  j->bases = h;
  j->n = subset ? slen / sw : (size_t)inf.n;
  j->scalar_bits = has_bits ? (uint32_t)bits : 0;
  j->subset = subset;
  j->indexed = has_idx;
  j->first = (uint64_t)first;
  if (has_idx) j->indices.assign(ix, ix + ilen);  // the worker reads a copy, as it does the scalars'
  if (sshared) {
    j->p_scalars = sc;
    if (napi_create_reference(env, argv[1], 1, &j->ref_scalars) != napi_ok) {
      delete j;
      napi_throw_error(env, nullptr, "cannot reference the input array");
      return nullptr;
    }
  } else {  // detachable memory: the worker reads a copy
    j->scalars.resize(j->n * sw);
    copy_words(j->scalars.data(), sc, j->n * sw);
  }
  return start_job(env, j);
}

napi_value ComputeMsmPreparedTyped(napi_env env, size_t argc, napi_value* argv) {
  const msm_bases* h = get_handle(env, argv[0]);
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  const bool has_first = given(2), has_idx = given(3), has_bits = given(4), has_count = given(6);
  const WideType* wt = wide_type(env, argv[5]);
  const NativeType* ty = wt ? nullptr : native_type(env, argv[5]);
  double first = 0, bits = 0, count = 0;
  const void* sc = nullptr;
  const uint32_t* ix = nullptr;
  size_t slen = 0, ilen = 0, welem = 0;  // welem: bytes per element of a wide vector's array
  bool sshared = false;
  if (wt) {
    const struct { napi_typedarray_type cls; size_t bytes; } classes[] = {
        {napi_biguint64_array, 8}, {napi_uint32_array, 4}, {napi_uint8_array, 1}};
    for (const auto& k : classes)
      if (!welem && get_typed_array(env, argv[1], k.cls, &sc, &slen, &sshared)) welem = k.bytes;
  }
  if (!h || (!ty && !welem) || (ty && !get_typed_array(env, argv[1], ty->cls, &sc, &slen, &sshared)) ||
      (has_first && (napi_get_value_double(env, argv[2], &first) != napi_ok || !(first >= 0) ||
                     first > 9007199254740992.0 || first != (double)(uint64_t)first)) ||
      (has_idx && !get_u32_array(env, argv[3], &ix, &ilen)) ||
      (has_bits && (napi_get_value_double(env, argv[4], &bits) != napi_ok || bits != (double)(uint32_t)bits)) ||
      (has_count && (napi_get_value_double(env, argv[6], &count) != napi_ok || !(count >= 0) ||
                     count > 1073741824.0 || count != (double)(uint64_t)count))) {
    napi_throw_type_error(env, nullptr,
                          "computeMsmPrepared(id, scalars, first?, indices?, scalarBits?, scalarType, count?): scalars "
                          "must be the typed array of scalarType (Uint8Array for bit and u8, Int8Array .. "
                          "BigInt64Array / BigUint64Array for the rest; a BigUint64Array, Uint32Array or Uint8Array "
                          "for u128, i128, u256 and fr_mont)");
    return nullptr;
  }
  const uint32_t ebits = wt ? wt->bytes * 8 : ty->bits;
  if (has_bits && (bits < 1 || bits > ebits)) return throw_rc(env, MSM_ERR_INVALID_ARG);
  if (wt && (slen * welem) % wt->bytes) {
    napi_throw_range_error(env, nullptr, "the array is not a whole number of elements");
    return nullptr;
  }
  msm_bases_info_t inf;
  int rc = msm_bases_info(h, &inf);
  if (rc != MSM_OK) return throw_rc(env, rc);  // released, or never a handle
  const bool subset = has_first || has_idx;
  const size_t held = wt ? slen * welem / wt->bytes : ty->bits == 1 ? slen * 8 : slen;  // scalars the array can hold
  const size_t m = has_count ? (size_t)count : has_idx ? ilen : subset ? held : (size_t)inf.n;
  // (a wide vector holds exactly the call's terms: its length is the only count there is to check)
  if (m > held || (!subset && m < inf.n) || (wt && m != held)) {
    napi_throw_range_error(env, nullptr, "fewer scalars than the call has terms");
    return nullptr;
  }
  if (has_idx && ilen != m) {
    napi_throw_range_error(env, nullptr, "one index per scalar");
    return nullptr;
  }
  Job* j = new Job();
  j->bases = h;
  j->n = m;
  j->scalar_bits = has_bits ? (uint32_t)bits : 0;
  j->scalar_type = ty ? ty->type : 0;
  j->scalar_field = wt ? wt->field : 0;
  j->subset = subset;
  j->indexed = has_idx;
  j->first = (uint64_t)first;
  if (has_idx) j->indices.assign(ix, ix + ilen);
  // (a wide vector wants 8-byte alignment, which a Uint8Array view need not have: then a copy)
  if (sshared && !(wt && (reinterpret_cast<uintptr_t>(sc) & 7))) {
    j->p_scalars = static_cast<const uint32_t*>(sc);
    if (napi_create_reference(env, argv[1], 1, &j->ref_scalars) != napi_ok) {
      delete j;
      napi_throw_error(env, nullptr, "cannot reference the input array");
      return nullptr;
    }
  } else {  // detachable memory: the worker reads a copy (the vector's storage is aligned for any element)
    const size_t bytes = ((size_t)m * ebits + 7) / 8;
    j->scalars.resize((bytes + 3) / 4 + 1);
    memcpy(j->scalars.data(), sc, bytes);
  }
  return start_job(env, j);
}

napi_value ReleaseBases(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  napi_value r;
  NAPI_OK(napi_create_int32(env, h ? msm_bases_destroy(const_cast<msm_bases*>(h)) : MSM_ERR_INVALID_ARG, &r));
  return r;
}

// ---- fixed-base tables (msm_fixed_*) --------------------------------------------------------------
// prepareFixedBase(id, first?, count?, indices?, windowBits?, scalarBits?, vector?): the table of k <= 8
// bases of handle `id` -- or with `vector` of up to 4096 (msm_fixed_create_vector) -- all of them, the
// range [first, first + count), or bases indices[j] -- as an object of its token and what msm_fixed_info
// says.  Synchronous, as prepareBases is.
napi_value PrepareFixedBase(napi_env env, napi_callback_info info) {
  size_t argc = 7;
  napi_value argv[7];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  const bool has_range = given(1) || given(2), has_idx = given(3);
  const uint32_t* ix = nullptr;
  size_t ilen = 0;
  double first = 0, count = 0;
  auto whole = [](double v) { return v >= 0 && v <= 9007199254740992.0 && v == (double)(uint64_t)v; };
  bool vector = false;
  if (!h || (given(1) && (napi_get_value_double(env, argv[1], &first) != napi_ok || !whole(first))) ||
      (given(2) && (napi_get_value_double(env, argv[2], &count) != napi_ok || !whole(count))) ||
      (has_idx && !get_u32_array(env, argv[3], &ix, &ilen)) ||
      (given(6) && napi_get_value_bool(env, argv[6], &vector) != napi_ok)) {
    napi_throw_type_error(env, nullptr,
                          "prepareFixedBase(id: number, first?: number, count?: number, indices?: Uint32Array, "
                          "windowBits?: number, scalarBits?: number, vector?: boolean)");
    return nullptr;
  }
  msm_subset_t sub;
  sub.first = (uint64_t)first;
  sub.m = has_idx ? ilen : (uint64_t)count;
  sub.indices = has_idx ? &ix : nullptr;
  if (has_range && !given(2)) {  // from `first` to the handle's end
    msm_bases_info_t inf;
    int rc = msm_bases_info(h, &inf);
    if (rc != MSM_OK) return throw_rc(env, rc);
    sub.m = inf.n > sub.first ? inf.n - sub.first : 0;
  }
  msm_fixed* t = nullptr;
  int rc = (vector ? msm_fixed_create_vector : msm_fixed_create)(
      h, has_range || has_idx ? &sub : nullptr, given(4) ? get_window(env, argv[4]) : 0,
      given(5) ? get_window(env, argv[5]) : 0, nullptr, &t);
  if (rc != MSM_OK) return throw_rc(env, rc);
  msm_fixed_info_t inf;
  if ((rc = msm_fixed_info(t, &inf)) != MSM_OK) return throw_rc(env, rc);
  napi_value obj, v;
  NAPI_OK(napi_create_object(env, &obj));
  const struct {
    const char* name;
    double val;
  } fields[] = {{"id", (double)reinterpret_cast<uintptr_t>(t)}, {"bases", (double)inf.bases},
                {"windowBits", (double)inf.window_bits}, {"scalarBits", (double)inf.scalar_bits},
                {"windows", (double)inf.windows}, {"records", (double)inf.records}, {"bytes", (double)inf.bytes}};
  for (const auto& f : fields) {
    NAPI_OK(napi_create_double(env, f.val, &v));
    NAPI_OK(napi_set_named_property(env, obj, f.name, v));
  }
  return obj;
}

// fixedBaseMul(id, scalars, scalarBits?, asBases?, levels?, windowSize?): sum_j s_ij * B_j for the m
// rows of one scalar per base of the table (msm_fixed_info) in the array (msm_fixed_mul; synchronous): a Uint32Array of m x 32 wire
// words, or with `asBases` the object of a new handle (msm_fixed_mul_create).
napi_value FixedBaseMul(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  auto given = [&](size_t at) {
    napi_valuetype vt = napi_undefined;
    return argc > at && napi_typeof(env, argv[at], &vt) == napi_ok && vt != napi_undefined && vt != napi_null;
  };
  const msm_fixed* t = argc > 0 ? reinterpret_cast<const msm_fixed*>(get_handle(env, argv[0])) : nullptr;
  const bool has_bits = given(2);
  const uint32_t* sc;
  size_t slen;
  double bits = 0;
  bool as_bases = false;
  if (argc < 2 || !t || !get_u32_array(env, argv[1], &sc, &slen) ||
      (has_bits && (napi_get_value_double(env, argv[2], &bits) != napi_ok || bits != (double)(uint32_t)bits)) ||
      (given(3) && napi_get_value_bool(env, argv[3], &as_bases) != napi_ok)) {
    napi_throw_type_error(env, nullptr,
                          "fixedBaseMul(id: number, scalars: Uint32Array, scalarBits?: number, asBases?: boolean, "
                          "levels?: number, windowSize?: number)");
    return nullptr;
  }
  if (has_bits && (bits < 1 || bits > 256)) return throw_rc(env, MSM_ERR_INVALID_ARG);
  // the row length is the table's own base count: the library reads m * k * sw words
  msm_fixed_info_t inf;
  if (int irc = msm_fixed_info(t, &inf)) return throw_rc(env, irc);  // released, or never a table
  const size_t sw = has_bits ? ((size_t)bits + 31) / 32 : 8;  // words per scalar
  const size_t row = sw * inf.bases;
  if (slen % row) {
    napi_throw_range_error(env, nullptr, "the scalars are no whole rows of one per base");
    return nullptr;
  }
  const size_t m = slen / row;
  msm_opts o;
  memset(&o, 0, sizeof(o));
  o.device = -1;
  o.window_bits = given(5) ? get_window(env, argv[5]) : 0;
  if (has_bits) {
    o.flags |= MSM_FLAG_SCALAR_BITS;
    o.scalar_bits = (uint32_t)bits;
  }
  if (as_bases) {
    msm_bases* nh = nullptr;
    int rc = msm_fixed_mul_create(t, sc, m, &o, given(4) ? get_window(env, argv[4]) : 0, &nh);
    if (rc != MSM_OK) return throw_rc(env, rc);
    return bases_object(env, nh);
  }
  std::vector<uint32_t> out(m * 32 + 1);
  int rc = msm_fixed_mul(t, sc, m, &o, out.data());
  if (rc != MSM_OK) return throw_rc(env, rc);
  return make_u32(env, out.data(), m * 32);
}

napi_value ReleaseFixedBase(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const msm_bases* h = argc > 0 ? get_handle(env, argv[0]) : nullptr;
  napi_value r;
  NAPI_OK(napi_create_int32(
      env, h ? msm_fixed_destroy(reinterpret_cast<msm_fixed*>(const_cast<msm_bases*>(h))) : MSM_ERR_INVALID_ARG, &r));
  return r;
}

napi_value BestWindowSize(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  double n = 0;
  if (argc > 0) napi_get_value_double(env, argv[0], &n);
  napi_value r;
  NAPI_OK(napi_create_uint32(env, msm_best_window((size_t)n), &r));
  return r;
}

napi_value Init(napi_env env, napi_callback_info) {
  napi_value r;
  NAPI_OK(napi_create_int32(env, msm_init(), &r));
  return r;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
  napi_value r;
  NAPI_OK(napi_create_int32(env, msm_device_count(), &r));
  return r;
}

// HIP ordinals of the gfx950 devices (the values a `devices` list takes).
napi_value DeviceOrdinals(napi_env env, napi_callback_info) {
  napi_value arr;
  const int n = msm_device_count();
  NAPI_OK(napi_create_array_with_length(env, n > 0 ? n : 0, &arr));
  for (int i = 0; i < n; i++) {
    napi_value v;
    NAPI_OK(napi_create_int32(env, msm_device_ordinal(i), &v));
    NAPI_OK(napi_set_element(env, arr, i, v));
  }
  return arr;
}

napi_value StrError(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  int32_t code = 0;
  if (argc > 0) napi_get_value_int32(env, argv[0], &code);
  napi_value r;
  NAPI_OK(napi_create_string_utf8(env, msm_strerror(code), NAPI_AUTO_LENGTH, &r));
  return r;
}

// Explicit teardown when the last environment that loaded the addon is torn down (process exit
// of the main thread, or the last worker): the library's streams, buffers and parked pool threads
// are released and joined then, not left to the shared objects' finalizers.  (A call in flight
// holds its device context, which msm_shutdown waits for.)
std::atomic<int> g_envs{0};
void CleanupEnv(void*) {
  if (g_envs.fetch_sub(1) == 1) msm_shutdown();
}

napi_value ModuleInit(napi_env env, napi_value exports) {
  if (napi_add_env_cleanup_hook(env, CleanupEnv, nullptr) == napi_ok) g_envs.fetch_add(1);
  napi_property_descriptor props[] = {
      {"computeMsmU32", nullptr, ComputeMsmU32, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"computeMsmBigInt", nullptr, ComputeMsmBigInt, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"pointAddAffine", nullptr, PointAddAffine, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"split", nullptr, Split, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"flattenU32", nullptr, FlattenU32, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"bestWindowSize", nullptr, BestWindowSize, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"init", nullptr, Init, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"deviceOrdinals", nullptr, DeviceOrdinals, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"strerror", nullptr, StrError, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
      {"prepareBases", nullptr, PrepareBases, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"computeMsmPrepared", nullptr, ComputeMsmPrepared, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"releaseBases", nullptr, ReleaseBases, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"decompressPoints", nullptr, DecompressPoints, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"scaleBases", nullptr, ScaleBases, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"combineBases", nullptr, CombineBases, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"prepareFixedBase", nullptr, PrepareFixedBase, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fixedBaseMul", nullptr, FixedBaseMul, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"releaseFixedBase", nullptr, ReleaseFixedBase, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, ModuleInit)
