// libmsm host driver: C ABI (include/msm.h), device workspaces, launch sequence, host tail.
//
// The reference's host orchestration this replaces:
//   compute_msm            src/submission/submission.ts:25-157   -> msm_compute / msm_compute_device
//   getBestWindowSize      submission.ts:18-23                    -> msm_best_window
//   gpuIntraBucketReduction src/submission/gpu.ts:36-285          -> k_prepare_points .. k_lead_scan
//     (its staging ring, gpu.ts:146-155 / 244-271)                -> the packed pinned ring (PinRing,
//                                                                    PackPool) and the uploader thread
//   split_dynamic          msm-wasm/src/lib.rs:196-202            -> msm_split (host) / k_recode_* (device)
//   inter_bucket_reduce    lib.rs:46-56, 123-133                  -> k_bucket_reduce_1, k_red2_groups / _terms
//   reduce_last            lib.rs:88-104                          -> horner_tail (host)
//   point_add_affine       lib.rs:240-253                         -> msm_point_add_affine
//   msm_end_to_end         lib.rs:24-44, 106-121                  -> msm_compute_cpu (msm_cpu.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <immintrin.h>

#include "../../include/msm.h"
#include "hostfield.h"
#include "msm_cpu.h"
#include "msm_util.h"
#include "msm_kernels.hip"

using namespace msm;
using namespace msmh;

// The host driver's layers, in order: each header uses only the ones before it.  All of it is this file's
// one anonymous namespace (opened here, so the headers hold plain definitions); the test hooks come last
// and open their own `extern "C"` block.
namespace {
#include "host_knobs.h"
#include "host_ctx.h"
#include "host_guard.h"
#include "host_plan.h"
#include "host_tail.h"
#include "host_launch.h"
#include "host_upload.h"
#include "host_single.h"
#include "host_pipeline.h"
#include "host_split.h"
#include "host_multi.h"
#include "host_bases.h"
#include "host_fixed.h"
#include "host_combine.h"
#include "host_fr.h"
#include "host_fr_scan.h"
}  // namespace
#include "host_test_hooks.h"

extern "C" {

int msm_init(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return probe_devices() > 0 ? MSM_OK : MSM_ERR_NO_DEVICE;
}

void msm_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (DevCtx* c : g_ctx) {
    if (!c) continue;
    std::lock_guard<std::mutex> lk2(c->mu);
    c->destroy();  // the records of every handle on the device with it
  }
  for (DevCtx*& c : g_ctx) {
    delete c;
    c = nullptr;
  }
  g_bases.clear();  // every handle was freed with its device context above
  g_fixed.clear();  // and every fixed-base table
  std::lock_guard<std::mutex> lk3(g_test_mu);
  g_test_pools.stop();
}

int msm_device_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return probe_devices();
}

int msm_device_ordinal(int index) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int n = probe_devices();
  return index >= 0 && index < n ? g_gfx950[index] : -1;
}

const char* msm_strerror(int code) {
  switch (code) {
    case MSM_OK: return "ok";
    case MSM_ERR_INVALID_ARG: return "invalid argument";
    case MSM_ERR_UNSUPPORTED_WINDOW: return "unsupported window size";
    case MSM_ERR_COORD_RANGE: return "coordinate not in [0, p)";
    case MSM_ERR_BAD_POINT: return "invalid point (z == 0, or a compressed x of no such point)";
    case MSM_ERR_HIP: return "HIP runtime error";
    case MSM_ERR_NO_DEVICE: return "no gfx950 (MI355X) device available";
    case MSM_ERR_OOM: return "device out of memory";
    default: return "unknown error";
  }
}

uint32_t msm_best_window(size_t n) {
  // Measured on MI355X (tools/window_sweep.sh, balanced windows): c = 16 is fastest from 2^16 to
  // 2^20 -- the bucket reduction is latency-bound, so its cost hardly grows with 2^c, while
  // every extra window adds n entries and narrow windows make dense, chained buckets.  Below
  // that, keep ~8+ entries per bucket; the bucket tables (W * 2^(c-1) points) shrink with c.
  if (n >= (1u << 15)) return 16;
  uint32_t c = 8;
  while (c < 16 && (size_t)(1u << (c + 3)) <= n) c++;
  return c;
}

int msm_compute(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                uint32_t out_xy_be[16]) {
  if (!out_xy_be) return MSM_ERR_INVALID_ARG;
  Pt r;
  int rc = multi_host_entry(points_be, scalars_be, n, opts, &r);
  if (rc != MSM_OK) return rc;
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

// CPU/GPU co-compute (submission.ts:94-154): the host Pippenger (msm_cpu.h) takes points
// [0, share) on a thread of its own while the device path runs [share, n) as msm_compute, and the
// two affine results join with one EC add (point_add_affine, lib.rs:240-253).
int msm_compute_cocompute(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                          double cpu_work_ratio, int cpu_threads, uint32_t out_xy_be[16]) {
  if (!out_xy_be || ((!points_be || !scalars_be) && n) || !(cpu_work_ratio >= 0.0)) return MSM_ERR_INVALID_ARG;
  // a window range has no CPU counterpart (the host Pippenger computes every window): joining a
  // range's GPU share with a whole CPU share would be silently wrong
  if (opts && (opts->flags & (MSM_FLAG_WINDOWS | MSM_FLAG_SCALAR_BITS | MSM_FLAG_SCALAR_TYPE | MSM_FLAG_SCALAR_FIELD)))
    return MSM_ERR_INVALID_ARG;
  // cpuShare = floor(cpuWorkRatio * n) (submission.ts:98); >= n is the reference's CPU-only branch
  const double share_d = cpu_work_ratio * (double)n;
  const size_t share = share_d >= (double)n ? n : (size_t)share_d;
  if (share == 0) return msm_compute(points_be, scalars_be, n, opts, out_xy_be);
  int rc = msm_init();  // a device entry all the same: no gfx950, no result (the CPU-only entry is msm_compute_cpu)
  if (rc != MSM_OK) return rc;
  uint32_t cpu_xy[16];
  int cpu_rc = MSM_OK;
  std::thread cpu([&] { cpu_rc = cpu_msm(points_be, scalars_be, share, 0, cpu_threads, cpu_xy); });
  Pt r = pt_identity();
  if (share < n) rc = multi_host_entry(points_be + 32 * share, scalars_be + 8 * share, n - share, opts, &r);
  cpu.join();
  if (rc != MSM_OK) return rc;
  if (cpu_rc != MSM_OK) return cpu_rc;
  uint64_t x[4], y[4];
  be_words_to_std(cpu_xy, x);
  be_words_to_std(cpu_xy + 8, y);
  r = pt_add(r, pt_from_affine_std(x, y));
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

int msm_compute_partial(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                        uint32_t out_xyzt_be[32]) {
  if (!out_xyzt_be) return MSM_ERR_INVALID_ARG;
  Pt r;
  int rc = multi_host_entry(points_be, scalars_be, n, opts, &r);
  if (rc != MSM_OK) return rc;
  pt_to_be_xyzt(r, out_xyzt_be);
  return MSM_OK;
}

int msm_compute_device(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, const msm_opts* opts,
                       void* hip_stream, uint32_t out_xy_be[16]) {
  if (!out_xy_be) return MSM_ERR_INVALID_ARG;
  Pt r;
  int rc = multi_device_entry(d_points_be, d_scalars_be, n, opts, hip_stream, &r);
  if (rc != MSM_OK) return rc;
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

int msm_compute_device_partial(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n,
                               const msm_opts* opts, void* hip_stream, uint32_t out_xyzt_be[32]) {
  if (!out_xyzt_be) return MSM_ERR_INVALID_ARG;
  Pt r;
  int rc = multi_device_entry(d_points_be, d_scalars_be, n, opts, hip_stream, &r);
  if (rc != MSM_OK) return rc;
  pt_to_be_xyzt(r, out_xyzt_be);
  return MSM_OK;
}

int msm_compute_many_device(const uint32_t* const* d_points_be, const uint32_t* const* d_scalars_be, size_t n,
                            size_t count, const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be) {
  ManyInputs in;
  in.points = d_points_be;
  in.scalars = d_scalars_be;
  return multi_many_entry(in, n, count, opts, hip_stream, out_xy_be, false);
}

int msm_compute_many_device_partial(const uint32_t* const* d_points_be, const uint32_t* const* d_scalars_be,
                                    size_t n, size_t count, const msm_opts* opts, void* hip_stream,
                                    uint32_t* out_xyzt_be) {
  ManyInputs in;
  in.points = d_points_be;
  in.scalars = d_scalars_be;
  return multi_many_entry(in, n, count, opts, hip_stream, out_xyzt_be, true);
}

int msm_compute_batch_device(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, size_t count,
                             const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be) {
  if (!out_xy_be || ((!d_points_be || !d_scalars_be) && n && count)) return MSM_ERR_INVALID_ARG;
  std::vector<const uint32_t*> pp(count), ss(count);
  for (size_t b = 0; b < count; b++) {
    pp[b] = d_points_be + b * n * 32;
    ss[b] = d_scalars_be + b * n * 8;
  }
  return msm_compute_many_device(pp.data(), ss.data(), n, count, opts, hip_stream, out_xy_be);
}

int msm_compute_shared_device(const uint32_t* d_points_be, const uint32_t* const* d_scalars_be, size_t n,
                              size_t count, const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be) {
  if (!d_points_be && n && count) return MSM_ERR_INVALID_ARG;
  ManyInputs in;
  in.shared_points = d_points_be;
  in.scalars = d_scalars_be;
  if (!n) in.points = d_scalars_be;  // n = 0: identities, no input is read
  return multi_many_entry(in, n, count, opts, hip_stream, out_xy_be, false);
}

int msm_compute_many(const uint32_t* const* points_be, const uint32_t* const* scalars_be, size_t n, size_t count,
                     const msm_opts* opts, uint32_t* out_xy_be) {
  ManyInputs in;
  in.kind = ManyInputs::HOST;
  in.points = points_be;
  in.scalars = scalars_be;
  in.packed = host_pack();  // x|y (x|y|z) through the pinned ring into the slots' wire buffers
  return multi_many_entry(in, n, count, opts, nullptr, out_xy_be, false);
}

int msm_compute_shared(const uint32_t* points_be, const uint32_t* const* scalars_be, size_t n, size_t count,
                       const msm_opts* opts, uint32_t* out_xy_be) {
  if (!points_be && n && count) return MSM_ERR_INVALID_ARG;
  ManyInputs in;
  in.kind = ManyInputs::HOST;
  in.shared_points = points_be;
  in.scalars = scalars_be;
  if (!n) in.points = scalars_be;
  return multi_many_entry(in, n, count, opts, nullptr, out_xy_be, false);
}

int msm_bases_create(const uint32_t* points_be, size_t n, const msm_opts* opts, uint32_t levels, msm_bases** out) {
  return create_bases(points_be, true, n, 0, opts, levels, nullptr, out);
}

int msm_bases_create_device(const uint32_t* d_points_be, size_t n, const msm_opts* opts, uint32_t levels,
                            void* hip_stream, msm_bases** out) {
  return create_bases(d_points_be, false, n, 0, opts, levels, (hipStream_t)hip_stream, out);
}

int msm_bases_create_compressed(const uint32_t* xs_be, size_t n, uint32_t form, const msm_opts* opts, uint32_t levels,
                                msm_bases** out) {
  if (out) *out = nullptr;
  if (!points_form_ok(form)) return MSM_ERR_INVALID_ARG;
  return create_bases(xs_be, true, n, form, opts, levels, nullptr, out);
}

int msm_bases_create_compressed_device(const uint32_t* d_xs_be, size_t n, uint32_t form, const msm_opts* opts,
                                       uint32_t levels, void* hip_stream, msm_bases** out) {
  if (out) *out = nullptr;
  if (!points_form_ok(form)) return MSM_ERR_INVALID_ARG;
  return create_bases(d_xs_be, false, n, form, opts, levels, (hipStream_t)hip_stream, out);
}

int msm_decompress_points(const uint32_t* xs_be, size_t n, uint32_t form, const msm_opts* opts, uint32_t* points_be) {
  return decompress_points(xs_be, true, n, form, opts, nullptr, points_be);
}

int msm_decompress_points_device(const uint32_t* d_xs_be, size_t n, uint32_t form, const msm_opts* opts,
                                 void* hip_stream, uint32_t* d_points_be) {
  return decompress_points(d_xs_be, false, n, form, opts, (hipStream_t)hip_stream, d_points_be);
}

int msm_compress_points(const uint32_t* xy_be, size_t n, uint32_t form, uint32_t* xs_be) {
  return compress_points(xy_be, n, form, xs_be);
}

int msm_bases_destroy(msm_bases* h) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_bases.find(reinterpret_cast<uintptr_t>(h));
  if (!h || it == g_bases.end()) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = it->second;
  g_bases.erase(it);
  // under the device context's lock: a compute call on this handle has returned, or will find it dead
  DevCtx* c = b->device >= 0 && b->device < (int)g_ctx.size() ? g_ctx[b->device] : nullptr;
  if (c) {
    std::lock_guard<std::mutex> lk2(c->mu);
    DeviceGuard g(c->device);
    b->alive = false;
    b->rec.release();
  } else {
    b->alive = false;
  }
  return MSM_OK;
}

int msm_bases_info(const msm_bases* h, msm_bases_info_t* out) {
  if (!h || !out) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = find_bases(h);
  if (!b) return MSM_ERR_INVALID_ARG;
  *out = msm_bases_info_t{};
  out->n = b->n;
  out->levels = b->levels;
  out->window_bits = b->window_bits;
  out->chunk_bits = b->levels > 1 ? b->geo.S : 0;
  out->windows = b->levels > 1 ? b->geo.Wc : 0;
  out->device = b->device;
  out->bytes = (uint64_t)b->levels * b->n * PRE_WORDS * 4;
  return MSM_OK;
}

int msm_bases_compute(const msm_bases* h, const uint32_t* scalars_be, const msm_opts* opts, uint32_t out_xy_be[16]) {
  return bases_compute(h, &scalars_be, true, 1, opts, nullptr, out_xy_be);
}

int msm_bases_compute_device(const msm_bases* h, const uint32_t* d_scalars_be, const msm_opts* opts,
                             void* hip_stream, uint32_t out_xy_be[16]) {
  return bases_compute(h, &d_scalars_be, false, 1, opts, hip_stream, out_xy_be);
}

int msm_bases_compute_many(const msm_bases* h, const uint32_t* const* scalars_be, size_t count, const msm_opts* opts,
                           uint32_t* out_xy_be) {
  return bases_compute(h, scalars_be, true, count, opts, nullptr, out_xy_be);
}

int msm_bases_compute_subset(const msm_bases* h, const msm_subset_t* sub, const uint32_t* scalars_be,
                             const msm_opts* opts, uint32_t out_xy_be[16]) {
  return bases_compute(h, &scalars_be, true, 1, opts, nullptr, out_xy_be, sub, true);
}

int msm_bases_compute_subset_device(const msm_bases* h, const msm_subset_t* sub, const uint32_t* d_scalars_be,
                                    const msm_opts* opts, void* hip_stream, uint32_t out_xy_be[16]) {
  return bases_compute(h, &d_scalars_be, false, 1, opts, hip_stream, out_xy_be, sub, true);
}

int msm_bases_compute_subset_many(const msm_bases* h, const msm_subset_t* sub, const uint32_t* const* scalars_be,
                                  size_t count, const msm_opts* opts, uint32_t* out_xy_be) {
  return bases_compute(h, scalars_be, true, count, opts, nullptr, out_xy_be, sub, true);
}

int msm_bases_compute_subset_many_device(const msm_bases* h, const msm_subset_t* sub,
                                         const uint32_t* const* d_scalars_be, size_t count, const msm_opts* opts,
                                         void* hip_stream, uint32_t* out_xy_be) {
  return bases_compute(h, d_scalars_be, false, count, opts, hip_stream, out_xy_be, sub, true);
}

int msm_bases_compute_many_device(const msm_bases* h, const uint32_t* const* d_scalars_be, size_t count,
                                  const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be) {
  return bases_compute(h, d_scalars_be, false, count, opts, hip_stream, out_xy_be);
}

int msm_bases_scale(const msm_bases* h, const msm_subset_t* sub, const uint32_t* scalars_be, const msm_opts* opts,
                    uint32_t* points_be) {
  return bases_scale(h, sub, scalars_be, true, opts, nullptr, points_be, 0, nullptr);
}

int msm_bases_scale_device(const msm_bases* h, const msm_subset_t* sub, const uint32_t* d_scalars_be,
                           const msm_opts* opts, void* hip_stream, uint32_t* d_points_be) {
  return bases_scale(h, sub, d_scalars_be, false, opts, (hipStream_t)hip_stream, d_points_be, 0, nullptr);
}

int msm_bases_scale_create(const msm_bases* h, const msm_subset_t* sub, const uint32_t* scalars_be,
                           const msm_opts* opts, uint32_t levels, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return bases_scale(h, sub, scalars_be, true, opts, nullptr, nullptr, levels, out);
}

int msm_bases_scale_create_device(const msm_bases* h, const msm_subset_t* sub, const uint32_t* d_scalars_be,
                                  const msm_opts* opts, uint32_t levels, void* hip_stream, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return bases_scale(h, sub, d_scalars_be, false, opts, (hipStream_t)hip_stream, nullptr, levels, out);
}

int msm_bases_combine(const msm_bases* h, const msm_combine_t* combine, const msm_opts* opts, uint32_t* points_be) {
  return bases_combine(h, combine, true, opts, nullptr, points_be, 0, nullptr);
}

int msm_bases_combine_device(const msm_bases* h, const msm_combine_t* combine, const msm_opts* opts, void* hip_stream,
                             uint32_t* d_points_be) {
  return bases_combine(h, combine, false, opts, (hipStream_t)hip_stream, d_points_be, 0, nullptr);
}

int msm_bases_combine_create(const msm_bases* h, const msm_combine_t* combine, const msm_opts* opts, uint32_t levels,
                             msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return bases_combine(h, combine, true, opts, nullptr, nullptr, levels, out);
}

int msm_bases_combine_create_device(const msm_bases* h, const msm_combine_t* combine, const msm_opts* opts,
                                    uint32_t levels, void* hip_stream, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return bases_combine(h, combine, false, opts, (hipStream_t)hip_stream, nullptr, levels, out);
}

int msm_fixed_create(const msm_bases* h, const msm_subset_t* sub, uint32_t window_bits, uint32_t scalar_bits,
                     const msm_opts* opts, msm_fixed** out) {
  return fixed_create(h, sub, window_bits, scalar_bits, opts, out);
}

int msm_fixed_create_vector(const msm_bases* h, const msm_subset_t* sub, uint32_t window_bits, uint32_t scalar_bits,
                            const msm_opts* opts, msm_fixed** out) {
  return fixed_create(h, sub, window_bits, scalar_bits, opts, out, true);
}

int msm_fixed_destroy(msm_fixed* h) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_fixed.find(reinterpret_cast<uintptr_t>(h));
  if (!h || it == g_fixed.end()) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Fixed> t = it->second;
  g_fixed.erase(it);
  // under the device context's lock, as msm_bases_destroy
  DevCtx* c = t->device >= 0 && t->device < (int)g_ctx.size() ? g_ctx[t->device] : nullptr;
  if (c) {
    std::lock_guard<std::mutex> lk2(c->mu);
    DeviceGuard g(c->device);
    t->alive = false;
    t->rec.release();
  } else {
    t->alive = false;
  }
  return MSM_OK;
}

int msm_fixed_info(const msm_fixed* h, msm_fixed_info_t* out) {
  if (!h || !out) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Fixed> t = find_fixed(h);
  if (!t) return MSM_ERR_INVALID_ARG;
  *out = msm_fixed_info_t{};
  out->bases = t->k;
  out->window_bits = t->w;
  out->scalar_bits = t->b;
  out->windows = t->Wn;
  out->records = t->records();
  out->bytes = (uint64_t)t->records() * PRE_WORDS * 4;
  out->device = t->device;
  return MSM_OK;
}

int msm_fixed_mul(const msm_fixed* h, const uint32_t* scalars_be, size_t m, const msm_opts* opts, uint32_t* points_be) {
  return fixed_mul(h, scalars_be, m, true, opts, nullptr, points_be, 0, nullptr);
}

int msm_fixed_mul_device(const msm_fixed* h, const uint32_t* d_scalars_be, size_t m, const msm_opts* opts,
                         void* hip_stream, uint32_t* d_points_be) {
  return fixed_mul(h, d_scalars_be, m, false, opts, (hipStream_t)hip_stream, d_points_be, 0, nullptr);
}

int msm_fixed_mul_create(const msm_fixed* h, const uint32_t* scalars_be, size_t m, const msm_opts* opts,
                         uint32_t levels, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return fixed_mul(h, scalars_be, m, true, opts, nullptr, nullptr, levels, out);
}

int msm_fixed_mul_create_device(const msm_fixed* h, const uint32_t* d_scalars_be, size_t m, const msm_opts* opts,
                                uint32_t levels, void* hip_stream, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  return fixed_mul(h, d_scalars_be, m, false, opts, (hipStream_t)hip_stream, nullptr, levels, out);
}

int msm_fr_combine(const msm_fr_combine_t* combine, size_t m, const msm_opts* opts, uint32_t* out) {
  return fr_combine(combine, m, true, opts, nullptr, out);
}

int msm_fr_combine_device(const msm_fr_combine_t* combine, size_t m, const msm_opts* opts, void* hip_stream,
                          uint32_t* d_out) {
  return fr_combine(combine, m, false, opts, (hipStream_t)hip_stream, d_out);
}

int msm_fr_powers(const uint32_t g_be[8], const uint32_t* c_be, size_t n, uint32_t out_form, const msm_opts* opts,
                  uint32_t* out) {
  return fr_powers(g_be, c_be, n, out_form, true, opts, nullptr, out);
}

int msm_fr_powers_device(const uint32_t g_be[8], const uint32_t* c_be, size_t n, uint32_t out_form, const msm_opts* opts,
                         void* hip_stream, uint32_t* d_out) {
  return fr_powers(g_be, c_be, n, out_form, false, opts, (hipStream_t)hip_stream, d_out);
}

int msm_fr_dot(const uint32_t* a, const uint32_t* b, size_t n, uint32_t in_form, uint32_t out_form, const msm_opts* opts,
               uint32_t out[8]) {
  return fr_dot(a, b, n, in_form, out_form, true, opts, nullptr, out);
}

int msm_fr_dot_device(const uint32_t* d_a, const uint32_t* d_b, size_t n, uint32_t in_form, uint32_t out_form,
                      const msm_opts* opts, void* hip_stream, uint32_t out[8]) {
  return fr_dot(d_a, d_b, n, in_form, out_form, false, opts, (hipStream_t)hip_stream, out);
}

int msm_fr_inverse(const uint32_t* a, const uint32_t* c_be, size_t m, uint32_t in_form, uint32_t out_form,
                   const msm_opts* opts, uint32_t* out) {
  return fr_inverse(a, c_be, m, in_form, out_form, true, opts, nullptr, out);
}

int msm_fr_inverse_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t in_form, uint32_t out_form,
                          const msm_opts* opts, void* hip_stream, uint32_t* d_out) {
  return fr_inverse(d_a, c_be, m, in_form, out_form, false, opts, (hipStream_t)hip_stream, d_out);
}

int msm_fr_scan(const uint32_t* a, const uint32_t* c_be, size_t m, uint32_t flags, uint32_t in_form, uint32_t out_form,
                const msm_opts* opts, uint32_t* out) {
  return fr_scan(a, c_be, m, flags, in_form, out_form, true, opts, nullptr, out);
}

int msm_fr_scan_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t flags, uint32_t in_form,
                       uint32_t out_form, const msm_opts* opts, void* hip_stream, uint32_t* d_out) {
  return fr_scan(d_a, c_be, m, flags, in_form, out_form, false, opts, (hipStream_t)hip_stream, d_out);
}

int msm_fr_tensor(const uint32_t* lo_be, const uint32_t* hi_be, uint32_t k, const uint32_t* c_be, uint32_t out_form,
                  const msm_opts* opts, uint32_t* out) {
  return fr_tensor(lo_be, hi_be, k, c_be, out_form, true, opts, nullptr, out);
}

int msm_fr_tensor_device(const uint32_t* lo_be, const uint32_t* hi_be, uint32_t k, const uint32_t* c_be, uint32_t out_form,
                         const msm_opts* opts, void* hip_stream, uint32_t* d_out) {
  return fr_tensor(lo_be, hi_be, k, c_be, out_form, false, opts, (hipStream_t)hip_stream, d_out);
}

int msm_combine_partials(const uint32_t* partials_xyzt_be, size_t count, uint32_t out_xy_be[16]) {
  if ((!partials_xyzt_be && count) || !out_xy_be) return MSM_ERR_INVALID_ARG;
  Pt acc = pt_identity();
  for (size_t i = 0; i < count; i++) {
    Pt p;
    int rc = pt_from_be_xyzt(partials_xyzt_be + 32 * i, &p);
    if (rc != MSM_OK) return rc;
    if (fq_is_zero(p.Z)) return MSM_ERR_BAD_POINT;
    acc = pt_add(acc, p);
  }
  pt_to_be_affine(acc, out_xy_be);
  return MSM_OK;
}

int msm_combine_partials_many(const uint32_t* partials_xyzt_be, size_t world, size_t count, uint32_t* out_xy_be) {
  if ((!partials_xyzt_be && world && count) || (!out_xy_be && count)) return MSM_ERR_INVALID_ARG;
  std::vector<Pt> acc(count, pt_identity());
  for (size_t k = 0; k < count; k++)
    for (size_t w = 0; w < world; w++) {
      Pt p;
      int rc = pt_from_be_xyzt(partials_xyzt_be + 32 * (w * count + k), &p);
      if (rc != MSM_OK) return rc;
      if (fq_is_zero(p.Z)) return MSM_ERR_BAD_POINT;
      acc[k] = w == 0 ? p : pt_add(acc[k], p);
    }
  if (!count) return MSM_OK;
  // Montgomery's trick: one inversion of the product of every Z, then each Z^-1 from prefix
  // products (complete formulas: a sum of valid points never has Z = 0)
  std::vector<Fq> pre(count);
  pre[0] = acc[0].Z;
  for (size_t k = 1; k < count; k++) pre[k] = fq_mul(pre[k - 1], acc[k].Z);
  Fq inv = fq_inv(pre[count - 1]);
  for (size_t k = count; k-- > 0;) {
    const Fq zi = k ? fq_mul(inv, pre[k - 1]) : inv;
    if (k) inv = fq_mul(inv, acc[k].Z);
    uint64_t x[4], y[4];
    fq_to_std(fq_mul(acc[k].X, zi), x);
    fq_to_std(fq_mul(acc[k].Y, zi), y);
    std_to_be_words(x, out_xy_be + 16 * k);
    std_to_be_words(y, out_xy_be + 16 * k + 8);
  }
  return MSM_OK;
}

int msm_point_add_affine(const uint32_t a_xy_be[16], const uint32_t b_xy_be[16], uint32_t out_xy_be[16]) {
  if (!a_xy_be || !b_xy_be || !out_xy_be) return MSM_ERR_INVALID_ARG;
  uint64_t ax[4], ay[4], bx[4], by[4];
  be_words_to_std(a_xy_be, ax);
  be_words_to_std(a_xy_be + 8, ay);
  be_words_to_std(b_xy_be, bx);
  be_words_to_std(b_xy_be + 8, by);
  if (!std_lt_p(ax) || !std_lt_p(ay) || !std_lt_p(bx) || !std_lt_p(by)) return MSM_ERR_COORD_RANGE;
  Pt r = pt_add(pt_from_affine_std(ax, ay), pt_from_affine_std(bx, by));
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

uint32_t msm_window_count(uint32_t window_bits) {
  if (window_bits < 4 || window_bits > 20) return 0;
  return (MAIN_BITS + window_bits - 1) / window_bits + 1;  // balanced main windows + the overflow window
}

uint32_t msm_split_windows(uint32_t window_bits) {
  if (window_bits == 0 || window_bits > 32) return 0;
  return (256 + window_bits - 1) / window_bits;
}

int msm_split(uint32_t c, const uint32_t* scalars_be, size_t n, uint32_t* out) {
  // Reference semantics (msm-macro/src/lib.rs:90-176): window i (0 = least significant) takes bits
  // [c*i, c*i + c) of the big-endian u32[8] scalar; output index j = n_windows - 1 - i (MSB first).
  if (c == 0 || c > 31) return MSM_ERR_UNSUPPORTED_WINDOW;
  if ((!scalars_be || !out) && n) return MSM_ERR_INVALID_ARG;
  const uint32_t nw = msm_split_windows(c);
  for (size_t s = 0; s < n; s++) {
    const uint32_t* be = scalars_be + 8 * s;
    for (uint32_t i = 0; i < nw; i++) {
      uint32_t bit = c * i, v = 0;
      for (uint32_t b = 0; b < c && bit + b < 256; b++) {
        uint32_t pos = bit + b;
        uint32_t word = be[7 - pos / 32];
        v |= ((word >> (pos % 32)) & 1u) << b;
      }
      out[(size_t)(nw - 1 - i) * n + s] = v;
    }
  }
  return MSM_OK;
}

int msm_compute_cpu(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, uint32_t window_bits,
                    int n_threads, uint32_t out_xy_be[16]) {
  if (!out_xy_be || ((!points_be || !scalars_be) && n)) return MSM_ERR_INVALID_ARG;
  return cpu_msm(points_be, scalars_be, n, window_bits, n_threads, out_xy_be);
}

int msm_set_profiling(int enable) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_profiling.store(enable < 0 ? 0 : enable > 2 ? 1 : enable);
  for (DevCtx* c : g_ctx)
    if (c) {
      std::lock_guard<std::mutex> lk2(c->mu);  // a call in flight on another thread finishes first
      c->profiling = g_profiling.load();
      c->last.accumulate_sum = c->last.device_total_sum = c->last.accumulate_union_sum = 0;
      c->last.profiled = 0;
    }
  return MSM_OK;
}

int msm_last_profile(msm_profile_t* out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  *out = c->last;
  return MSM_OK;
}

int msm_gen_points(const uint32_t g_xy_be[16], uint64_t k0, uint64_t step, size_t n, uint32_t* points_be) {
  if (!g_xy_be || (!points_be && n)) return MSM_ERR_INVALID_ARG;
  uint64_t gx[4], gy[4];
  be_words_to_std(g_xy_be, gx);
  be_words_to_std(g_xy_be + 8, gy);
  if (!std_lt_p(gx) || !std_lt_p(gy)) return MSM_ERR_COORD_RANGE;
  gen_points(pt_from_affine_std(gx, gy), k0, step, n, points_be);
  return MSM_OK;
}

int msm_gen_scalars(uint64_t seed, size_t n, uint32_t* scalars_be) {
  if (!scalars_be && n) return MSM_ERR_INVALID_ARG;
  gen_scalars(seed, n, scalars_be);
  return MSM_OK;
}

}  // extern "C"
