// Layer 10, several devices in one call: device lists, shards, peer copies and the multi_*_entry functions
// the public entries call.  Depends on the layers above it (knobs .. split).
#pragma once
// ---- several devices in one call (msm_opts.flags & MSM_FLAG_DEVICES, include/msm.h) ----------
// The reference's one sharding precedent is inside compute_msm: the point vector split between
// the CPU and the GPU worker (submission.ts:116-154, gpu_worker.ts:9-18) and the two partials
// joined with point_add_affine (lib.rs:240-253).  Here the split is over gfx950 devices, one
// host thread each, and the join is projective (one EC add per shard, one inversion at the end).

bool devices_listed(const msm_opts* o) { return o && (o->flags & MSM_FLAG_DEVICES); }
// MSM_FLAG_SCALAR_BITS, MSM_FLAG_SCALAR_TYPE and MSM_FLAG_SCALAR_FIELD belong to the msm_bases_compute*
// entries: every other entry refuses them before it touches a device (their scalars are the 8-word format).
bool narrow_flagged(const msm_opts* o) {
  return o && (o->flags & (MSM_FLAG_SCALAR_BITS | MSM_FLAG_SCALAR_TYPE | MSM_FLAG_SCALAR_FIELD));
}

// The listed ordinals, checked for shape (non-null, 1..MSM_MAX_DEVICES entries, non-negative,
// distinct) before any device is touched, then for being gfx950 devices.
int device_list(const msm_opts* o, std::vector<int>* devs) {
  devs->clear();
  if (!o->devices || o->n_devices == 0 || o->n_devices > MSM_MAX_DEVICES) return MSM_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < o->n_devices; i++) {
    const int d = o->devices[i];
    if (d < 0 || std::find(devs->begin(), devs->end(), d) != devs->end()) return MSM_ERR_INVALID_ARG;
    devs->push_back(d);
  }
  for (int d : *devs) {
    DevCtx* c;
    if (int rc = get_ctx(d, &c)) return rc;
  }
  return MSM_OK;
}

// One listed device's single-device options (a window range carried over).
msm_opts opts_on(const msm_opts* o, int device) {
  msm_opts r = copy_opts(o);
  r.flags &= ~MSM_FLAG_DEVICES;
  r.device = device;
  return r;
}

// Contiguous shard i of D over n items: [n i / D, n (i+1) / D) (sizes differ by at most one).
void shard_range(size_t n, size_t i, size_t D, size_t* lo, size_t* hi) {
  *lo = n * i / D;
  *hi = n * (i + 1) / D;
}

// fn(i) for every listed device, device i on its own host thread (device 0 on the caller's); the
// first error in list order is returned once all have finished.
template <typename F>
int for_each_device(size_t D, F&& fn) {
  std::vector<int> rc(D, MSM_OK);
  std::vector<std::thread> th;
  for (size_t i = 1; i < D; i++)
    th.emplace_back([&, i] {
      t_call_devices = (int)D;
      rc[i] = fn(i);
    });
  const int own = t_call_devices;
  t_call_devices = (int)D;
  rc[0] = fn(0);
  t_call_devices = own;
  for (std::thread& t : th) t.join();
  for (int r : rc)
    if (r != MSM_OK) return r;
  return MSM_OK;
}

// msm_compute / msm_compute_partial: each listed device uploads and reduces its own shard.
// (`devs` may repeat a device only through the test hook msm_test_sharded: its shards then run
// one after another on that device.)
int sharded_host(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                 const std::vector<int>& devs, Pt* r) {
  const size_t D = devs.size();
  std::vector<Pt> part(D, pt_identity());
  int rc = for_each_device(D, [&](size_t i) {
    size_t lo, hi;
    shard_range(n, i, D, &lo, &hi);
    const msm_opts od = opts_on(opts, devs[i]);
    return host_entry(points_be + lo * 32, scalars_be + lo * 8, hi - lo, &od, &part[i]);
  });
  if (rc != MSM_OK) return rc;
  *r = join_partials(part);
  return MSM_OK;
}

int multi_host_entry(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts, Pt* r) {
  if (narrow_flagged(opts)) return MSM_ERR_INVALID_ARG;
  if (!devices_listed(opts)) return host_entry(points_be, scalars_be, n, opts, r);
  if ((!points_be || !scalars_be) && n) return MSM_ERR_INVALID_ARG;
  std::vector<int> devs;
  if (int rc = device_list(opts, &devs)) return rc;
  return sharded_host(points_be, scalars_be, n, opts, devs, r);
}

// Peer access of the current device `dev` to `owner`'s memory, enabled once per ordered pair, so
// the peer copies of peer_shard run device to device over xGMI (without it the runtime may stage
// them through host memory).  "Already enabled" (another library in the process, e.g. RCCL, did it)
// counts as enabled; a pair without peer support is remembered and left to the runtime's staged
// copies.  Returns 1 when enabled, 0 otherwise (msm_test_peer_state).
std::mutex g_peer_mu;
std::vector<int8_t> g_peer;  // [g_nhip * g_nhip]: 0 untried, 1 enabled, -1 unavailable

int enable_peer(int dev, int owner) {
  if (dev == owner) return 1;
  std::lock_guard<std::mutex> lk(g_peer_mu);
  if (g_nhip <= 0 || dev >= g_nhip || owner >= g_nhip) return 0;
  if (g_peer.size() != (size_t)g_nhip * g_nhip) g_peer.assign((size_t)g_nhip * g_nhip, 0);
  int8_t& st = g_peer[(size_t)dev * g_nhip + owner];
  if (st == 0) {
    int can = 0;
    st = -1;
    if (hipDeviceCanAccessPeer(&can, dev, owner) == hipSuccess && can) {
      const hipError_t e = hipDeviceEnablePeerAccess(owner, 0);
      if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) st = 1;
    }
    (void)hipGetLastError();  // a refused enable leaves no sticky error for the next call
  }
  return st > 0 ? 1 : 0;
}

// One shard of device-resident inputs that live on another device: copied over xGMI (a peer copy
// on the slot's stream, peer access enabled first) into this device's wire buffers, then reduced
// here.
int peer_shard(int owner, const uint32_t* d_points, const uint32_t* d_scalars, size_t cnt, const msm_opts* od,
               Pt* r) {
  return on_device(od, [&](DevCtx* c) -> int {
    if (cnt == 0) {
      *r = msmh::pt_identity();
      return MSM_OK;
    }
    enable_peer(c->device, owner);
    Slot& sl = c->slot[0];
    Workspace& w = sl.ws;
    int rc;
    if ((rc = w.wire_pts.ensure(cnt * 128)) != MSM_OK || (rc = w.wire_sc.ensure(cnt * 32)) != MSM_OK) return rc;
    HIPCHECK(hipMemcpyPeerAsync(w.wire_pts.p, c->device, d_points, owner, cnt * 128, sl.stream));
    HIPCHECK(hipMemcpyPeerAsync(w.wire_sc.p, c->device, d_scalars, owner, cnt * 32, sl.stream));
    rc = run_device(c, w.wire_pts.as<uint32_t>(), w.wire_sc.as<uint32_t>(), cnt, od, nullptr, r);
    if (rc != MSM_OK) hipStreamSynchronize(sl.stream);  // the copies read the caller's buffers
    return rc;
  });
}

// msm_compute_device / msm_compute_device_partial: the inputs live on one listed device (the
// owner), which reduces its shard in place; every other listed device copies its shard over.
// (Through msm_test_sharded a device may be listed again: its later shards take the copy path.)
int sharded_device(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, const msm_opts* opts,
                   void* hip_stream, const std::vector<int>& devs, Pt* r) {
  int owner = devs[0];
  if (n) {
    hipPointerAttribute_t ap{}, as{};
    if (hipPointerGetAttributes(&ap, d_points_be) != hipSuccess ||
        hipPointerGetAttributes(&as, d_scalars_be) != hipSuccess) {
      (void)hipGetLastError();
      return MSM_ERR_INVALID_ARG;
    }
    owner = ap.device;
    if (as.device != owner || std::find(devs.begin(), devs.end(), owner) == devs.end()) return MSM_ERR_INVALID_ARG;
  }
  if (hip_stream && n) {
    // the peer copies start on other devices' streams: the inputs' producers finish first
    DeviceGuard g(owner);
    HIPCHECK(hipStreamSynchronize(hip_stream == MSM_STREAM_NULL ? nullptr : (hipStream_t)hip_stream));
  }
  const size_t D = devs.size();
  const size_t own = (size_t)(std::find(devs.begin(), devs.end(), owner) - devs.begin());
  std::vector<Pt> part(D, pt_identity());
  int rc = for_each_device(D, [&](size_t i) {
    size_t lo, hi;
    shard_range(n, i, D, &lo, &hi);
    const msm_opts od = opts_on(opts, devs[i]);
    if (i == own)
      return device_entry(d_points_be + lo * 32, d_scalars_be + lo * 8, hi - lo, &od, nullptr, &part[i]);
    return peer_shard(owner, d_points_be + lo * 32, d_scalars_be + lo * 8, hi - lo, &od, &part[i]);
  });
  if (rc != MSM_OK) return rc;
  *r = join_partials(part);
  return MSM_OK;
}

int multi_device_entry(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, const msm_opts* opts,
                       void* hip_stream, Pt* r) {
  if (narrow_flagged(opts)) return MSM_ERR_INVALID_ARG;
  if (!devices_listed(opts)) return device_entry(d_points_be, d_scalars_be, n, opts, hip_stream, r);
  if ((!d_points_be || !d_scalars_be) && n) return MSM_ERR_INVALID_ARG;
  std::vector<int> devs;
  if (int rc = device_list(opts, &devs)) return rc;
  return sharded_device(d_points_be, d_scalars_be, n, opts, hip_stream, devs, r);
}

// msm_compute_many / msm_compute_shared: a contiguous block of the MSMs per listed device
// (whole MSMs, nothing to join).  Device batches take one device.
int multi_many_entry(const ManyInputs& in, size_t n, size_t count, const msm_opts* opts, void* hip_stream,
                     uint32_t* out, bool projective) {
  if (narrow_flagged(opts)) return MSM_ERR_INVALID_ARG;
  if (!devices_listed(opts)) return many_entry(in, n, count, opts, hip_stream, out, projective);
  if (in.kind != ManyInputs::HOST) return MSM_ERR_INVALID_ARG;
  if (!out || (!in.scalars && count) || (!in.points && !in.shared_points && count)) return MSM_ERR_INVALID_ARG;
  std::vector<int> devs;
  if (int rc = device_list(opts, &devs)) return rc;
  const size_t D = devs.size();
  return for_each_device(D, [&](size_t i) -> int {
    size_t b0, b1;
    shard_range(count, i, D, &b0, &b1);
    if (b0 == b1) return MSM_OK;
    ManyInputs sub = in;
    if (in.points) sub.points = in.points + b0;
    sub.scalars = in.scalars + b0;
    const msm_opts od = opts_on(opts, devs[i]);
    return many_entry(sub, n, b1 - b0, &od, nullptr, out + b0 * (projective ? 32 : 16), projective);
  });
}
