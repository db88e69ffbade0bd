// Layer 11, resident prepared bases: the handle registry, creation, and the compute entries' common path.
// Depends on the layers above it (knobs .. multi).
#pragma once
// A handle's state.  The caller's msm_bases* is a token (the registry key, never an address), so a
// stale or foreign handle is a failed lookup, not a dereference.  `rec` is freed, and `alive`
// cleared, under the owning device context's lock (msm_bases_destroy, msm_shutdown); a compute
// call holds a reference and checks `alive` under that lock before it reads the records.
struct Bases {
  int device = -1;
  size_t n = 0;
  uint32_t levels = 1;
  uint32_t window_bits = 0;  // levels > 1: the width the levels were shifted for
  BasesGeo geo{};            // levels > 1
  Buf rec;                   // levels * n records, level j at [j n, (j + 1) n)
  bool alive = false;
  template <typename F>
  void each_buf(F&& f) {  // as Workspace::each_buf
    f("bases_rec", rec);
  }
};
std::map<uintptr_t, std::shared_ptr<Bases>> g_bases;  // under g_mu
uintptr_t g_bases_next = 1;

std::shared_ptr<Bases> find_bases(const msm_bases* h) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_bases.find(reinterpret_cast<uintptr_t>(h));
  return it == g_bases.end() ? nullptr : it->second;
}

// Every live handle's records on `device` (DevCtx::destroy, under g_mu and the context's lock); its
// next use fails the registry lookup.
void release_bases_on(int device) {
  for (auto& kv : g_bases)
    if (kv.second->device == device) {
      kv.second->alive = false;
      kv.second->each_buf([](const char*, Buf& b) { b.release(); });
    }
}

bool bases_flags_ok(const msm_opts* o) {  // a handle lives on one device and runs whole MSMs
  return !o || !(o->flags & (MSM_FLAG_DEVICES | MSM_FLAG_WINDOWS | MSM_FLAG_HALF_WINDOWS));
}

// Compressed points (msm.h MSM_POINTS_X_*): k_decompress_x over n device-resident x vectors into `dst`,
// x|y (wire = 0) or wire records (wire = 1), errors into err[0].
static_assert(DX_FORM_SUBGROUP == MSM_POINTS_X_SUBGROUP && DX_FORM_YSIGN == MSM_POINTS_X_YSIGN, "k_decompress_x's forms");
bool points_form_ok(uint32_t form) { return form == MSM_POINTS_X_SUBGROUP || form == MSM_POINTS_X_YSIGN; }
bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15u); }
void launch_decompress(const uint32_t* d_xs, uint32_t* dst, uint32_t n, uint32_t form, uint32_t wire, uint32_t* err,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_decompress_x, dim3(grid_for(n, DX_THREADS)), dim3(DX_THREADS), 0, s, d_xs, dst, n, form, wire,
                     err);
}

// A creation's argument rules that need no device: the levels (0 = the library's choice for n), the
// window width and the geometry of the shifted levels, and levels * n inside the record limit.
int bases_shape(Bases* b, size_t n, uint32_t levels, uint32_t wb) {
  if (levels > 8) return MSM_ERR_INVALID_ARG;
  if (wb && (wb < 4 || wb > 20)) return MSM_ERR_UNSUPPORTED_WINDOW;
  if (!levels) levels = bases_auto_levels(n);
  b->n = n;
  b->levels = levels;
  if (levels > 1) {
    b->window_bits = wb ? wb : bases_auto_window(n, levels);
    if (!bases_geometry(b->window_bits, levels, &b->geo)) return MSM_ERR_INVALID_ARG;
  }
  if ((uint64_t)levels * n >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  return MSM_OK;
}

// The launch plan of one MSM on a handle's records must exist (finish_plan's Mmax limit).
int bases_plan_exists(DevCtx* c, const Bases& b, uint32_t wb) {
  msm_opts op{};
  op.window_bits = b.levels > 1 ? b.window_bits : wb;
  if (b.levels > 1) {
    op.flags = MSM_FLAG_WINDOWS;
    op.window_hi = b.geo.Wc;
  }
  Plan pl;
  return make_plan(b.n * b.levels, &op, c->shape, &pl, false, 1, true);
}

// Level j of a handle's records from level j - 1, for every shifted level (k_shift_bases).
void launch_shift_levels(const Bases& b, uint32_t nt, hipStream_t s) {
  uint32_t* rec = b.rec.as<uint32_t>();
  for (uint32_t j = 1; j < b.levels; j++)
    hipLaunchKernelGGL(k_shift_bases, dim3(grid_for(b.n, PP_THREADS)), dim3(PP_THREADS), 0, s,
                       rec + (size_t)(j - 1) * b.n * PRE_WORDS, rec + (size_t)j * b.n * PRE_WORDS, (uint32_t)b.n,
                       b.geo.S, nt);
}

// A finished creation (a handle, or host_fixed.h's table) into its registry: *out is the new token.
// `has_rec` is false for a handle of no points, which allocated nothing.
template <typename H, typename Tok>
int register_handle(std::map<uintptr_t, std::shared_ptr<H>>& registry, const std::shared_ptr<H>& h, bool has_rec,
                    Tok** out) {
  h->alive = true;
  std::lock_guard<std::mutex> lk(g_mu);
  // msm_shutdown may have run since the records were made (it frees only registered handles and tables)
  if (has_rec && ((int)g_ctx.size() <= h->device || !g_ctx[h->device])) {
    h->rec.release();
    return MSM_ERR_INVALID_ARG;
  }
  const uintptr_t id = g_bases_next++;
  registry[id] = h;
  *out = reinterpret_cast<Tok*>(id);
  return MSM_OK;
}
int register_bases(const std::shared_ptr<Bases>& b, msm_bases** out) { return register_handle(g_bases, b, b->n != 0, out); }

// The device's error bits as the entry's return code.  A kernel that never raises a bit never sets it,
// so one order serves every caller.
int dev_err_code(uint32_t bits) {
  if (bits & (MSM_DEV_ERR_BAD_INDEX | MSM_DEV_ERR_SCALAR_RANGE)) return MSM_ERR_INVALID_ARG;
  if (bits & MSM_DEV_ERR_COORD_RANGE) return MSM_ERR_COORD_RANGE;
  if (bits & MSM_DEV_ERR_BAD_POINT) return MSM_ERR_BAD_POINT;
  return MSM_OK;
}

// The call frame of the entries that run the per-point kernels on slot 0's stream (create_bases,
// decompress_points, bases_scale, fixed_create, fixed_mul): the kernels' error word, the new records
// (if the call makes any), and every exit past the allocations.
struct PointCall {
  DevCtx* c = nullptr;
  Buf errb;             // the error word
  Buf* rec = nullptr;   // the new records: released on failure, so a failure leaves nothing allocated
  hipStream_t stream() const { return c->slot[0].stream; }
  uint32_t* errp() { return errb.as<uint32_t>(); }
  // The error word, then `rec_bytes` of new records in *new_rec (null: the call makes none), then the
  // word zeroed on the stream.
  int begin(DevCtx* ctx, Buf* new_rec = nullptr, size_t rec_bytes = 0) {
    c = ctx;
    int r = errb.ensure(16);
    if (r != MSM_OK) return r;
    if (new_rec && (r = new_rec->ensure(rec_bytes)) != MSM_OK) {
      errb.release();
      return r;
    }
    rec = new_rec;
    if (hipMemsetAsync(errp(), 0, 16, stream()) != hipSuccess) return done(MSM_ERR_HIP);
    return MSM_OK;
  }
  // The stream behind the caller's.
  int after_user(hipStream_t user_stream) {
    const int r = order_after_user(c, user_stream, 1);
    return r != MSM_OK ? done(r) : r;
  }
  int done(int code) {
    drain_streams(c, 1, code);
    if (errb.base) {  // guarded (host_guard.h): the word does not outlive the call, so it is looked at here
      std::lock_guard<std::mutex> gl(g_guard_mu);
      (void)guard_scan(errb, guard_id("bases_prep_err"), c->device, -1, &g_guard_pending);
    }
    errb.release();
    if (code != MSM_OK && rec) rec->release();
    return code;
  }
  // After the last launch: m wire records from `d_points` to the host's `points` (null: none), the
  // error word back, and the call's code.
  int finish(uint32_t* points = nullptr, const uint32_t* d_points = nullptr, size_t m = 0) {
    if (hipGetLastError() != hipSuccess) return done(MSM_ERR_HIP);
    uint32_t e[4] = {};
    if ((points && hipMemcpyAsync(points, d_points, m * 128, hipMemcpyDeviceToHost, stream()) != hipSuccess) ||
        hipMemcpyAsync(e, errp(), 16, hipMemcpyDeviceToHost, stream()) != hipSuccess ||
        hipStreamSynchronize(stream()) != hipSuccess)
      return done(MSM_ERR_HIP);
    return done(dev_err_code(e[0]));
  }
};

// Host words up into slot buffers on the copy stream -- every buffer sized first, then every copy --
// and slot 0's stream behind them.  An entry without words (src null) is skipped.
struct HostWords {
  Buf* dst;
  const uint32_t* src;
  size_t bytes;
};
int upload_words(DevCtx* c, std::initializer_list<HostWords> sets) {
  for (const HostWords& w : sets)
    if (w.src)
      if (int r = w.dst->ensure(w.bytes)) return r;
  for (const HostWords& w : sets)
    if (w.src)
      if (int r = upload(c, w.dst->p, w.src, w.bytes, w.bytes, [](size_t, size_t) { return MSM_OK; })) return r;
  HIPCHECK(hipEventRecord(c->ev_chunk[0], c->copy_stream));
  HIPCHECK(hipStreamWaitEvent(c->slot[0].stream, c->ev_chunk[0], 0));
  return MSM_OK;
}

// msm_bases_scale* and msm_fixed_mul*: a device caller's pointers, from their values -- the scalars'
// alignment (`per` words per output point, `sw` of them per scalar), and the m wire records of `points`
// (null: the call creates a handle) 16-byte aligned and clear of the scalars.
bool point_call_ptrs_ok(const uint32_t* scalars, size_t sw, size_t per, size_t m, const uint32_t* points) {
  const uintptr_t sp = reinterpret_cast<uintptr_t>(scalars), pp = reinterpret_cast<uintptr_t>(points);
  if (sp & (sw == 8 ? 15u : 3u)) return false;
  return !points || !((pp & 15u) || (pp < sp + m * per * 4 && sp < pp + m * 128));
}
// Where their kernels write: the caller's `points`, or the slot's dx_pts for a host call (wire records,
// copied down by PointCall::finish) and for a creation (x|y, prepared by launch_created).
int point_call_output(Slot& s0, bool host, bool created, size_t m, uint32_t** d_out) {
  if (!host && !created) return MSM_OK;
  if (int r = s0.ws.dx_pts.ensure(m * (created ? 64 : 128))) return r;
  *d_out = s0.ws.dx_pts.as<uint32_t>();
  return MSM_OK;
}
// A creation's tail: the m x|y points at `xy` into nb's level 0, as a compressed creation's are, and its
// shifted levels.
void launch_created(const Bases& nb, const uint32_t* xy, size_t m, uint32_t* errp, hipStream_t s) {
  const uint32_t nt = prep_nt((size_t)nb.levels * m);
  launch_prepare(xy, nb.rec.as<uint32_t>(), (uint32_t)m, errp, nt, s, PT_FMT_XY);
  launch_shift_levels(nb, nt, s);
}

// `form` 0: `points` are wire records; MSM_POINTS_X_*: compressed points, decompressed into the slot's
// dx_pts as x|y and prepared from there, so the records are those of the wire creation of the same points.
int create_bases(const uint32_t* points, bool host, size_t n, uint32_t form, const msm_opts* opts, uint32_t levels,
                 hipStream_t user_stream, msm_bases** out) {
  if (!out) return MSM_ERR_INVALID_ARG;
  *out = nullptr;
  if ((!points && n) || !bases_flags_ok(opts) || narrow_flagged(opts)) return MSM_ERR_INVALID_ARG;
  if (form && (!points_form_ok(form) || (!host && !aligned16(points)))) return MSM_ERR_INVALID_ARG;
  const uint32_t wb = opts ? opts->window_bits : 0;
  auto b = std::make_shared<Bases>();
  if (int src = bases_shape(b.get(), n, levels, wb)) return src;
  levels = b->levels;
  msm_opts od{};
  od.device = opts ? opts->device : -1;
  int rc = on_device(&od, [&](DevCtx* c) -> int {
    b->device = c->device;
    if (!n) return MSM_OK;
    if (int prc = bases_plan_exists(c, *b, wb)) return prc;
    Slot& s0 = c->slot[0];
    PointCall f;
    int r = f.begin(c, &b->rec, (size_t)levels * n * PRE_WORDS * 4);
    if (r != MSM_OK || (r = f.after_user(user_stream)) != MSM_OK) return r;
    uint32_t* rec = b->rec.as<uint32_t>();
    uint32_t* errp = f.errp();
    const uint32_t nt = prep_nt((size_t)levels * n);
    if (form) {
      const uint32_t* d_xs = points;
      if (host) {  // 32 n bytes up, into the wire buffer
        if ((r = s0.ws.wire_pts.ensure(n * 32)) != MSM_OK) return f.done(r);
        if ((r = upload_scalars(c, points, n, s0.ws.wire_pts.as<uint32_t>(), s0.stream, c->ev_chunk[0])) != MSM_OK)
          return f.done(r);
        d_xs = s0.ws.wire_pts.as<uint32_t>();
      }
      if ((r = s0.ws.dx_pts.ensure(n * 64)) != MSM_OK) return f.done(r);
      launch_decompress(d_xs, s0.ws.dx_pts.as<uint32_t>(), (uint32_t)n, form, 0, errp, s0.stream);
      launch_prepare(s0.ws.dx_pts.as<uint32_t>(), rec, (uint32_t)n, errp, nt, s0.stream, PT_FMT_XY);
    } else if (host) {
      if ((r = s0.ws.wire_pts.ensure(n * 128)) != MSM_OK) return f.done(r);
      if ((r = upload_points(c, points, n, s0.ws.wire_pts.as<uint32_t>(), rec, errp, s0.stream)) != MSM_OK)
        return f.done(r);
    } else {
      launch_prepare(points, rec, (uint32_t)n, errp, nt, s0.stream);
    }
    launch_shift_levels(*b, nt, s0.stream);
    return f.finish();
  });
  if (rc != MSM_OK) return rc;
  return register_bases(b, out);
}

// msm_decompress_points*: n compressed points to wire records, host to host (through the slot's wire
// buffer and dx_pts) or device to device (the caller's buffers).
int decompress_points(const uint32_t* xs, bool host, size_t n, uint32_t form, const msm_opts* opts,
                      hipStream_t user_stream, uint32_t* points) {
  if (((!xs || !points) && n) || !points_form_ok(form) || !bases_flags_ok(opts) || narrow_flagged(opts))
    return MSM_ERR_INVALID_ARG;
  if (!host && (!aligned16(xs) || !aligned16(points))) return MSM_ERR_INVALID_ARG;
  if (n >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  msm_opts od{};
  od.device = opts ? opts->device : -1;
  return on_device(&od, [&](DevCtx* c) -> int {
    if (!n) return MSM_OK;
    Slot& s0 = c->slot[0];
    PointCall f;
    int r = f.begin(c);
    if (r != MSM_OK || (r = f.after_user(user_stream)) != MSM_OK) return r;
    const uint32_t* d_xs = xs;
    uint32_t* d_out = points;
    if (host) {
      if ((r = s0.ws.wire_pts.ensure(n * 32)) != MSM_OK || (r = s0.ws.dx_pts.ensure(n * 128)) != MSM_OK)
        return f.done(r);
      if ((r = upload_scalars(c, xs, n, s0.ws.wire_pts.as<uint32_t>(), s0.stream, c->ev_chunk[0])) != MSM_OK)
        return f.done(r);
      d_xs = s0.ws.wire_pts.as<uint32_t>();
      d_out = s0.ws.dx_pts.as<uint32_t>();
    }
    launch_decompress(d_xs, d_out, (uint32_t)n, form, 1, f.errp(), s0.stream);
    return f.finish(host ? points : nullptr, d_out, n);
  });
}

// msm_compress_points: affine x|y to x, with y's sign flag in bit 255 for MSM_POINTS_X_YSIGN.
int compress_points(const uint32_t* xy, size_t n, uint32_t form, uint32_t* xs) {
  if (((!xy || !xs) && n) || !points_form_ok(form)) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++) {
    uint64_t x[4], y[4];
    be_words_to_std(xy + 16 * i, x);
    be_words_to_std(xy + 16 * i + 8, y);
    if (!std_lt_p(x) || !std_lt_p(y)) return MSM_ERR_COORD_RANGE;
  }
  for (size_t i = 0; i < n; i++) {
    uint64_t y[4], y2[4];
    be_words_to_std(xy + 16 * i + 8, y);
    for (int k = 3; k >= 0; k--) y2[k] = (y[k] << 1) | (k ? y[k - 1] >> 63 : 0);
    // y > p - y: 2 y > p, and 2 y (even, below 2^254) is never p
    const bool big = !std_lt_p(y2);
    for (int k = 0; k < 8; k++) xs[8 * i + k] = xy[16 * i + k];
    if (form == MSM_POINTS_X_YSIGN && big) xs[8 * i] |= 0x80000000u;
  }
  return MSM_OK;
}

// msm_bases_scale*: Q_i = s_i P_i for the m bases of `sub` (null: all n) of a handle's level 0, one
// k_scale_points launch on slot 0's stream.  With `created` the points become a new handle: the x|y
// output goes through the preparation, as a compressed creation's does, so level 0 is what
// msm_bases_create makes from the wire records.  Else they are written to `points` as wire records
// (host entries: through the slot's dx_pts).  Host scalars (and indices) go up into the slot's wire_pts
// (and sub_idx) after every one of them was checked.
int bases_scale(const msm_bases* h, const msm_subset_t* sub, const uint32_t* scalars, bool host, const msm_opts* opts,
                hipStream_t user_stream, uint32_t* points, uint32_t levels, msm_bases** created) {
  if (created) *created = nullptr;
  if (!h || !bases_flags_ok(opts) || typed_flagged(opts)) return MSM_ERR_INVALID_ARG;
  const uint32_t bits = opts && (opts->flags & MSM_FLAG_SCALAR_BITS) ? opts->scalar_bits : 256u;
  if (bits < 1 || bits > 256) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = find_bases(h);
  if (!b) return MSM_ERR_INVALID_ARG;
  if (opts && opts->device >= 0 && opts->device != b->device) return MSM_ERR_INVALID_ARG;
  const uint32_t* indices = sub && sub->indices ? sub->indices[0] : nullptr;
  const size_t m = sub ? (size_t)sub->m : b->n, first = sub ? (size_t)sub->first : 0;
  if (sub) {
    if (int rc = subset_check(b->n, 1, sub->first, sub->m, sub->indices != nullptr)) return rc;
    if (sub->indices && !indices && m) return MSM_ERR_INVALID_ARG;
  }
  if (m && (!scalars || (!created && !points))) return MSM_ERR_INVALID_ARG;
  const uint32_t wb = opts ? opts->window_bits : 0;
  auto nb = std::make_shared<Bases>();
  if (created)
    if (int rc = bases_shape(nb.get(), m, levels, wb)) return rc;
  const size_t sw = (bits + 31) / 32;
  if (!host && m &&
      (!point_call_ptrs_ok(scalars, sw, sw, m, created ? nullptr : points) || (reinterpret_cast<uintptr_t>(indices) & 3u)))
    return MSM_ERR_INVALID_ARG;
  if (host) {  // every scalar and every index, before anything is uploaded or enqueued
    if (bits & 31u) {
      const uint32_t excess = ~((1u << (bits & 31u)) - 1u);
      uint32_t any = 0;
      for (size_t i = 0; i < m; i++) any |= scalars[i * sw];
      if (any & excess) return MSM_ERR_INVALID_ARG;
    }
    for (size_t i = 0; indices && i < m; i++)
      if (indices[i] >= b->n) return MSM_ERR_INVALID_ARG;
  }
  msm_opts od{};
  od.device = b->device;
  int rc = on_device(&od, [&](DevCtx* c) -> int {
    if (!b->alive) return MSM_ERR_INVALID_ARG;  // destroyed, or the library shut down, meanwhile
    nb->device = c->device;
    if (!m) return MSM_OK;
    if (created)
      if (int prc = bases_plan_exists(c, *nb, wb)) return prc;
    Slot& s0 = c->slot[0];
    PointCall f;
    int r = f.begin(c, created ? &nb->rec : nullptr, (size_t)nb->levels * m * PRE_WORDS * 4);
    if (r != MSM_OK || (r = f.after_user(user_stream)) != MSM_OK) return r;
    const uint32_t* d_sc = scalars;
    const uint32_t* d_ix = indices;
    uint32_t* d_out = points;
    if (host) {
      if ((r = upload_words(c, {{&s0.ws.wire_pts, scalars, m * sw * 4}, {&s0.ws.sub_idx, indices, m * 4}})) != MSM_OK)
        return f.done(r);
      d_sc = s0.ws.wire_pts.as<uint32_t>();
      if (indices) d_ix = s0.ws.sub_idx.as<uint32_t>();
    }
    if ((r = point_call_output(s0, host, created, m, &d_out)) != MSM_OK) return f.done(r);
    hipLaunchKernelGGL(k_scale_points, dim3(grid_for(m, SC_THREADS)), dim3(SC_THREADS), 0, s0.stream,
                       b->rec.as<uint32_t>(), (uint32_t)b->n, (uint32_t)first, d_ix, d_sc, (uint32_t)sw, bits, d_out,
                       (uint32_t)m, created ? 0u : 1u, f.errp());
    if (created) launch_created(*nb, d_out, m, f.errp(), s0.stream);
    return f.finish(host && !created ? points : nullptr, d_out, m);
  });
  if (rc != MSM_OK || !created) return rc;
  return register_bases(nb, created);
}

// `count` MSMs over a handle's records: run_many's pipelined path with the records in the place
// of a shared base vector's (count = 1: the single entries, which then have no preparation to fork).
// With `sub`, over a subset of the bases (msm_bases_compute_subset*).
int bases_compute(const msm_bases* h, const uint32_t* const* scalars, bool host, size_t count, const msm_opts* opts,
                  void* hip_stream, uint32_t* out, const msm_subset_t* sub = nullptr, bool is_subset = false) {
  if (!h || !out || (!scalars && count) || !bases_flags_ok(opts) || (is_subset && !sub)) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = find_bases(h);
  if (!b) return MSM_ERR_INVALID_ARG;
  const bool indexed = sub && sub->indices;
  const size_t terms = sub ? (size_t)sub->m : b->n;  // scalars per vector
  // Narrow scalars (MSM_FLAG_SCALAR_BITS): below 254 bits the call runs unfolded on the level-0
  // records, whatever the handle's levels -- they are plain prepared records -- over the scalars'
  // own geometry (make_plan); 254 bits and more are the 8-word call as it is.
  // Native scalar types (MSM_FLAG_SCALAR_TYPE): the narrow call of b = scalar_bits, or of the element's
  // own width where that is unset, on the caller's own integer array.
  // Wide types (MSM_FLAG_SCALAR_FIELD): the same on little-endian 128- / 256-bit elements; always unfolded,
  // a 256-bit integer of 254 bits and more included (the full-width launch on the level-0 records).
  const bool bits_set = opts && (opts->flags & MSM_FLAG_SCALAR_BITS);
  const uint32_t stype = opts_scalar_type(opts);
  if (typed_flagged(opts) && !typed_width(stype, bits_set, bits_set ? opts->scalar_bits : 0)) return MSM_ERR_INVALID_ARG;
  const uint32_t ebits = scalar_type_bits(stype);
  const uint32_t sbits = stype ? typed_width(stype, bits_set, bits_set ? opts->scalar_bits : 0)
                               : bits_set ? opts->scalar_bits : 256;
  if (sbits < 1 || sbits > 256) return MSM_ERR_INVALID_ARG;
  const bool narrow = sbits < MAIN_BITS;
  const bool wide = stype_wide(stype);
  const uint32_t levels = narrow || wide ? 1u : b->levels;
  if (sub) {
    if (int rc = subset_check(b->n, levels, sub->first, sub->m, indexed)) return rc;
    for (size_t k = 0; indexed && terms && k < count; k++) {
      const uint32_t* ix = sub->indices[k];
      if (!ix) return MSM_ERR_INVALID_ARG;
      // host index vectors are checked here, before anything is uploaded or enqueued (the device
      // entries' are checked by k_stage_indices); a vector given again is checked once
      if (!host || (k && ix == sub->indices[k - 1])) continue;
      for (size_t i = 0; i < terms; i++)
        if (ix[i] >= b->n) return MSM_ERR_INVALID_ARG;
    }
  }
  if (opts && opts->device >= 0 && opts->device != b->device) return MSM_ERR_INVALID_ARG;
  msm_opts_typed ot{};
  msm_opts& o = ot.opts;
  o.run_length = opts ? opts->run_length : 0;
  o.flags = opts ? (opts->flags & MSM_FLAG_SERIAL) : 0;
  o.device = b->device;
  o.window_bits = opts ? opts->window_bits : 0;
  if (narrow) {
    o.flags |= MSM_FLAG_SCALAR_BITS;
    o.scalar_bits = sbits;
  }
  if (wide) {
    o.flags |= MSM_FLAG_SCALAR_FIELD;
    ot.scalar_field = stype & ~STYPE_WIDE;
  } else if (stype) {
    o.flags |= MSM_FLAG_SCALAR_TYPE;
    ot.scalar_type = stype;
  }
  if (levels > 1) {
    if (o.window_bits && o.window_bits != b->window_bits) return MSM_ERR_INVALID_ARG;
    o.window_bits = b->window_bits;
    o.flags |= MSM_FLAG_WINDOWS;
    o.window_lo = 0;
    o.window_hi = b->geo.Wc;
  }
  if (count == 0) return MSM_OK;
  for (size_t k = 0; k < count; k++) {
    if (!scalars[k] && terms) return MSM_ERR_INVALID_ARG;
    // a native vector's alignment, from the pointer value: the element's own on the host (a wide
    // element's u64 limbs': 8 bytes), 4 bytes on the device (the recode reads whole words)
    if (stype && (reinterpret_cast<uintptr_t>(scalars[k]) & (host ? std::min(std::max(ebits / 8, 1u), 8u) - 1u : 3u)))
      return MSM_ERR_INVALID_ARG;
  }
  // A bit at or above scalar_bits: host vectors are checked on the host, before anything is uploaded
  // or enqueued (the device entries' by k_recode_narrow); only the most significant word can hold
  // one.  Large vectors go over the device context's parked packing threads (the strided read of
  // 2^20 8-word scalars is ~0.5 ms on one thread); a vector given again is checked once.
  // A native type's magnitude of 2^sbits or more (possible only below the element's width): the OR of
  // the vector's magnitudes, formed as the recode forms them, has a bit at or above sbits.
  auto native_scan = [&](const uint32_t* vec, size_t i0, size_t i1) -> uint64_t {
    uint64_t a = 0;
    auto mags = [&](auto* p, auto zero) {
      using U = decltype(zero);
      for (size_t i = i0; i < i1; i++) {
        const U u = (U)p[i];
        a |= p[i] < 0 ? (U)((U)0 - u) : u;
      }
    };
    switch (stype) {
      case MSM_SCALAR_U8: mags(reinterpret_cast<const uint8_t*>(vec), (uint8_t)0); break;
      case MSM_SCALAR_I8: mags(reinterpret_cast<const int8_t*>(vec), (uint8_t)0); break;
      case MSM_SCALAR_U16: mags(reinterpret_cast<const uint16_t*>(vec), (uint16_t)0); break;
      case MSM_SCALAR_I16: mags(reinterpret_cast<const int16_t*>(vec), (uint16_t)0); break;
      case MSM_SCALAR_U32: mags(reinterpret_cast<const uint32_t*>(vec), (uint32_t)0); break;
      case MSM_SCALAR_I32: mags(reinterpret_cast<const int32_t*>(vec), (uint32_t)0); break;
      case MSM_SCALAR_U64: mags(reinterpret_cast<const uint64_t*>(vec), (uint64_t)0); break;
      case MSM_SCALAR_I64: mags(reinterpret_cast<const int64_t*>(vec), (uint64_t)0); break;
      default: break;  // MSM_SCALAR_BIT: b = e = 1
    }
    return a;
  };
  // A wide vector's elements [i0, i1): whether any magnitude has a bit at or above sbits, or, for
  // Montgomery-form Fr, any a >= r (fr.cuh's test, the recode kernel's own).
  auto wide_bad = [&](const uint32_t* vec, size_t i0, size_t i1) -> bool {
    const uint32_t ew = ebits / 32;
    if (stype == STYPE_FR_MONT) {
      for (size_t i = i0; i < i1; i++)
        if (!fr_is_canonical(vec + i * 8)) return true;
      return false;
    }
    uint32_t acc[8] = {};  // the OR of the magnitudes, little-endian words
    for (size_t i = i0; i < i1; i++) {
      const uint32_t* e = vec + i * ew;
      if (stype == STYPE_I128 && (e[3] >> 31)) {
        uint32_t cy = 1;
        for (uint32_t k = 0; k < 4; k++) {
          const uint64_t x = (uint64_t)(~e[k]) + cy;
          acc[k] |= (uint32_t)x;
          cy = (uint32_t)(x >> 32);
        }
      } else {
        for (uint32_t k = 0; k < ew; k++) acc[k] |= e[k];
      }
    }
    for (uint32_t k = 0; k < ew; k++) {
      const uint32_t keep = sbits >= 32 * k + 32 ? 0xffffffffu : sbits > 32 * k ? (1u << (sbits - 32 * k)) - 1u : 0u;
      if (acc[k] & ~keep) return true;
    }
    return false;
  };
  auto host_scalars_ok = [&](DevCtx* c) -> bool {
    if (wide) {
      // (a 256-bit integer of 254 bits and more checks nothing, as the 254- and 255-bit word format)
      if (!host || (stype != STYPE_FR_MONT && (sbits >= ebits || sbits >= MAIN_BITS))) return true;
      for (size_t k = 0; k < count; k++) {
        if (k && scalars[k] == scalars[k - 1]) continue;
        std::atomic<uint32_t> any{0};
        auto scan = [&](int t, int nt) {
          if (wide_bad(scalars[k], terms * t / nt, terms * (t + 1) / nt)) any.store(1);
        };
        if (terms >= (1u << 17)) ctx_packer(c)->run(scan);
        else scan(0, 1);
        if (any.load()) return false;
      }
      return true;
    }
    if (stype) {
      if (!host || sbits >= ebits) return true;
      for (size_t k = 0; k < count; k++) {
        if (k && scalars[k] == scalars[k - 1]) continue;
        std::atomic<uint64_t> any{0};
        auto scan = [&](int t, int nt) { any.fetch_or(native_scan(scalars[k], terms * t / nt, terms * (t + 1) / nt)); };
        if (terms >= (1u << 17)) ctx_packer(c)->run(scan);
        else scan(0, 1);
        if (any.load() >> sbits) return false;
      }
      return true;
    }
    if (!host || sbits == 256 || !(sbits & 31u)) return true;
    const size_t sw = (sbits + 31) / 32;
    const uint32_t excess = ~((1u << (sbits & 31u)) - 1u);
    for (size_t k = 0; k < count; k++) {
      if (k && scalars[k] == scalars[k - 1]) continue;
      const uint32_t* v = scalars[k];
      std::atomic<uint32_t> any{0};
      auto scan = [&](int t, int nt) {
        uint32_t a = 0;
        for (size_t i = terms * t / nt, e = terms * (t + 1) / nt; i < e; i++) a |= v[i * sw];
        any.fetch_or(a);
      };
      if (terms >= (1u << 17)) ctx_packer(c)->run(scan);
      else scan(0, 1);
      if (any.load() & excess) return false;
    }
    return true;
  };
  return on_device(&o, [&](DevCtx* c) -> int {
    if (!b->alive) return MSM_ERR_INVALID_ARG;  // destroyed, or the library shut down, meanwhile
    if (!host_scalars_ok(c)) return MSM_ERR_INVALID_ARG;
    ManyInputs in;
    in.kind = host ? ManyInputs::HOST : ManyInputs::DEVICE;
    in.scalars = scalars;
    in.prepared = b->rec.as<uint32_t>();
    in.levels = levels;
    in.chunk_bits = b->geo.S;
    if (sub) {
      in.sub = subset_kind(levels, sub->first, indexed);
      in.sub_first = (size_t)sub->first;
      in.rec_n = b->n;
      in.indices = sub->indices;
    }
    return run_many(c, in, terms, count, &o, (hipStream_t)hip_stream, out, false);
  });
}
