// Layer 12, fixed-base tables (msm_fixed_*): the table registry, the table build, and the evaluation
// entries' common path.  Depends on the layers above it (knobs .. bases).
#pragma once
// A table's state, kept as a handle's is (host_bases.h Bases): the caller's msm_fixed* is a registry
// token out of the handles' own counter, so no token names both a handle and a table; `rec` is freed,
// and `alive` cleared, under the owning device context's lock.
struct Fixed {
  int device = -1;
  uint32_t k = 0;   // bases
  uint32_t w = 0;   // window width
  uint32_t b = 0;   // widest scalar the table serves
  uint32_t Wn = 0;  // windows per base: fixed_windows(b, w)
  Buf rec;          // k Wn 2^(w-1) records, entry (j, win, d) at (j Wn + win) 2^(w-1) + d - 1
  bool alive = false;
  size_t records() const { return ((size_t)k * Wn) << (w - 1); }
  template <typename F>
  void each_buf(F&& f) {  // as Workspace::each_buf; the guard reports name a table's records as a handle's
    f("bases_rec", rec);
  }
};
std::map<uintptr_t, std::shared_ptr<Fixed>> g_fixed;  // under g_mu

std::shared_ptr<Fixed> find_fixed(const msm_fixed* h) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_fixed.find(reinterpret_cast<uintptr_t>(h));
  return it == g_fixed.end() ? nullptr : it->second;
}

// Every live table's records on `device` (DevCtx::destroy, under g_mu and the context's lock).
void release_fixed_on(int device) {
  for (auto& kv : g_fixed)
    if (kv.second->device == device) {
      kv.second->alive = false;
      kv.second->each_buf([](const char*, Buf& b) { b.release(); });
    }
}

// The shape of a table of k bases: window width (0: FX_AUTO_W, the width DESIGN.md §9's sweep chose),
// scalar width (0: 256), windows and records, inside the limits msm.h states.  Needs no device.
constexpr uint32_t FX_AUTO_W = 12;
constexpr uint64_t FX_MAX_BYTES = 256ull << 20;
struct FixedPlan {
  uint32_t w, b, Wn;
  uint64_t records, bytes;
};
int fixed_plan(uint64_t k, uint32_t w, uint32_t b, FixedPlan* out) {
  if (k < 1 || k > FX_MAX_BASES) return MSM_ERR_INVALID_ARG;
  if (!w) w = FX_AUTO_W;
  if (!b) b = 256;
  if (w < 2 || w > 16 || b > 256) return MSM_ERR_INVALID_ARG;
  out->w = w;
  out->b = b;
  out->Wn = fixed_windows(b, w);
  out->records = (k * out->Wn) << (w - 1);
  out->bytes = out->records * PRE_WORDS * 4;
  return out->bytes > FX_MAX_BYTES ? MSM_ERR_INVALID_ARG : MSM_OK;
}

// The shape of msm_fixed_create_vector's table: fixed_plan's rules with k up to VX_MAX_BASES, and for
// w = 0 the widest window in 2..VX_AUTO_W_MAX whose table stays within FX_MAX_BYTES (w = 2 always does).
// The sweep of DESIGN.md §9 chose it: a call's time followed its window count at every shape, whatever
// the table's size, so the widest table allowed is the fastest.  Needs no device.
constexpr uint32_t VX_AUTO_W_MAX = 12;
int vector_table_plan(uint64_t k, uint32_t w, uint32_t b, FixedPlan* out) {
  if (k < 1 || k > VX_MAX_BASES) return MSM_ERR_INVALID_ARG;
  if (!b) b = 256;
  if (b > 256) return MSM_ERR_INVALID_ARG;
  if (!w)
    for (w = VX_AUTO_W_MAX; w > 2; w--)
      if (((k * fixed_windows(b, w)) << (w - 1)) * PRE_WORDS * 4 <= FX_MAX_BYTES) break;
  if (w < 2 || w > 16) return MSM_ERR_INVALID_ARG;
  out->w = w;
  out->b = b;
  out->Wn = fixed_windows(b, w);
  out->records = (k * out->Wn) << (w - 1);
  out->bytes = out->records * PRE_WORDS * 4;
  return out->bytes > FX_MAX_BYTES ? MSM_ERR_INVALID_ARG : MSM_OK;
}

// How an evaluation over k > FX_MAX_BASES bases is cut (k_vector_eval, k_vector_fold): G bases per part,
// P = ceil(k / G) parts, the fold's passes ceil(log_VX_FOLD P), and the rows of one slab -- whole blocks
// of 64, as many as keep the partial buffer (the evaluation's P parts and the first pass's ceil(P / VX_FOLD),
// which later passes reuse) within the cap, one block at the least.  Needs no device.
// G: a launch wants VX_FULL_LANES lanes before it gives any of them more than one base (the fold's
// share of the additions is 1 / Wn whatever G is), so the largest G in 2..VX_MAX_GROUP with G sw <=
// VX_LANE_WORDS that still leaves m P >= VX_FULL_LANES, else 1.
constexpr uint64_t VEC_PART_MAX_BYTES = 256ull << 20;
constexpr uint64_t VX_FULL_LANES = 1ull << 18;
constexpr uint64_t VX_BLOCK_BYTES = (uint64_t)VX_PART_WORDS * FX_THREADS * 4;  // one part of 64 rows
std::atomic<uint64_t> g_vec_part_cap{VEC_PART_MAX_BYTES};  // msm_test_vector_slab
std::atomic<uint32_t> g_vec_group{0};                      // msm_test_vector_group: 0, or the G every plan takes
struct VectorPlan {
  uint32_t G, P, passes;
  uint64_t slab_rows, part_bytes;  // part_bytes: the partial buffer of one full slab
};
uint32_t vec_fold_parts(uint32_t parts) { return (parts + VX_FOLD - 1) / VX_FOLD; }
VectorPlan vector_plan(uint32_t k, uint64_t m, uint32_t sw) {
  VectorPlan v{};
  const uint32_t gmax = std::min(VX_MAX_GROUP, VX_LANE_WORDS / sw);
  v.G = 1;
  if (const uint32_t forced = g_vec_group.load()) {
    v.G = std::min(forced, gmax);
  } else {
    for (uint32_t g = gmax; g > 1; g--)
      if (m * ((k + g - 1) / g) >= VX_FULL_LANES) {
        v.G = g;
        break;
      }
  }
  v.P = (k + v.G - 1) / v.G;
  for (uint32_t p = v.P; p > 1; p = vec_fold_parts(p)) v.passes++;
  const uint64_t per_block = (uint64_t)(v.P + vec_fold_parts(v.P)) * VX_BLOCK_BYTES;
  const uint64_t blocks = std::max<uint64_t>(1, g_vec_part_cap.load() / per_block);
  v.slab_rows = std::min<uint64_t>(blocks, std::max<uint64_t>(1, (m + FX_THREADS - 1) / FX_THREADS)) * FX_THREADS;
  v.part_bytes = v.slab_rows / FX_THREADS * per_block;
  return v;
}

// msm_fixed_create and msm_fixed_create_vector (`vector`: k up to VX_MAX_BASES, vector_table_plan): the
// table of the k bases `sub` selects from a handle's level 0 (null: all of them), built on slot 0's
// stream -- k_fixed_build, or k_vector_build with the indices uploaded into the slot's sub_idx, writes
// every entry's x|y into the slot's dx_pts, and the preparation makes the records from there, as a
// compressed creation's does.
int fixed_create(const msm_bases* h, const msm_subset_t* sub, uint32_t w, uint32_t bits, const msm_opts* opts,
                 msm_fixed** out, bool vector = false) {
  if (!out) return MSM_ERR_INVALID_ARG;
  *out = nullptr;
  if (!h || !bases_flags_ok(opts) || narrow_flagged(opts)) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = find_bases(h);
  if (!b) return MSM_ERR_INVALID_ARG;
  if (opts && opts->device >= 0 && opts->device != b->device) return MSM_ERR_INVALID_ARG;
  const uint32_t* indices = sub && sub->indices ? sub->indices[0] : nullptr;
  const uint64_t k = sub ? sub->m : b->n, first = sub ? sub->first : 0;
  FixedPlan fp;
  if (int rc = vector ? vector_table_plan(k, w, bits, &fp) : fixed_plan(k, w, bits, &fp)) return rc;
  if (sub) {
    if (int rc = subset_check(b->n, 1, sub->first, sub->m, sub->indices != nullptr)) return rc;
    if (sub->indices && !indices) return MSM_ERR_INVALID_ARG;
  }
  FixedBaseIdx bi{};
  std::vector<uint32_t> idx(vector ? k : 0);  // (lives until the build has finished)
  for (uint32_t j = 0; j < k; j++) {
    const uint32_t v = indices ? indices[j] : (uint32_t)(first + j);
    if (v >= b->n) return MSM_ERR_INVALID_ARG;
    if (vector) idx[j] = v;
    else bi.v[j] = v;
  }
  auto t = std::make_shared<Fixed>();
  t->k = (uint32_t)k;
  t->w = fp.w;
  t->b = fp.b;
  t->Wn = fp.Wn;
  msm_opts od{};
  od.device = b->device;
  int rc = on_device(&od, [&](DevCtx* c) -> int {
    if (!b->alive) return MSM_ERR_INVALID_ARG;  // destroyed, or the library shut down, meanwhile
    t->device = c->device;
    Slot& s0 = c->slot[0];
    PointCall f;  // (no caller's stream to order after)
    int r = f.begin(c, &t->rec, fp.bytes);
    if (r != MSM_OK) return r;
    if ((r = s0.ws.dx_pts.ensure(fp.records * 64)) != MSM_OK) return f.done(r);
    uint32_t* xy = s0.ws.dx_pts.as<uint32_t>();
    if (vector) {
      if ((r = upload_words(c, {{&s0.ws.sub_idx, idx.data(), idx.size() * 4}})) != MSM_OK) return f.done(r);
      hipLaunchKernelGGL(k_vector_build, dim3(grid_for(fp.records, FX_THREADS)), dim3(FX_THREADS), 0, s0.stream,
                         b->rec.as<uint32_t>(), s0.ws.sub_idx.as<uint32_t>(), fp.w, fp.Wn, xy, (uint32_t)fp.records);
    } else {
      hipLaunchKernelGGL(k_fixed_build, dim3(grid_for(fp.records, FX_THREADS)), dim3(FX_THREADS), 0, s0.stream,
                         b->rec.as<uint32_t>(), bi, fp.w, fp.Wn, xy, (uint32_t)fp.records);
    }
    launch_prepare(xy, t->rec.as<uint32_t>(), (uint32_t)fp.records, f.errp(), 0u, s0.stream, PT_FMT_XY);
    return f.finish();
  });
  if (rc != MSM_OK) return rc;
  return register_handle(g_fixed, t, true, out);
}

// The device buffer k_fixed_eval leaves its points in: whole blocks of 64.
size_t fixed_proj_bytes(size_t m) { return (size_t)grid_for(m, FX_THREADS) * FX_THREADS * FX_PROJ_WORDS * 4; }

// The rows of a table of k > FX_MAX_BASES bases into proj, slab by slab on stream `s`: k_vector_eval
// writes the slab's P parts into the first half of `part`, k_vector_fold goes back and forth between
// the halves (at most ceil(P / VX_FOLD) parts after the first pass) until its last pass writes the
// slab's blocks of proj.  Each slab reads its own rows of the scalars; slab_rows is whole blocks, so a
// slab's scalars keep the vector's alignment.
void launch_vector_rows(const Fixed& t, const VectorPlan& vp, const uint32_t* d_sc, uint32_t sw, uint32_t width, size_t m,
                        uint32_t* part, uint32_t* proj, uint32_t* errp, hipStream_t s) {
  uint32_t* half[2] = {part, part + (size_t)vp.P * (vp.slab_rows / FX_THREADS) * VX_PART_WORDS * FX_THREADS};
  for (size_t row0 = 0; row0 < m; row0 += vp.slab_rows) {
    const uint32_t rows = (uint32_t)std::min<size_t>(vp.slab_rows, m - row0);
    const uint32_t nblk = grid_for(rows, FX_THREADS);
    hipLaunchKernelGGL(k_vector_eval, dim3(nblk, vp.P), dim3(FX_THREADS), FX_THREADS * vp.G * sw * 4, s,
                       t.rec.as<uint32_t>(), t.k, t.w, t.Wn, vp.G, d_sc + row0 * t.k * sw, sw, width, half[0], rows, errp);
    uint32_t parts = vp.P, from = 0;
    do {
      const uint32_t outs = vec_fold_parts(parts);
      uint32_t* dst = outs == 1 ? proj + row0 / FX_THREADS * FX_PROJ_WORDS * FX_THREADS : half[from ^ 1];
      hipLaunchKernelGGL(k_vector_fold, dim3(nblk, outs), dim3(FX_THREADS), 0, s, half[from], dst, parts,
                         outs == 1 ? 1u : 0u);
      parts = outs;
      from ^= 1;
    } while (parts > 1);
  }
}

// msm_fixed_mul*: Q_i = sum_j s_ij B_j for i < m, k_fixed_eval into the slot's fx_proj and
// k_fixed_normalise out of it, on slot 0's stream.  With `created` the points become a new handle: the
// x|y output goes through the preparation, as msm_bases_scale_create's does.  Else they are written to
// `points` as wire records (host entries: through the slot's dx_pts).  Host scalars go up into the
// slot's wire_pts after every one of them was checked.
int fixed_mul(const msm_fixed* h, const uint32_t* scalars, size_t m, bool host, const msm_opts* opts,
              hipStream_t user_stream, uint32_t* points, uint32_t levels, msm_bases** created) {
  if (created) *created = nullptr;
  if (!h || !bases_flags_ok(opts) || typed_flagged(opts)) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Fixed> t = find_fixed(h);
  if (!t) return MSM_ERR_INVALID_ARG;
  const uint32_t bits = opts && (opts->flags & MSM_FLAG_SCALAR_BITS) ? opts->scalar_bits : 256u;
  if (bits < 1 || bits > 256) return MSM_ERR_INVALID_ARG;
  const size_t sw = (bits + 31) / 32;
  // a narrow call may be no wider than the table; the 8-word call is read at the table's width
  if (opts && (opts->flags & MSM_FLAG_SCALAR_BITS) && bits > t->b) return MSM_ERR_INVALID_ARG;
  const uint32_t width = std::min(bits, t->b);
  if (opts && opts->device >= 0 && opts->device != t->device) return MSM_ERR_INVALID_ARG;
  if (m >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  const bool vec = t->k > FX_MAX_BASES;  // whichever creator made the table
  const VectorPlan vp = vec ? vector_plan(t->k, m, (uint32_t)sw) : VectorPlan{};
  if (vec && (uint64_t)m * vp.P >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  if (m && (!scalars || (!created && !points))) return MSM_ERR_INVALID_ARG;
  const uint32_t wb = opts ? opts->window_bits : 0;
  auto nb = std::make_shared<Bases>();
  if (created)
    if (int rc = bases_shape(nb.get(), m, levels, wb)) return rc;
  const size_t ksw = t->k * sw;
  if (!host && m && !point_call_ptrs_ok(scalars, sw, ksw, m, created ? nullptr : points)) return MSM_ERR_INVALID_ARG;
  if (host && width < 32 * sw) {  // every scalar, before anything is uploaded or enqueued
    const size_t wi = sw - 1 - ((width - 1) >> 5);  // the word that holds bit width - 1
    const uint32_t excess = (width & 31u) ? ~((1u << (width & 31u)) - 1u) : 0u;
    uint32_t any = 0;
    for (size_t i = 0; i < m * t->k; i++) {
      for (size_t q = 0; q < wi; q++) any |= scalars[i * sw + q];
      any |= scalars[i * sw + wi] & excess;
    }
    if (any) return MSM_ERR_INVALID_ARG;
  }
  msm_opts od{};
  od.device = t->device;
  int rc = on_device(&od, [&](DevCtx* c) -> int {
    if (!t->alive) return MSM_ERR_INVALID_ARG;  // destroyed, or the library shut down, meanwhile
    nb->device = c->device;
    if (!m) return MSM_OK;
    if (created)
      if (int prc = bases_plan_exists(c, *nb, wb)) return prc;
    Slot& s0 = c->slot[0];
    PointCall f;
    int r = f.begin(c, created ? &nb->rec : nullptr, (size_t)nb->levels * m * PRE_WORDS * 4);
    if (r != MSM_OK || (r = f.after_user(user_stream)) != MSM_OK) return r;
    const uint32_t* d_sc = scalars;
    uint32_t* d_out = points;
    if (host) {
      if ((r = upload_words(c, {{&s0.ws.wire_pts, scalars, m * ksw * 4}})) != MSM_OK) return f.done(r);
      d_sc = s0.ws.wire_pts.as<uint32_t>();
    }
    if ((r = point_call_output(s0, host, created, m, &d_out)) != MSM_OK) return f.done(r);
    if ((r = s0.ws.fx_proj.ensure(fixed_proj_bytes(m))) != MSM_OK) return f.done(r);
    uint32_t* proj = s0.ws.fx_proj.as<uint32_t>();
    if (vec) {
      if ((r = s0.ws.vx_part.ensure(vp.part_bytes)) != MSM_OK) return f.done(r);
      launch_vector_rows(*t, vp, d_sc, (uint32_t)sw, width, m, s0.ws.vx_part.as<uint32_t>(), proj, f.errp(), s0.stream);
    } else {
      hipLaunchKernelGGL(k_fixed_eval, dim3(grid_for(m, FX_THREADS)), dim3(FX_THREADS), FX_THREADS * ksw * 4, s0.stream,
                         t->rec.as<uint32_t>(), t->k, t->w, t->Wn, d_sc, (uint32_t)sw, width, proj, (uint32_t)m, f.errp());
    }
    hipLaunchKernelGGL(k_fixed_normalise, dim3(grid_for(m, FX_THREADS * FX_NORM_E)), dim3(FX_THREADS), 0, s0.stream,
                       proj, d_out, (uint32_t)m, created ? 0u : 1u);
    if (created) launch_created(*nb, d_out, m, f.errp(), s0.stream);
    return f.finish(host && !created ? points : nullptr, d_out, m);
  });
  if (rc != MSM_OK || !created) return rc;
  return register_bases(nb, created);
}
