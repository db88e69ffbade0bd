// Layer 13, pairwise combinations of bases handles (msm_bases_combine*): the entries' common path.
// Depends on the layers above it (knobs .. fixed).
#pragma once

// One side of a combination as the call reads it: the handle, the subset's range or index list, and
// the scalars (null: every scalar is 1) with their row count (1 for a broadcast scalar, else m).
struct CombineArm {
  std::shared_ptr<Bases> h;
  uint64_t first = 0;
  const uint32_t* indices = nullptr;
  const uint32_t* scalars = nullptr;
  size_t rows = 0;
  CombineSide side(const uint32_t* d_indices) const {
    return CombineSide{h->rec.as<uint32_t>(), d_indices, (uint32_t)h->n, (uint32_t)first};
  }
};

// msm_bases_combine*: R_i = a_i A_i +- b_i B_i for i < m, the A_i and B_i subsets of the level 0 of one
// handle or of two on one device.  One launch of k_combine_sum (no scalars), k_combine_one (one side's)
// or k_combine_joint (both) into the slot's fx_proj and k_fixed_normalise out of it, on slot 0's stream.
// With `created` the points become a new handle: the x|y output goes through the preparation, as
// msm_bases_scale_create's does.  Else they are written to `points` as wire records (host entries:
// through the slot's dx_pts).  Host scalars go up into the slot's wire_pts (a's, then b's) and host
// indices into sub_idx (a's, then b's) after every one of them was checked.
int bases_combine(const msm_bases* h, const msm_combine_t* cb, bool host, const msm_opts* opts, hipStream_t user_stream,
                  uint32_t* points, uint32_t levels, msm_bases** created) {
  if (created) *created = nullptr;
  if (!h || !cb || !bases_flags_ok(opts) || typed_flagged(opts)) return MSM_ERR_INVALID_ARG;
  const uint32_t bits = opts && (opts->flags & MSM_FLAG_SCALAR_BITS) ? opts->scalar_bits : 256u;
  if (bits < 1 || bits > 256) return MSM_ERR_INVALID_ARG;
  constexpr uint32_t known = MSM_COMBINE_SUB | MSM_COMBINE_A_BROADCAST | MSM_COMBINE_B_BROADCAST;
  if ((cb->flags & ~known) || cb->reserved || cb->a.m != cb->b.m) return MSM_ERR_INVALID_ARG;
  if (((cb->flags & MSM_COMBINE_A_BROADCAST) && !cb->a_scalars) || ((cb->flags & MSM_COMBINE_B_BROADCAST) && !cb->b_scalars))
    return MSM_ERR_INVALID_ARG;
  const size_t m = (size_t)cb->a.m;
  CombineArm arm[2];
  arm[0].h = find_bases(h);
  arm[1].h = cb->b_bases ? find_bases(cb->b_bases) : arm[0].h;
  if (!arm[0].h || !arm[1].h || arm[0].h->device != arm[1].h->device) return MSM_ERR_INVALID_ARG;
  if (opts && opts->device >= 0 && opts->device != arm[0].h->device) return MSM_ERR_INVALID_ARG;
  const size_t sw = (bits + 31) / 32;
  for (int s = 0; s < 2; s++) {
    const msm_subset_t& sub = s ? cb->b : cb->a;
    CombineArm& a = arm[s];
    if (int rc = subset_check(a.h->n, 1, sub.first, sub.m, sub.indices != nullptr)) return rc;
    a.first = sub.first;
    a.indices = sub.indices ? sub.indices[0] : nullptr;
    if (sub.indices && !a.indices && m) return MSM_ERR_INVALID_ARG;
    a.scalars = s ? cb->b_scalars : cb->a_scalars;
    a.rows = (cb->flags & (s ? MSM_COMBINE_B_BROADCAST : MSM_COMBINE_A_BROADCAST)) ? 1 : m;
  }
  if (m && !created && !points) return MSM_ERR_INVALID_ARG;
  const uint32_t wb = opts ? opts->window_bits : 0;
  auto nb = std::make_shared<Bases>();
  if (created)
    if (int rc = bases_shape(nb.get(), m, levels, wb)) return rc;
  for (const CombineArm& a : arm) {
    if (!m) break;
    if (!host) {  // a device caller's pointers, from their values
      if (a.scalars && !point_call_ptrs_ok(a.scalars, sw, sw, a.rows, created ? nullptr : points)) return MSM_ERR_INVALID_ARG;
      if ((reinterpret_cast<uintptr_t>(a.indices) & 3u) || (!created && (reinterpret_cast<uintptr_t>(points) & 15u)))
        return MSM_ERR_INVALID_ARG;
      const uintptr_t ip = reinterpret_cast<uintptr_t>(a.indices), pp = reinterpret_cast<uintptr_t>(points);
      if (a.indices && !created && ip < pp + m * 128 && pp < ip + m * 4) return MSM_ERR_INVALID_ARG;
      continue;
    }
    // every scalar and every index, before anything is uploaded or enqueued
    if (a.scalars && (bits & 31u)) {
      const uint32_t excess = ~((1u << (bits & 31u)) - 1u);
      uint32_t any = 0;
      for (size_t i = 0; i < a.rows; i++) any |= a.scalars[i * sw];
      if (any & excess) return MSM_ERR_INVALID_ARG;
    }
    for (size_t i = 0; a.indices && i < m; i++)
      if (a.indices[i] >= a.h->n) return MSM_ERR_INVALID_ARG;
  }
  msm_opts od{};
  od.device = arm[0].h->device;
  int rc = on_device(&od, [&](DevCtx* c) -> int {
    if (!arm[0].h->alive || !arm[1].h->alive) return MSM_ERR_INVALID_ARG;  // destroyed, or the library shut down, meanwhile
    nb->device = c->device;
    if (!m) return MSM_OK;
    if (created)
      if (int prc = bases_plan_exists(c, *nb, wb)) return prc;
    Slot& s0 = c->slot[0];
    PointCall f;
    int r = f.begin(c, created ? &nb->rec : nullptr, (size_t)nb->levels * m * PRE_WORDS * 4);
    if (r != MSM_OK || (r = f.after_user(user_stream)) != MSM_OK) return r;
    const uint32_t* d_sc[2] = {arm[0].scalars, arm[1].scalars};
    const uint32_t* d_ix[2] = {arm[0].indices, arm[1].indices};
    uint32_t* d_out = points;
    if (host) {
      // a's words, then b's from the next 256-byte boundary, in one buffer each for scalars and indices
      const size_t sc0 = arm[0].scalars ? (arm[0].rows * sw * 4 + 255) / 256 * 256 : 0;
      const size_t sc1 = arm[1].scalars ? arm[1].rows * sw * 4 : 0;
      const size_t ix0 = arm[0].indices ? (m * 4 + 255) / 256 * 256 : 0;
      const size_t ix1 = arm[1].indices ? m * 4 : 0;
      if ((sc0 + sc1 && (r = s0.ws.wire_pts.ensure(sc0 + sc1)) != MSM_OK) ||
          (ix0 + ix1 && (r = s0.ws.sub_idx.ensure(ix0 + ix1)) != MSM_OK))
        return f.done(r);
      const auto none = [](size_t, size_t) { return MSM_OK; };
      for (int s = 0; s < 2; s++) {
        if (arm[s].scalars) {
          uint32_t* dst = s0.ws.wire_pts.as<uint32_t>() + (s ? sc0 / 4 : 0);
          const size_t bytes = arm[s].rows * sw * 4;
          if ((r = upload(c, dst, arm[s].scalars, bytes, bytes, none)) != MSM_OK) return f.done(r);
          d_sc[s] = dst;
        }
        if (arm[s].indices) {
          uint32_t* dst = s0.ws.sub_idx.as<uint32_t>() + (s ? ix0 / 4 : 0);
          if ((r = upload(c, dst, arm[s].indices, m * 4, m * 4, none)) != MSM_OK) return f.done(r);
          d_ix[s] = dst;
        }
      }
      if (hipEventRecord(c->ev_chunk[0], c->copy_stream) != hipSuccess ||
          hipStreamWaitEvent(s0.stream, c->ev_chunk[0], 0) != hipSuccess)
        return f.done(MSM_ERR_HIP);
    }
    if ((r = point_call_output(s0, host, created, m, &d_out)) != MSM_OK) return f.done(r);
    if ((r = s0.ws.fx_proj.ensure(fixed_proj_bytes(m))) != MSM_OK) return f.done(r);
    uint32_t* proj = s0.ws.fx_proj.as<uint32_t>();
    const CombineSide A = arm[0].side(d_ix[0]), B = arm[1].side(d_ix[1]);
    const uint32_t sub = cb->flags & MSM_COMBINE_SUB ? 1u : 0u;
    const uint32_t bca = cb->flags & MSM_COMBINE_A_BROADCAST ? 1u : 0u;
    const uint32_t bcb = cb->flags & MSM_COMBINE_B_BROADCAST ? 1u : 0u;
    const dim3 grid(grid_for(m, CB_THREADS)), block(CB_THREADS);
    if (d_sc[0] && d_sc[1])
      hipLaunchKernelGGL(k_combine_joint, grid, block, 0, s0.stream, A, B, d_sc[0], d_sc[1], bca | bcb << 1, (uint32_t)sw,
                         bits, sub, proj, (uint32_t)m, f.errp());
    else if (d_sc[0])  // the ladder runs on A; the sign stays on B, the plain side
      hipLaunchKernelGGL(k_combine_one, grid, block, 0, s0.stream, A, B, d_sc[0], bca, (uint32_t)sw, bits, sub << 1, proj,
                         (uint32_t)m, f.errp());
    else if (d_sc[1])  // the ladder runs on B, negated before it
      hipLaunchKernelGGL(k_combine_one, grid, block, 0, s0.stream, B, A, d_sc[1], bcb, (uint32_t)sw, bits, sub, proj,
                         (uint32_t)m, f.errp());
    else
      hipLaunchKernelGGL(k_combine_sum, grid, block, 0, s0.stream, A, B, sub, proj, (uint32_t)m, f.errp());
    hipLaunchKernelGGL(k_fixed_normalise, dim3(grid_for(m, FX_THREADS * FX_NORM_E)), dim3(FX_THREADS), 0, s0.stream, proj,
                       d_out, (uint32_t)m, created ? 0u : 1u);
    if (created) launch_created(*nb, d_out, m, f.errp(), s0.stream);
    return f.finish(host && !created ? points : nullptr, d_out, m);
  });
  if (rc != MSM_OK || !created) return rc;
  return register_bases(nb, created);
}
