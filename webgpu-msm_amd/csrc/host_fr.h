// Layer 14, scalar-field vectors (msm_fr_combine*, msm_fr_powers*, msm_fr_dot*): the entries' common
// paths.  Depends on the layers above it (knobs .. combine); the kernels are fr_kernels.cuh's.
#pragma once

static_assert(FR_FORM_WIRE == MSM_FR_WIRE && FR_FORM_MONT == MSM_FR_MONT, "the kernels' element forms");

bool fr_form_ok(uint32_t form) { return form == MSM_FR_WIRE || form == MSM_FR_MONT; }
// The options carry the device only.
bool fr_opts_ok(const msm_opts* o) {
  return bases_flags_ok(o) && !narrow_flagged(o) && !typed_flagged(o);
}
// Every element of a host vector in Montgomery form is below r.
bool fr_host_canonical(const uint32_t* v, size_t rows) {
  for (size_t i = 0; v && i < rows; i++)
    if (!fr_is_canonical(v + 8 * i)) return false;
  return true;
}
// Eight wire words (most significant first) as little-endian words.
void fr_from_wire(const uint32_t be[8], uint32_t le[8]) {
  for (int k = 0; k < 8; k++) le[k] = be[7 - k];
}
bool fr_ranges_overlap(const uint32_t* p, size_t p_rows, const uint32_t* q, size_t q_rows) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + q_rows * 32 && b < a + p_rows * 32;
}

// One vector operand of a call: its elements (null: absent) and how many rows it holds.
struct FrOperand {
  const uint32_t* p = nullptr;
  size_t rows = 0;
};

// The call frame of the three entries, on PointCall's (the error word, slot 0's stream behind the
// caller's, every exit): host operands go up into the slot's wire_pts, each from the next 256-byte
// boundary, after the entry has checked every one of them.
struct FrCall : PointCall {
  int open(DevCtx* ctx, hipStream_t user_stream) {
    const int r = begin(ctx);
    return r != MSM_OK ? r : after_user(user_stream);
  }
  // ops[k].p becomes the device copy.  Returns through done() on failure.
  int stage(FrOperand* ops, int count) {
    Slot& s0 = c->slot[0];
    size_t off[4] = {}, total = 0;
    for (int k = 0; k < count; k++) {
      off[k] = total;
      if (ops[k].p) total += (ops[k].rows * 32 + 255) / 256 * 256;
    }
    if (int r = s0.ws.wire_pts.ensure(total)) return done(r);
    const auto none = [](size_t, size_t) { return MSM_OK; };
    for (int k = 0; k < count; k++) {
      if (!ops[k].p) continue;
      uint32_t* dst = s0.ws.wire_pts.as<uint32_t>() + off[k] / 4;
      if (int r = upload(c, dst, ops[k].p, ops[k].rows * 32, ops[k].rows * 32, none)) return done(r);
      ops[k].p = dst;
    }
    if (hipEventRecord(c->ev_chunk[0], c->copy_stream) != hipSuccess ||
        hipStreamWaitEvent(s0.stream, c->ev_chunk[0], 0) != hipSuccess)
      return done(MSM_ERR_HIP);
    return MSM_OK;
  }
  // After the last launch: `rows` elements from d_src down to the host's dst (null: none), then the error word.
  int close(uint32_t* dst = nullptr, const uint32_t* d_src = nullptr, size_t rows = 0) {
    if (hipGetLastError() != hipSuccess) return done(MSM_ERR_HIP);
    if (dst && hipMemcpyAsync(dst, d_src, rows * 32, hipMemcpyDeviceToHost, stream()) != hipSuccess) return done(MSM_ERR_HIP);
    return finish();
  }
};

msm_opts fr_device_opts(const msm_opts* opts) {
  msm_opts od{};
  od.device = opts ? opts->device : -1;
  return od;
}

// msm_fr_combine*: out_i = x_i a_i +- y_i b_i mod r, one launch of k_fr_combine on slot 0's stream.  A host
// call's result comes down through the slot's dx_pts.
int fr_combine(const msm_fr_combine_t* cb, size_t m, bool host, const msm_opts* opts, hipStream_t user_stream,
               uint32_t* out) {
  if (!cb || !fr_opts_ok(opts)) return MSM_ERR_INVALID_ARG;
  constexpr uint32_t known = MSM_FR_SUB | MSM_FR_X_BROADCAST | MSM_FR_Y_BROADCAST;
  if ((cb->flags & ~known) || cb->reserved || !fr_form_ok(cb->in_form) || !fr_form_ok(cb->out_form))
    return MSM_ERR_INVALID_ARG;
  if (((cb->flags & MSM_FR_X_BROADCAST) && !cb->x) || ((cb->flags & MSM_FR_Y_BROADCAST) && !cb->y))
    return MSM_ERR_INVALID_ARG;
  if (!cb->b && (cb->y || (cb->flags & MSM_FR_SUB))) return MSM_ERR_INVALID_ARG;  // no second term to scale or subtract
  if (!m) return MSM_OK;
  if (!cb->a || !out || m >= (1ull << 32)) return MSM_ERR_INVALID_ARG;
  FrOperand ops[4];  // a, b, x, y
  ops[0] = {cb->a, m};
  ops[1] = {cb->b, cb->b ? m : 0};
  ops[2] = {cb->x, cb->x ? ((cb->flags & MSM_FR_X_BROADCAST) ? 1 : m) : 0};
  ops[3] = {cb->y, cb->y ? ((cb->flags & MSM_FR_Y_BROADCAST) ? 1 : m) : 0};
  if (host) {  // every element, before anything is uploaded
    if (cb->in_form == MSM_FR_MONT)
      for (const FrOperand& o : ops)
        if (!fr_host_canonical(o.p, o.rows)) return MSM_ERR_INVALID_ARG;
  } else {  // a device caller's pointers, from their values: `out` may be exactly a or exactly b
    if (!aligned16(out)) return MSM_ERR_INVALID_ARG;
    for (int k = 0; k < 4; k++) {
      if (!ops[k].p) continue;
      if (!aligned16(ops[k].p)) return MSM_ERR_INVALID_ARG;
      if (k < 2 && ops[k].p == out) continue;
      if (fr_ranges_overlap(out, m, ops[k].p, ops[k].rows)) return MSM_ERR_INVALID_ARG;
    }
  }
  uint32_t shape = (cb->b ? FR_SHAPE_B : 0u) | ((cb->flags & MSM_FR_SUB) ? FR_SHAPE_SUB : 0u);
  shape |= (ops[2].rows == 0 ? FR_OP_NONE : ops[2].rows == 1 && (cb->flags & MSM_FR_X_BROADCAST) ? FR_OP_BCAST : FR_OP_EACH);
  shape |= (ops[3].rows == 0 ? FR_OP_NONE : ops[3].rows == 1 && (cb->flags & MSM_FR_Y_BROADCAST) ? FR_OP_BCAST : FR_OP_EACH) << 2;
  const msm_opts od = fr_device_opts(opts);
  return on_device(&od, [&](DevCtx* c) -> int {
    Slot& s0 = c->slot[0];
    FrCall f;
    int r = f.open(c, user_stream);
    if (r != MSM_OK) return r;
    uint32_t* d_out = out;
    if (host) {
      if ((r = f.stage(ops, 4)) != MSM_OK) return r;
      if ((r = s0.ws.dx_pts.ensure(m * 32)) != MSM_OK) return f.done(r);
      d_out = s0.ws.dx_pts.as<uint32_t>();
    }
    const unsigned grid = std::min<unsigned>(grid_for(m, FR_THREADS), FR_COMBINE_CAP);
    hipLaunchKernelGGL(k_fr_combine, dim3(grid), dim3(FR_THREADS), 0, s0.stream, ops[0].p, ops[1].p, ops[2].p, ops[3].p,
                       d_out, m, shape, cb->in_form, cb->out_form, f.errp());
    return f.close(host ? out : nullptr, d_out, m);
  });
}

// a^e for a in Montgomery form, on the host.
void fr_pow_host(const uint32_t a[8], uint64_t e, uint32_t out[8]) {
  constexpr FrWords one = fr_r_power(1);
  uint32_t p[8];
  memcpy(p, one.v, 32);
  for (int bit = 63; bit >= 0; bit--) {
    fr_mont_mul(p, p, p);
    if ((e >> bit) & 1u) fr_mont_mul(p, a, p);
  }
  memcpy(out, p, 32);
}

// msm_fr_powers*: out_i = c g^i mod r, one launch of k_fr_powers of T lanes, FR_POW_STEPS elements a lane.
// The host turns g into Montgomery form, c into the output's form and raises g to the T-th power.
int fr_powers(const uint32_t* g_be, const uint32_t* c_be, size_t n, uint32_t out_form, bool host, const msm_opts* opts,
              hipStream_t user_stream, uint32_t* out) {
  if (!g_be || !fr_opts_ok(opts) || !fr_form_ok(out_form)) return MSM_ERR_INVALID_ARG;
  if (!n) return MSM_OK;
  if (!out || n >= (1ull << 32) || (!host && !aligned16(out))) return MSM_ERR_INVALID_ARG;
  const unsigned grid = grid_for(grid_for(n, FR_POW_STEPS), FR_THREADS);
  const uint64_t T = (uint64_t)grid * FR_THREADS;
  uint32_t tbits = 0;
  while ((1ull << tbits) < T) tbits++;
  FrElem g, gT, cf;
  uint32_t le[8];
  fr_from_wire(g_be, le);
  fr_to_mont(le, g.v);
  fr_pow_host(g.v, T, gT.v);
  constexpr FrWords r0 = fr_r_power(0), r1 = fr_r_power(1);
  if (c_be) fr_from_wire(c_be, le);
  else memcpy(le, r0.v, 32);
  if (out_form == MSM_FR_MONT) fr_to_mont(le, cf.v);
  else fr_mont_mul(le, r1.v, cf.v);  // c mod r
  const msm_opts od = fr_device_opts(opts);
  return on_device(&od, [&](DevCtx* c) -> int {
    Slot& s0 = c->slot[0];
    FrCall f;
    int r = f.open(c, user_stream);
    if (r != MSM_OK) return r;
    uint32_t* d_out = out;
    if (host) {
      if ((r = s0.ws.dx_pts.ensure(n * 32)) != MSM_OK) return f.done(r);
      d_out = s0.ws.dx_pts.as<uint32_t>();
    }
    hipLaunchKernelGGL(k_fr_powers, dim3(grid), dim3(FR_THREADS), 0, s0.stream, g, gT, cf, tbits, d_out, n, out_form);
    return f.close(host ? out : nullptr, d_out, n);
  });
}

// msm_fr_dot*: sum_i a_i b_i mod r (b null: sum_i a_i) into the host's out[8].  k_fr_dot_partial leaves one
// partial per workgroup in the slot's fr_part, k_fr_dot_final sums them into the element after the last.
int fr_dot(const uint32_t* a, const uint32_t* b, size_t n, uint32_t in_form, uint32_t out_form, bool host,
           const msm_opts* opts, hipStream_t user_stream, uint32_t* out) {
  if (!fr_opts_ok(opts) || !fr_form_ok(in_form) || !fr_form_ok(out_form)) return MSM_ERR_INVALID_ARG;
  if (!n) return MSM_OK;
  if (!a || !out || n >= (1ull << 32)) return MSM_ERR_INVALID_ARG;
  FrOperand ops[2] = {{a, n}, {b, b ? n : 0}};
  if (host) {
    if (in_form == MSM_FR_MONT && (!fr_host_canonical(a, n) || !fr_host_canonical(b, b ? n : 0))) return MSM_ERR_INVALID_ARG;
  } else if (!aligned16(a) || !aligned16(b)) {
    return MSM_ERR_INVALID_ARG;
  }
  const msm_opts od = fr_device_opts(opts);
  return on_device(&od, [&](DevCtx* c) -> int {
    Slot& s0 = c->slot[0];
    FrCall f;
    int r = f.open(c, user_stream);
    if (r != MSM_OK) return r;
    if (host && (r = f.stage(ops, 2)) != MSM_OK) return r;
    const unsigned grid = std::min<unsigned>(grid_for(n, FR_THREADS), FR_DOT_CAP);
    if ((r = s0.ws.fr_part.ensure(((size_t)grid + 1) * 32)) != MSM_OK) return f.done(r);
    uint32_t* part = s0.ws.fr_part.as<uint32_t>();
    hipLaunchKernelGGL(k_fr_dot_partial, dim3(grid), dim3(FR_THREADS), 0, s0.stream, ops[0].p, ops[1].p, n, in_form, part,
                       f.errp());
    hipLaunchKernelGGL(k_fr_dot_final, dim3(1), dim3(FR_THREADS), 0, s0.stream, part, grid, in_form, out_form);
    return f.close(out, part + (size_t)grid * 8, 1);
  });
}
