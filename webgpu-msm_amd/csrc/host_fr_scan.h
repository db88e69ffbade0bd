// Layer 15, scalar-field vectors, second set (msm_fr_inverse*, msm_fr_scan*, msm_fr_tensor*): the entries'
// common paths, on host_fr.h's call frame and argument rules.  The kernels are fr_scan_kernels.cuh's.
#pragma once

static_assert(FR_SCAN_OP_SUM == MSM_FR_SCAN_SUM && FR_SCAN_OP_EXCLUSIVE == MSM_FR_SCAN_EXCLUSIVE, "the scan kernels' flags");
static_assert(FR_TENSOR_MAX_K == MSM_FR_TENSOR_MAX_K, "the tensor kernel's arguments");

// c (eight wire words, null: 1) as the factor the kernels take in: c R^e_out mod r, canonical.
FrElem fr_first(const uint32_t* c_be, uint32_t out_form) {
  constexpr FrWords r0 = fr_r_power(0), r1 = fr_r_power(1);
  uint32_t le[8];
  if (c_be) fr_from_wire(c_be, le);
  else memcpy(le, r0.v, 32);
  FrElem cf;
  if (out_form == MSM_FR_MONT) fr_to_mont(le, cf.v);
  else fr_mont_mul(le, r1.v, cf.v);  // c mod r
  return cf;
}

// The rules msm_fr_inverse* and msm_fr_scan* share once their flags are checked: one input vector, one
// output vector of the same length, which a device caller may make the input itself.
int fr_unary_args(const uint32_t* a, size_t m, uint32_t in_form, bool host, const uint32_t* out) {
  if (!a || !out || m >= (1ull << 32)) return MSM_ERR_INVALID_ARG;
  if (host) return in_form == MSM_FR_MONT && !fr_host_canonical(a, m) ? MSM_ERR_INVALID_ARG : MSM_OK;
  if (!aligned16(a) || !aligned16(out)) return MSM_ERR_INVALID_ARG;
  return out != a && fr_ranges_overlap(out, m, a, m) ? MSM_ERR_INVALID_ARG : MSM_OK;
}

// msm_fr_inverse*: out_i = c / a_i mod r (0 for a zero), one launch of k_fr_inverse on slot 0's stream, at
// most grid_cap workgroups striding over the tiles (the entries' cap is FR_COMBINE_CAP; the test hook gives
// its own).
int fr_inverse(const uint32_t* a, const uint32_t* c_be, size_t m, uint32_t in_form, uint32_t out_form, bool host,
               const msm_opts* opts, hipStream_t user_stream, uint32_t* out, uint32_t grid_cap = FR_COMBINE_CAP) {
  if (!fr_opts_ok(opts) || !fr_form_ok(in_form) || !fr_form_ok(out_form) || !grid_cap) return MSM_ERR_INVALID_ARG;
  if (!m) return MSM_OK;
  if (int r = fr_unary_args(a, m, in_form, host, out)) return r;
  const FrElem cf = fr_first(c_be, out_form);
  const msm_opts od = fr_device_opts(opts);
  return on_device(&od, [&](DevCtx* c) -> int {
    Slot& s0 = c->slot[0];
    FrCall f;
    int r = f.open(c, user_stream);
    if (r != MSM_OK) return r;
    FrOperand op{a, m};
    uint32_t* d_out = out;
    if (host) {
      if ((r = f.stage(&op, 1)) != MSM_OK) return r;
      if ((r = s0.ws.dx_pts.ensure(m * 32)) != MSM_OK) return f.done(r);
      d_out = s0.ws.dx_pts.as<uint32_t>();
    }
    const size_t ntiles = (m + FR_TILE - 1) / FR_TILE;
    const unsigned grid = (unsigned)std::min<size_t>(ntiles, grid_cap);
    hipLaunchKernelGGL(k_fr_inverse, dim3(grid), dim3(FR_THREADS), 0, s0.stream, op.p, d_out, m, cf, in_form, out_form,
                       f.errp());
    return f.close(host ? out : nullptr, d_out, m);
  });
}

// The launch plan of a scan of m elements with at most `cap` spans: spans are whole tiles, none is empty,
// the last span and the last tile are ragged.  The entry and msm_test_fr_scan_plan both come here.
struct FrScanPlan {
  uint32_t e, tile, grid, tiles_per_span;
};
FrScanPlan fr_scan_plan(size_t m, uint32_t cap) {
  const size_t ntiles = (m + FR_TILE - 1) / FR_TILE;
  const size_t spans = std::min<size_t>(ntiles, cap);
  const size_t tps = spans ? (ntiles + spans - 1) / spans : 0;
  return FrScanPlan{FR_TILE_E, FR_TILE, tps ? (uint32_t)((ntiles + tps - 1) / tps) : 0u, (uint32_t)tps};
}

// msm_fr_scan*: the running product (times c) or sum of a, three launches on slot 0's stream --
// k_fr_scan_spans, k_fr_scan_totals, k_fr_scan_apply -- with the span totals and then the carries in the
// slot's fr_part.  No workgroup waits for another: the launches' order is the only dependence.
int fr_scan(const uint32_t* a, const uint32_t* c_be, size_t m, uint32_t flags, uint32_t in_form, uint32_t out_form,
            bool host, const msm_opts* opts, hipStream_t user_stream, uint32_t* out, uint32_t grid_cap = FR_SCAN_CAP) {
  constexpr uint32_t known = MSM_FR_SCAN_SUM | MSM_FR_SCAN_EXCLUSIVE;
  if (!fr_opts_ok(opts) || (flags & ~known) || !fr_form_ok(in_form) || !fr_form_ok(out_form)) return MSM_ERR_INVALID_ARG;
  const bool sum = flags & MSM_FR_SCAN_SUM;
  if ((sum && c_be) || !grid_cap || grid_cap > FR_SCAN_CAP) return MSM_ERR_INVALID_ARG;
  if (!m) return MSM_OK;
  if (int r = fr_unary_args(a, m, in_form, host, out)) return r;
  // a product runs in Montgomery form; a sum in the output's form, which its elements take on load (a
  // canonical Montgomery input that stays one is taken as it is)
  const int k_load = sum ? (in_form == MSM_FR_MONT && out_form == MSM_FR_MONT ? -1 : (int)out_form - (int)in_form + 1)
                         : (in_form == MSM_FR_MONT ? -1 : 2);
  FrElem first{};
  if (!sum) first = fr_first(c_be, out_form);
  const FrScanPlan pl = fr_scan_plan(m, grid_cap);
  const size_t span = (size_t)pl.tiles_per_span * pl.tile;
  const msm_opts od = fr_device_opts(opts);
  return on_device(&od, [&](DevCtx* c) -> int {
    Slot& s0 = c->slot[0];
    FrCall f;
    int r = f.open(c, user_stream);
    if (r != MSM_OK) return r;
    FrOperand op{a, m};
    uint32_t* d_out = out;
    if (host) {
      if ((r = f.stage(&op, 1)) != MSM_OK) return r;
      if ((r = s0.ws.dx_pts.ensure(m * 32)) != MSM_OK) return f.done(r);
      d_out = s0.ws.dx_pts.as<uint32_t>();
    }
    if ((r = s0.ws.fr_part.ensure((size_t)pl.grid * 32)) != MSM_OK) return f.done(r);
    uint32_t* part = s0.ws.fr_part.as<uint32_t>();
    hipLaunchKernelGGL(k_fr_scan_spans, dim3(pl.grid), dim3(FR_THREADS), 0, s0.stream, op.p, m, span, flags, in_form, k_load,
                       part, f.errp());
    hipLaunchKernelGGL(k_fr_scan_totals, dim3(1), dim3(FR_THREADS), 0, s0.stream, part, pl.grid, flags, first);
    hipLaunchKernelGGL(k_fr_scan_apply, dim3(pl.grid), dim3(FR_THREADS), 0, s0.stream, op.p, d_out, m, span, flags, in_form,
                       out_form, k_load, (const uint32_t*)part);
    return f.close(host ? out : nullptr, d_out, m);
  });
}

// msm_fr_tensor*: out_i = c prod_(j<k) (bit_j(i) ? hi_j : lo_j) for i < 2^k, one launch of k_fr_tensor of
// 2^tb lanes, tb = max(k - 4, 0).  The host turns the pairs into Montgomery form and multiplies out the
// products over the top k - tb bits, with c and the output's form in them.
int fr_tensor(const uint32_t* lo_be, const uint32_t* hi_be, uint32_t k, const uint32_t* c_be, uint32_t out_form, bool host,
              const msm_opts* opts, hipStream_t user_stream, uint32_t* out) {
  if (!fr_opts_ok(opts) || !fr_form_ok(out_form) || k > MSM_FR_TENSOR_MAX_K) return MSM_ERR_INVALID_ARG;
  if ((k && (!lo_be || !hi_be)) || !out || (!host && !aligned16(out))) return MSM_ERR_INVALID_ARG;
  const uint32_t tb = k > 4 ? k - 4 : 0, nhi = k - tb, steps = 1u << nhi;
  const size_t n = (size_t)1 << k;
  FrTensorArgs ta{};
  FrElem lo[MSM_FR_TENSOR_MAX_K], hi[MSM_FR_TENSOR_MAX_K];
  for (uint32_t j = 0; j < k; j++) {
    uint32_t le[8];
    fr_from_wire(lo_be + 8 * j, le);
    fr_to_mont(le, lo[j].v);
    fr_from_wire(hi_be + 8 * j, le);
    fr_to_mont(le, hi[j].v);
  }
  for (uint32_t j = 0; j < tb; j++) ta.lo[j] = lo[j], ta.hi[j] = hi[j];
  const FrElem cf = fr_first(c_be, out_form);
  for (uint32_t u = 0; u < steps; u++) {
    ta.high[u] = cf;
    for (uint32_t j = 0; j < nhi; j++) fr_mont_mul(ta.high[u].v, ((u >> j) & 1u ? hi : lo)[tb + j].v, ta.high[u].v);
  }
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
    hipLaunchKernelGGL(k_fr_tensor, dim3(grid_for((size_t)1 << tb, FR_THREADS)), dim3(FR_THREADS), 0, s0.stream, ta, tb, steps,
                       d_out, out_form);
    return f.close(host ? out : nullptr, d_out, n);
  });
}
