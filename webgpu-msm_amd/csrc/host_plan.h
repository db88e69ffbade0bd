// Layer 3, the planner: window widths, run lengths, launch plans, pipeline and fold geometry -- pure
// arithmetic, no HIP call.  Depends on host_knobs.h and host_ctx.h (Plan, DevShape).
#pragma once
uint32_t ilog2(uint32_t v) {
  uint32_t r = 0;
  while ((1u << (r + 1)) <= v) r++;
  return r;
}

// Window width for MSMs kept in flight by the pipelined entries (whole-job throughput rather
// than one MSM's latency): there the bucket reduction's work, not its latency, is what counts,
// so sub-2^20 sizes prefer narrower windows.  Measured on MI355X (tools/window_sweep.sh; round 2
// re-check with the current launch plan, profiles/r2ab_window_ab.jsonl): c = 14 at 2^16, 15 at
// 2^17..2^18, 16 from 2^19 (2^19: 0.584-0.592 vs 0.604-0.614 ms at c = 15).
uint32_t pipelined_window(size_t n) {
  // c = 16 from 7/8 of 2^19: 2^19 - 1 points ran 0.571-0.576 ms at c = 16 against 0.619-0.621 at
  // c = 15, 3/4 of 2^19 0.451-0.454 at c = 15 against 0.457-0.469 (tools/window_boundary_probe.sh)
  if (n >= (7u << 16)) return 16;
  if (n >= (1u << 17)) return 15;
  if (n >= (1u << 15)) return 14;
  return msm_best_window(n);
}

// The chunk lengths the first reduction stage is instantiated for, written out here alone (RED1_TABLE of
// host_launch.h has a row of kernels per entry); RED1_KNOB_ONLY is reachable only through MSM_RED_L.
#define RED1_LENGTHS(X) X(4), X(8), X(9), X(10), X(12), X(16), X(17), X(20)
constexpr uint32_t RED1_LS[] = {RED1_LENGTHS(uint32_t)};
constexpr uint32_t RED1_KNOB_ONLY = 4;
bool red_l_known(uint32_t L) { return std::count(std::begin(RED1_LS), std::end(RED1_LS), L) != 0; }

// Buckets per k_bucket_reduce_1 lane: the shortest chain (L) for which the live lanes of every
// MSM's main windows fit in one wave per SIMD (see msm_kernels.hip); 16 if none does.  Measured
// (profiles/r2i_ks17*): c = 15 with two MSMs per launch ran L = 8 as 1,056 waves -- two chains on
// some SIMDs, 140 us -- where L = 9 fits.  Chains past 16 serve the four-MSM launches of small
// sizes (2^17: L = 17, 994 waves).  MSM_RED_L overrides (any of RED1_LS).
uint32_t bucket_reduce_L(const MsmDims& d, const DevShape& sh) {
  const int n_cu = sh.n_cu;
  const uint32_t l_env = knob_red_l();
  if (red_l_known(l_env)) return l_env;
  const uint64_t simds = 4ull * (uint64_t)(n_cu > 0 ? n_cu : 256);
  for (uint32_t L : RED1_LS) {
    if (L == RED1_KNOB_ONLY) continue;
    const uint32_t nchunks = (d.B + L - 1) / L;
    uint64_t lanes = 0;
    for (uint32_t l = 0; l < d.Wr; l++) lanes += red1_live_chunks(d, L, nchunks, d.w0 + l);
    lanes *= d.nm;
    if ((lanes + 63) / 64 <= simds) return L;
  }
  return 16;
}

// The shortest run length that keeps random scalars off the skew joins.  A bucket that holds
// three whole runs (3 K + 2 entries or more) sends its workgroup to k_chain_join, and the launch
// through a second reduction (~0.25 ms at 2^20: DESIGN.md §2.4).  The largest buckets are the top
// main window's: its digits only reach p >> offset (p < 2^253; 9,551 values at c = 16), so at 2^20
// they hold ~110 entries each, against 32-64 in the other windows.  K is sized for the largest
// expected bucket of the launch's range, lambda + 5 sqrt(lambda) + 2 entries (Poisson, uniform
// scalars mod p).  This is what made 2^20 + 1 points 14% slower than 2^20 (round 4): K = 44 there,
// so a top-window bucket of ~134+ entries (one in ~10^4) held three runs in every launch.
uint32_t run_length_skew_floor(const MsmDims& d) {
  double lam_max = 0;
  for (uint32_t l = 0; l < d.Wr; l++) {
    const uint32_t w = d.w0 + l;
    if (w + 1 >= d.Wm) continue;  // the overflow window: empty for canonical scalars
    double vals = (double)(1u << (win_bits(d, w) - 1));
    // (a narrow launch's top window holds 2^(width - 1) values like the others: its top bit is
    // clear, and so are its negative digits)
    if (w + 2 == d.Wm && !d.sw) {  // the top main window: digits below (p >> off) + 1
      const uint32_t off = win_off(d, w);
      const double top = off >= 192 ? (double)(P[3] >> (off - 192)) + 1.0 : vals;
      vals = std::min(vals, top);
    }
    lam_max = std::max(lam_max, (double)d.n / vals);
  }
  const double maxb = lam_max + 5.0 * std::sqrt(lam_max) + 2.0;
  const uint32_t k = (uint32_t)std::floor((maxb - 2.0) / 3.0) + 1;  // 3 K + 2 > maxb
  return (k + 3) & ~3u;
}

// Run length K (entries per k_accumulate lane, a multiple of 4 for the 16-B entry loads): the
// accumulation holds sh.acc_waves waves per SIMD (4: VGPR- and LDS-bound, from the runtime's
// occupancy query for the device), so its lanes run in rounds of that many x 4 x CUs waves.
// - A launch under one round at K = 64 takes the smallest K that fills the round (2^17, four MSMs:
//   K = 36, 3,868 waves, where K = 32 needed 4,352: a 6% second round that runs on few SIMDs).
// - Pipelined launches past one round take the K of whole rounds (2^20, two MSMs: K = 64, two
//   rounds) unless that K is under the skew floor: then K = 64 (or the floor), and the next
//   launch's kernels fill whatever a short last round leaves idle.  2^20 + 1 points, two MSMs:
//   1.030 ms per MSM at K = 64 against 1.062 at K = 68 (two rounds) and 1.170 at the balanced
//   K = 44 (skew joins) (profiles/r5/run_length.jsonl).
// - A lone MSM past one round (its latency counts, and nothing fills its tail) takes the K up to
//   128 whose whole rounds cost least (rounds x K): 2^20 + 1 points run one round of K = 68.
// K never drops below run_length_skew_floor.  (Upper bound of the entries: every main-window
// digit nonzero.)
uint32_t run_length_for(const MsmDims& d, const DevShape& sh, bool pipelined) {
  // main windows of the launch's range (the overflow window holds no entry for canonical scalars)
  const uint64_t nmain = d.Wr - ((d.w0 + d.Wr == d.Wm) ? 1u : 0u);
  const uint64_t m = (uint64_t)d.nm * std::max<uint64_t>(1, nmain) * d.n;
  const uint64_t round_lanes =
      64ull * (uint64_t)std::max(1, sh.acc_waves) * 4 * (uint64_t)(sh.n_cu > 0 ? sh.n_cu : 256);
  const uint64_t kfloor = std::max<uint64_t>(16, run_length_skew_floor(d));
  const uint64_t r64 = std::max<uint64_t>(1, (m + 64 * round_lanes - 1) / (64 * round_lanes));
  uint64_t K;
  if (r64 == 1) {
    K = (m + round_lanes - 1) / round_lanes;  // one round
  } else if (pipelined) {
    // whole rounds of a shorter K where that clears the skew floor (2^18, four MSMs: K = 36,
    // 0.332-0.337 ms per MSM against 0.340-0.342 at K = 64), else K = 64
    K = (m + r64 * round_lanes - 1) / (r64 * round_lanes);
    K = (K + 3) & ~3ull;
    if (K < kfloor) K = std::max<uint64_t>(64, kfloor);
  } else {
    uint64_t best = ~0ull;
    K = 64;
    for (uint64_t k = 16; k <= 128; k += 4) {
      if (k < kfloor) continue;
      const uint64_t cost = (m + k * round_lanes - 1) / (k * round_lanes) * k;
      if (cost < best) best = cost, K = k;
    }
  }
  K = (K + 3) & ~3ull;
  return (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(kfloor, K));
}

int finish_plan(const MsmDims& d, const msm_opts* o, const DevShape& sh, Plan* pl, bool pipelined = false);

// A subset launch on a handle's records (msm_bases_compute_subset*): the plan's n is levels * m
// terms, but its entries index the handle's whole record space, levels * rec_n records.
struct SubsetGeo {
  uint32_t kind = MSM_SUB_NONE;  // MSM_SUB_RANGE / MSM_SUB_INDEXED
  uint32_t levels = 1;
  size_t rec_n = 0;  // the handle's n: records per level
  size_t first = 0;  // range form
};

constexpr uint32_t NARROW_WIDE_C = 17, NARROW_DENSE = 64;  // the narrow launches' auto width (make_plan)

// Native scalar types (include/msm.h MSM_FLAG_SCALAR_TYPE): element bits e and signedness of a
// MSM_SCALAR_* value (e = 0: unknown), and the type an options struct carries (0: none).
// Wide types (MSM_FLAG_SCALAR_FIELD) share the plan's one type field and every function below: inside
// the library MSM_FIELD_x is the type STYPE_WIDE | MSM_FIELD_x (the public MSM_SCALAR_* values stay nine).
constexpr uint32_t STYPE_WIDE = 0x100u;
constexpr uint32_t STYPE_U128 = STYPE_WIDE | MSM_FIELD_U128, STYPE_I128 = STYPE_WIDE | MSM_FIELD_I128,
                   STYPE_U256 = STYPE_WIDE | MSM_FIELD_U256, STYPE_FR_MONT = STYPE_WIDE | MSM_FIELD_FR_MONT;
bool stype_wide(uint32_t type) { return (type & STYPE_WIDE) != 0; }
uint32_t scalar_type_bits(uint32_t type) {
  switch (type) {
    case STYPE_U128: case STYPE_I128: return 128;
    case STYPE_U256: case STYPE_FR_MONT: return 256;
    case MSM_SCALAR_BIT: return 1;
    case MSM_SCALAR_U8: case MSM_SCALAR_I8: return 8;
    case MSM_SCALAR_U16: case MSM_SCALAR_I16: return 16;
    case MSM_SCALAR_U32: case MSM_SCALAR_I32: return 32;
    case MSM_SCALAR_U64: case MSM_SCALAR_I64: return 64;
    default: return 0;
  }
}
bool scalar_type_signed(uint32_t type) { return (type >= MSM_SCALAR_I8 && type <= MSM_SCALAR_I64) || type == STYPE_I128; }
bool typed_flagged(const msm_opts* o) { return o && (o->flags & (MSM_FLAG_SCALAR_TYPE | MSM_FLAG_SCALAR_FIELD)); }
// (both flags together, or a value outside its flag's table: a type of no width, which typed_width refuses)
uint32_t opts_scalar_type(const msm_opts* o) {
  if (!typed_flagged(o)) return 0u;
  const msm_opts_typed* t = reinterpret_cast<const msm_opts_typed*>(o);
  if (!(o->flags & MSM_FLAG_SCALAR_FIELD)) return t->scalar_type & STYPE_WIDE ? ~0u : t->scalar_type;
  if ((o->flags & MSM_FLAG_SCALAR_TYPE) || t->scalar_field >= STYPE_WIDE) return ~0u;
  return STYPE_WIDE | t->scalar_field;
}
// The magnitude bits b of a typed call: scalar_bits where MSM_FLAG_SCALAR_BITS is set (1..e; a bit
// vector's must be 1), else e.  A Montgomery-form Fr is below r < 2^251: b = 251, said or unsaid.
// 0: an argument error.
uint32_t typed_width(uint32_t type, bool has_bits, uint32_t bits) {
  const uint32_t e = scalar_type_bits(type);
  if (!e) return 0;
  if (type == STYPE_FR_MONT) return !has_bits || bits == FR_BITS ? FR_BITS : 0;
  if (!has_bits) return e;
  return bits >= 1 && bits <= e ? bits : 0;
}
// Bytes of a vector of n elements, and of its region in a slot's wire buffer (whole 16-B units, so
// that every MSM's vector starts aligned for the recode's vector loads).
size_t typed_vector_bytes(size_t n, uint32_t type) { return (n * scalar_type_bits(type) + 7) / 8; }
size_t typed_region_bytes(size_t n, uint32_t type) { return (typed_vector_bytes(n, type) + 15) & ~(size_t)15; }

int make_plan(size_t n, const msm_opts* o, const DevShape& sh, Plan* pl, bool pipelined = false, uint32_t nm = 1,
              bool shared = false, const SubsetGeo* sub = nullptr) {
  *pl = Plan{};
  uint32_t c = (o && o->window_bits) ? o->window_bits : pipelined ? pipelined_window(n) : msm_best_window(n);
  if (c < 4 || c > 20) return MSM_ERR_UNSUPPORTED_WINDOW;
  if (n >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  MsmDims d{};
  d.n = (uint32_t)n;
  d.c = c;
  // balanced main windows of at most c bits over MAIN_BITS, plus the overflow window
  const uint32_t wm = (MAIN_BITS + c - 1) / c;
  d.q = MAIN_BITS / wm;
  d.nhi = MAIN_BITS - d.q * wm;
  d.Wm = wm + 1;
  d.nm = nm;
  d.w0 = 0;
  d.Wr = d.Wm;
  d.half_lo = d.half_hi = 0;
  if (o && (o->flags & MSM_FLAG_SCALAR_BITS)) {
    // Narrow scalars (msm_bases_compute* only; every other entry has refused the flag): below 254
    // bits the windows are balanced over the scalar's own T = max(b + 1, 4) bits -- one bit more
    // than the scalar has, so the top window's top bit is clear, its value plus the carry is at
    // most 2^(width - 1) and nothing carries out.  Wm keeps counting an overflow window that the
    // range [0, Wm - 1) leaves out (msm_dev.h).  254 bits and more are the 8-word launch as it is.
    const uint32_t b = o->scalar_bits;
    if (b < 1 || b > 256 || (o->flags & MSM_FLAG_WINDOWS)) return MSM_ERR_INVALID_ARG;
    if (b < MAIN_BITS) {
      const uint32_t T = std::max(b + 1, 4u);
      auto widest = [&](uint32_t cw) { return (T + (T + cw - 1) / cw - 1) / ((T + cw - 1) / cw); };
      // The auto width: a short scalar balanced at the size's usual width may end up with a few
      // narrow windows whose buckets hold hundreds of entries each (b = 16 at c = 16 is 9 + 8 bits:
      // 4,096 entries per bucket at 2^20, 9.89 ms against 0.26 ms as one 17-bit window).  From
      // NARROW_DENSE entries per bucket of the widest window the launch takes NARROW_WIDE_C = 17
      // where that widens the windows: profiles/bases_narrow_sweep.jsonl, every (n, b) row at that
      // density or more is faster at c = 17 awaited and within 0.004 ms pipelined (2^20, b = 64: 0.41
      // against 0.63 ms; b = 128: 0.63 against 0.77), the rows at 16 per bucket are not (2^16, b = 128:
      // 0.110 against 0.070 ms per MSM pipelined), and c = 19 triples the reduction (same file,
      // b = 128: 0.234 + 0.133 against 0.076 + 0.047 ms).
      if (!o->window_bits && c < NARROW_WIDE_C && ((uint64_t)n >> (widest(c) - 1)) >= NARROW_DENSE &&
          widest(NARROW_WIDE_C) > widest(c))
        c = NARROW_WIDE_C;
      const uint32_t wn = (T + c - 1) / c;
      d.q = T / wn;
      d.nhi = T - d.q * wn;
      d.Wm = wn + 1;
      d.Wr = wn;
      d.sw = (b + 31) / 32;
      d.sbits = b;
      // a native type: the narrow geometry of b as it is; the plan only remembers the type
      if (const uint32_t ty = opts_scalar_type(o)) {
        if (typed_width(ty, true, b) != b) return MSM_ERR_INVALID_ARG;
        pl->stype = ty;
        pl->sc_bytes = typed_vector_bytes(n, ty);
      }
    } else if (typed_flagged(o)) {
      return MSM_ERR_INVALID_ARG;
    }
  } else if (typed_flagged(o)) {
    // (the entry resolves an unset width to the element's before it plans)  Only a 256-bit integer of
    // 254 bits and more comes here unset: the full-width geometry above as it is, on little-endian words.
    if (opts_scalar_type(o) != STYPE_U256 || (o->flags & MSM_FLAG_WINDOWS)) return MSM_ERR_INVALID_ARG;
    pl->stype = STYPE_U256;
    pl->sc_bytes = typed_vector_bytes(n, STYPE_U256);
  }
  if (o && (o->flags & MSM_FLAG_WINDOWS)) {
    // a window range needs an explicit width, so that every caller's ranges cut the same windows
    const uint32_t units = (o->flags & MSM_FLAG_HALF_WINDOWS) ? 2u : 1u;
    if (!o->window_bits || o->window_lo >= o->window_hi || o->window_hi > units * d.Wm) return MSM_ERR_INVALID_ARG;
    d.w0 = o->window_lo / units;
    d.Wr = (o->window_hi + units - 1) / units - d.w0;
    if (units == 2) {
      d.half_lo = o->window_lo & 1u;  // starts at window w0's upper half
      d.half_hi = o->window_hi & 1u;  // ends after window w0 + Wr - 1's lower half
    }
  }
  d.W = d.Wr * nm;
  d.c = d.nhi ? d.q + 1 : d.q;
  d.B = 1u << (d.c - 1);
  // Coarse bins: aim at ~4K entries per bin (half the LDS staging capacity of k_fine_sort) with at
  // most FS_MAXF buckets per bin.  Partition chunks hold >= 64 entries per bin slice.
  uint32_t nbc = 1;
  while (nbc < d.B && nbc < 256 && (size_t)nbc * 4096 < n) nbc <<= 1;
  while (nbc < d.B && (d.B / nbc) > FS_MAXF) nbc <<= 1;
  d.nbc = nbc;
  d.fb = ilog2(d.B / nbc);
  d.shared = shared ? 1u : 0u;
  uint64_t npts = shared ? n : (uint64_t)nm * n;  // point records the entries index
  if (sub && sub->kind != MSM_SUB_NONE) {
    // every count follows the launch's levels * m terms; the entry width alone follows the records
    npts = (uint64_t)sub->levels * sub->rec_n;
    if (npts >= (1ull << 30) || sub->first >= (1ull << 30) || n % sub->levels) return MSM_ERR_INVALID_ARG;
    d.sub = sub->kind;
    d.rstride = (uint32_t)sub->rec_n;
    d.first = (uint32_t)sub->first;
    d.sm = (uint32_t)(n / sub->levels);
  }
  d.packed = npts <= (1ull << (31 - d.fb)) ? 1u : 0u;
  d.nbins = d.W * d.nbc;
  d.ch = PT_THREADS * PS_R;  // 16384 digits per partition chunk (>= 64 per bin slice while nbc <= 256)
  d.nch = (uint32_t)((n + d.ch - 1) / d.ch);
  return finish_plan(d, o, sh, pl, pipelined);
}

// ---- the dense-bucket accumulation (k_dense_segments / k_dense_units / k_dense_fold) -------------
// A narrow launch whose buckets hold DENSE_MIN entries or more (n over the buckets of its widest
// window) and whose key space is at most DENSE_MAX_KEYS takes the dense accumulation in the place of
// k_accumulate.  There k_accumulate is short of lanes: run_length_skew_floor keeps K above a third
// of the largest bucket, so the launch has ~3 lanes per bucket whatever n is (2^20 bytes in one
// 9-bit window: ~710 lanes of ~1,476 dependent adds, 4.964 of the launch's 5.111 ms).  A dense unit
// pays a six-level tree (~8 adds of a whole wave) per segment instead, whatever the segment holds, so
// the path wins where buckets are large and few, and loses where the keys alone fill the machine.
// profiles/bases_dense_sweep.jsonl (tools/bases_probe.py --dense), ms awaited device-resident /
// ms per MSM pipelined, path on against off (MSM_DENSE_MIN=1 / 2^30):
//   b = 8, 256 keys (x 4 pipelined), 32 / 64 / 128 / 256 per bucket (2^13..2^16):
//     0.212 / 0.214 / 0.218 / 0.220 against 0.247 / 0.288 / 0.377 / 0.580 awaited,
//     0.024 / 0.025 / 0.026 / 0.033 against 0.026 / 0.033 / 0.048 / 0.077 pipelined: on wins from 32
//   b = 12, 4,096 keys (x 4, x 2 at 2^19), 32 / 64 / 128 per bucket (2^17..2^19):
//     0.278 / 0.283 / 0.295 against 0.260 / 0.321 / 0.419 awaited,
//     0.126 / 0.133 / 0.162 against 0.048 / 0.061 / 0.163 pipelined: on loses below 128, level at 128
//     (and wins at 256, 2^20: 0.393 against 0.605, 0.185 against 0.254)
//   b = 13, 8,192 keys (x 2: 16,384), 128 per bucket (2^20): 0.418 against 0.422 awaited,
//     0.284 against 0.170 pipelined; b = 14 / 15 (16,384 / 32,768 keys, 64 / 32 per bucket): 0.608 /
//     1.001 against 0.332 / 0.282 awaited.
// So DENSE_MIN stays at 128 -- also where the skew floor first pushes K past its usual 64 (lambda =
// 128: K = 64; 192: K = 88) -- since below it only the launches of few keys gain, and DENSE_MAX_KEYS
// is 8,192, the most keys a measured row wins or draws with (the two-MSM 2^20 launch of 12-bit
// scalars; 16,384 keys at 128 per bucket lose by two thirds).  k_dense_segments, one workgroup, then
// walks 8 keys per thread.  MSM_DENSE_MIN overrides the threshold.
constexpr uint32_t DENSE_MIN = 128;
constexpr uint32_t DENSE_MAX_KEYS = 1u << 13;
constexpr uint32_t DENSE_K = 4096;  // a dense plan's run length: it sizes run_key and the cross_key index only

bool dense_launch(const MsmDims& d) {
  const uint32_t dmin = knob_dense_min() ? knob_dense_min() : DENSE_MIN;
  return d.sw != 0 && (d.n >> (d.c - 1)) >= dmin && (uint64_t)d.W * d.B <= DENSE_MAX_KEYS;
}
// The unit kernel's grid for segments of 64 E entries: sum_k ceil(s_k / S) <= floor(M / S) + #nonempty
// for any bucket sizes s_k of sum M <= Mmax over nkeys buckets.
uint64_t dense_unit_bound(uint64_t Mmax, uint32_t nkeys, uint32_t E) { return Mmax / (64ull * E) + nkeys; }
// Entries per unit lane: the smallest multiple of 4 in 4..64 whose grid is one round of resident
// waves (sh.dense_waves per SIMD, the runtime's occupancy query for k_dense_units) -- a unit pays a
// six-level tree whatever E is, so no more units than the machine holds at once -- and past one
// round at E = 64, the smallest E of that many whole rounds.
uint32_t dense_entries(uint64_t Mmax, uint32_t nkeys, const DevShape& sh) {
#ifdef MSM_DENSE_E
  return MSM_DENSE_E;  // tuning builds: one E for every launch (make variant NAME=e16 DEFS=-DMSM_DENSE_E=16)
#endif
  const uint64_t round = (uint64_t)std::max(1, sh.dense_waves) * 4 * (uint64_t)(sh.n_cu > 0 ? sh.n_cu : 256);
  const uint64_t rounds = std::max<uint64_t>(1, (dense_unit_bound(Mmax, nkeys, 64) + round - 1) / round);
  for (uint32_t E = 4; E < 64; E += 4)
    if (dense_unit_bound(Mmax, nkeys, E) <= rounds * round) return E;
  return 64;
}

// The reduction's fields of a plan whose geometry is set, for chunks of L buckets (finish_plan; the
// test hooks of host_test_hooks.h give an L of their own).
void plan_chunks(Plan* pl, uint32_t L) {
  pl->L = L;
  pl->nchunks = (pl->d.B + L - 1) / L;
  // every k_bucket_reduce_2 workgroup sums at most pow2ceil(nchunks)/2 points (the R_k terms' size)
  pl->nv = pl->nchunks >= 2 ? 2 : 1;
  uint32_t cbits = 0;
  while ((1u << cbits) < pl->nchunks) cbits++;
  pl->nterms = pl->nv + cbits;
}

// The launch-shape fields that follow from the geometry d.
int finish_plan(const MsmDims& d, const msm_opts* o, const DevShape& sh, Plan* pl, bool pipelined) {
  const size_t n = d.n;
  pl->d = d;
  pl->dense = dense_launch(d) ? 1u : 0u;
  // (a dense plan's K is not governed by the skew floor: no lane walks a run)
  pl->K = (o && o->run_length) ? o->run_length : pl->dense ? DENSE_K : run_length_for(d, sh, pipelined);
  if (pl->K < 1 || pl->K > 4096) return MSM_ERR_INVALID_ARG;
  if (pl->dense) {
    pl->dense_E = dense_entries((uint64_t)d.W * n, d.W * d.B, sh);
    pl->dense_units = (uint32_t)dense_unit_bound((uint64_t)d.W * n, d.W * d.B, pl->dense_E);
  }
  plan_chunks(pl, bucket_reduce_L(d, sh));
  pl->Mmax = (size_t)d.W * n;
  pl->runs_max = (pl->Mmax + pl->K - 1) / pl->K + 1;
  if (pl->Mmax >= (1ull << 31)) return MSM_ERR_INVALID_ARG;
  return MSM_OK;
}

// The second bucket-reduction stage as k_red2_groups + k_red2_terms (default; MSM_RED2_TREE=0:
// k_bucket_reduce_2), for windows of at most RG_MAXG groups of RG_CH chunks (k_bucket_reduce_2
// past that).  Single stream, 2^20, two MSMs per launch: 50 against 58 us.
uint32_t red2_groups(const Plan& pl) { return (pl.nchunks + RG_CH - 1) / RG_CH; }
bool red2_tree(const Plan& pl) { return knob_red2_tree() && red2_groups(pl) <= RG_MAXG; }

// MSMs kept in flight by the pipelined entries.  Small MSMs are latency-bound (their reduction
// and sort kernels leave most of the chip idle), so several run side by side; MSM_SLOTS
// overrides (1 = everything in order on one stream: clean per-kernel profiles), and so does the
// MSM_FLAG_SERIAL option flag.
int pipeline_slots(size_t n, const msm_opts* o) {
  if (o && (o->flags & MSM_FLAG_SERIAL)) return 1;
  if (knob_slots() >= 1) return std::min(knob_slots(), NSLOT);
  (void)n;
  // Two launches in flight.  Round 1 measured three best (one or two MSMs per launch); with two
  // to four MSMs per launch and the one-wave-per-SIMD reduction, two beat three at every size
  // (profiles/r2s_slots_ab.jsonl, ms per MSM, 50 steps: 2^16 0.137 vs 0.145-0.175, 2^17
  // 0.210-0.236 vs 0.219-0.222, 2^18 0.354-0.358 vs 0.374, 2^20 1.083-1.114 vs 1.095-1.128).
  return 2;
}

// MSMs per launch (batch) for the pipelined entries: the latency-bound kernels (reduction trees,
// scans, small sorts) of two MSMs fill the machine together.  Measured on MI355X
// (tools/batch_sweep.sh, ms per MSM, batch 1 -> 2): 2^16 0.218 -> 0.162, 2^17 0.273 -> 0.247,
// 2^18 0.420 -> 0.381, 2^19 0.679 -> 0.638, 2^20 1.162 -> 1.136.  Four per launch up to 2^18,
// measured once the reduction kept one wave per SIMD and two launches are in flight
// (profiles/r2mn_*, r2y_*): 2^17 0.268 -> 0.248, 2^18 0.363 -> 0.347 ms per MSM; 2^19 +1.5%,
// 2^20 +4.5% (kept at two).  Eight up to 2^16: a four-MSM 2^16 launch costs ~0.64 ms of pipeline
// time and an eight-MSM one ~1.04 (profiles/r3/batch_sizes.txt: 0.13 against 0.16 ms per MSM over
// 50 MSMs, the last launch padded; 2^17 and 2^18 are 2-13% slower with eight), so eight is taken
// whenever its launches, padded last one included, cost less: ceil(count/8) * 13 < ceil(count/4) * 8.
// Two also above 2^20, up to 2^21: 2^21 measured 2.31-2.33 ms per MSM with two against 2.36-2.43
// with one, and one extra point past 2^20 cost 17% with one per launch
// (1.194 against 1.023 ms, profiles/r4/pipelined_sizes.jsonl).  MSM_BATCH overrides (1..MSM_MAX_BATCH).
uint32_t pipeline_batch(size_t n, size_t count) {
  const int env = knob_batch();
  uint32_t nm = env >= 1 ? (uint32_t)std::min(env, (int)MSM_MAX_BATCH)
                         : (n <= (1u << 18) ? 4u : n <= (1u << 21) ? 2u : 1u);
  if (env < 1 && n <= (1u << 16) && count >= 8 && (count + 7) / 8 * 13 < (count + 3) / 4 * 8) nm = 8;
  return (uint32_t)std::max<size_t>(1, std::min<size_t>(nm, count));
}

// ---- resident prepared bases (msm_bases_*, include/msm.h) ----------------------------------------
// The fold geometry of `levels` = k shifted levels at window width c: with the
// library's balanced windows (make_plan), Wc is the smallest window count whose offset, less one
// bit, times k covers the 256 scalar bits, and the chunk is S = off(Wc) - 1 bits: one bit less than
// windows [0, Wc) hold, so the top window's value plus its carry is at most 2^(b-1) and nothing
// carries out of the range.  k = 1 is the plain MSM: every window, no cut (S reported as 256).
struct BasesGeo {
  uint32_t c, Wc, S;
};
bool bases_geometry(uint32_t c, uint32_t k, BasesGeo* g) {
  if (c < 4 || c > 20 || k < 1 || k > 8) return false;
  const uint32_t wm = (MAIN_BITS + c - 1) / c, q = MAIN_BITS / wm, nhi = MAIN_BITS - q * wm;
  g->c = c;
  if (k == 1) {
    g->Wc = wm + 1;
    g->S = 256;
    return true;
  }
  for (uint32_t w = 1; w <= wm; w++) {
    const uint32_t off = w * q + std::min(w, nhi);
    if (k * (off - 1) >= 256) {  // off(wm) = 254: always met for k >= 2
      g->Wc = w;
      g->S = off - 1;
      return true;
    }
  }
  return false;
}

// What levels = 0 and window_bits = 0 resolve to at creation.  Every row is a measurement of
// tools/bases_probe.py committed as profiles/bases_sweep.jsonl; a size that file does not hold
// gets levels = 1, and no row picks records past the 256 MiB Infinity Cache unless they won there.
struct BasesAutoRow {
  size_t n_lo, n_hi;  // sizes [n_lo, n_hi) the row was measured for
  uint32_t levels, window_bits;
};
constexpr BasesAutoRow BASES_AUTO[] = {
    // profiles/bases_sweep.jsonl, n = 2^16: levels 2 at c = 15 does not beat levels 1 pipelined (0.125
    // against 0.123 ms per MSM at c = 14); levels 4 loses
    {1u << 16, (1u << 16) + 1, 1, 0},
    // profiles/bases_sweep.jsonl, n = 2^18: levels 2 at c = 15 wins pipelined (0.272 against 0.292 ms per
    // MSM at levels 1, c = 15) and awaited (0.438 against 0.479 ms at levels 1, c = 16); 64 MiB of records
    {1u << 18, (1u << 18) + 1, 2, 15},
    // profiles/bases_sweep.jsonl, n = 2^20: levels 2 loses (1.121 against 0.921 ms per MSM), levels 4 more
    {1u << 20, (1u << 20) + 1, 1, 0},
};
uint32_t bases_auto_levels(size_t n) {
  for (const BasesAutoRow& r : BASES_AUTO)
    if (n >= r.n_lo && n < r.n_hi) return r.levels;
  return 1;
}
// The width of a folded handle created with window_bits = 0: the table's where the size was
// measured, else the pipelined width of the folded problem's k n points, at most 16 (wider windows
// take the 32-bit digit codes).
uint32_t bases_auto_window(size_t n, uint32_t levels) {
  for (const BasesAutoRow& r : BASES_AUTO)
    if (n >= r.n_lo && n < r.n_hi && r.levels == levels && r.window_bits) return r.window_bits;
  return std::min(16u, pipelined_window(n * levels));
}

// The argument rules of a subset that need no device: the range inside the handle's n bases, no
// `first` beside an index list, and levels * m inside the creation limit.
int subset_check(size_t n_handle, uint32_t levels, uint64_t first, uint64_t m, bool indexed) {
  if (indexed ? first != 0 || (m && !n_handle) : first > n_handle || m > n_handle - first) return MSM_ERR_INVALID_ARG;
  if (m >= (1ull << 30) || (uint64_t)levels * m >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  return MSM_OK;
}
// The range [0, m) of an unfolded handle is the plain launch on its first m records (the existing
// kernels with n := m); every other subset is a subset launch (MsmDims::sub).
uint32_t subset_kind(uint32_t levels, uint64_t first, bool indexed) {
  return indexed ? MSM_SUB_INDEXED : (first == 0 && levels == 1) ? MSM_SUB_NONE : MSM_SUB_RANGE;
}
