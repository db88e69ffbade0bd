// Pippenger MSM kernels for MI355X (gfx950).  Replaces the reference's GPU intra-bucket
// reduction (src/submission/gpu.ts:36-285 + wgsl/entry_padd_idx.wgsl:23-46) and its Rust
// split / inter-bucket reduce (src/submission/msm-wasm/src/lib.rs:46-133) with one on-device
// pipeline:
//
//   k_prepare_points   wire points (BE x|y|t|z, 128 B) -> halved precomputed affine records
//                      ((y-x)/2, (y+x)/2, d t) in 29-bit Montgomery limbs, 128 B (one cache line)
//   k_recode_hist      signed c-bit digits per scalar (window-carry recoding, |d| <= 2^(c-1)),
//                      written window-major (= first sort level: one contiguous array per window),
//                      with the coarse-bin totals (LDS histogram, flushed with global atomics);
//                      k_recode_fixed is the same with the common geometries at compile time.  Three
//                      more recode over the windows of the scalars' own bits, each a load of its own
//                      around one shared bias-add and window loop (bias_add, recode_windows):
//                      k_recode_narrow for scalars of 1..8 words (MSM_FLAG_SCALAR_BITS), k_recode_native
//                      for the caller's own integer arrays (bit / 8 / 16 / 32 / 64-bit elements, signed
//                      ones included: MSM_FLAG_SCALAR_TYPE), k_recode_wide for little-endian 128- /
//                      256-bit integers and Montgomery-form Fr (MSM_FLAG_SCALAR_FIELD; k_recode_hist_le,
//                      k_recode_hist's body on little-endian words, where a 256-bit integer takes the
//                      full-width geometry)
//   k_part_scatter     digits -> coarse bins (each chunk reserves and writes one contiguous slice
//                      per bin); its range / indexed variants map a subset launch's positions to
//                      a handle's records (k_stage_indices checks a device caller's indices first)
//   k_fine_sort        per coarse bin: LDS counting sort by bucket -> (entry, bucket key) lists
//   k_accumulate       fixed-length runs per lane over the sorted list (mixed adds), whole buckets
//                      written directly, buckets cut by run boundaries joined through LDS
//                      (segmented scan for long chains)
//   k_lead_scan        chains bucket continuations that run through whole workgroups (skew only)
//   k_bucket_reduce_1  per (window, chunk of L buckets): running sums -> U_c = sum (i+1) B, T_c = sum B
//   k_red2_groups      per (window, group of 128 chunks): V_g = sum U_c, S_g = sum T_c and the
//                      group's low bit terms R_{g,k}, in LDS (quad-cooperative adds)
//   k_red2_terms       per (window, term): R_{w,V} = sum V_g, R_{w,k} = sum_g R_{g,k} or
//                      sum_{g: bit k-7} S_g, in the host's Montgomery form for the host Horner
//   k_bucket_reduce_2  the same terms straight from every chunk's U_c / T_c (windows of more than
//                      64 groups, or MSM_RED2_TREE=0)
//
// Digit semantics differ from the reference's (unsigned, MSB-first, lib.rs:58-84 + msm-macro) on
// purpose: only the final affine (x, y) is the parity contract, and signed digits halve the
// bucket count.
#include "ec.cuh"
#include "msm_dev.h"
#include "fr.cuh"


namespace msm {

// Phase probe (tuning builds only, -DMSM_PHASE_PROBE=1): thread 0 of each workgroup of the sort
// kernels stamps the shader clock at its phase boundaries into g_probe[kernel][workgroup][slot]
// (slots 8 and 9: the 100 MHz real-time clock at slots 0 and 7); msm_test_probe_dump writes the
// last launch's stamps to a file (tools/phase_probe.py reads them).
#ifdef MSM_PHASE_PROBE
constexpr uint32_t PROBE_WG = 16384, PROBE_SLOTS = 10;
__device__ uint64_t g_probe[4][PROBE_WG][PROBE_SLOTS];
#define PROBE(k, wg, s)                                                                   \
  do {                                                                                   \
    if (threadIdx.x == 0 && (wg) < PROBE_WG) {                                           \
      g_probe[k][wg][s] = __builtin_readcyclecounter();                                  \
      if ((s) == 0 || (s) == 7) g_probe[k][wg][8 + ((s) == 7)] = __builtin_amdgcn_s_memrealtime(); \
    }                                                                                    \
  } while (0)
#define PROBE_WAIT_VM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define PROBE(k, wg, s) \
  do {                  \
  } while (0)
#define PROBE_WAIT_VM() \
  do {                  \
  } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// point preparation
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_be_words(const uint32_t* src, uint32_t le[8]) {
  uint4 a = reinterpret_cast<const uint4*>(src)[0];
  uint4 b = reinterpret_cast<const uint4*>(src)[1];
  // big-endian word order: src[0] is the most significant 32 bits (bytes.rs:11-20)
  le[7] = a.x; le[6] = a.y; le[5] = a.z; le[4] = a.w;
  le[3] = b.x; le[2] = b.y; le[1] = b.z; le[0] = b.w;
}

__device__ __forceinline__ void store_fe(uint32_t* dst, const fe& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) dst[i] = a.v[i];
}
__device__ __forceinline__ fe load_fe(const uint32_t* src) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = src[i];
  return r;
}

// One workgroup = PP_THREADS points.  Wire records and output records (128 B each) move between
// HBM and LDS with fully coalesced 16-B accesses (a wave covers 1 KiB contiguous per
// instruction); each lane then works on its own point out of LDS.  The 16-B slots of a record are
// XOR-swizzled by the record index so the per-lane 128-B-strided LDS reads and writes are free of
// bank conflicts.  With `nt` the records are written with nontemporal stores: the host sets it
// when a launch's records outgrow the 256 MiB Infinity Cache, where the regular write-back stores
// only evict lines that the gather in k_accumulate will not find there anyway (measured -11% on
// this kernel at 2 x 2^20 points; smaller launches keep their records cache-resident).
#ifndef MSM_PP_THREADS
#define MSM_PP_THREADS 256
#endif
constexpr uint32_t PP_THREADS = MSM_PP_THREADS;
static_assert(PP_THREADS * 8 <= (1u << 16), "k_prepare_points' multiply-high slot division");
typedef uint32_t pp_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t pp_slot(uint32_t rec, uint32_t q) { return rec * 8 + (q ^ (rec & 7)); }

// Input point formats (`fmt`): PT_FMT_WIRE the reference's 128-B x|y|t|z records; the compact
// forms of host uploads (run_host_split) leave t out -- PT_FMT_XYZ 96 B x|y|z, PT_FMT_XY 64 B x|y
// with z = 1 -- and the record's d t is derived from x and y (the oracle's own semantics: Aleo's
// msm reads affine (x, y)).
constexpr uint32_t PT_FMT_WIRE = 0, PT_FMT_XY = 1, PT_FMT_XYZ = 2;
__host__ __device__ constexpr uint32_t pt_fmt_slots(uint32_t fmt) {  // 16-B slots per input point
  return fmt == PT_FMT_XY ? 4u : fmt == PT_FMT_XYZ ? 6u : 8u;
}

// ---- the lane frame: what the per-lane point kernels (one lane = one point) share ---------------
// A workgroup of T lanes (PP_THREADS, or one wave of 64) owns a staging array of 8 T 16-byte slots,
// record i in slots pp_slot(i, 0 .. 7).  `np` is the number of the block's live records or points.
//
// The block's np prepared records (128 B each, `in` = the first one) into the staging array: coalesced
// 16-byte loads.  A barrier comes before lane_read_record.
template <uint32_t T>
__device__ __forceinline__ void lane_stage_records(uint4* st, const uint4* in, uint32_t np) {
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t g = j * T + threadIdx.x;  // 16-B slot within the block's records
    if (g < np * 8) st[pp_slot(g >> 3, g & 7)] = in[g];
  }
}
// Lane i's record out of its slots.  A lane past the block's last record works on zeros (x = y = 0:
// every doubling, addition and the inversion stay 0) and nothing of its is written back.
__device__ __forceinline__ void lane_read_record(const uint4* st, uint32_t i, bool live, uint32_t (&rec)[32]) {
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    const uint4 v = live ? st[pp_slot(i, q)] : make_uint4(0u, 0u, 0u, 0u);
    rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
  }
}
// Record `idx` of `recs` straight from HBM, a 128-byte gather per lane; zeros for a dead lane.
__device__ __forceinline__ void lane_gather_record(const uint32_t* __restrict__ recs, size_t idx, bool live,
                                                   uint32_t (&rec)[32]) {
  const uint4* in = reinterpret_cast<const uint4*>(recs) + idx * 8;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    const uint4 v = live ? in[q] : make_uint4(0u, 0u, 0u, 0u);
    rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
  }
}
// The extended point (X : Y : T : Z) = (x : y : x y : 1) of a halved record, every coordinate an
// fe_mul output as pt_dbl's and pt_add's bound proofs take them.  (y-x)/2 may reach 10p with a top
// limb above K8P's, so it goes through one multiply by R (value kept, < 2p) before it is subtracted.
__device__ __forceinline__ xyzt pt_from_record(const uint32_t (&rec)[32]) {
  fe ymx, ypx;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    ymx.v[k] = rec[k];
    ypx.v[k] = rec[PRE_HALF + k];
  }
  const fe one = fe_one();
  const fe a = fe_mul(ymx, one);   // (y-x)/2, N_MUL
  const fe xs = fe_sub(ypx, a);    // x + 8p: normalised, < 12p
  const fe ys = fe_add_n(ypx, a);  // y: normalised, < 6p
  xyzt p;
  p.X = fe_mul(xs, one);
  p.Y = fe_mul(ys, one);
  p.T = fe_mul(xs, ys);            // 72 p^2 < p R
  p.Z = one;
  return p;
}
// The halved record (ec.cuh pt_madd; layout: msm_dev.h PRE_WORDS) of the affine point whose x/2 and
// y/2 are `x` and `y`, Montgomery form, fe_mul outputs (N_MUL).  Limb forms written, which
// tests/test_limb_bounds.py test_madd_bounds proves for pt_madd's record operand: (y-x)/2 =
// fe_sub(N_MUL, N_MUL) (normalised, < 10p), (y+x)/2 = fe_norm(fe_add(N_MUL, N_MUL)) (normalised,
// < 4p) and d t = fe_mul_d of an fe_mul output (normalised, < 2p: N_MUL).
__device__ __forceinline__ void record_from_halved(const fe& x, const fe& y, uint32_t (&rec)[32]) {
  // d x y: (2 (x/2)) (2 (y/2)) = x y in Montgomery form (S x S operands), then d by limb scaling
  const fe kt = fe_mul_d(fe_mul(fe_add(x, x), fe_add(y, y)));
  const fe ymx = fe_sub(y, x);
  const fe ypx = fe_add_n(y, x);
#pragma unroll
  for (int k = 0; k < 32; k++) rec[k] = 0;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    rec[k] = ymx.v[k];
    rec[PRE_HALF + k] = ypx.v[k];
  }
#pragma unroll
  for (int k = 0; k < NL - 1; k++) rec[PRE_KT + k] = kt.v[k];
  // each half also carries d*t's top limb and the OTHER half's top limb: the half read first
  // supplies both, so the half read second needs only its eight low limbs (seven loads in all)
  rec[NL] = rec[PRE_HALF + NL] = kt.v[NL - 1];
  rec[NL + 1] = ypx.v[NL - 1];
  rec[PRE_HALF + NL + 1] = ymx.v[NL - 1];
}
// Lane i's record into its slots, and the block's np records out to `dst` (the first one's place) in
// coalesced 16-byte stores, nontemporal with `nt`.  A barrier goes between the two.
__device__ __forceinline__ void lane_put_record(uint4* st, uint32_t i, const uint32_t (&rec)[32]) {
#pragma unroll
  for (uint32_t q = 0; q < 8; q++)
    st[pp_slot(i, q)] = make_uint4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
}
template <uint32_t T>
__device__ __forceinline__ void lane_flush_records(const uint4* st, uint4* dst, uint32_t np, uint32_t nt) {
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t g = j * T + threadIdx.x;
    if (g < np * 8) {
      const uint4 v = st[pp_slot(g >> 3, g & 7)];
      if (nt) {
        const pp_v4 w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<pp_v4*>(dst + g));
      } else {
        dst[g] = v;
      }
    }
  }
}
// Lane i's point as the canonical big-endian record x | y | t | z = 1 in its slots: from little-endian
// words, or from the affine Montgomery (x, y) with t = x y.
__device__ __forceinline__ void lane_stage_words(uint4* st, uint32_t i, const uint32_t (&xw)[8],
                                                 const uint32_t (&yw)[8], const uint32_t (&tw)[8]) {
  // big-endian word order: word 0 is the most significant 32 bits
  st[pp_slot(i, 0)] = make_uint4(xw[7], xw[6], xw[5], xw[4]);
  st[pp_slot(i, 1)] = make_uint4(xw[3], xw[2], xw[1], xw[0]);
  st[pp_slot(i, 2)] = make_uint4(yw[7], yw[6], yw[5], yw[4]);
  st[pp_slot(i, 3)] = make_uint4(yw[3], yw[2], yw[1], yw[0]);
  st[pp_slot(i, 4)] = make_uint4(tw[7], tw[6], tw[5], tw[4]);
  st[pp_slot(i, 5)] = make_uint4(tw[3], tw[2], tw[1], tw[0]);
  st[pp_slot(i, 6)] = make_uint4(0u, 0u, 0u, 0u);
  st[pp_slot(i, 7)] = make_uint4(0u, 0u, 0u, 1u);
}
__device__ __forceinline__ void lane_stage_affine(uint4* st, uint32_t i, const fe& x, const fe& y) {
  uint32_t xw[8], yw[8], tw[8];
  fe_to_words_le(fe_to_std(x), xw);
  fe_to_words_le(fe_to_std(y), yw);
  fe_to_words_le(fe_to_std(fe_mul(x, y)), tw);
  lane_stage_words(st, i, xw, yw, tw);
}
// A staged block's first np points out to `out`, block at point p0: 128-byte wire records (wire = 1)
// or the 64-byte x | y that k_prepare_points(PT_FMT_XY) reads (wire = 0), coalesced 16-byte stores.
template <uint32_t T>
__device__ __forceinline__ void lane_flush_points(const uint4* st, uint32_t* __restrict__ out, size_t p0, uint32_t np,
                                                  uint32_t wire) {
  const uint32_t sh = wire ? 3u : 2u;  // 16-byte slots per output point: 8 or 4
  uint4* dst = reinterpret_cast<uint4*>(out) + (p0 << sh);
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t g = j * T + threadIdx.x;
    if (g < (np << sh)) dst[g] = st[pp_slot(g >> sh, g & ((1u << sh) - 1u))];
  }
}
// `total` scalar words of the vector `scalars`, from word `w0` on (a multiple of 64 words), into LDS:
// 16-byte loads where the vector is 16-byte aligned, word by word where it is not.
template <uint32_t T>
__device__ __forceinline__ void lane_stage_scalars(uint4* ssc4, const uint32_t* __restrict__ scalars, size_t w0,
                                                   uint32_t total) {
  uint32_t* ssc = reinterpret_cast<uint32_t*>(ssc4);
  const uint32_t* sp = scalars + w0;
  const uint32_t nv = (reinterpret_cast<uintptr_t>(scalars) & 15u) ? 0u : total >> 2;
  for (uint32_t g = threadIdx.x; g < nv; g += T) ssc4[g] = reinterpret_cast<const uint4*>(sp)[g];
  for (uint32_t g = (nv << 2) + threadIdx.x; g < total; g += T) ssc[g] = sp[g];
}

// blockIdx.y = MSM of the batch: its wire points come from wires.p[y], its records go to
// pts[y n ..).
extern "C" __global__ void __launch_bounds__(PP_THREADS) k_prepare_points(BatchPtrs wires,
                                                                          uint32_t* __restrict__ pts, uint32_t n,
                                                                          uint32_t* __restrict__ err, uint32_t nt,
                                                                          uint32_t fmt) {
  __shared__ uint4 st[PP_THREADS * 8];
  const uint32_t S = pt_fmt_slots(fmt);
  // g / S for the wave-uniform S in {4, 6, 8} as one multiply-high (exact for g < 2^16; the
  // generic unsigned division it replaces cost ~12 VALU per slot)
  const uint32_t s_inv = S == 8 ? (1u << 29) : S == 4 ? (1u << 30) : 0x2AAAAAABu;
  const uint32_t p0 = blockIdx.x * PP_THREADS;
  const uint32_t np = min(PP_THREADS, n - p0);
  const uint4* src = reinterpret_cast<const uint4*>(wires.p[blockIdx.y]) + (size_t)p0 * S;
  pts += (size_t)blockIdx.y * n * PRE_WORDS;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t g = j * PP_THREADS + threadIdx.x;  // 16-B slot within the block's records
    const uint32_t rec = __umulhi(g, s_inv);
    if (g < np * S) st[pp_slot(rec, g - rec * S)] = src[g];
  }
  __syncthreads();
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  const bool has_t = fmt == PT_FMT_WIRE, has_z = fmt != PT_FMT_XY;  // t: range check only
  uint32_t xw[8], yw[8], tw[8], zw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) xw[k] = yw[k] = tw[k] = zw[k] = 0;
  zw[0] = 1;
  if (live) {
    uint4 v[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) v[q] = q < S ? st[pp_slot(i, q)] : make_uint4(0u, 0u, 0u, 0u);
    // big-endian word order: word 0 is the most significant 32 bits (bytes.rs:11-20); the
    // compact forms hold x, y (and z) in that order
    uint32_t* dsts[4] = {xw, yw, has_t ? tw : zw, zw};
#pragma unroll
    for (int f = 0; f < 4; f++) {
      if (f == 3 && !has_t) break;   // x|y|z: z was the third field
      if (f == 2 && !has_z) break;   // x|y
      const uint4 a = v[2 * f], b = v[2 * f + 1];
      uint32_t* le = dsts[f];
      le[7] = a.x; le[6] = a.y; le[5] = a.z; le[4] = a.w;
      le[3] = b.x; le[2] = b.y; le[1] = b.z; le[0] = b.w;
    }
  }
  __syncthreads();
  bool ok = words_lt_p(xw) && words_lt_p(yw) && words_lt_p(tw) && words_lt_p(zw);
  if (live && !ok) atomicOr(err, MSM_DEV_ERR_COORD_RANGE);
  bool z_one = zw[0] == 1u;
  bool z_zero = zw[0] == 0u;
#pragma unroll
  for (int k = 1; k < 8; k++) {
    z_one = z_one && zw[k] == 0u;
    z_zero = z_zero && zw[k] == 0u;
  }
  if (live && z_zero) atomicOr(err, MSM_DEV_ERR_BAD_POINT);
  // the halved record (ec.cuh pt_madd): x/2, y/2 and d*t in Montgomery form
  // d t is derived from the affine x and y in every format: the input t is range-checked above
  // but not used, so a record's result depends on (x, y, z) alone, as the oracle's does (Aleo's
  // msm reads affine points), whichever entry and upload form carried it
  fe x, y;
  if (z_one) {
    x = fe_mul(fe_from_words_le(xw), fe_const(R2H_29));
    y = fe_mul(fe_from_words_le(yw), fe_const(R2H_29));
  } else {
    // Projective input (z != 1, README.md:92 allows it): normalise to affine with one inversion.
    fe zi = fe_inv(fe_to_mont(fe_from_words_le(zw)));
    fe zh = fe_mul(zi, fe_const(HALF29));
    x = fe_mul(fe_to_mont(fe_from_words_le(xw)), zh);
    y = fe_mul(fe_to_mont(fe_from_words_le(yw)), zh);
  }
  uint32_t rec[32];
  record_from_halved(x, y, rec);
  // lane_put_record and lane_flush_records, written out: through the helpers this kernel, which every
  // MSM runs, compiles to a dozen instructions more (the input stage above is its own as well)
#pragma unroll
  for (uint32_t q = 0; q < 8; q++)
    st[pp_slot(i, q)] = make_uint4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(pts) + (size_t)p0 * 8;
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) {
    const uint32_t g = j * PP_THREADS + threadIdx.x;
    if (g < np * 8) {
      const uint4 v = st[pp_slot(g >> 3, g & 7)];
      if (nt) {
        const pp_v4 w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<pp_v4*>(dst + g));
      } else {
        dst[g] = v;
      }
    }
  }
}

// Pads a short host-input slice on the device (run_host_split with n not a multiple of its slice
// count): `count` points set to the identity (x, y, t, z) = (0, 1, 0, 1) -- in the input format
// `fmt` of the slice's point buffer (wire records, or the compact x|y|z of a compact upload) --
// and `count` scalars set to 0, so the padding contributes no bucket entry.  16-B stores, one
// per thread.
extern "C" __global__ void __launch_bounds__(256) k_pad_identity(uint32_t* __restrict__ wire_pts,
                                                                   uint32_t* __restrict__ wire_sc, uint32_t count,
                                                                   uint32_t fmt) {
  const uint32_t S = pt_fmt_slots(fmt);
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;  // 16-B slot: S per point, then 2 per scalar
  if (g < count * S) {
    // BE words: the least significant word of y (slot 3), and of z (the point's last slot) unless
    // the format has no z
    const uint32_t q = g % S;
    const bool one = q == 3 || (fmt != PT_FMT_XY && q == S - 1);
    reinterpret_cast<uint4*>(wire_pts)[g] = make_uint4(0u, 0u, 0u, one ? 1u : 0u);
  } else if (g < count * (S + 2)) {
    reinterpret_cast<uint4*>(wire_sc)[g - count * S] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// ---------------------------------------------------------------------------------------------
// resident prepared bases (msm_bases_*): shifted levels and the scalar cut
// ---------------------------------------------------------------------------------------------
// Level j + 1 of a handle's records from level j: record i of `src` (the halved affine form of
// Q_i = 2^(jS) P_i) -> record i of `dst` for 2^S Q_i.  One workgroup = PP_THREADS records, in and
// out through the lane frame (lane_stage_records .. lane_flush_records); each lane rebuilds its
// extended point (pt_from_record), doubles it S times (pt_dbl, complete: the identity, the order-2
// point (0, -1) and the order-4 points with y = 0 need no branch), and normalises with one fe_inv
// (~260 of the lane's 8 S + ~270 multiplies) into record_from_halved's operands.
// Results are specified for on-curve points (Z of a multiple is then never 0).
extern "C" __global__ void __launch_bounds__(PP_THREADS) k_shift_bases(const uint32_t* __restrict__ src,
                                                                       uint32_t* __restrict__ dst, uint32_t n,
                                                                       uint32_t S, uint32_t nt) {
  __shared__ uint4 st[PP_THREADS * 8];
  const uint32_t p0 = blockIdx.x * PP_THREADS;
  const uint32_t np = min(PP_THREADS, n - p0);
  lane_stage_records<PP_THREADS>(st, reinterpret_cast<const uint4*>(src) + (size_t)p0 * 8, np);
  __syncthreads();
  const uint32_t i = threadIdx.x;
  uint32_t rec[32];
  lane_read_record(st, i, i < np, rec);
  __syncthreads();
  xyzt p = pt_from_record(rec);
#pragma unroll 1
  for (uint32_t s = 0; s < S; s++) p = pt_dbl(p);
  // x/2 and y/2, as k_prepare_points' projective branch makes them
  const fe zh = fe_mul(fe_inv(p.Z), fe_const(HALF29));
  record_from_halved(fe_mul(p.X, zh), fe_mul(p.Y, zh), rec);
  lane_put_record(st, i, rec);
  __syncthreads();
  lane_flush_records<PP_THREADS>(st, reinterpret_cast<uint4*>(dst) + (size_t)p0 * 8, np, nt);
}

// ---------------------------------------------------------------------------------------------
// compressed points (msm_decompress_points*, msm_bases_create_compressed*): y from x
// ---------------------------------------------------------------------------------------------
// p - 1 = 2^47 q with q odd, so a square root is Tonelli-Shanks over the 2^47-part of the
// multiplicative group.  The constants below are functions, so that the host's test hook
// (msm_test_decompress_constants) reads the very values the kernel uses; tests/test_sqrt_model.py
// recomputes each of them from p.
constexpr uint32_t DX_TWO_ADICITY = 47;
constexpr uint32_t DX_EXP_WORDS = 7;  // (q - 1) / 2 has 205 bits
// (q - 1) / 2, little-endian words.
__host__ __device__ constexpr uint32_t dx_exp_word(uint32_t i) {
  constexpr uint32_t E[8] = {0x00010a11u, 0x76fed000u, 0xb00159aau, 0x4d1e5c37u,
                             0xa55660b4u, 0x655e9a2cu, 0x000012abu, 0u};
  return E[i];
}
// The order r of the prime-order subgroup (251 bits), little-endian words.
constexpr uint32_t DX_ORDER_BITS = 251;
__host__ __device__ constexpr uint32_t dx_order_word(uint32_t i) {
  constexpr uint32_t E[8] = {0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu,
                             0x970dec00u, 0x982d1347u, 0xa68b2955u, 0x04aad957u};
  return E[i];
}
// omega = 11^q, a generator of the 2^47-th roots of unity (11 is the least non-residue), as
// Montgomery limbs.
__host__ __device__ constexpr uint32_t dx_omega_limb(uint32_t i) {
  constexpr uint32_t W[NL] = {117700138u, 288663353u, 196695082u, 116731750u, 508254431u,
                              393715903u, 414881643u, 49231371u, 571788u};
  return W[i];
}

__device__ __forceinline__ bool fe_eq_limbs(const fe& a, const fe& b) {
  bool eq = true;
#pragma unroll
  for (int i = 0; i < NL; i++) eq = eq && a.v[i] == b.v[i];
  return eq;
}
// Whether an fe_mul output is 1.  Its value is below 2p and its limbs are normalised, so it is one of
// two integers, R mod p and R mod p + p, each with one limb pattern: the comparison is exact without
// a reduction (unlike one between two lazy values, which goes through fe_to_std).
__device__ __forceinline__ bool fe_mul_out_is_one(const fe& t, const fe& one, const fe& one_p) {
  return fe_eq_limbs(t, one) || fe_eq_limbs(t, one_p);
}
// p - a for a canonical standard-form a in (0, p); 0 stays 0.
__device__ __forceinline__ fe fe_std_neg(const fe& a) {
  fe r;
  int32_t borrow = 0;
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int32_t t = (int32_t)P29[i] - (int32_t)a.v[i] + borrow;
    borrow = t < 0 ? -1 : 0;
    r.v[i] = (uint32_t)t & LMASK;
    any |= a.v[i];
  }
  return any ? r : a;
}

// A square root of u (Montgomery form, an fe_mul output) by Tonelli-Shanks, or some value whose
// square is not u when u is a non-residue: the caller compares r^2 with u (which also accepts
// u = 0, r = 0).  w = u^((q-1)/2), r = u w, t = u^q; while t != 1, with 2^i the order of t,
// b = c^(2^(m-i-1)) moves r by b and t by b^2.  The loops' trip counts differ per lane (a wave
// pays its deepest lane); none is unrolled.
__device__ inline fe fe_sqrt_ts(const fe& u) {
  const fe one = fe_one();
  const fe one_p = fe_add_n(one, fe_const(P29));
  fe w = one;
#pragma unroll 1
  for (int wi = DX_EXP_WORDS - 1; wi >= 0; wi--) {
    const uint32_t e = dx_exp_word(wi);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      w = fe_sqr(w);
      if ((e >> b) & 1u) w = fe_mul(w, u);
    }
  }
  fe r = fe_mul(u, w);
  fe t = fe_mul(r, w);
  fe c;
#pragma unroll
  for (int i = 0; i < NL; i++) c.v[i] = dx_omega_limb(i);
  uint32_t m = DX_TWO_ADICITY;
#pragma unroll 1
  while (!fe_mul_out_is_one(t, one, one_p)) {
    uint32_t i = 0;
    fe t2 = t;
#pragma unroll 1
    do {
      t2 = fe_sqr(t2);
      i++;
    } while (i < m && !fe_mul_out_is_one(t2, one, one_p));
    if (i >= m) break;  // t's order is not below 2^m: u is 0 or a non-residue
    fe b = c;
#pragma unroll 1
    for (uint32_t j = i + 1; j < m; j++) b = fe_sqr(b);
    c = fe_sqr(b);
    t = fe_mul(t, c);
    r = fe_mul(r, b);
    m = i;
  }
  return r;
}

// [r] P for the subgroup order r: double-and-add over the constant's bits, so every lane takes the
// same path.  P's coordinates are fe_mul outputs (Z = 1), as pt_dbl's and pt_add's bound proofs
// take them.
__device__ inline xyzt pt_mul_order(const xyzt& p) {
  xyzt acc = pt_identity();
#pragma unroll 1
  for (int k = DX_ORDER_BITS - 1; k >= 0; k--) {
    acc = pt_dbl(acc);
    if ((dx_order_word((uint32_t)k >> 5) >> (k & 31)) & 1u) acc = pt_add(acc, p);
  }
  return acc;
}

// Compressed points -> affine points: x (8 big-endian words, msm.h MSM_POINTS_X_*) to the 64-byte
// x|y that k_prepare_points(PT_FMT_XY) reads, or with `wire` to a whole 128-byte record
// (t = x y, z = 1).  One lane per point; a wave's 2 KiB of input arrives with two 16-byte loads per
// lane, and the output leaves through the lane frame (lane_stage_words, lane_flush_points).
//   y^2 = (a x^2 - 1) / (d x^2 - 1) = (x^2 + 1) / (1 - d x^2)       (a = -1)
// The denominator is never 0: d = 3021 is a non-residue, so d x^2 = 1 has no solution.
// form 1 (subgroup): y is the root with [r](x, y) = O.  (x, -y) = -(x, y) + (0, -1) and r is odd, so
// [r](x, -y) = O exactly when [r](x, y) = (0, -1): one ladder decides both roots.
// form 2 (ysign): bit 255 says whether y > p - y; bits 253 and 254 must be zero.
// A bad lane (MSM_DEV_ERR_COORD_RANGE, MSM_DEV_ERR_BAD_POINT into err[0]) writes the identity, so
// whatever runs next reads a valid point.
// One wave per workgroup: a lane's work differs with its input's depth, and small workgroups spread a
// vector over more compute units; two waves per SIMD (256 VGPRs) keep the multiplies' latency covered.
constexpr uint32_t DX_THREADS = 64;
constexpr uint32_t DX_FORM_SUBGROUP = 1, DX_FORM_YSIGN = 2;
extern "C" __global__ void __launch_bounds__(DX_THREADS, 2) k_decompress_x(const uint32_t* __restrict__ xs,
                                                                        uint32_t* __restrict__ out, uint32_t n,
                                                                        uint32_t form, uint32_t wire,
                                                                        uint32_t* __restrict__ err) {
  __shared__ uint4 st[DX_THREADS * 8];
  const uint32_t p0 = blockIdx.x * DX_THREADS;
  const uint32_t np = min(DX_THREADS, n - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  uint32_t xw[8];
#pragma unroll
  for (int k = 0; k < 8; k++) xw[k] = 0;
  if (live) load_be_words(xs + (size_t)(p0 + i) * 8, xw);
  bool flag = false, in_range = true;
  if (form == DX_FORM_YSIGN) {
    flag = (xw[7] >> 31) != 0;
    in_range = (xw[7] & 0x60000000u) == 0;
    xw[7] &= 0x1FFFFFFFu;
  }
  in_range = in_range && words_lt_p(xw);
  if (!in_range) {  // (a lane past the block's last point holds x = 0)
    atomicOr(err, MSM_DEV_ERR_COORD_RANGE);
#pragma unroll
    for (int k = 0; k < 8; k++) xw[k] = 0;  // goes on as the identity
    flag = false;
  }
  const fe one = fe_one();
  const fe xm = fe_to_mont(fe_from_words_le(xw));
  const fe x2 = fe_sqr(xm);
  const fe num = fe_add_n(x2, one);
  const fe den = fe_sub(one, fe_mul_d(x2));
  const fe u = fe_mul(num, fe_inv(den));
  const fe r = fe_sqrt_ts(u);
  // the non-residue test, on canonical values (the limbs of two lazy values do not compare)
  bool bad = !fe_eq_limbs(fe_to_std(fe_sqr(r)), fe_to_std(u));
  fe ys = fe_to_std(r);
  bool neg;
  if (form == DX_FORM_SUBGROUP) {
    xyzt p;
    p.X = xm;
    p.Y = r;
    p.T = fe_mul(xm, r);
    p.Z = one;
    const xyzt q = pt_mul_order(p);
    const fe qx = fe_to_std(q.X), qy = fe_to_std(q.Y), qz = fe_to_std(q.Z);
    const bool x0 = fe_eq_limbs(qx, fe_zero());
    const bool is_o = x0 && fe_eq_limbs(qy, qz);                          // (0 : z : z)
    const bool is_t2 = x0 && fe_eq_limbs(fe_add_n(qy, qz), fe_const(P29));  // (0 : -z : z)
    bad = bad || !(is_o || is_t2);
    neg = is_t2;
  } else {
    // y > p - y on canonical integers: 2 y > p (2 y < 2^254 is even, p odd: never equal)
    uint32_t yw[8], y2[8];
    fe_to_words_le(ys, yw);
#pragma unroll
    for (int k = 7; k >= 0; k--) y2[k] = (yw[k] << 1) | (k ? yw[k - 1] >> 31 : 0u);
    const bool big = !words_lt_p(y2);
    const bool zero = fe_eq_limbs(ys, fe_zero());
    bad = bad || (zero && flag);  // y = 0 has no sign: the flag must be clear
    neg = big != flag;
  }
  fe ts = fe_to_std(fe_mul(xm, r));
  if (neg) {
    ys = fe_std_neg(ys);
    ts = fe_std_neg(ts);
  }
  if (bad) {
    if (live) atomicOr(err, MSM_DEV_ERR_BAD_POINT);
#pragma unroll
    for (int k = 0; k < 8; k++) xw[k] = 0;
    ys = fe_zero();
    ys.v[0] = 1;
    ts = fe_zero();
  }
  uint32_t yw[8], tw[8];
  fe_to_words_le(ys, yw);
  fe_to_words_le(ts, tw);
  lane_stage_words(st, i, xw, yw, tw);
  __syncthreads();
  lane_flush_points<DX_THREADS>(st, out, p0, np, wire);
}

// ---------------------------------------------------------------------------------------------
// per-point scalar multiples of a handle's bases (msm_bases_scale*): Q_i = s_i P_i
// ---------------------------------------------------------------------------------------------
// The ladder reads the scalar in fixed windows of SC_W bits, most significant first.  SC_W divides 32,
// so no window straddles a word.  Both functions run on the host too (msm_test_scale_digits), so the
// test of the window index -> digit mapping exercises the very code the kernel runs.
constexpr uint32_t SC_W = 2;
static_assert(SC_W == 2, "k_scale_points' table holds P, 2P, 3P");
// The ladder's trip count for b-bit scalars: wave-uniform, from the kernel argument alone.
__host__ __device__ constexpr uint32_t scale_windows(uint32_t b) { return (b + SC_W - 1) / SC_W; }
// Window j (j < scale_windows(b)) of a b-bit scalar held as sw = ceil(b / 32) big-endian words: bits
// [SC_W j, SC_W j + SC_W) of the integer.  The top window keeps only the bits below b, so a stray bit
// at or above b (flagged by the kernel) never reaches the ladder.
__host__ __device__ inline uint32_t scale_digit(const uint32_t* s_be, uint32_t sw, uint32_t b, uint32_t j) {
  const uint32_t bit = j * SC_W;
  const uint32_t d = (s_be[sw - 1 - (bit >> 5)] >> (bit & 31u)) & ((1u << SC_W) - 1u);
  return b - bit < SC_W ? d & ((1u << (b - bit)) - 1u) : d;
}

// Q_i = s_i P_(first + i) (indices == nullptr) or s_i P_(indices[i]) for i < m, over the n prepared
// records `recs` of a handle's level 0.  One lane per output point, one wave per workgroup, two waves
// per SIMD as k_decompress_x (225 VGPRs, no scratch: the table and the accumulator are 144 of them).
// The plain double-and-add with a selected add was measured beside this ladder and lost by a quarter
// (DESIGN.md §9).
//   records  range form: the workgroup's 8 KiB arrive through the lane frame (lane_stage_records,
//            lane_read_record); indexed form: lane_gather_record.  An index >= n is replaced by 0 and
//            raises MSM_DEV_ERR_BAD_INDEX.  pt_from_record rebuilds the extended point.
//   scalars  sw big-endian words each (the full integer: nothing is reduced mod r), the workgroup's
//            64 sw words staged in LDS (lane_stage_scalars).  A bit at or above b is masked
//            (scale_digit) and raises MSM_DEV_ERR_SCALAR_RANGE.
//   ladder   scale_windows(b) rounds of SC_W doublings and one addition of {O, P, 2P, 3P}[digit],
//            chosen with pt_sel: no lane takes a branch of its own, and the unified addition is
//            complete, so the identity, the torsion points and P + P need none either.
//   output   one fe_inv per lane, then lane_stage_affine and lane_flush_points: wire records
//            (wire = 1) or x | y (wire = 0).  The identity comes out as (0 : Z : 0 : Z) and is written
//            (0, 1, 0, 1).  Results are specified for on-curve bases (Z is then never 0).
constexpr uint32_t SC_THREADS = 64;
extern "C" __global__ void __launch_bounds__(SC_THREADS, 2) k_scale_points(
    const uint32_t* __restrict__ recs, uint32_t n, uint32_t first, const uint32_t* __restrict__ indices,
    const uint32_t* __restrict__ scalars, uint32_t sw, uint32_t b, uint32_t* __restrict__ out, uint32_t m,
    uint32_t wire, uint32_t* __restrict__ err) {
  __shared__ uint4 st[SC_THREADS * 8];
  __shared__ uint4 ssc4[SC_THREADS * 2];
  uint32_t* ssc = reinterpret_cast<uint32_t*>(ssc4);
  const uint32_t p0 = blockIdx.x * SC_THREADS;
  const uint32_t np = min(SC_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  // the workgroup's np * sw scalar words; p0 * sw * 4 is a multiple of 256 bytes
  lane_stage_scalars<SC_THREADS>(ssc4, scalars, (size_t)p0 * sw, np * sw);
  uint32_t rec[32];
  if (indices) {
    uint32_t idx = live ? indices[p0 + i] : 0u;
    if (idx >= n) {
      idx = 0;
      atomicOr(err, MSM_DEV_ERR_BAD_INDEX);
    }
    lane_gather_record(recs, idx, live, rec);
    __syncthreads();
  } else {
    lane_stage_records<SC_THREADS>(st, reinterpret_cast<const uint4*>(recs) + ((size_t)first + p0) * 8, np);
    __syncthreads();
    lane_read_record(st, i, live, rec);
  }
  const uint32_t* my = ssc + i * sw;
  const uint32_t top_mask = (b & 31u) ? (1u << (b & 31u)) - 1u : 0xffffffffu;
  if (live && (my[0] & ~top_mask)) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
  const xyzt p1 = pt_from_record(rec);
  xyzt acc = pt_identity();
  const xyzt p2 = pt_dbl(p1);
  const xyzt p3 = pt_add(p2, p1);
  const xyzt p0i = pt_identity();
#pragma unroll 1
  for (uint32_t j = scale_windows(b); j-- > 0;) {
    acc = pt_dbl(pt_dbl(acc));
    const uint32_t d = live ? scale_digit(my, sw, b, j) : 0u;
    const bool hi = (d & 2u) != 0;
    acc = pt_add(acc, pt_sel((d & 1u) != 0, pt_sel(hi, p0i, p2), pt_sel(hi, p1, p3)));
  }
  const fe zi = fe_inv(acc.Z);
  const fe x = fe_mul(acc.X, zi);
  const fe y = fe_mul(acc.Y, zi);
  __syncthreads();
  lane_stage_affine(st, i, x, y);
  __syncthreads();
  lane_flush_points<SC_THREADS>(st, out, p0, np, wire);
}

// The virtual scalars of a folded launch (levels = k > 1): out[m][j n + i] = bits [j S, (j+1) S)
// of scalar i of MSM m, wire layout (32 B, big-endian words, upper bits zero).  blockIdx.y = level
// j, blockIdx.z = MSM of the batch (its wire scalars from scalar_sets.p[z], its k n virtual
// scalars at out + z k n 8 words).  Two 16-B loads and two 16-B stores per lane; the shift
// amounts are wave-uniform, so the scalar moves down by whole words in a uniform loop and by the
// rest with v_alignbit (no dynamically indexed register array).
extern "C" __global__ void __launch_bounds__(256) k_split_scalars(BatchPtrs scalar_sets, uint32_t* __restrict__ out,
                                                                    uint32_t n, uint32_t k, uint32_t S) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = blockIdx.y;
  uint32_t s[8];
  load_be_words(scalar_sets.p[blockIdx.z] + (size_t)i * 8, s);
  const uint32_t lo = j * S;  // may pass 256 (k = 8 at wide windows): such a level's chunks are zero
  for (uint32_t w = 0; w < (lo >> 5); w++) {
#pragma unroll
    for (int q = 0; q < 7; q++) s[q] = s[q + 1];
    s[7] = 0;
  }
  const uint32_t sh = lo & 31u;  // v_alignbit by 0 returns the low word
#pragma unroll
  for (int q = 0; q < 7; q++) s[q] = __builtin_amdgcn_alignbit(s[q + 1], s[q], sh);
  s[7] >>= sh;
  const uint32_t sw = S >> 5, sb = S & 31u;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) s[q] = q < sw ? s[q] : q == sw ? s[q] & ((1u << sb) - 1u) : 0u;
  uint4* dst = reinterpret_cast<uint4*>(out + ((size_t)blockIdx.z * k * n + (size_t)j * n + i) * 8);
  dst[0] = make_uint4(s[7], s[6], s[5], s[4]);
  dst[1] = make_uint4(s[3], s[2], s[1], s[0]);
}

// Gathers the record of sorted entry `ent` (point index << 1 | sign) as the point it adds:
// a negated point's (y-x)/2 and (y+x)/2 swap by reading the record's halves in the other order
// (msm_dev.h PRE_WORDS), and its d*t is negated (kt_neg_if).
__device__ __forceinline__ pre load_pre_signed(const uint32_t* __restrict__ pts, uint32_t ent) {
  const uint32_t sgn = ent & 1u;
  const bool neg = sgn != 0;
  // byte offsets: record (ent >> 1) * 128 = (ent & ~1) * 64; halves at 48 sgn and 48 (1 - sgn)
  const char* rec = reinterpret_cast<const char*>(pts) + ((size_t)(ent & ~1u) << 6);
  const uint32_t o0 = sgn * (PRE_HALF * 4);
  const uint32_t* h0 = reinterpret_cast<const uint32_t*>(rec + o0);
  const uint32_t* h1 = reinterpret_cast<const uint32_t*>(rec + (o0 ^ (PRE_HALF * 4)));
  const uint4 a0 = reinterpret_cast<const uint4*>(h0)[0], a1 = reinterpret_cast<const uint4*>(h0)[1];
  const uint4 a2 = reinterpret_cast<const uint4*>(h0)[2];  // top limb, d*t's top limb, the other half's top limb
  const uint4 b0 = reinterpret_cast<const uint4*>(h1)[0], b1 = reinterpret_cast<const uint4*>(h1)[1];
  const uint32_t b2 = a2.z;
  const uint4 c0 = reinterpret_cast<const uint4*>(rec + PRE_KT * 4)[0];
  const uint4 c1 = reinterpret_cast<const uint4*>(rec + PRE_KT * 4)[1];
  const uint32_t av[NL] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x};
  const uint32_t bv[NL] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2};
  const uint32_t kv[NL] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, a2.y};
  pre q;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    q.ymx.v[k] = av[k];
    q.ypx.v[k] = bv[k];
    q.kt.v[k] = kv[k];
  }
  q.kt = kt_neg_if(q.kt, neg);
  return q;
}

// ---------------------------------------------------------------------------------------------
// fixed-base tables (msm_fixed_*): Q_i = sum_j s_ij B_j from windowed tables, no doubling
// ---------------------------------------------------------------------------------------------
// A table of k bases for windows of w bits and scalars below 2^b holds, for every base j and every
// window win < Wn = fixed_windows(b, w), the 2^(w-1) multiples d 2^(w win) B_j, d = 1 .. 2^(w-1), as
// ordinary prepared records: entry (j, win, d) is record (j Wn + win) 2^(w-1) + d - 1.  A scalar is
// read as Wn signed digits, so an output is one mixed addition per window and base.
// Both digit functions run on the host too (msm_test_fixed_digits), as scale_digit does.
__host__ __device__ constexpr uint32_t fixed_windows(uint32_t b, uint32_t w) { return (b + w) / w; }  // ceil((b + 1) / w)
// Bits [w win, w win + w) of a b-bit scalar held as sw = ceil(b / 32) big-endian words (w <= 16: at
// most two words).  Bits at or above b read as zero, so a stray bit there (flagged by the kernel)
// never reaches a digit, and windows past the scalar's words are zero.
__host__ __device__ inline uint32_t fixed_window_bits(const uint32_t* s_be, uint32_t sw, uint32_t b, uint32_t w,
                                                      uint32_t win) {
  const uint32_t bit = win * w;
  if (bit >= b) return 0u;
  const uint32_t wi = bit >> 5, sh = bit & 31u;
  uint32_t v = s_be[sw - 1 - wi] >> sh;
  if (sh + w > 32u && wi + 1 < sw) v |= s_be[sw - 2 - wi] << (32u - sh);
  const uint32_t keep = b - bit < w ? b - bit : w;
  return v & ((1u << keep) - 1u);
}
// Signed digit `win` of the scalar, in [-(2^(w-1) - 1), 2^(w-1)], with sum_win d_win 2^(w win) the
// scalar itself as an integer.  `carry` (0 before window 0) goes from each window to the next one up.
// The top bit of window fixed_windows(b, w) - 1 lies at or above b, so that window's value is at most
// 2^(w-1) - 1 + carry and nothing carries out of it.
__host__ __device__ inline int32_t fixed_digit(const uint32_t* s_be, uint32_t sw, uint32_t b, uint32_t w, uint32_t win,
                                               uint32_t& carry) {
  const uint32_t v = fixed_window_bits(s_be, sw, b, w, win) + carry;  // 0 .. 2^w
  carry = v > (1u << (w - 1)) ? 1u : 0u;
  return (int32_t)v - (int32_t)(carry << w);
}

constexpr uint32_t FX_THREADS = 64;       // one wave per workgroup, as k_scale_points
constexpr uint32_t FX_MAX_BASES = 8;
constexpr uint32_t FX_PROJ_WORDS = 3 * NL;  // (X : Y : Z) of one evaluated point
constexpr uint32_t FX_NO_ENTRY = 0xffffffffu;
struct FixedBaseIdx {  // the table's bases as records of the source handle (kernel argument, by value)
  uint32_t v[FX_MAX_BASES];
};

// The table's points, one lane per entry e < total = k Wn 2^(w-1): e = (j Wn + win) 2^(w-1) + d - 1
// gives d 2^(w win) B_j, B_j record bases.v[j] of `recs` (a handle's level 0; every index was checked
// on the host).  The lane gathers the record (lane_gather_record), rebuilds the extended point
// (pt_from_record), doubles it w win times, takes the multiple d with a w-round double-and-add whose
// addition is selected (pt_sel, complete formulas: no branch for the identity or the torsion points),
// and normalises with its own fe_inv -- the table is built once.
// Output: x | y canonical (lane_stage_affine, lane_flush_points); k_prepare_points(PT_FMT_XY) makes
// the records, so they are msm_bases_create's records of these points.
extern "C" __global__ void __launch_bounds__(FX_THREADS, 2) k_fixed_build(const uint32_t* __restrict__ recs,
                                                                        FixedBaseIdx bases, uint32_t w, uint32_t Wn,
                                                                        uint32_t* __restrict__ out_xy,
                                                                        uint32_t total) {
  __shared__ uint4 st[FX_THREADS * 8];
  const uint32_t p0 = blockIdx.x * FX_THREADS;
  const uint32_t np = min(FX_THREADS, total - p0);
  const uint32_t i = threadIdx.x;
  // lanes past the last entry repeat it and write nothing
  const uint32_t e = min(p0 + i, total - 1u);
  const uint32_t d = (e & ((1u << (w - 1)) - 1u)) + 1u;
  const uint32_t t = e >> (w - 1);
  const uint32_t win = t % Wn, j = t / Wn;
  uint32_t base = bases.v[0];
#pragma unroll
  for (uint32_t q = 1; q < FX_MAX_BASES; q++) base = j == q ? bases.v[q] : base;
  uint32_t rec[32];
  lane_gather_record(recs, base, true, rec);
  xyzt p = pt_from_record(rec);
#pragma unroll 1
  for (uint32_t s = w * win; s > 0; s--) p = pt_dbl(p);
  xyzt acc = pt_identity();
#pragma unroll 1
  for (uint32_t bit = w; bit-- > 0;) {
    acc = pt_dbl(acc);
    acc = pt_sel(((d >> bit) & 1u) != 0, acc, pt_add(acc, p));  // (c ? b : a)
  }
  const fe zi = fe_inv(acc.Z);
  lane_stage_affine(st, i, fe_mul(acc.X, zi), fe_mul(acc.Y, zi));
  __syncthreads();
  lane_flush_points<FX_THREADS>(st, out_xy, p0, np, 0u);
}

// The evaluation: Q_i = sum_j s_ij B_j for i < m as (X : Y : Z).  One lane per output, one wave per
// workgroup, four waves per SIMD (k_dense_units' budget and loop: the next entry is worked out beside
// the current addition).
//   scalars  [m][k][sw] big-endian words (the full integers: nothing is reduced mod r), the
//            workgroup's 64 k sw words staged in LDS (lane_stage_scalars).  A bit at or above b is
//            masked (fixed_window_bits) and raises MSM_DEV_ERR_SCALAR_RANGE.
//   digits   fixed_windows(b, w) signed digits per scalar, least significant window first (no
//            doubling orders them); b is the call's width, at most the table's, so the windows read are
//            the table's first ones.  Digit d != 0 of base j, window win, is record
//            (j Wn + win) 2^(w-1) + |d| - 1, gathered with its sign (load_pre_signed) and added with
//            pt_madd; digit 0 adds nothing and reads nothing.
//   output   proj[(g FX_PROJ_WORDS + q) 64 + l] = limb q of X | Y | Z of point 64 g + l: every store and
//            k_fixed_normalise's every load is one coalesced 256-byte row.  Lanes past m store the
//            identity, so the buffer holds whole blocks of 64 and its reader needs no bound.
extern "C" __global__ void __launch_bounds__(FX_THREADS, 4) k_fixed_eval(const uint32_t* __restrict__ table, uint32_t k,
                                                                       uint32_t w, uint32_t Wn,
                                                                       const uint32_t* __restrict__ scalars,
                                                                       uint32_t sw, uint32_t b,
                                                                       uint32_t* __restrict__ proj, uint32_t m,
                                                                       uint32_t* __restrict__ err) {
  extern __shared__ uint4 fx_sc4[];  // FX_THREADS k sw words
  uint32_t* ssc = reinterpret_cast<uint32_t*>(fx_sc4);
  const uint32_t p0 = blockIdx.x * FX_THREADS;
  const uint32_t np = min(FX_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  const uint32_t ksw = k * sw;
  // the workgroup's np k sw scalar words; p0 k sw 4 is a multiple of 256 bytes
  lane_stage_scalars<FX_THREADS>(fx_sc4, scalars, (size_t)p0 * ksw, np * ksw);
  __syncthreads();
  const uint32_t* my = ssc + (live ? i : 0u) * ksw;
  const uint32_t top_mask = (b & 31u) ? (1u << (b & 31u)) - 1u : 0xffffffffu;
  const uint32_t hw = sw - 1u - ((b - 1u) >> 5);  // the word that holds bit b - 1 (0 unless an 8-word call meets a narrower table)
  const uint32_t wn = fixed_windows(b, w);
  uint32_t j = 0, win = 0, carry = 0;
  // the entry (record << 1 | sign) of the digit at (j, win), FX_NO_ENTRY for digit 0; steps (j, win) on
  auto next_entry = [&]() -> uint32_t {
    if (win == 0) {
      uint32_t stray = my[j * sw + hw] & ~top_mask;
      for (uint32_t q = 0; q < hw; q++) stray |= my[j * sw + q];
      if (live && stray) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
    }
    const int32_t d = fixed_digit(my + j * sw, sw, b, w, win, carry);
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const uint32_t ent = d && live ? ((((j * Wn + win) << (w - 1)) + mag - 1u) << 1) | (d < 0 ? 1u : 0u) : FX_NO_ENTRY;
    if (++win == wn) {
      win = 0;
      carry = 0;
      j++;
    }
    return ent;
  };
  xyzt acc = pt_identity();
  const uint32_t steps = k * wn;
  uint32_t ent = next_entry();
#pragma unroll 1
  for (uint32_t s = 1; s <= steps; s++) {
    const uint32_t cur = ent;
    if (s < steps) ent = next_entry();  // the next digit beside this one's add
    if (cur != FX_NO_ENTRY) acc = pt_madd(acc, load_pre_signed(table, cur));
  }
  uint32_t* dst = proj + (size_t)blockIdx.x * FX_PROJ_WORDS * FX_THREADS + i;
#pragma unroll
  for (int q = 0; q < NL; q++) {
    dst[q * FX_THREADS] = acc.X.v[q];
    dst[(NL + q) * FX_THREADS] = acc.Y.v[q];
    dst[(2 * NL + q) * FX_THREADS] = acc.Z.v[q];
  }
}

// The affine output of k_fixed_eval's points with one inversion per E of them (Montgomery's trick
// down a lane, not across the wave: lanes of one SIMD invert in the same issue slots whether one or
// all of them do).  A workgroup takes E consecutive blocks of 64 points, lane l point l of each: the
// prefix products Z_0 .. Z_0 ... Z_(E-1) stay in registers, the last one is inverted, and the walk
// back gives 1 / Z_e = inv prefix_(e-1), inv <- inv Z_e.  3 (E - 1) / E multiplies per point for the
// trick, 3 for x, y and t = x y, 3 for the canonical forms, and fe_inv's ~380 / E: ~56 at E = 8.
// Blocks past the last one are skipped (wave-uniform); the lanes past m in the last block hold the
// identity (Z = 1) and write nothing.  Output through lane_stage_affine and lane_flush_points: wire = 1
// canonical wire records, the identity (0, 1, 0, 1); wire = 0 x | y.  Results are specified for on-curve bases (no Z is 0).
#ifndef MSM_FX_NORM_E
#define MSM_FX_NORM_E 8
#endif
constexpr uint32_t FX_NORM_E = MSM_FX_NORM_E;
__device__ __forceinline__ fe fx_load_coord(const uint32_t* __restrict__ blk, uint32_t c) {
  fe r;
#pragma unroll
  for (int q = 0; q < NL; q++) r.v[q] = blk[(c * NL + q) * FX_THREADS];
  return r;
}
// The two walks over a workgroup's E blocks, unrolled by recursion over the block's number so that the
// prefix products stay in registers (the unroller gives up on loops of this size).  Forward: the prefix
// product through block E0; blocks past the last one (wave-uniform) repeat the one before.
template <uint32_t E0>
__device__ __forceinline__ void fx_norm_prefix(fe (&prefix)[FX_NORM_E], const uint32_t* __restrict__ mine, uint32_t g0,
                                               uint32_t nblk) {
  if constexpr (E0 < FX_NORM_E) {
    prefix[E0] = prefix[E0 - 1];
    if (g0 + E0 < nblk)
      prefix[E0] = fe_mul(prefix[E0 - 1], fx_load_coord(mine + (size_t)E0 * FX_PROJ_WORDS * FX_THREADS, 2));
    fx_norm_prefix<E0 + 1>(prefix, mine, g0, nblk);
  }
}
// Backward from block E0: 1 / Z of the block's point out of `inv` = 1 / (Z_0 ... Z_E0), the affine
// point staged and stored, and `inv` handed down without Z_E0.
template <uint32_t E0>
__device__ __forceinline__ void fx_norm_emit(const fe (&prefix)[FX_NORM_E], fe inv, const uint32_t* __restrict__ mine,
                                             uint32_t g0, uint32_t nblk, uint4* st, uint32_t* __restrict__ out,
                                             uint32_t m, uint32_t wire) {
  if (g0 + E0 < nblk) {  // wave-uniform
    const uint32_t* blk = mine + (size_t)E0 * FX_PROJ_WORDS * FX_THREADS;
    fe zi = inv;
    if constexpr (E0 > 0) {
      zi = fe_mul(inv, prefix[E0 - 1]);
      inv = fe_mul(inv, fx_load_coord(blk, 2));
    }
    const fe x = fe_mul(fx_load_coord(blk, 0), zi);
    const fe y = fe_mul(fx_load_coord(blk, 1), zi);
    __syncthreads();  // the previous block's stores have read st
    lane_stage_affine(st, threadIdx.x, x, y);
    __syncthreads();
    const uint32_t pb = (g0 + E0) * FX_THREADS;
    lane_flush_points<FX_THREADS>(st, out, pb, min(FX_THREADS, m - pb), wire);
  }
  if constexpr (E0 > 0) fx_norm_emit<E0 - 1>(prefix, inv, mine, g0, nblk, st, out, m, wire);
}
extern "C" __global__ void __launch_bounds__(FX_THREADS) k_fixed_normalise(const uint32_t* __restrict__ proj,
                                                                          uint32_t* __restrict__ out, uint32_t m,
                                                                          uint32_t wire) {
  __shared__ uint4 st[FX_THREADS * 8];
  const uint32_t nblk = (m + FX_THREADS - 1) / FX_THREADS;
  const uint32_t g0 = blockIdx.x * FX_NORM_E;
  const uint32_t* mine = proj + (size_t)g0 * FX_PROJ_WORDS * FX_THREADS + threadIdx.x;
  fe prefix[FX_NORM_E];
  prefix[0] = fx_load_coord(mine, 2);
  fx_norm_prefix<1>(prefix, mine, g0, nblk);
  fx_norm_emit<FX_NORM_E - 1>(prefix, fe_inv(prefix[FX_NORM_E - 1]), mine, g0, nblk, st, out, m, wire);
}

// ---------------------------------------------------------------------------------------------
// vector tables (msm_fixed_create_vector): the same tables over 9 .. 4096 bases, rows cut into parts
// ---------------------------------------------------------------------------------------------
// One lane per output over all k Wn digits (k_fixed_eval) is a chain of tens of thousands of dependent
// additions at k = 1024, and m rows fill m / 64 waves.  Here the k bases are cut into P = ceil(k / G)
// parts of G consecutive bases (the last one may be shorter): k_vector_eval sums one part of 64 rows per
// wave, k_vector_fold adds up to VX_FOLD parts of a row per lane and pass, and the last pass leaves
// (X : Y : Z) in k_fixed_eval's blocks for k_fixed_normalise.
constexpr uint32_t VX_MAX_BASES = 4096;
constexpr uint32_t VX_MAX_GROUP = 8;          // G: bases per part, with G sw <= VX_LANE_WORDS
constexpr uint32_t VX_LANE_WORDS = 64;        // scalar words a lane keeps in LDS
constexpr uint32_t VX_FOLD = 16;              // parts one lane of k_vector_fold adds
constexpr uint32_t VX_PART_WORDS = 4 * NL;    // X | Y | Z | T of one partial sum

// k_fixed_build's lane with the k base indices in device memory (the slot's sub_idx; every index was
// checked on the host): the same statements, so the same records.
extern "C" __global__ void __launch_bounds__(FX_THREADS, 2) k_vector_build(const uint32_t* __restrict__ recs,
                                                                         const uint32_t* __restrict__ bases,
                                                                         uint32_t w, uint32_t Wn,
                                                                         uint32_t* __restrict__ out_xy,
                                                                         uint32_t total) {
  __shared__ uint4 st[FX_THREADS * 8];
  const uint32_t p0 = blockIdx.x * FX_THREADS;
  const uint32_t np = min(FX_THREADS, total - p0);
  const uint32_t i = threadIdx.x;
  // lanes past the last entry repeat it and write nothing
  const uint32_t e = min(p0 + i, total - 1u);
  const uint32_t d = (e & ((1u << (w - 1)) - 1u)) + 1u;
  const uint32_t t = e >> (w - 1);
  const uint32_t win = t % Wn, j = t / Wn;
  uint32_t rec[32];
  lane_gather_record(recs, bases[j], true, rec);
  xyzt p = pt_from_record(rec);
#pragma unroll 1
  for (uint32_t s = w * win; s > 0; s--) p = pt_dbl(p);
  xyzt acc = pt_identity();
#pragma unroll 1
  for (uint32_t bit = w; bit-- > 0;) {
    acc = pt_dbl(acc);
    acc = pt_sel(((d >> bit) & 1u) != 0, acc, pt_add(acc, p));  // (c ? b : a)
  }
  const fe zi = fe_inv(acc.Z);
  lane_stage_affine(st, i, fe_mul(acc.X, zi), fe_mul(acc.Y, zi));
  __syncthreads();
  lane_flush_points<FX_THREADS>(st, out_xy, p0, np, 0u);
}

// `cnt` scalar words of each of a wave's np rows into LDS, row l's at ssc[l * stride ..): row l's words
// start at word row0 + l * pitch of `scalars` (lane_stage_scalars takes one contiguous block; a part's
// scalars are a column of the [m][k][sw] array).  16-byte loads where the vector is 16-byte aligned and
// sw is a multiple of 4 -- every row's start and count are then multiples of 4 words --, word by word
// elsewhere, as the narrow recode loads.
__device__ __forceinline__ void vx_stage_rows(uint32_t* ssc, const uint32_t* __restrict__ scalars, size_t row0,
                                              size_t pitch, uint32_t np, uint32_t cnt, uint32_t stride, uint32_t sw) {
  if (!(reinterpret_cast<uintptr_t>(scalars) & 15u) && !(sw & 3u)) {
    const uint32_t c4 = cnt >> 2;
    for (uint32_t g = threadIdx.x; g < np * c4; g += FX_THREADS) {
      const uint32_t l = g / c4, q = g - l * c4;
      reinterpret_cast<uint4*>(ssc + l * stride)[q] = reinterpret_cast<const uint4*>(scalars + row0 + l * pitch)[q];
    }
  } else {
    for (uint32_t g = threadIdx.x; g < np * cnt; g += FX_THREADS) {
      const uint32_t l = g / cnt, q = g - l * cnt;
      ssc[l * stride + q] = scalars[row0 + l * pitch + q];
    }
  }
}

// Part blockIdx.y of rows [64 blockIdx.x, +64): sum over the part's bases j in [G y, min(k, G y + G)) of
// s_ij B_j as (X : Y : Z : T).  One lane per row, one wave per workgroup, k_fixed_eval's budget and
// loop; j and win are wave-uniform, so the 64 lanes of a step gather from one sub-table of 2^(w-1)
// records.
//   scalars  [m][k][sw] big-endian words; the wave's 64 rows of the part's G sw words staged in LDS
//            (vx_stage_rows), G sw <= VX_LANE_WORDS.  A bit at or above b is masked (fixed_window_bits)
//            and raises MSM_DEV_ERR_SCALAR_RANGE.
//   digits   as k_fixed_eval's: digit d != 0 of base j, window win, is record (j Wn + win) 2^(w-1) +
//            |d| - 1; digit 0 adds nothing and reads nothing.
//   output   part[((y nblk + x) VX_PART_WORDS + q) 64 + l] = limb q of X | Y | Z | T of row 64 x + l, nblk
//            = gridDim.x: coalesced 256-byte rows, as proj's.  Lanes past m store the identity.
extern "C" __global__ void __launch_bounds__(FX_THREADS, 4) k_vector_eval(const uint32_t* __restrict__ table, uint32_t k,
                                                                        uint32_t w, uint32_t Wn, uint32_t G,
                                                                        const uint32_t* __restrict__ scalars,
                                                                        uint32_t sw, uint32_t b,
                                                                        uint32_t* __restrict__ part, uint32_t m,
                                                                        uint32_t* __restrict__ err) {
  extern __shared__ uint4 vx_sc4[];  // FX_THREADS G sw words
  uint32_t* ssc = reinterpret_cast<uint32_t*>(vx_sc4);
  const uint32_t p0 = blockIdx.x * FX_THREADS;
  const uint32_t np = min(FX_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  const uint32_t j0 = blockIdx.y * G;
  const uint32_t g = min(G, k - j0);  // the part's bases
  const uint32_t gsw = G * sw;
  vx_stage_rows(ssc, scalars, ((size_t)p0 * k + j0) * sw, (size_t)k * sw, np, g * sw, gsw, sw);
  __syncthreads();
  const uint32_t* my = ssc + (live ? i : 0u) * gsw;
  const uint32_t top_mask = (b & 31u) ? (1u << (b & 31u)) - 1u : 0xffffffffu;
  const uint32_t hw = sw - 1u - ((b - 1u) >> 5);  // the word that holds bit b - 1
  const uint32_t wn = fixed_windows(b, w);
  uint32_t j = 0, win = 0, carry = 0;
  // k_fixed_eval's next_entry over the part's bases: scalar j of the lane's staged row is base j0 + j
  auto next_entry = [&]() -> uint32_t {
    if (win == 0) {
      uint32_t stray = my[j * sw + hw] & ~top_mask;
      for (uint32_t q = 0; q < hw; q++) stray |= my[j * sw + q];
      if (live && stray) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
    }
    const int32_t d = fixed_digit(my + j * sw, sw, b, w, win, carry);
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const uint32_t ent =
        d && live ? (((((j0 + j) * Wn + win) << (w - 1)) + mag - 1u) << 1) | (d < 0 ? 1u : 0u) : FX_NO_ENTRY;
    if (++win == wn) {
      win = 0;
      carry = 0;
      j++;
    }
    return ent;
  };
  xyzt acc = pt_identity();
  const uint32_t steps = g * wn;
  uint32_t ent = next_entry();
#pragma unroll 1
  for (uint32_t s = 1; s <= steps; s++) {
    const uint32_t cur = ent;
    if (s < steps) ent = next_entry();  // the next digit beside this one's add
    if (cur != FX_NO_ENTRY) acc = pt_madd(acc, load_pre_signed(table, cur));
  }
  uint32_t* dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VX_PART_WORDS * FX_THREADS + i;
#pragma unroll
  for (int q = 0; q < NL; q++) {
    dst[q * FX_THREADS] = acc.X.v[q];
    dst[(NL + q) * FX_THREADS] = acc.Y.v[q];
    dst[(2 * NL + q) * FX_THREADS] = acc.Z.v[q];
    dst[(3 * NL + q) * FX_THREADS] = acc.T.v[q];
  }
}

// A lane's partial sum out of a block of k_vector_eval's layout (`blk` = the block's first word + lane).
__device__ __forceinline__ xyzt vx_load_point(const uint32_t* __restrict__ blk) {
  xyzt r;
#pragma unroll
  for (int q = 0; q < NL; q++) {
    r.X.v[q] = blk[q * FX_THREADS];
    r.Y.v[q] = blk[(NL + q) * FX_THREADS];
    r.Z.v[q] = blk[(2 * NL + q) * FX_THREADS];
    r.T.v[q] = blk[(3 * NL + q) * FX_THREADS];
  }
  return r;
}
// One pass of the sum over a row's parts: output part blockIdx.y of rows [64 blockIdx.x, +64) is the
// sum of input parts [VX_FOLD y, min(parts, VX_FOLD y + VX_FOLD)), one lane per row.  The additions
// are the complete pt_add: parts of a row may cancel or coincide, and every input is a pt_madd or
// pt_add output or the identity.  `last` (one output part): X | Y | Z into proj's blocks, k_fixed_eval's
// layout; else X | Y | Z | T into `out` in the layout read.
extern "C" __global__ void __launch_bounds__(FX_THREADS) k_vector_fold(const uint32_t* __restrict__ in,
                                                                      uint32_t* __restrict__ out, uint32_t parts,
                                                                      uint32_t last) {
  const uint32_t nblk = gridDim.x;
  const uint32_t q0 = blockIdx.y * VX_FOLD;
  const uint32_t cnt = min(VX_FOLD, parts - q0);
  const size_t step = (size_t)nblk * VX_PART_WORDS * FX_THREADS;  // from a part to the next
  const uint32_t* src = in + ((size_t)q0 * nblk + blockIdx.x) * VX_PART_WORDS * FX_THREADS + threadIdx.x;
  xyzt acc = vx_load_point(src);
#pragma unroll 1
  for (uint32_t q = 1; q < cnt; q++) acc = pt_add(acc, vx_load_point(src + q * step));
  if (last) {
    uint32_t* dst = out + (size_t)blockIdx.x * FX_PROJ_WORDS * FX_THREADS + threadIdx.x;
#pragma unroll
    for (int q = 0; q < NL; q++) {
      dst[q * FX_THREADS] = acc.X.v[q];
      dst[(NL + q) * FX_THREADS] = acc.Y.v[q];
      dst[(2 * NL + q) * FX_THREADS] = acc.Z.v[q];
    }
  } else {
    uint32_t* dst = out + ((size_t)blockIdx.y * nblk + blockIdx.x) * VX_PART_WORDS * FX_THREADS + threadIdx.x;
#pragma unroll
    for (int q = 0; q < NL; q++) {
      dst[q * FX_THREADS] = acc.X.v[q];
      dst[(NL + q) * FX_THREADS] = acc.Y.v[q];
      dst[(2 * NL + q) * FX_THREADS] = acc.Z.v[q];
      dst[(3 * NL + q) * FX_THREADS] = acc.T.v[q];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// pairwise combinations of bases handles (msm_bases_combine*): R_i = a_i A_i +- b_i B_i
// ---------------------------------------------------------------------------------------------
// One lane per output point and one wave per workgroup, as k_scale_points.  Three kernels, chosen on
// the host (the form is wave-uniform): k_combine_sum (no scalars), k_combine_one (one side has
// scalars) and k_combine_joint (both).  Every one leaves (X : Y : Z) in k_fixed_eval's block layout
// and k_fixed_normalise writes the points, so eight outputs share one inversion.
constexpr uint32_t CB_THREADS = FX_THREADS;
static_assert(CB_THREADS == 64, "the combine kernels write k_fixed_eval's blocks of 64");
// One side's m bases: records `first + i` (indices == nullptr) or `indices[i]` of the n records `recs`
// of a handle's level 0 (kernel argument, by value).
struct CombineSide {
  const uint32_t* recs;
  const uint32_t* indices;
  uint32_t n, first;
};
// Digit j (j < b) of the joint ladder: bit j of a + 2 * bit j of b, both b-bit scalars of sw =
// ceil(b / 32) big-endian words.  The ladder asks for the digits below b only, so a stray bit at or
// above b (flagged by the kernel) never reaches it; a j past them reads as 0.  Runs on the host too
// (msm_test_combine_digits).
__host__ __device__ inline uint32_t combine_digit(const uint32_t* a_be, const uint32_t* b_be, uint32_t sw, uint32_t b,
                                                  uint32_t j) {
  if (j >= b) return 0u;
  const uint32_t wi = sw - 1 - (j >> 5), sh = j & 31u;
  return ((a_be[wi] >> sh) & 1u) | (((b_be[wi] >> sh) & 1u) << 1);
}
// A side's records into the staging array (range form; the indexed form stages nothing), and lane i's
// record out of it or gathered by its index.  An index >= n is replaced by 0 and raises
// MSM_DEV_ERR_BAD_INDEX.  A barrier goes between the two, and before the array is staged again.
__device__ __forceinline__ void cb_stage_side(uint4* st, const CombineSide& s, uint32_t p0, uint32_t np) {
  if (!s.indices)
    lane_stage_records<CB_THREADS>(st, reinterpret_cast<const uint4*>(s.recs) + ((size_t)s.first + p0) * 8, np);
}
__device__ __forceinline__ void cb_read_side(const uint4* st, const CombineSide& s, uint32_t p0, uint32_t i, bool live,
                                             uint32_t* __restrict__ err, uint32_t (&rec)[32]) {
  if (s.indices) {
    uint32_t idx = live ? s.indices[p0 + i] : 0u;
    if (idx >= s.n) {
      idx = 0;
      atomicOr(err, MSM_DEV_ERR_BAD_INDEX);
    }
    lane_gather_record(s.recs, idx, live, rec);
  } else {
    lane_read_record(st, i, live, rec);
  }
}
// -P for `neg` (wave-uniform): X and T negated (fe_neg: normalised, at most 8p) and put through a
// multiply by one, so every coordinate is again an fe_mul output as pt_add and pt_dbl take them.
__device__ __forceinline__ xyzt cb_neg_if(const xyzt& p, bool neg) {
  xyzt r = p;
  if (neg) {
    const fe unit = fe_one();
    r.X = fe_mul(fe_neg(p.X), unit);
    r.T = fe_mul(fe_neg(p.T), unit);
  }
  return r;
}
// The workgroup's scalars into LDS: np sw words, or the one scalar every lane reads (`bcast`); and
// lane i's scalar there.  A bit at or above b raises MSM_DEV_ERR_SCALAR_RANGE (the digit functions mask it).
__device__ __forceinline__ void cb_stage_scalars(uint4* ssc4, const uint32_t* __restrict__ scalars, bool bcast,
                                                 uint32_t p0, uint32_t np, uint32_t sw) {
  if (bcast) lane_stage_scalars<CB_THREADS>(ssc4, scalars, 0, sw);
  else lane_stage_scalars<CB_THREADS>(ssc4, scalars, (size_t)p0 * sw, np * sw);
}
__device__ __forceinline__ const uint32_t* cb_my_scalar(const uint4* ssc4, bool bcast, uint32_t i, bool live, uint32_t sw,
                                                        uint32_t b, uint32_t* __restrict__ err) {
  const uint32_t* my = reinterpret_cast<const uint32_t*>(ssc4) + (bcast ? 0u : i * sw);
  const uint32_t top_mask = (b & 31u) ? (1u << (b & 31u)) - 1u : 0xffffffffu;
  if (live && (my[0] & ~top_mask)) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
  return my;
}
// Lane i's point into the block's (X : Y : Z) rows (k_fixed_eval's layout); a lane past m stores the
// identity, so k_fixed_normalise needs no bound and meets no Z = 0.
__device__ __forceinline__ void cb_store_proj(uint32_t* __restrict__ proj, const xyzt& acc, bool live) {
  const xyzt r = pt_sel(live, pt_identity(), acc);
  uint32_t* dst = proj + (size_t)blockIdx.x * FX_PROJ_WORDS * CB_THREADS + threadIdx.x;
#pragma unroll
  for (int q = 0; q < NL; q++) {
    dst[q * CB_THREADS] = r.X.v[q];
    dst[(NL + q) * CB_THREADS] = r.Y.v[q];
    dst[(2 * NL + q) * CB_THREADS] = r.Z.v[q];
  }
}

// R_i = A_i + B_i, or A_i - B_i with `sub`: one complete addition per lane.
extern "C" __global__ void __launch_bounds__(CB_THREADS) k_combine_sum(CombineSide A, CombineSide B, uint32_t sub,
                                                                      uint32_t* __restrict__ proj, uint32_t m,
                                                                      uint32_t* __restrict__ err) {
  __shared__ uint4 st[CB_THREADS * 8];
  const uint32_t p0 = blockIdx.x * CB_THREADS;
  const uint32_t np = min(CB_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  uint32_t rec[32];
  cb_stage_side(st, A, p0, np);
  __syncthreads();
  cb_read_side(st, A, p0, i, live, err, rec);
  const xyzt pa = pt_from_record(rec);
  __syncthreads();
  cb_stage_side(st, B, p0, np);
  __syncthreads();
  cb_read_side(st, B, p0, i, live, err, rec);
  const xyzt pb = cb_neg_if(pt_from_record(rec), sub != 0);
  cb_store_proj(proj, pt_add(pa, pb), live);
}

// R_i = s_i S_i + Q_i: k_scale_points' ladder (scale_digit, scale_windows: 2-bit windows over
// {O, S, 2S, 3S}) on the side with scalars, then one addition of the plain side's point.  The host
// names the sides, so that MSM_COMBINE_SUB stays on B: `neg` bit 0 negates S_i, bit 1 negates Q_i.
// Q's record is staged in the array S's has left, and read (or gathered) after the ladder, so that it
// holds no registers across the loop.
extern "C" __global__ void __launch_bounds__(CB_THREADS, 2) k_combine_one(CombineSide S, CombineSide Q,
                                                                         const uint32_t* __restrict__ scalars,
                                                                         uint32_t bcast, uint32_t sw, uint32_t b,
                                                                         uint32_t neg, uint32_t* __restrict__ proj,
                                                                         uint32_t m, uint32_t* __restrict__ err) {
  __shared__ uint4 st[CB_THREADS * 8];
  __shared__ uint4 ssc4[CB_THREADS * 2];
  const uint32_t p0 = blockIdx.x * CB_THREADS;
  const uint32_t np = min(CB_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  cb_stage_scalars(ssc4, scalars, bcast != 0, p0, np, sw);
  uint32_t rec[32];
  cb_stage_side(st, S, p0, np);
  __syncthreads();
  cb_read_side(st, S, p0, i, live, err, rec);
  const xyzt p1 = cb_neg_if(pt_from_record(rec), (neg & 1u) != 0);
  __syncthreads();
  cb_stage_side(st, Q, p0, np);
  __syncthreads();
  const uint32_t* my = cb_my_scalar(ssc4, bcast != 0, i, live, sw, b, err);
  xyzt acc = pt_identity();
  const xyzt p2 = pt_dbl(p1);
  const xyzt p3 = pt_add(p2, p1);
  const xyzt p0i = pt_identity();
#pragma unroll 1
  for (uint32_t j = scale_windows(b); j-- > 0;) {
    acc = pt_dbl(pt_dbl(acc));
    const uint32_t d = live ? scale_digit(my, sw, b, j) : 0u;
    const bool hi = (d & 2u) != 0;
    acc = pt_add(acc, pt_sel((d & 1u) != 0, pt_sel(hi, p0i, p2), pt_sel(hi, p1, p3)));
  }
  cb_read_side(st, Q, p0, i, live, err, rec);
  const xyzt pq = cb_neg_if(pt_from_record(rec), (neg & 2u) != 0);
  cb_store_proj(proj, pt_add(acc, pq), live);
}

// R_i = a_i A_i + b_i B_i (B negated with `sub`): the joint (Straus) ladder over {O, A, B, A + B},
// b rounds of one doubling and one complete addition of the entry combine_digit names, most
// significant bit first.  The entry is chosen with pt_sel: no lane takes a branch of its own.  The
// trip count is the kernel argument alone.  Table and accumulator are 144 VGPRs, as k_scale_points'.
extern "C" __global__ void __launch_bounds__(CB_THREADS, 2) k_combine_joint(
    CombineSide A, CombineSide B, const uint32_t* __restrict__ a_scalars, const uint32_t* __restrict__ b_scalars,
    uint32_t bcast, uint32_t sw, uint32_t b, uint32_t sub, uint32_t* __restrict__ proj, uint32_t m,
    uint32_t* __restrict__ err) {
  __shared__ uint4 st[CB_THREADS * 8];
  __shared__ uint4 sa4[CB_THREADS * 2];
  __shared__ uint4 sb4[CB_THREADS * 2];
  const uint32_t p0 = blockIdx.x * CB_THREADS;
  const uint32_t np = min(CB_THREADS, m - p0);
  const uint32_t i = threadIdx.x;
  const bool live = i < np;
  cb_stage_scalars(sa4, a_scalars, (bcast & 1u) != 0, p0, np, sw);
  cb_stage_scalars(sb4, b_scalars, (bcast & 2u) != 0, p0, np, sw);
  uint32_t rec[32];
  cb_stage_side(st, A, p0, np);
  __syncthreads();
  cb_read_side(st, A, p0, i, live, err, rec);
  const xyzt pa = pt_from_record(rec);
  __syncthreads();
  cb_stage_side(st, B, p0, np);
  __syncthreads();
  cb_read_side(st, B, p0, i, live, err, rec);
  const xyzt pb = cb_neg_if(pt_from_record(rec), sub != 0);
  const uint32_t* mya = cb_my_scalar(sa4, (bcast & 1u) != 0, i, live, sw, b, err);
  const uint32_t* myb = cb_my_scalar(sb4, (bcast & 2u) != 0, i, live, sw, b, err);
  const xyzt pab = pt_add(pa, pb);
  const xyzt p0i = pt_identity();
  xyzt acc = pt_identity();
#pragma unroll 1
  for (uint32_t j = b; j-- > 0;) {
    acc = pt_dbl(acc);
    const uint32_t d = live ? combine_digit(mya, myb, sw, b, j) : 0u;
    const bool hi = (d & 2u) != 0;
    acc = pt_add(acc, pt_sel((d & 1u) != 0, pt_sel(hi, p0i, pb), pt_sel(hi, pa, pab)));
  }
  cb_store_proj(proj, acc, live);
}

// ---------------------------------------------------------------------------------------------
// scalar recoding
// ---------------------------------------------------------------------------------------------
// Signed recoding of one scalar (little-endian words, consumed in place).  Calls f(window,
// digit) for every window, digit in [-(2^(b-1)-1), 2^(b-1)] for a window of b bits (win_bits);
// sum_w digit_w 2^win_off(w) == scalar exactly.  The scalar is shifted down b bits per window
// with v_alignbit so no register array is ever indexed dynamically (that would spill it to
// scratch).
template <typename F>
__device__ __forceinline__ void recode(uint32_t s[8], const MsmDims& d, F&& f) {
  uint32_t carry = 0;
  // carries only climb: a window range's digits need the windows below it, never those above
  // (a lower share of a windows split stops at its top window)
  const uint32_t wend = d.w0 + d.Wr;
  for (uint32_t w = 0; w < wend; w++) {
    const uint32_t b = win_bits(d, w);
    const uint32_t half = 1u << (b - 1);
    const uint32_t v = (s[0] & ((1u << b) - 1u)) + carry;
#pragma unroll
    for (int q = 0; q < 7; q++) s[q] = __builtin_amdgcn_alignbit(s[q + 1], s[q], b);
    s[7] >>= b;
    int32_t digit;
    if (v > half) {
      digit = (int32_t)v - (int32_t)(2 * half);
      carry = 1;
    } else {
      digit = (int32_t)v;
      carry = 0;
    }
    f(w, digit);
  }
}

__device__ __forceinline__ void load_scalar(const uint32_t* __restrict__ scalars, uint32_t i, uint32_t s[8]) {
  load_be_words(scalars + (size_t)i * 8, s);
}

// Wave-level inclusive scan of one u32 per lane (64 lanes, all active) by DPP: four row shifts
// scan each 16-lane row, two row broadcasts carry the rows' totals across.  No LDS round trips
// (the ds_bpermute form took ~0.5 us of latency per scan, a tenth of a k_fine_sort workgroup's life).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
}
// Exclusive scan of one u32 per lane; `total` = the wave sum.
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total) {
  const uint32_t x = wave_incl_scan(v);
  total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
  return x - v;
}

// Exclusive scan of cnt[0..nf) in LDS by the first wave of the workgroup.  256 counters (the
// scatter's bins, the wide fine sorts) go as one 16-B vector per lane and 128 as one 8-B vector;
// other multiples of 256 as runs of vectors read twice (a register array would cost the calling
// kernels their occupancy); other counts take the scalar loop.
__device__ __forceinline__ void lds_excl_scan_wave0(uint32_t* cnt, uint32_t nf) {
  if (threadIdx.x >= 64) return;
  const uint32_t lane = threadIdx.x;
  if (nf == 256) {
    uint4* c4 = reinterpret_cast<uint4*>(cnt) + lane;
    const uint4 v = *c4;
    uint32_t tot;
    const uint32_t run = wave_excl_scan(v.x + v.y + v.z + v.w, tot);
    *c4 = make_uint4(run, run + v.x, run + v.x + v.y, run + v.x + v.y + v.z);
    return;
  }
  if ((nf & 255u) == 0) {
    const uint32_t n4 = nf / 256;  // uint4s per lane
    uint4* c4 = reinterpret_cast<uint4*>(cnt) + lane * n4;
    uint32_t local = 0;
    for (uint32_t k = 0; k < n4; k++) {
      const uint4 v = c4[k];
      local += v.x + v.y + v.z + v.w;
    }
    uint32_t tot;
    uint32_t run = wave_excl_scan(local, tot);
    for (uint32_t k = 0; k < n4; k++) {
      const uint4 v = c4[k];
      c4[k] = make_uint4(run, run + v.x, run + v.x + v.y, run + v.x + v.y + v.z);
      run += v.x + v.y + v.z + v.w;
    }
    return;
  }
  if (nf == 128) {
    uint2* c2 = reinterpret_cast<uint2*>(cnt) + lane;
    const uint2 v = *c2;
    uint32_t tot;
    const uint32_t run = wave_excl_scan(v.x + v.y, tot);
    *c2 = make_uint2(run, run + v.x);
    return;
  }
  const uint32_t per = (nf + 63) / 64;
  const uint32_t lo = lane * per;
  uint32_t local = 0;
  for (uint32_t k = 0; k < per; k++)
    if (lo + k < nf) local += cnt[lo + k];
  uint32_t tot;
  uint32_t run = wave_excl_scan(local, tot);
  for (uint32_t k = 0; k < per; k++) {
    if (lo + k < nf) {
      const uint32_t c = cnt[lo + k];
      cnt[lo + k] = run;
      run += c;
    }
  }
}

// Fine bits of MSM window `wm`: every window keeps nbc coarse bins over its OWN buckets, so a
// window narrower than the widest (the balanced 15-bit windows at c = 16, the 13-bit ones at
// c = 14, the 3-bit overflow window) sorts fb - (c - b) fine bits per bin and its bins are as full
// as the others'.  (With one fb for all, half of such a window's bins held all its entries --
// 8,192 per bin at 2^20, past k_fine_sort's LDS staging -- and took the slow unstaged path.)
__device__ __forceinline__ uint32_t win_fb(const MsmDims& d, uint32_t wm) {
  const uint32_t drop = d.c - win_bits(d, wm);
  return d.fb > drop ? d.fb - drop : 0u;
}
// The same for window w of a launch's batch (w in [0, W): MSM w / Wr, local window w % Wr).
__device__ __forceinline__ uint32_t batch_win_fb(const MsmDims& d, uint32_t w) { return win_fb(d, d.w0 + w % d.Wr); }

// Digit codes, window-major digits[w][i]: bucket b = |d| - 1 plus a sign bit, or ZERO.
//   c <= 16: uint16_t, sign = bit 15, ZERO = 0xffff (b = 0x7fff with the sign set would be
//            d = -2^15, which signed recoding never produces)
//   c >  16: uint32_t, sign = bit 31, ZERO = 0xffffffff
template <typename T>
struct DigitCode;
template <>
struct DigitCode<uint16_t> {
  static constexpr uint32_t ZERO = 0xffffu, SIGN = 0x8000u, MAG = 0x7fffu, SHIFT = 15;
};
template <>
struct DigitCode<uint32_t> {
  static constexpr uint32_t ZERO = 0xffffffffu, SIGN = 0x80000000u, MAG = 0x7fffffffu, SHIFT = 31;
};

// Pass 0+1 (fused): each workgroup recodes RC_SPAN scalars into window-major digit codes (the
// window-major layout is the first sort level for free: each window is one contiguous array) and
// builds, in LDS, their histogram over every window's nbc coarse bins, flushed with global
// atomics into the bin totals colsum[w][bin] (kept zeroed between MSMs by k_fine_sort).  Digits
// are read back only once, by k_part_scatter.
#ifndef MSM_PT_THREADS
#define MSM_PT_THREADS 1024
#endif
#ifndef MSM_PS_R
#define MSM_PS_R 16
#endif
constexpr uint32_t PT_THREADS = MSM_PT_THREADS;
constexpr uint32_t PS_R = MSM_PS_R;  // digits per lane (ch = PT_THREADS * PS_R)
#ifndef MSM_RC_THREADS
#define MSM_RC_THREADS 1024
#endif
constexpr uint32_t RC_THREADS = MSM_RC_THREADS;
#ifndef MSM_RC_SPAN
#define MSM_RC_SPAN 4096
#endif
constexpr uint32_t RC_SPAN = MSM_RC_SPAN;  // scalars per recode workgroup
// Signed recoding with the window geometry fixed at compile time (the common widths: q = 15,
// nhi = 14 is c = 16; 14/16 c = 15; 13/7 c = 14; 12/14 c = 13).  Adding the constant
// C = sum_w (2^(b_w - 1) - 1) 2^off_w to the scalar makes every window independent: digit_w =
// bits_w(s + C) - (2^(b_w - 1) - 1) is exactly the carry recoding of `recode` (a window's bits plus
// the carry v give v when v <= 2^(b-1), else v - 2^b with a carry out -- the same as
// (v + 2^(b-1) - 1) mod 2^b - (2^(b-1) - 1) and the add's own carry), and the overflow window is
// t's bits 254 and up, the add's carry out included (<= 4, never negative).  So each window is one
// funnel shift of two known words and a mask: no 256-bit shift per window and no per-window scalar
// bookkeeping (the generic loop issued more scalar than vector instructions).
template <uint32_t Q, uint32_t NHI>
struct FixedGeo {
  static constexpr uint32_t WMAIN = (MAIN_BITS - NHI) / Q;
  static constexpr uint32_t bits(uint32_t w) { return w < NHI ? Q + 1 : Q; }
  static constexpr uint32_t off(uint32_t w) { return w * Q + (w < NHI ? w : NHI); }
  struct Words {
    uint32_t v[8];
  };
  static constexpr Words bias() {
    Words c{};
    for (uint32_t w = 0; w < WMAIN; w++) {
      const uint64_t h = (1ull << (bits(w) - 1)) - 1ull;  // < 2^16, spans at most two words
      const uint32_t o = off(w), k = o / 32, sh = o % 32;
      const uint64_t lo = (uint64_t)c.v[k] + ((h << sh) & 0xffffffffull);
      c.v[k] = (uint32_t)lo;
      uint64_t carry = (lo >> 32) + ((h << sh) >> 32);
      for (uint32_t j = k + 1; j < 8 && carry; j++) {
        const uint64_t x = (uint64_t)c.v[j] + carry;
        c.v[j] = (uint32_t)x;
        carry = x >> 32;
      }
    }
    return c;
  }
};

// The recode's LDS histogram [Wr][nbc] into the bin totals colsum[w][bin] (global atomics), and
// the windows' totals (LDS words after the histogram, summed per wave when a wave's 64 bins lie in
// one window) into wtot[w] = colsum[nbins + w]: k_part_scatter takes a window's first slot from
// the totals of the windows below it.  colsum and wtot are zeroed again by k_fine_sort.
__device__ __forceinline__ void flush_hist(uint32_t* lds_hist, const MsmDims& d, uint32_t w0,
                                           uint32_t* __restrict__ colsum) {
  const uint32_t nh = d.Wr * d.nbc, lg = __builtin_ctz(d.nbc);
  uint32_t* wt = lds_hist + nh;
  for (uint32_t b = threadIdx.x; b < nh; b += RC_THREADS) {
    const uint32_t v = lds_hist[b];
    if (v) atomicAdd(&colsum[w0 * d.nbc + b], v);
    if (d.nbc >= 64) {
      const uint32_t t = wave_incl_scan(v);
      if ((threadIdx.x & 63) == 63 && t) atomicAdd(&wt[b >> lg], t);
    } else if (v) {
      atomicAdd(&wt[b >> lg], v);
    }
  }
  __syncthreads();
  if (threadIdx.x < d.Wr && wt[threadIdx.x]) atomicAdd(&colsum[d.nbins + w0 + threadIdx.x], wt[threadIdx.x]);
}

// The frame every recode kernel shares.  recode_begin zeroes the LDS histogram [Wr][nbc] and the
// window totals after it; recode_end reports a lane's out-of-range scalar (`bad`, the kernels that
// take `err`) and flushes the histogram.  (k_recode_hist and k_recode_fixed spell the end out: a
// phase probe stands between its barrier and its flush.)
__device__ __forceinline__ void recode_begin(uint32_t* lds_hist, const MsmDims& d) {
  for (uint32_t b = threadIdx.x; b < d.Wr * d.nbc + d.Wr; b += RC_THREADS) lds_hist[b] = 0;
  __syncthreads();
}
__device__ __forceinline__ void recode_end(uint32_t* lds_hist, const MsmDims& d, uint32_t w0,
                                           uint32_t* __restrict__ colsum, bool bad = false,
                                           uint32_t* __restrict__ err = nullptr) {
  if (bad) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
  __syncthreads();
  flush_hist(lds_hist, d, w0, colsum);
}

// One scalar of the carry recodes (k_recode_hist, k_recode_hist_le): s is scalar i's little-endian
// words.  Carries only climb, so windows below the launch's range [d.w0, d.w0 + d.Wr) are recoded
// for their carries (the generic loop stops at the range's top); only the range is written and
// counted.  HALF: the range may end in half windows (never on the little-endian launch, and the
// test cost it a third of its time).
template <typename T, bool HALF>
__device__ __forceinline__ void recode_carry(uint32_t s[8], uint32_t i, const MsmDims& d, uint32_t w0,
                                             T* __restrict__ digits, uint32_t* lds_hist) {
  recode(s, d, [&](uint32_t wa, int32_t digit) {
    const uint32_t w = wa - d.w0;  // local window (wraps to >= Wr below the range)
    if (w >= d.Wr) return;
    uint32_t code = DigitCode<T>::ZERO;
    if (digit != 0) {
      const uint32_t mag = (uint32_t)(digit < 0 ? -digit : digit) - 1u;
      // half windows at the range's ends: a bucket outside the kept half is another share's
      const uint32_t hb = 1u << (win_bits(d, wa) - 2);
      if (HALF && ((w == 0 && d.half_lo && mag < hb) || (w + 1 == d.Wr && d.half_hi && mag >= hb))) {
        digits[(size_t)(w0 + w) * d.n + i] = (T)code;
        return;
      }
      code = mag | (digit < 0 ? DigitCode<T>::SIGN : 0u);
      atomicAdd(&lds_hist[w * d.nbc + (mag >> win_fb(d, wa))], 1u);
    }
    digits[(size_t)(w0 + w) * d.n + i] = (T)code;
  });
}

// Pass 0+1 (fused), blockIdx.y = MSM of the batch: scalars from scalar_sets.p[y] (8 big-endian
// words each), digits into its windows [y Wr, (y+1) Wr).  The generic form (`recode`, through
// recode_carry) serves any geometry.
template <typename T>
__global__ void __launch_bounds__(RC_THREADS) k_recode_hist(BatchPtrs scalar_sets, MsmDims d,
                                                            T* __restrict__ digits, uint32_t* __restrict__ colsum) {
  extern __shared__ uint32_t lds_hist[];  // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  [[maybe_unused]] const uint32_t pwg = blockIdx.y * gridDim.x + blockIdx.x;
  PROBE(0, pwg, 0);
  recode_begin(lds_hist, d);
  PROBE(0, pwg, 1);
  // (loading all of a lane's scalars before recoding any measured slower: 43 vs 37 us per
  // two-MSM 2^20 launch)
  for (uint32_t i = lo + threadIdx.x; i < hi; i += RC_THREADS) {
    uint32_t s[8];
    load_scalar(scalars, i, s);
    recode_carry<T, true>(s, i, d, w0, digits, lds_hist);
  }
  __syncthreads();
  PROBE(0, pwg, 2);
  flush_hist(lds_hist, d, w0, colsum);
  PROBE(0, pwg, 7);
}

// The same with the geometry fixed at compile time (FixedGeo above) and 16-bit codes.  FULL: the
// launch covers every window (no range, no half windows), so nothing per window is uniform but
// the two fine-bit counts; else each window checks the range.  Row and histogram addresses advance
// by a stride per window kept in the range.
// (__launch_bounds__ with 8 waves per SIMD: two workgroups per CU need <= 80 SGPRs, which the
// unrolled windows' constants otherwise exceed -- one workgroup per CU took 37 against 31 us.)
template <uint32_t Q, uint32_t NHI, bool FULL>
__global__ void __launch_bounds__(RC_THREADS, 8) k_recode_fixed(BatchPtrs scalar_sets, MsmDims d,
                                                             uint16_t* __restrict__ digits,
                                                             uint32_t* __restrict__ colsum) {
  using G = FixedGeo<Q, NHI>;
  using DC = DigitCode<uint16_t>;
  static_assert(G::off(G::WMAIN) == MAIN_BITS, "main windows cover bits [0, 254)");
  constexpr typename G::Words C = G::bias();
  extern __shared__ uint32_t lds_hist[];  // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  const uint32_t nh = d.Wr * d.nbc;
  [[maybe_unused]] const uint32_t pwg = blockIdx.y * gridDim.x + blockIdx.x;
  PROBE(0, pwg, 0);
  for (uint32_t b = threadIdx.x; b < nh + d.Wr; b += RC_THREADS) lds_hist[b] = 0;  // + the window totals
  // fine bits of the wide (Q + 1) windows, the narrow (Q) ones and the overflow window (win_fb)
  const uint32_t fb_w = d.fb - (d.c - (NHI ? Q + 1 : Q));
  const uint32_t fb_n = d.fb > d.c - Q ? d.fb - (d.c - Q) : 0u;
  const uint32_t fb_o = d.fb > d.c - OVF_BITS ? d.fb - (d.c - OVF_BITS) : 0u;
  const uint32_t wlo = d.w0, whi = d.w0 + d.Wr;
  __syncthreads();
  PROBE(0, pwg, 1);
  // Each lane recodes two adjacent scalars: their loads are one 64-B run, and a window's two
  // codes go out as one 4-B store (when n is even, so that every row stays 4-B aligned).
  const bool pair_store = (d.n & 1u) == 0;
  for (uint32_t i = lo + 2 * threadIdx.x; i < hi; i += 2 * RC_THREADS) {
    const bool two = i + 1 < hi;
    uint32_t t0[8], t1[8], cy0 = 0, cy1 = 0;
    {
      uint32_t s0[8], s1[8];
      load_scalar(scalars, i, s0);
      if (two)
        load_scalar(scalars, i + 1, s1);
      else
#pragma unroll
        for (int k = 0; k < 8; k++) s1[k] = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint64_t x0 = (uint64_t)s0[k] + C.v[k] + cy0;
        const uint64_t x1 = (uint64_t)s1[k] + C.v[k] + cy1;
        t0[k] = (uint32_t)x0;
        t1[k] = (uint32_t)x1;
        cy0 = (uint32_t)(x0 >> 32);
        cy1 = (uint32_t)(x1 >> 32);
      }
    }
    uint16_t* row = digits + (size_t)w0 * d.n + i;
    uint32_t* h = lds_hist;
#pragma unroll
    for (uint32_t wa = 0; wa <= G::WMAIN; wa++) {
      if (!FULL && (wa < wlo || wa >= whi)) continue;
      int32_t dg[2];
      uint32_t fbits, hb;
      if (wa < G::WMAIN) {
        const uint32_t o = G::off(wa), b = G::bits(wa), k = o / 32, sh = o % 32;
        const uint32_t x0 = (sh + b <= 32 ? t0[k] >> sh : __builtin_amdgcn_alignbit(t0[k + 1], t0[k], sh)) & ((1u << b) - 1u);
        const uint32_t x1 = (sh + b <= 32 ? t1[k] >> sh : __builtin_amdgcn_alignbit(t1[k + 1], t1[k], sh)) & ((1u << b) - 1u);
        dg[0] = (int32_t)x0 - (int32_t)((1u << (b - 1)) - 1u);
        dg[1] = (int32_t)x1 - (int32_t)((1u << (b - 1)) - 1u);
        fbits = b == Q + 1 ? fb_w : fb_n;
        hb = 1u << (b - 2);
      } else {
        dg[0] = (int32_t)((t0[7] >> 30) | (cy0 << 2));
        dg[1] = (int32_t)((t1[7] >> 30) | (cy1 << 2));
        fbits = fb_o;
        hb = 1u << (OVF_BITS - 2);
      }
      uint32_t code[2];
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const int32_t digit = dg[q];
        const uint32_t mag = (uint32_t)(digit < 0 ? -digit : digit) - 1u;
        bool live = digit != 0 && (q == 0 || two);
        if (!FULL) {
          // half windows at the range's ends: a bucket outside the kept half is another share's
          if (wa == wlo && d.half_lo) live = live && mag >= hb;
          if (wa + 1 == whi && d.half_hi) live = live && mag < hb;
        }
        // every lane adds (0 for a zero digit): no divergent branch around the LDS atomic
        atomicAdd(&h[live ? mag >> fbits : 0u], live ? 1u : 0u);
        code[q] = live ? mag | (digit < 0 ? DC::SIGN : 0u) : DC::ZERO;
      }
      if (pair_store && two) {
        *reinterpret_cast<uint32_t*>(row) = code[0] | code[1] << 16;
      } else {
        row[0] = (uint16_t)code[0];
        if (two) row[1] = (uint16_t)code[1];
      }
      row += d.n;
      h += d.nbc;
    }
  }
  __syncthreads();
  PROBE(0, pwg, 2);
  flush_hist(lds_hist, d, w0, colsum);
  PROBE(0, pwg, 7);
}

// A lane's run of LW adjacent words at p.  `vec`: as 16-B vector loads (8-B where LW is no multiple of
// 4; a single word is one load either way) -- the caller vouches for the run's alignment; else word by
// word, the first nw of them, zeros after.
template <uint32_t LW>
__device__ __forceinline__ void load_words(uint32_t (&raw)[LW], const uint32_t* p, bool vec, uint32_t nw) {
  if (vec && LW % 4 == 0) {
#pragma unroll
    for (uint32_t k = 0; k < LW / 4; k++) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[k];
      raw[4 * k] = v.x, raw[4 * k + 1] = v.y, raw[4 * k + 2] = v.z, raw[4 * k + 3] = v.w;
    }
  } else if (vec && LW % 2 == 0) {
#pragma unroll
    for (uint32_t k = 0; k < LW / 2; k++) {
      const uint2 v = reinterpret_cast<const uint2*>(p)[k];
      raw[2 * k] = v.x, raw[2 * k + 1] = v.y;
    }
  } else {
#pragma unroll
    // (from the top word down: in ascending order the compiler shares the first words' loads between
    // the two paths and cuts the vector loads into words and 12-B pieces to do so)
    for (uint32_t k = LW; k-- > 0;) raw[k] = k < nw ? p[k] : 0u;
  }
}

// The biased recodes -- k_recode_narrow, k_recode_native, k_recode_wide -- are the bias-add form of
// k_recode_fixed with the geometry at run time: the launch's own balanced windows [0, d.Wr) of q + 1 /
// q bits that sum to T = max(sbits + 1, 4) bits, no overflow window.  Each kernel loads its format and
// forms magnitudes of SW little-endian words below 2^sbits -- bits at or above sbits are masked off
// and reported (MSM_DEV_ERR_SCALAR_RANGE in the slot's err word), so the digits stay inside their
// windows and the launch runs to its end -- and a sign; the two helpers below do the rest.
//
// t = m + C (C from the host, NarrowBias) makes the windows independent, and since the widths sum to
// more than sbits the top window's top bit is clear before the add, so t < 2^T and nothing carries
// out.  t is SW + 1 words (T may be 32 SW + 1).
template <uint32_t SW>
__device__ __forceinline__ void bias_add(const uint32_t (&m)[SW], const NarrowBias& bias, uint32_t (&t)[SW + 1]) {
  uint32_t cy = 0;
#pragma unroll
  for (uint32_t k = 0; k < SW; k++) {
    const uint64_t x = (uint64_t)m[k] + bias.v[k] + cy;
    t[k] = (uint32_t)x;
    cy = (uint32_t)(x >> 32);
  }
  t[SW] = cy;
}
// The windows of CH adjacent scalars, the first `cnt` of them live (cnt >= 1; more than CH is CH): t is
// shifted down one window at a time -- SW funnel shifts by a uniform amount per window, which is what
// a run-time geometry costs without indexing the register array dynamically (see `recode`).  The
// histogram counts by magnitude; the scalar's sign is one XOR into the digit's: code sign =
// (digit < 0) != neg[r].  `row` is the scalars' place in the launch's first window; 16-bit codes go out
// in pairs as k_recode_fixed's do.
template <typename T, uint32_t SW, uint32_t CH>
__device__ __forceinline__ void recode_windows(uint32_t (&t)[CH][SW + 1], const bool (&neg)[CH], uint32_t cnt,
                                               T* __restrict__ row, uint32_t* h, const MsmDims& d) {
  using DC = DigitCode<T>;
  static_assert(CH % 2 == 0, "codes are stored two at a time");
  const bool pair_store = sizeof(T) == 2 && (d.n & 1u) == 0;  // every row stays 4-B aligned
  for (uint32_t w = 0; w < d.Wr; w++) {
    const uint32_t b = w < d.nhi ? d.q + 1 : d.q;
    const uint32_t mask = (1u << b) - 1u, hb = (1u << (b - 1)) - 1u;
    const uint32_t fbits = d.fb > d.c - b ? d.fb - (d.c - b) : 0u;  // win_fb
    uint32_t code[CH];
#pragma unroll
    for (uint32_t r = 0; r < CH; r++) {
      const int32_t digit = (int32_t)(t[r][0] & mask) - (int32_t)hb;
#pragma unroll
      for (uint32_t k = 0; k < SW; k++) t[r][k] = __builtin_amdgcn_alignbit(t[r][k + 1], t[r][k], b);
      t[r][SW] >>= b;
      const uint32_t mag = (uint32_t)(digit < 0 ? -digit : digit) - 1u;
      const bool live = digit != 0 && r < cnt;
      // every lane adds (0 for a zero digit): no divergent branch around the LDS atomic
      atomicAdd(&h[live ? mag >> fbits : 0u], live ? 1u : 0u);
      code[r] = live ? mag | ((digit < 0) != neg[r] ? DC::SIGN : 0u) : DC::ZERO;
    }
#pragma unroll
    for (uint32_t r = 0; r < CH; r += 2) {
      if (pair_store && r + 1 < cnt) {
        *reinterpret_cast<uint32_t*>(row + r) = code[r] | code[r + 1] << 16;
      } else {
        if (r < cnt) row[r] = (T)code[r];
        if (r + 1 < cnt) row[r + 1] = (T)code[r + 1];
      }
    }
    row += d.n;
    h += d.nbc;
  }
}

// Narrow scalars (MsmDims::sw words of MsmDims::sbits bits each, big-endian words like the 8-word
// format; no sign).  A lane takes R adjacent scalars (16 or 32 B at one or two words each, so a wave's
// loads are whole cache lines; two scalars at three words and more) as vector loads where the MSM's
// scalar pointer is 16-B aligned.  Only the most significant word can hold bits at or above sbits.
template <typename T, uint32_t SW>
__global__ void __launch_bounds__(RC_THREADS) k_recode_narrow(BatchPtrs scalar_sets, MsmDims d,
                                                              T* __restrict__ digits, uint32_t* __restrict__ colsum,
                                                              NarrowBias bias, uint32_t* __restrict__ err) {
  constexpr uint32_t R = SW <= 2 ? 4 : 2;  // scalars per lane
  constexpr uint32_t LW = R * SW;          // words per lane
  extern __shared__ uint32_t lds_hist[];   // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  // value bits of the most significant word
  const uint32_t top_mask = (d.sbits & 31u) ? (1u << (d.sbits & 31u)) - 1u : 0xffffffffu;
  const bool vec = (reinterpret_cast<uintptr_t>(scalars) & 15u) == 0;
  const bool neg[R] = {};
  bool bad = false;
  recode_begin(lds_hist, d);
  for (uint32_t i = lo + R * threadIdx.x; i < hi; i += R * RC_THREADS) {
    const uint32_t cnt = min(R, hi - i);
    uint32_t raw[LW];
    load_words(raw, scalars + (size_t)i * SW, cnt == R && vec, cnt * SW);
    uint32_t t[R][SW + 1];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
      bad = bad || (raw[r * SW] & ~top_mask) != 0;
      raw[r * SW] &= top_mask;
      uint32_t m[SW];
#pragma unroll
      for (uint32_t k = 0; k < SW; k++) m[k] = raw[r * SW + SW - 1 - k];  // raw[r SW] is the most significant
      bias_add(m, bias, t[r]);
    }
    recode_windows<T, SW, R>(t, neg, cnt, digits + (size_t)w0 * d.n + i, lds_hist, d);
  }
  recode_end(lds_hist, d, w0, colsum, bad, err);
}

// Native integer scalars (msm_opts_typed, MSM_FLAG_SCALAR_TYPE): the vector is the caller's own array
// of E-bit elements -- E = 1: bit (i & 7) of byte (i >> 3); 8 / 16 / 32 / 64: little-endian integers,
// two's complement when SIGNED -- of d.sbits = b <= E magnitude bits.  The magnitude |v| is SW words
// (SW = 2 at 64 bits, else 1), formed in unsigned arithmetic so that -2^(E-1) is 2^(E-1).
// A lane takes one 32-bit word of bit / 8 / 16-bit elements (32 / 4 / 2 scalars) or 16 B of 32 /
// 64-bit ones (4 / 2 scalars; word by word where the vector is only 4-B aligned), so a wave reads
// whole cache lines, and recodes them four at a time.  The lanes that hold the tail of the workgroup's
// span or of the vector read element by element: nothing past byte ceil(n E / 8) is touched.
template <uint32_t E>
__device__ __forceinline__ uint64_t native_elem(const uint32_t* __restrict__ scalars, uint32_t i) {
  if (E == 1) return (reinterpret_cast<const uint8_t*>(scalars)[i >> 3] >> (i & 7u)) & 1u;
  if (E == 8) return reinterpret_cast<const uint8_t*>(scalars)[i];
  if (E == 16) return reinterpret_cast<const uint16_t*>(scalars)[i];
  if (E == 32) return scalars[i];
  return (uint64_t)scalars[2 * (size_t)i] | (uint64_t)scalars[2 * (size_t)i + 1] << 32;
}
template <typename T, uint32_t E, bool SIGNED>
__global__ void __launch_bounds__(RC_THREADS) k_recode_native(BatchPtrs scalar_sets, MsmDims d,
                                                              T* __restrict__ digits, uint32_t* __restrict__ colsum,
                                                              NarrowBias bias, uint32_t* __restrict__ err) {
  constexpr uint32_t SW = E == 64 ? 2 : 1;                     // words of a magnitude
  constexpr uint32_t R = E <= 16 ? 32 / E : E == 32 ? 4 : 2;   // scalars per lane
  constexpr uint32_t LW = E <= 16 ? 1 : 4;                     // words per lane
  constexpr uint32_t CH = R < 4 ? R : 4;                       // scalars recoded together
  static_assert(E == 1 || E == 8 || E == 16 || E == 32 || E == 64, "element bits");
  static_assert(!(SIGNED && E == 1), "a bit has no sign");
  extern __shared__ uint32_t lds_hist[];  // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  const uint64_t mag_mask = d.sbits >= 64 ? ~0ull : (1ull << d.sbits) - 1ull;
  const bool vec = (reinterpret_cast<uintptr_t>(scalars) & 15u) == 0;
  bool bad = false;
  recode_begin(lds_hist, d);
  for (uint32_t i = lo + R * threadIdx.x; i < hi; i += R * RC_THREADS) {
    const uint32_t cnt = min(R, hi - i);
    uint32_t raw[LW] = {};
    // (i is a multiple of R: a whole lane's words start at word i E / 32)
    if (cnt == R) load_words(raw, scalars + ((size_t)i * E >> 5), vec, LW);
    for (uint32_t g = 0; g < R; g += CH) {
      if (g >= cnt) break;
      uint32_t t[CH][SW + 1];
      bool neg[CH];
#pragma unroll
      for (uint32_t r = 0; r < CH; r++) {
        uint64_t v;
        if (cnt != R) {
          v = g + r < cnt ? native_elem<E>(scalars, i + g + r) : 0ull;
        } else if constexpr (E == 64) {
          v = (uint64_t)raw[2 * r] | (uint64_t)raw[2 * r + 1] << 32;
        } else if constexpr (E == 32) {
          v = raw[r];
        } else {
          v = (raw[0] >> ((g + r) * E)) & (0xffffffffu >> (32 - E));
        }
        // the magnitude, in E-bit unsigned arithmetic
        neg[r] = SIGNED && ((v >> (E - 1)) & 1u);
        if (neg[r]) v = (0ull - v) & (~0ull >> (64 - E));
        bad = bad || (v & ~mag_mask) != 0;
        v &= mag_mask;
        uint32_t m[SW];
#pragma unroll
        for (uint32_t k = 0; k < SW; k++) m[k] = (uint32_t)(v >> (32 * k));
        bias_add(m, bias, t[r]);
      }
      recode_windows<T, SW, CH>(t, neg, cnt - g, digits + (size_t)w0 * d.n + i + g, lds_hist, d);
    }
  }
  recode_end(lds_hist, d, w0, colsum, bad, err);
}

// Wide scalars (msm_opts_typed.scalar_field, MSM_FLAG_SCALAR_FIELD): elements of SW = 4 or 8 LITTLE-endian
// words -- u128 / i128, u256 (arkworks BigInt<4>) and Fr in Montgomery form -- of d.sbits = b <= 253
// magnitude bits.  Word 0 is the least significant; WIDE_I takes the magnitude and sign as
// k_recode_native does (|v| in 128-bit unsigned arithmetic, so -2^127 is 2^127), and WIDE_MONT runs
// fr_from_mont (fr.cuh: v = a 2^-256 mod r, 8 rounds of word REDC) ahead of the bias-add, with a >= r
// reported.  A lane takes R = 2 adjacent scalars, 32 or 64 B, as 16-B vector loads where the vector is
// 16-B aligned and word by word where it is only 4-B aligned; the lane that holds the odd tail of the
// span reads only its own scalar's words, so nothing past byte n SW 4 is touched.
// REDC's output is below r whatever a was, and is masked like the rest.
constexpr uint32_t WIDE_U = 0, WIDE_I = 1, WIDE_MONT = 2;
template <typename T, uint32_t SW, uint32_t MODE>
__global__ void __launch_bounds__(RC_THREADS) k_recode_wide(BatchPtrs scalar_sets, MsmDims d,
                                                            T* __restrict__ digits, uint32_t* __restrict__ colsum,
                                                            NarrowBias bias, uint32_t* __restrict__ err) {
  constexpr uint32_t R = 2;        // scalars per lane
  constexpr uint32_t LW = R * SW;  // words per lane
  static_assert(SW == 4 || SW == 8, "128- or 256-bit elements");
  static_assert(MODE == WIDE_U || (MODE == WIDE_I && SW == 4) || (MODE == WIDE_MONT && SW == 8), "element kinds");
  extern __shared__ uint32_t lds_hist[];  // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  // value bits of every word (little-endian): all of it below b, none of it at and above
  uint32_t wmask[SW];
#pragma unroll
  for (uint32_t k = 0; k < SW; k++)
    wmask[k] = d.sbits >= 32 * k + 32 ? 0xffffffffu : d.sbits > 32 * k ? (1u << (d.sbits - 32 * k)) - 1u : 0u;
  const bool vec = (reinterpret_cast<uintptr_t>(scalars) & 15u) == 0;
  bool bad = false;
  recode_begin(lds_hist, d);
  for (uint32_t i = lo + R * threadIdx.x; i < hi; i += R * RC_THREADS) {
    const uint32_t cnt = min(R, hi - i);
    uint32_t raw[LW];
    // (i is even and an element 16 or 32 B: a whole lane's run is 16-B aligned)
    load_words(raw, scalars + (size_t)i * SW, cnt == R && vec, cnt * SW);
    uint32_t t[R][SW + 1];
    bool neg[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
      uint32_t m[SW];  // the magnitude, little-endian words
#pragma unroll
      for (uint32_t k = 0; k < SW; k++) m[k] = raw[r * SW + k];
      neg[r] = MODE == WIDE_I && (m[SW - 1] >> 31) != 0;
      if (MODE == WIDE_I) {  // |v| = ~v + 1 in SW-word unsigned arithmetic
        uint32_t cy = 1;
#pragma unroll
        for (uint32_t k = 0; k < SW; k++) {
          const uint64_t x = (uint64_t)(~m[k]) + cy;
          m[k] = neg[r] ? (uint32_t)x : m[k];
          cy = (uint32_t)(x >> 32);
        }
      }
      if constexpr (MODE == WIDE_MONT) {
        bad = bad || !fr_is_canonical(m);
        fr_from_mont(m, m);
      }
#pragma unroll
      for (uint32_t k = 0; k < SW; k++) {
        bad = bad || (m[k] & ~wmask[k]) != 0;
        m[k] &= wmask[k];
      }
      bias_add(m, bias, t[r]);
    }
    recode_windows<T, SW, R>(t, neg, cnt, digits + (size_t)w0 * d.n + i, lds_hist, d);
  }
  recode_end(lds_hist, d, w0, colsum, bad, err);
}

// MSM_FIELD_U256 of 254..256 bits: k_recode_hist on little-endian words -- the full-width geometry,
// overflow window included, on the caller's BigInt<4> array (the launch covers every window: w0 = 0,
// no half windows).  A kernel of its own, so that the 8-word launches keep theirs as they are.  16-B
// vector loads where the vector is 16-B aligned, else word by word.
template <typename T>
__global__ void __launch_bounds__(RC_THREADS) k_recode_hist_le(BatchPtrs scalar_sets, MsmDims d,
                                                               T* __restrict__ digits, uint32_t* __restrict__ colsum) {
  extern __shared__ uint32_t lds_hist[];  // [Wr][nbc]
  const uint32_t* __restrict__ scalars = scalar_sets.p[blockIdx.y];
  const uint32_t lo = blockIdx.x * RC_SPAN, hi = min(d.n, lo + RC_SPAN);
  const uint32_t w0 = blockIdx.y * d.Wr;
  const bool vec = (reinterpret_cast<uintptr_t>(scalars) & 15u) == 0;
  recode_begin(lds_hist, d);
  for (uint32_t i = lo + threadIdx.x; i < hi; i += RC_THREADS) {
    uint32_t s[8];
    load_words(s, scalars + (size_t)i * 8, vec, 8);
    recode_carry<T, false>(s, i, d, w0, digits, lds_hist);
  }
  recode_end(lds_hist, d, w0, colsum);
}

// k_fine_sort geometry
#ifndef MSM_FS_THREADS
#define MSM_FS_THREADS 512
#endif
// Bins staged in LDS: up to FS_CAP entries.  A bin averages ~4K entries, but the top window of
// scalars reduced mod r (< 0.58 * 2^253, as any prover's are) fills only 58% of its buckets, so
// its bins hold ~7K: 8,192 keeps them on the staged path (at 6,144 they took the unstaged one and
// were the kernel's stragglers, ~25 us each).
#ifndef MSM_FS_CAP
#define MSM_FS_CAP 8192
#endif
constexpr uint32_t FS_THREADS = MSM_FS_THREADS;
constexpr uint32_t FS_R = MSM_FS_CAP / FS_THREADS;
constexpr uint32_t FS_CAP = FS_THREADS * FS_R;  // (512 threads: -12% vs 256 at 6,144, measured)
constexpr uint32_t FS_MAXF = 2048;

// Pass 2: each (window, chunk) workgroup moves its digits into its own contiguous slice of every
// coarse bin.  The chunk is counting-sorted by bin inside LDS -- the LDS atomic that counts an
// entry also returns its rank inside its bin, so every entry is placed without a second atomic
// -- and each bin's slice is reserved with one global atomic on the bin's cursor (bin_cur, counted
// from zero; the slices' order inside a bin is immaterial: the bucket sums commute).  The
// staged chunk is then streamed out so that consecutive lanes write consecutive addresses of a
// slice (>= 64 entries per slice by construction of ch).  (Writing each entry straight from
// registers to its slice, with no LDS staging, measured 59 -> 153 us per two-MSM 2^20 launch; the
// same in k_fine_sort 96 -> 168 us.)
//
// Staging keeps 4 B per entry for 16-bit codes: code << PS_POS | position in the chunk (ch = 2^PS_POS),
// 64 KiB, so two workgroups share a CU; 32-bit codes (c > 16) stage (code, position) pairs.
constexpr uint32_t PS_POS = __builtin_ctz(PT_THREADS * PS_R);  // bits of a position in a chunk
template <typename T>
struct PartStage;
template <>
struct PartStage<uint16_t> {
  using V = uint32_t;
  static __device__ __forceinline__ V pack(uint32_t code, uint32_t li) { return code << PS_POS | li; }
  static __device__ __forceinline__ uint32_t code(V v) { return v >> PS_POS; }
  static __device__ __forceinline__ uint32_t pos(V v) { return v & ((1u << PS_POS) - 1u); }
};
template <>
struct PartStage<uint32_t> {
  using V = uint2;
  static __device__ __forceinline__ V pack(uint32_t code, uint32_t li) { return make_uint2(code, li); }
  static __device__ __forceinline__ uint32_t code(V v) { return v.x; }
  static __device__ __forceinline__ uint32_t pos(V v) { return v.y; }
};
static_assert(PT_THREADS * PS_R == (1u << PS_POS) && PS_POS <= 16, "PartStage<uint16_t> packs code and position in 32 bits");

//
// Which point record a position of the launch takes is the one thing a subset launch on a handle's
// records changes (MsmDims::sub): SUB is a compile-time variant, and MSM_SUB_NONE -- every launch
// but msm_bases_compute_subset*'s -- compiles to the plain `pbase + position`.
template <uint32_t SUB>
__device__ __forceinline__ uint32_t part_record(const MsmDims& d, uint32_t pbase, uint32_t p,
                                                const uint32_t* __restrict__ idx) {
  if constexpr (SUB == MSM_SUB_NONE) {
    return pbase + p;
  } else {
    // level j = p / sm by at most 7 compares against wave-uniform thresholds (levels <= 8; a
    // threshold past the launch's positions never fires), term i = p - j sm
    uint32_t i = p, base = 0;
#pragma unroll
    for (uint32_t k = 1; k < 8; k++) {
      const uint64_t t64 = (uint64_t)k * d.sm;
      const uint32_t t = t64 > 0xffffffffull ? 0xffffffffu : (uint32_t)t64;
      const bool up = p >= t;
      i -= up ? d.sm : 0u;
      base += up ? d.rstride : 0u;
    }
    // the indexed form gathers where the entry word is written: the workgroup's positions stay inside
    // one chunk-long span of the staged vector (L2-resident)
    return base + (SUB == MSM_SUB_RANGE ? d.first + i : idx[i]);
  }
}

__device__ __forceinline__ const uint32_t* part_sub_idx() { return nullptr; }
__device__ __forceinline__ const uint32_t* part_sub_idx(const uint32_t* p) { return p; }

// The subset variants take one more argument, the slot's staged index buffer [nm][sm]
// (k_stage_indices, or the host entries' upload; unread by the range form): IDX is that argument's
// type, and empty for the plain kernel, whose argument list and code are what they were before the
// variants existed.
template <typename T, uint32_t SUB = MSM_SUB_NONE, typename... IDX>
__global__ void __launch_bounds__(PT_THREADS) k_part_scatter(const T* __restrict__ digits, MsmDims d,
                                                             uint32_t* __restrict__ colsum,
                                                             uint32_t* __restrict__ bin_cur,
                                                             uint32_t* __restrict__ bin_base,
                                                             uint32_t* __restrict__ part_entry,
                                                             uint16_t* __restrict__ part_fine, IDX... sub_idx) {
  static_assert(sizeof...(IDX) == (SUB == MSM_SUB_NONE ? 0 : 1), "the subset variants take the index buffer");
  using S = PartStage<T>;
  __shared__ typename S::V st[PT_THREADS * PS_R];
  __shared__ uint32_t m_live;
  __shared__ uint32_t wpart[PT_THREADS / 64];
  // [nbc] count -> local start, [nbc] global slice start - local start, [nbc] bin start in window
  extern __shared__ uint4 dyn4[];
  uint32_t* lcnt = reinterpret_cast<uint32_t*>(dyn4);
  uint32_t* gdel = lcnt + d.nbc;
  uint32_t* bscan = gdel + d.nbc;
  const uint32_t w = blockIdx.y, ck = blockIdx.x;
  const uint32_t fbw = batch_win_fb(d, w);
  const uint32_t pbase = d.shared ? 0u : (w / d.Wr) * d.n;  // first point record of this window's MSM
  const T* dw = digits + (size_t)w * d.n;
  const uint32_t lo = ck * d.ch, hi = min(d.n, lo + d.ch);
  [[maybe_unused]] const uint32_t pwg = blockIdx.y * gridDim.x + blockIdx.x;
  PROBE(1, pwg, 0);
  // 16-bit codes carry their rank in the bin in their upper half (one register per digit: the
  // workgroup stays within 64 VGPRs, two per CU); 32-bit codes keep it apart
  constexpr bool PACK = sizeof(T) == 2;
  uint32_t code[PS_R], rank[PACK ? 1 : PS_R];
#pragma unroll
  for (uint32_t r = 0; r < PS_R; r++) {
    const uint32_t i = lo + r * PT_THREADS + threadIdx.x;
    code[r] = i < hi ? (uint32_t)dw[i] : DigitCode<T>::ZERO;
  }
  // Beside the digit loads: the window's bin totals (scanned below into the bins' starts inside
  // the window) and the sum of the lower windows' totals (the window's first slot) -- what a
  // separate one-workgroup scan kernel computed before (k_bin_scan, ~10 us per launch).
  // nbc <= 256 <= PT_THREADS (make_plan): one bin per thread.
  const bool bin_lane = threadIdx.x < d.nbc;
  const uint32_t tot_b = bin_lane ? colsum[w * d.nbc + threadIdx.x] : 0u;
  const uint32_t* wtot = colsum + d.nbins;
  uint32_t lower = 0;
  for (uint32_t v = threadIdx.x; v < w; v += PT_THREADS) lower += wtot[v];
  lower = wave_incl_scan(lower);
  if ((threadIdx.x & 63) == 63) wpart[threadIdx.x >> 6] = lower;
  if (bin_lane) {
    lcnt[threadIdx.x] = 0;
    bscan[threadIdx.x] = tot_b;
  }
  PROBE_WAIT_VM();
  PROBE(1, pwg, 1);
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < PS_R; r++) {
    if (code[r] != DigitCode<T>::ZERO) {
      const uint32_t rk = atomicAdd(&lcnt[(code[r] & DigitCode<T>::MAG) >> fbw], 1u);
      if constexpr (PACK)
        code[r] |= rk << 16;
      else
        rank[r] = rk;
    }
  }
  lds_excl_scan_wave0(bscan, d.nbc);
  __syncthreads();
  PROBE(1, pwg, 2);
  // each bin's slice is reserved with one global atomic on the bin's cursor (zero-based; its
  // latency overlaps the local scan)
  const uint32_t cb = bin_lane ? lcnt[threadIdx.x] : 0u;
  const uint32_t g = cb ? atomicAdd(&bin_cur[w * d.nbc + threadIdx.x], cb) : 0u;
  if (threadIdx.x == d.nbc - 1) m_live = cb;
  uint32_t wbase = 0;
#pragma unroll
  for (uint32_t k = 0; k < PT_THREADS / 64; k++) wbase += wpart[k];
  __syncthreads();
  PROBE(1, pwg, 3);
  lds_excl_scan_wave0(lcnt, d.nbc);
  __syncthreads();
  PROBE(1, pwg, 4);
  if (bin_lane) {
    const uint32_t start = wbase + bscan[threadIdx.x];  // the bin's first slot in the sorted order
    gdel[threadIdx.x] = start + g - lcnt[threadIdx.x];  // entry j of bin b goes to j + gdel[b]
    if (ck == 0) {
      bin_base[w * d.nbc + threadIdx.x] = start;
      if (w + 1 == d.W && threadIdx.x == d.nbc - 1) bin_base[d.nbins] = start + tot_b;
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < PS_R; r++) {
    const uint32_t cd = PACK ? code[r] & 0xffffu : code[r];
    if (cd != DigitCode<T>::ZERO)
      st[lcnt[(cd & DigitCode<T>::MAG) >> fbw] + (PACK ? code[r] >> 16 : rank[PACK ? 0 : r])] =
          S::pack(cd, r * PT_THREADS + threadIdx.x);
  }
  __syncthreads();
  PROBE(1, pwg, 5);
  const uint32_t m = lcnt[d.nbc - 1] + m_live;  // live digits of the chunk
  const uint32_t fmask = (1u << fbw) - 1u;
  // the staged index vector of this window's MSM (indexed subsets only)
  [[maybe_unused]] const uint32_t* idx = nullptr;
  if constexpr (SUB == MSM_SUB_INDEXED) idx = part_sub_idx(sub_idx...) + (size_t)(w / d.Wr) * d.sm;
  for (uint32_t j = threadIdx.x; j < m; j += PT_THREADS) {
    const typename S::V v = st[j];
    const uint32_t cd = S::code(v);
    const uint32_t b = cd & DigitCode<T>::MAG;
    const uint32_t fine = b & fmask;
    const uint32_t ent = (part_record<SUB>(d, pbase, lo + S::pos(v), idx) << 1) | (cd >> DigitCode<T>::SHIFT);
    const uint32_t dst = j + gdel[b >> fbw];
    // packed: the fine key in the low d.fb bits (a narrower window's fbw <= d.fb of them used)
    part_entry[dst] = d.packed ? (ent << d.fb) | fine : ent;
    if (!d.packed) part_fine[dst] = (uint16_t)fine;
  }
  PROBE(1, pwg, 6);
  PROBE(1, pwg, 7);
}

// The caller's base indices of a device-entry subset launch into the slot's buffer: out[z][i] =
// idx_sets.p[z][i] for the launch's nm MSMs (blockIdx.y = z) of m indices each.  An index >= n (the
// handle's points) is replaced by 0 -- it must never reach the record gather -- and raises
// MSM_DEV_ERR_BAD_INDEX in the slot's err word, which the reduction reports with the terms and
// clears, as it does the preparation's bits: the launch runs to its end and the entry then fails.
extern "C" __global__ void __launch_bounds__(256) k_stage_indices(BatchPtrs idx_sets, uint32_t* __restrict__ out,
                                                                    uint32_t m, uint32_t n,
                                                                    uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  uint32_t v = idx_sets.p[blockIdx.y][i];
  if (v >= n) {
    v = 0;
    atomicOr(err, MSM_DEV_ERR_BAD_INDEX);
  }
  out[(size_t)blockIdx.y * m + i] = v;
}

// Pass 3: one workgroup per coarse bin, counting sort by fine bucket (<= FS_MAXF per bin).  A bin
// of at most FS_CAP entries is sorted inside LDS and streamed out coalesced.  Besides the sorted
// entry list it writes the bucket boundaries the accumulation walks: bucket_start[key] (global
// position of bucket `key`'s first entry; bucket_start[W*B] = bucket_start[W*B+1] = total) and
// run_key[r] = the bucket holding position r*K (the first entry of accumulation run r).  A window
// narrower than the widest has fewer buckets than B (win_fb): the bins' workgroups also set its
// keys past them, each a share, to the window's end.
//
// A bigger bin (skewed scalars: one giant bucket, or few distinct digits) is sorted by its own
// workgroup in register tiles: a counting pass that collapses runs of equal keys per lane before
// touching LDS (a bin that is one giant bucket costs one atomic per lane, not per entry), then a
// placement pass in which the lanes of a wave holding the same key find each other by ballots over
// the key's bits and their leader reserves all their slots with one atomic -- so equal keys never
// serialise on one LDS address, and they are written coalesced.  (This replaced k_big_place, a
// tile-parallel kernel of its own that cost a launch, ~5 us, on every MSM for the skewed inputs'
// sake.)

// One coarse-binned entry: its fine key (bucket within the bin) and the sorted-list entry
// (idx << 1 | sign), from the packed word or the two arrays (MsmDims::packed).
__device__ __forceinline__ void part_load(const uint32_t* __restrict__ pe, const uint16_t* __restrict__ pf,
                                          const MsmDims& d, uint32_t i, uint32_t& fine, uint32_t& entry) {
  const uint32_t v = pe[i];
  if (d.packed) {
    fine = v & ((1u << d.fb) - 1u);
    entry = v >> d.fb;
  } else {
    fine = pf[i];
    entry = v;
  }
}

// floor(x / D) for a runtime, wave-uniform D, given inv = 1.0 / D: (x + 0.5) / D is at least
// 0.5 / D away from an integer, and the two roundings (inv, the product) err by < 2^-20 / D for any
// 32-bit x, so the truncation is exact.  Three VALU against the ~14 of an unsigned division.
__device__ __forceinline__ uint32_t div_by_inv(uint32_t x, double inv) {
  return (uint32_t)(((double)x + 0.5) * inv);
}

__device__ __forceinline__ void count_runs(uint32_t* cnt, uint32_t& last, uint32_t& run, uint32_t key) {
  if (key == last) {
    run++;
  } else {
    if (run) atomicAdd(&cnt[last], run);
    last = key;
    run = 1;
  }
}

// Lanes of the wave whose `key` (fbits bits) equals this lane's, among the lanes in `live`.
__device__ __forceinline__ uint64_t key_peers(uint32_t key, uint32_t fbits, uint64_t live) {
  uint64_t peers = live;
  for (uint32_t b = 0; b < fbits; b++) {
    const uint64_t set = __ballot((key >> b) & 1u);
    peers &= ((key >> b) & 1u) ? set : ~set;
  }
  return peers;
}

// MSM_FS_MINW: minimum waves per SIMD asked of the compiler.  8 = four workgroups per CU (<= 64
// VGPRs, a few spilled in the unstaged path): 57 against 63 us per two-MSM 2^20 launch at 76 VGPRs
// (three workgroups per CU).
#ifndef MSM_FS_MINW
#define MSM_FS_MINW 8
#endif
#if MSM_FS_MINW > 0
#define FS_BOUNDS __launch_bounds__(FS_THREADS, MSM_FS_MINW)
#else
#define FS_BOUNDS __launch_bounds__(FS_THREADS)
#endif
extern "C" __global__ void FS_BOUNDS k_fine_sort(const uint32_t* __restrict__ part_entry,
                                                                     const uint16_t* __restrict__ part_fine,
                                                                     const uint32_t* __restrict__ bin_base, MsmDims d,
                                                                     uint32_t K, uint32_t* __restrict__ sorted_entry,
                                                                     uint32_t* __restrict__ bucket_start,
                                                                     uint32_t* __restrict__ run_key,
                                                                     uint32_t* __restrict__ colsum,
                                                                     uint32_t* __restrict__ bin_cur) {
  __shared__ __attribute__((aligned(16))) uint32_t cnt[FS_MAXF];
  __shared__ uint32_t st_entry[FS_CAP];
  const uint32_t bin = blockIdx.x;
  PROBE(2, bin, 0);
  const uint32_t w = bin / d.nbc, cb = bin % d.nbc;
  const uint32_t fbw = batch_win_fb(d, w);
  const uint32_t nf = 1u << fbw;
  const uint32_t base = bin_base[bin];
  const uint32_t m = bin_base[bin + 1] - base;
  const uint32_t key0 = w * d.B + (cb << fbw);
  for (uint32_t f = threadIdx.x; f < nf; f += FS_THREADS) cnt[f] = 0;
  if (threadIdx.x == 0) {
    // the bin's total, cursor and window total are consumed (k_part_scatter): zero for the next MSM
    colsum[bin] = 0;
    bin_cur[bin] = 0;
    if (cb == 0) colsum[d.nbins + w] = 0;
  }
  if (bin + 1 == gridDim.x && threadIdx.x == 0) {
    bucket_start[d.W * d.B] = base + m;
    bucket_start[d.W * d.B + 1] = base + m;
  }
  {
    // a narrower window's keys past its buckets: empty, all at the window's end
    const uint32_t k1 = d.nbc << fbw;
    if (k1 < d.B) {
      const uint32_t span = (d.B - k1) / d.nbc, wend = bin_base[(w + 1) * d.nbc];
      for (uint32_t f = threadIdx.x; f < span; f += FS_THREADS) bucket_start[w * d.B + k1 + cb * span + f] = wend;
    }
  }
  __syncthreads();
  PROBE(2, bin, 1);
  const bool staged = m <= FS_CAP;
  const uint32_t fmask = (1u << d.fb) - 1u;  // the packed word's fine field (fbw <= d.fb bits used)
  // fk: fine key (< 2^11) of a staged entry, later | its rank in its bucket << 16 (< FS_CAP)
  uint32_t fk[FS_R], en[FS_R];
  if (staged) {
    // every load issued before any is used; the packed/unpacked choice is uniform
    if (d.packed) {
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const uint32_t e = r * FS_THREADS + threadIdx.x;
        en[r] = e < m ? part_entry[base + e] : 0u;
      }
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const uint32_t e = r * FS_THREADS + threadIdx.x;
        fk[r] = e < m ? en[r] & fmask : 0xffffu;
        en[r] >>= d.fb;
      }
      PROBE_WAIT_VM();
      PROBE(2, bin, 2);
    } else {
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const uint32_t e = r * FS_THREADS + threadIdx.x;
        fk[r] = e < m ? part_fine[base + e] : 0xffffu;
        en[r] = e < m ? part_entry[base + e] : 0u;
      }
    }
#pragma unroll
    for (uint32_t r = 0; r < FS_R; r++)
      if (fk[r] != 0xffffu) fk[r] |= atomicAdd(&cnt[fk[r]], 1u) << 16;
  } else {
    // register tiles of FS_R keys per lane (independent loads in flight); runs of equal keys
    // are collapsed before the LDS atomic
    uint32_t last = 0, run = 0;
    for (uint32_t t0 = 0; t0 < m; t0 += FS_CAP) {
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const uint32_t e = t0 + r * FS_THREADS + threadIdx.x;
        uint32_t en_unused;
        fk[r] = 0xffffu;
        if (e < m) part_load(part_entry, part_fine, d, base + e, fk[r], en_unused);
      }
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++)
        if (fk[r] != 0xffffu) count_runs(cnt, last, run, fk[r]);
    }
    if (run) atomicAdd(&cnt[last], run);
  }
  __syncthreads();
  PROBE(2, bin, 3);
  // per-bucket counts -> exclusive offsets; boundaries and run starts go out with them (a bucket
  // ends where the next one starts)
  lds_excl_scan_wave0(cnt, nf);
  const double kinv = 1.0 / (double)K;  // div_by_inv: the bucket's first run, ceil(gs / K)
  __syncthreads();
  PROBE(2, bin, 4);
#pragma unroll
  for (uint32_t q = 0; q < FS_MAXF / FS_THREADS; q++) {
    const uint32_t f = q * FS_THREADS + threadIdx.x;
    if (f < nf) {
      const uint32_t gs = base + cnt[f];
      const uint32_t ge = base + (f + 1 < nf ? cnt[f + 1] : m);
      bucket_start[key0 + f] = gs;
      const uint32_t r0 = div_by_inv(gs + K - 1, kinv);
      for (uint32_t r = r0; r * K < ge; r++) run_key[r] = key0 + f;
    }
  }
  __syncthreads();
  PROBE(2, bin, 5);
  if (!staged) {
    // placement: a wave's lanes with equal keys take consecutive slots of their bucket, reserved
    // by the lowest of them with one LDS atomic
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t t0 = 0; t0 < m; t0 += FS_CAP) {
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const uint32_t e = t0 + r * FS_THREADS + threadIdx.x;
        fk[r] = 0u;
        en[r] = 0u;
        if (e < m) part_load(part_entry, part_fine, d, base + e, fk[r], en[r]);
      }
#pragma unroll
      for (uint32_t r = 0; r < FS_R; r++) {
        const bool live = t0 + r * FS_THREADS + threadIdx.x < m;
        const uint64_t peers = key_peers(fk[r], fbw, __ballot(live));
        const uint32_t leader = (uint32_t)__builtin_ctzll(peers | (1ull << 63));
        uint32_t slot = 0;
        if (live && lane == leader) slot = atomicAdd(&cnt[fk[r]], (uint32_t)__popcll(peers));
        slot = (uint32_t)__shfl((int)slot, (int)leader, 64);
        if (live) sorted_entry[base + slot + (uint32_t)__popcll(peers & below)] = en[r];
      }
    }
    PROBE(2, bin, 6);
    PROBE(2, bin, 7);
    return;
  }
#pragma unroll
  for (uint32_t r = 0; r < FS_R; r++)
    if (fk[r] != 0xffffu) st_entry[cnt[fk[r] & 0xffffu] + (fk[r] >> 16)] = en[r];
  __syncthreads();
  PROBE(2, bin, 6);
  for (uint32_t j = threadIdx.x; j < m; j += FS_THREADS) sorted_entry[base + j] = st_entry[j];
  PROBE(2, bin, 7);
}

#ifdef MSM_GAP_KERNEL
// tuning builds: a no-op launch between the sort and the accumulation
extern "C" __global__ void k_gap(uint32_t* __restrict__ p) {
  if (p == nullptr && threadIdx.x == 1234567) p[0] = 0;
}
#endif

// ---------------------------------------------------------------------------------------------
// bucket accumulation
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_pt(uint32_t* __restrict__ dst, const xyzt& p) {
  uint32_t rec[36];
#pragma unroll
  for (int k = 0; k < NL; k++) {
    rec[k] = p.X.v[k];
    rec[NL + k] = p.Y.v[k];
    rec[2 * NL + k] = p.T.v[k];
    rec[3 * NL + k] = p.Z.v[k];
  }
  uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int k = 0; k < 9; k++) d4[k] = make_uint4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
}
__device__ __forceinline__ xyzt load_pt(const uint32_t* __restrict__ src) {
  uint32_t rec[36];
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
#pragma unroll
  for (int k = 0; k < 9; k++) {
    uint4 v = s4[k];
    rec[4 * k] = v.x; rec[4 * k + 1] = v.y; rec[4 * k + 2] = v.z; rec[4 * k + 3] = v.w;
  }
  xyzt p;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    p.X.v[k] = rec[k];
    p.Y.v[k] = rec[NL + k];
    p.T.v[k] = rec[2 * NL + k];
    p.Z.v[k] = rec[3 * NL + k];
  }
  return p;
}

__device__ __forceinline__ void store_fe_lds(uint32_t* dst, const fe& a) {
#pragma unroll
  for (int k = 0; k < NL; k++) dst[k] = a.v[k];
}
__device__ __forceinline__ fe load_fe_lds(const uint32_t* src) {
  fe a;
#pragma unroll
  for (int k = 0; k < NL; k++) a.v[k] = src[k];
  return a;
}
__device__ __forceinline__ void store_pt_lds(uint32_t* dst, const xyzt& p) {
#pragma unroll
  for (int k = 0; k < NL; k++) {
    dst[k] = p.X.v[k];
    dst[NL + k] = p.Y.v[k];
    dst[2 * NL + k] = p.T.v[k];
    dst[3 * NL + k] = p.Z.v[k];
  }
}
__device__ __forceinline__ xyzt load_pt_lds(const uint32_t* src) {
  xyzt p;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    p.X.v[k] = src[k];
    p.Y.v[k] = src[NL + k];
    p.T.v[k] = src[2 * NL + k];
    p.Z.v[k] = src[3 * NL + k];
  }
  return p;
}

// First bucket key k > cur whose end bucket_start[k + 1] lies past pos, given that bucket cur is
// empty (bucket_start[cur + 1] == pos).  bucket_start is non-decreasing and ends with the total
// (> pos), so an exponential search then a binary search find it in O(log gap) loads: a window
// narrower than the bucket table, or a stretch of empty windows (small or structured scalars),
// would otherwise cost one dependent load per empty bucket.
__device__ __forceinline__ uint32_t next_nonempty(const uint32_t* __restrict__ bucket_start, uint32_t cur, uint32_t pos,
                                               uint32_t nkeys) {
  uint32_t lo = cur, step = 1;  // bucket lo is empty
  uint32_t hi = cur + 1;        // bucket nkeys - 1 ends at the total (> pos): the search stops there
  while (bucket_start[hi + 1] == pos) {
    lo = hi;
    step <<= 1;
    hi = min(cur + step, nkeys - 1);
  }
  // bucket lo empty, bucket hi ends past pos: the answer is in (lo, hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bucket_start[mid + 1] == pos) lo = mid;
    else hi = mid;
  }
  return hi;
}

// Bucket accumulation over the sorted list.  Lane = run of K consecutive entries (perfect load
// balance whatever the bucket sizes).  Inside a run, whole buckets are written straight to the
// bucket table; bucket boundaries come from bucket_start (one load per bucket, issued a bucket
// ahead), the run's first bucket from run_key.
//
// A bucket cut by run boundaries is joined without a second pass over HBM.  Every run's leading
// piece (head: the entries of a bucket begun in an earlier run) is staged in LDS, flagged
// "pass" when the whole run lies inside that bucket and the bucket continues.  After one barrier
// the run where the bucket begins adds its trailing piece (tail) to the head of the next run.
// A workgroup with a pass-through run (skewed scalars: a bucket holding several runs) instead
// stages its heads and tails in HBM and leaves the joins to k_chain_join, which collapses the
// chains with a logarithmic segmented scan; that keeps this kernel's register budget (and
// occupancy) set by the main loop.
//
// A chain reaching the end of workgroup g continues in workgroup g+1's lane-0 chain ("lead"):
// the tail owner stores its part in the bucket table and cross_key[g] names the bucket;
// k_bucket_reduce_1 adds lead_val[g+1] to it, after k_lead_scan has chained leads that
// themselves run through whole workgroups.
#ifndef MSM_ACC_VEC
#define MSM_ACC_VEC 1
#endif
// Progress-ordered wave priority.  A SIMD's VALU issue goes by wave priority, then age, so of the
// four equal runs sharing a SIMD the oldest finished first and the youngest last (an 8-GPU share,
// one round of workgroups: 186 / 294 / 407 / 510 us by dispatch order, tools/phase_probe.py), and
// the last ~30% of the launch ran with one to three waves per SIMD.  Each wave therefore lowers
// its priority as it passes each quarter of its run (3, 2, 1, 0): a wave ahead of its partners
// yields to them, and the four finish within the last quarter's age order (share: 371 / 400 /
// 428 / 453 us).  A lone 2^20 MSM's accumulation 744 -> 717 us (latency 1.074 -> 1.045 ms);
// pipelined launches and the 8-GPU shares within noise (sessions t15, t16).
#ifndef MSM_ACC_PRIO
#define MSM_ACC_PRIO 1
#endif
constexpr uint32_t ACC_THREADS = 256;
// One workgroup-sized tile of the accumulation: runs [wg ACC_THREADS, (wg + 1) ACC_THREADS).
__device__ __forceinline__ void acc_tile(uint32_t wg, uint32_t (*sh_head)[PT_WORDS], uint32_t* sh_hkey,
                                         const uint32_t* __restrict__ pts,
                                         const uint32_t* __restrict__ sorted_entry,
                                         const uint32_t* __restrict__ bucket_start,
                                         const uint32_t* __restrict__ run_key,
                                         const uint32_t* __restrict__ total_ptr, uint32_t K,
                                         uint32_t nkeys,
                                         uint32_t* __restrict__ buckets,
                                         uint32_t* __restrict__ lead_val,
                                         uint32_t* __restrict__ lead_open,
                                         uint32_t* __restrict__ cross_key,
                                         uint32_t* __restrict__ skew_list,
                                         uint32_t* __restrict__ g_head,
                                         uint32_t* __restrict__ g_hkey,
                                         uint32_t* __restrict__ g_tkey) {
  const uint32_t M = *total_ptr;
  const uint32_t lt = threadIdx.x;
  const uint32_t t = wg * ACC_THREADS + lt;
  const uint32_t s = t * K;
  sh_hkey[lt] = KEY_INVALID;
  xyzt acc = pt_identity();
  uint32_t cur = KEY_INVALID;
  bool has_tail = false, cont = false;
  if (s < M) {
    const uint32_t e = min(s + K, M);
    cur = run_key[t];
    const bool started_before = bucket_start[cur] < s;
    uint32_t bend = bucket_start[cur + 1];   // end of bucket `cur`
    uint32_t bnext = bucket_start[cur + 2];  // end of the bucket after it (prefetched)
    bool seg_first = true;
#if MSM_ACC_VEC
    // sorted entries four at a time (one 16-B load per lane every fourth step: the lanes walk
    // runs K entries apart, so scalar loads cost one cache-line request per lane per step)
    const bool vec = (K & 3u) == 0;  // run starts (t K) are then 16-B aligned
    uint4 eb = make_uint4(0u, 0u, 0u, 0u);
#endif
#if MSM_ACC_PRIO
    // (levels at 70 / 84 / 95% of the run instead, so that the age order left inside the last
    // level decides only its last 5%: pipelined 2^20 +7%, session t16)
    const uint32_t q1 = K >> 2, q2 = K >> 1, q3 = q1 + q2;
#endif
    for (uint32_t pos = s; pos < e; pos++) {
#if MSM_ACC_PRIO
      {
        const uint32_t q = __builtin_amdgcn_readfirstlane(pos - s);  // uniform: every run is K long
        if (q == q1) __builtin_amdgcn_s_setprio(2);
        else if (q == q2) __builtin_amdgcn_s_setprio(1);
        else if (q == q3) __builtin_amdgcn_s_setprio(0);
      }
#endif
#if MSM_ACC_VEC
      const uint32_t jq = (pos - s) & 3u;  // uniform across the lanes still in the loop
      if (vec && jq == 0) eb = *reinterpret_cast<const uint4*>(sorted_entry + pos);
#endif
      if (pos == bend) {
        if (seg_first && started_before) {
          store_pt_lds(sh_head[lt], acc);
          sh_hkey[lt] = cur;
        } else {
          store_pt(buckets + (size_t)cur * PT_WORDS, acc);
        }
        // advance to the next non-empty bucket (a run of empty ones is skipped by galloping)
        cur++;
        bend = bnext;
        bnext = bucket_start[cur + 2];
        if (bend == pos) {
          cur = next_nonempty(bucket_start, cur, pos, nkeys);
          bend = bucket_start[cur + 1];
          bnext = bucket_start[cur + 2];
        }
        acc = pt_identity();
        seg_first = false;
      }
#if MSM_ACC_VEC
      const uint32_t ent = !vec ? sorted_entry[pos] : jq == 0 ? eb.x : jq == 1 ? eb.y : jq == 2 ? eb.z : eb.w;
#else
      const uint32_t ent = sorted_entry[pos];
#endif
      const pre q = load_pre_signed(pts, ent);
      acc = pt_madd(acc, q);
    }
    cont = bend > e;  // bucket `cur` continues into the next run
    if (seg_first && started_before) {  // the whole run belongs to a bucket begun earlier
      store_pt_lds(sh_head[lt], acc);
      sh_hkey[lt] = cur | (cont ? KEY_PASS : 0u);
    } else if (cont) {
      has_tail = true;  // acc = tail piece of bucket `cur`
    } else {
      store_pt(buckets + (size_t)cur * PT_WORDS, acc);
    }
  }
  // the last live run of the workgroup says whether a bucket leaves the workgroup
  const uint32_t nruns = (M + K - 1) / K;
  const uint32_t last = min(ACC_THREADS, nruns - min(nruns, wg * ACC_THREADS)) - 1;
  if (lt == last) cross_key[wg] = cont ? cur : KEY_INVALID;
  __syncthreads();
  // Chains of heads: a run whose head is "pass" continues into the next run.  Runs of three or
  // more pass heads in a row (buckets of ~200+ entries: skewed scalars), and a lead chain that
  // leaves the workgroup, are deferred to k_chain_join's logarithmic scan; otherwise every chain
  // has at most two pass heads and is joined right here with at most three adds.  (The top
  // window of canonical scalars holds ~110 entries per bucket, so two-pass chains are common.)
  // (The two lane-0 terms ask for a pass head in a workgroup of one or two live runs.  Only the
  // list's last workgroup has so few, and its last run never continues, so neither can fire:
  // tests/_acc_model.py UNREACHABLE.  A lead chain that leaves a full workgroup is 256 pass heads
  // and takes the first term.)
  const uint32_t hk = sh_hkey[lt];
  auto is_pass = [&](uint32_t r) {
    const uint32_t k = sh_hkey[r];
    return k != KEY_INVALID && (k & KEY_PASS) != 0;
  };
  const bool my_pass = hk != KEY_INVALID && (hk & KEY_PASS);
  const bool nxt_pass = lt < last && is_pass(lt + 1);
  const bool nxt2_pass = lt + 1 < last && is_pass(lt + 2);
  if (__syncthreads_or((my_pass && nxt_pass && nxt2_pass) ||
                       (lt == 0 && my_pass && (last == 0 || (nxt_pass && last == 1))))) {
    // skewed workgroup: stage heads and tail pieces for k_chain_join
    if (s < M) {
      g_hkey[t] = hk;
      if (hk != KEY_INVALID) store_pt(g_head + (size_t)t * PT_WORDS, load_pt_lds(sh_head[lt]));
      g_tkey[t] = has_tail ? cur : KEY_INVALID;
      if (has_tail) store_pt(buckets + (size_t)cur * PT_WORDS, acc);
    }
    if (lt == 0) skew_list[1 + atomicAdd(&skew_list[0], 1u)] = wg;
    return;
  }
  // Lane 0's head is the end of the previous workgroup's crossing bucket: the workgroup's lead.
  // If it is pass-through (a bucket spanning run 0 whole), the bucket ends in run 1 or 2 (not
  // past the workgroup here), and lane 0 joins those heads into the lead.
  const bool lead_join = lt == 0 && my_pass;
  if (lt == 0) {
    lead_open[wg] = 0u;
    if (s < M && hk != KEY_INVALID && !lead_join)
      store_pt(lead_val + (size_t)wg * PT_WORDS, load_pt_lds(sh_head[0]));
  }
  if (has_tail || lead_join) {
    // a tail's bucket continues in run lt+1 (and lt+2, lt+3 while those are pass-through), unless
    // it leaves the workgroup: then k_bucket_reduce_1 adds the next workgroup's lead
    // (cross_key).  (Straight-line adds: the same in a loop costs ~50 more VGPRs and occupancy.)
    const uint32_t nwalk =
        lead_join ? 1u + (nxt_pass ? 1u : 0u)
                  : (lt < last ? 1u + ((nxt_pass && lt + 1 < last) ? 1u + ((nxt2_pass && lt + 2 < last) ? 1u : 0u) : 0u)
                               : 0u);
    if (lead_join) acc = load_pt_lds(sh_head[0]);
    if (nwalk) acc = pt_add(acc, load_pt_lds(sh_head[lt + 1]));
    if (nwalk > 1) acc = pt_add(acc, load_pt_lds(sh_head[lt + 2]));
    if (nwalk > 2) acc = pt_add(acc, load_pt_lds(sh_head[lt + 3]));
    store_pt(lead_join ? lead_val + (size_t)wg * PT_WORDS : buckets + (size_t)cur * PT_WORDS, acc);
  }
}

// The kernel: one tile per workgroup.  (A persistent grid of 2-3 workgroups per CU striding over
// the tiles, to leave CU room for the other launch's kernels, measured no faster: DESIGN.md §4.1.)
extern "C" __global__ void __launch_bounds__(ACC_THREADS) k_accumulate(const uint32_t* __restrict__ pts,
                                         const uint32_t* __restrict__ sorted_entry,
                                         const uint32_t* __restrict__ bucket_start,
                                         const uint32_t* __restrict__ run_key,
                                         const uint32_t* __restrict__ total_ptr, uint32_t K,
                                         uint32_t nkeys,
                                         uint32_t* __restrict__ buckets,
                                         uint32_t* __restrict__ lead_val,
                                         uint32_t* __restrict__ lead_open,
                                         uint32_t* __restrict__ cross_key,
                                         uint32_t* __restrict__ skew_list,
                                         uint32_t* __restrict__ g_head,
                                         uint32_t* __restrict__ g_hkey,
                                         uint32_t* __restrict__ g_tkey) {
  __shared__ uint32_t sh_head[ACC_THREADS][PT_WORDS];
  __shared__ uint32_t sh_hkey[ACC_THREADS];
  PROBE(3, blockIdx.x, 0);
#if MSM_ACC_PRIO
  __builtin_amdgcn_s_setprio(3);
#endif
  acc_tile(blockIdx.x, sh_head, sh_hkey, pts, sorted_entry, bucket_start, run_key, total_ptr, K, nkeys, buckets,
           lead_val, lead_open, cross_key, skew_list, g_head, g_hkey, g_tkey);
  PROBE(3, blockIdx.x, 7);
}

// Joins for workgroups that k_accumulate found to hold a pass-through run (skewed scalars).
// Segmented suffix scan over the workgroup's heads by pointer jumping: after it, head r holds
// h_r + h_{r+1} + ... to the end of r's chain (or the workgroup's end), and its pass bit says
// whether the chain leaves the workgroup; log2(256) steps of one point add.  Then every tail
// owner adds the chain that follows it, and lane 0 publishes the workgroup's lead.
constexpr uint32_t CJ_GRID = 256;  // k_chain_join workgroups (they loop over the skewed list)
extern "C" __global__ void __launch_bounds__(ACC_THREADS) k_chain_join(const uint32_t* __restrict__ skew_list,
                                         const uint32_t* __restrict__ total_ptr,
                                         uint32_t K,
                                         const uint32_t* __restrict__ g_head,
                                         const uint32_t* __restrict__ g_hkey,
                                         const uint32_t* __restrict__ g_tkey,
                                         uint32_t* __restrict__ buckets,
                                         uint32_t* __restrict__ lead_val,
                                         uint32_t* __restrict__ lead_open,
                                         uint32_t* __restrict__ lead_flag) {
  const uint32_t nskew = skew_list[0];
  if (blockIdx.x >= nskew) return;
  const uint32_t M = *total_ptr;
  const uint32_t nruns = (M + K - 1) / K;
  __shared__ uint32_t sh_head[ACC_THREADS][PT_WORDS];
  __shared__ uint32_t sh_hkey[ACC_THREADS];
  const uint32_t lt = threadIdx.x;
  for (uint32_t li = blockIdx.x; li < nskew; li += gridDim.x) {
  const uint32_t wg = skew_list[1 + li];
  const uint32_t t = wg * ACC_THREADS + lt;
  const bool live = t < nruns;
  const uint32_t hk = live ? g_hkey[t] : KEY_INVALID;
  sh_hkey[lt] = hk;
  xyzt v = pt_identity();
  if (hk != KEY_INVALID) {
    v = load_pt(g_head + (size_t)t * PT_WORDS);
    store_pt_lds(sh_head[lt], v);
  }
  bool open = hk != KEY_INVALID && (hk & KEY_PASS);
  __syncthreads();
  for (uint32_t d = 1; d < ACC_THREADS; d <<= 1) {
    const bool take = open && lt + d < ACC_THREADS;
    xyzt nv;
    bool nopen = false;
    if (take) {
      nv = load_pt_lds(sh_head[lt + d]);
      nopen = (sh_hkey[lt + d] & KEY_PASS) != 0;
    }
    __syncthreads();
    if (take) {
      v = pt_add(v, nv);
      open = nopen;
      store_pt_lds(sh_head[lt], v);
      sh_hkey[lt] = (sh_hkey[lt] & ~KEY_PASS) | (open ? KEY_PASS : 0u);
    }
    __syncthreads();
  }
  if (lt == 0) {
    const uint32_t h0 = sh_hkey[0];
    const bool has_head = h0 != KEY_INVALID;
    const bool lopen = has_head && (h0 & KEY_PASS);
    if (has_head) store_pt(lead_val + (size_t)wg * PT_WORDS, load_pt_lds(sh_head[0]));
    lead_open[wg] = lopen ? 1u : 0u;
    if (lopen) atomicOr(lead_flag, 1u);
  }
  const uint32_t tk = live ? g_tkey[t] : KEY_INVALID;
  if (tk != KEY_INVALID) {
    xyzt acc = load_pt(buckets + (size_t)tk * PT_WORDS);
    if (lt + 1 < ACC_THREADS) acc = pt_add(acc, load_pt_lds(sh_head[lt + 1]));
    store_pt(buckets + (size_t)tk * PT_WORDS, acc);
  }
  __syncthreads();  // LDS reused by the next listed workgroup
  }
}

// Chains leads that run through whole workgroups (a bucket spanning three or more workgroups):
// segmented suffix scan lead_val[g] <- lead_val[g] + lead_val[g+1] + ... while lead_open.  One
// workgroup walks the leads from the end in tiles of LS_THREADS; a no-op unless k_chain_join found
// an open lead (lead_flag).
constexpr uint32_t LS_THREADS = 512;
extern "C" __global__ void __launch_bounds__(LS_THREADS) k_lead_scan(uint32_t* __restrict__ lead_val,
                                                                     const uint32_t* __restrict__ lead_open,
                                                                     const uint32_t* __restrict__ lead_flag,
                                                                     const uint32_t* __restrict__ total_ptr,
                                                                     uint32_t K) {
  if (*lead_flag == 0) return;
  __shared__ uint32_t sv[LS_THREADS][PT_WORDS];
  __shared__ uint32_t so[LS_THREADS];
  const uint32_t M = *total_ptr;
  const uint32_t nruns = (M + K - 1) / K;
  const uint32_t nwg = (nruns + ACC_THREADS - 1) / ACC_THREADS;
  const uint32_t i = threadIdx.x;
  const uint32_t ntiles = (nwg + LS_THREADS - 1) / LS_THREADS;
  for (int tile = (int)ntiles - 1; tile >= 0; tile--) {
    const uint32_t g = (uint32_t)tile * LS_THREADS + i;
    // every lead an open lead can reach is valid (an open chain enters the next workgroup's
    // lane 0); other slots may hold stale data and are never absorbed
    bool open = g < nwg && lead_open[g] != 0;
    xyzt v = g < nwg ? load_pt(lead_val + (size_t)g * PT_WORDS) : pt_identity();
    store_pt_lds(sv[i], v);
    so[i] = open ? 1u : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < LS_THREADS; d <<= 1) {
      const bool take = open && i + d < LS_THREADS && g + d < nwg;
      xyzt nv;
      bool nopen = false;
      if (take) {
        nv = load_pt_lds(sv[i + d]);
        nopen = so[i + d] != 0;
      }
      __syncthreads();
      if (take) {
        v = pt_add(v, nv);
        open = nopen;
        store_pt_lds(sv[i], v);
        so[i] = open ? 1u : 0u;
      }
      __syncthreads();
    }
    // still open at the tile's end: absorb the (final) value of the next tile's first lead
    const uint32_t gn = (uint32_t)(tile + 1) * LS_THREADS;
    if (open && gn < nwg) v = pt_add(v, load_pt(lead_val + (size_t)gn * PT_WORDS));
    __syncthreads();
    if (g < nwg && lead_open[g] != 0) store_pt(lead_val + (size_t)g * PT_WORDS, v);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// dense-bucket accumulation (narrow scalars whose buckets hold hundreds of entries: Plan::dense)
// ---------------------------------------------------------------------------------------------
// k_accumulate hands a lane a run of K sorted entries and must keep K above a third of the largest
// bucket (run_length_skew_floor), so a launch of few, large buckets has ~3 lanes per bucket whatever
// its size: 2^20 bytes in one 9-bit window are ~710 lanes of ~1,476 dependent adds each.  Here the
// work goes out by bucket and by position inside the bucket instead.  A unit is one wave; it owns
// one segment of S = 64 E consecutive entries of ONE bucket, lane l the entries l + 64 j (coalesced
// 4-byte loads), added from the identity with no boundary test, and the 64 lane sums join in a
// six-level tree through LDS.  A bucket of one segment is stored straight to the bucket table; the
// segments of a larger one go to partials[unit] and k_dense_fold adds them.  Which unit owns which
// segment is data (k_dense_segments builds the map from bucket_start on every launch), so the grid
// is a bound the host knows without the bucket sizes: sum_k ceil(s_k / S) <= floor(M / S) + #nonempty.
constexpr uint32_t DS_THREADS = 1024;  // k_dense_segments: one workgroup
constexpr uint32_t DU_THREADS = 256;   // k_dense_units: four units
constexpr uint32_t DF_THREADS = 256;   // k_dense_fold: one bucket

// Inclusive running maximum over the wave's lanes.
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
    if (lane >= d) x = max(x, y);
  }
  return x;
}

// The segment map.  seg_base[k] = segments of the buckets before k (seg_base[nkeys]: the live
// units), unit_key[u] = the bucket of unit u: every thread counts a stretch of consecutive buckets,
// one workgroup scan places them, each non-empty bucket marks its first unit and a running maximum
// over the units fills in the rest (keys only grow with the unit).  The same pass invalidates every
// cross_key word the bucket reduction may probe -- bucket_start[k] / (K ACC_THREADS) = KA, at most
// M / KA -- since no bucket of a dense launch continues in a lead.  Nothing is written at or past
// `ubound` units (the host's bound, which the sizes cannot exceed) or `ncross` words.
extern "C" __global__ void __launch_bounds__(DS_THREADS) k_dense_segments(const uint32_t* __restrict__ bucket_start,
                                                                          uint32_t nkeys, uint32_t S,
                                                                          uint32_t* __restrict__ seg_base,
                                                                          uint32_t* __restrict__ unit_key,
                                                                          uint32_t ubound,
                                                                          uint32_t* __restrict__ cross_key,
                                                                          uint32_t KA, uint32_t ncross) {
  __shared__ uint32_t sh_w[DS_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t kp = (nkeys + DS_THREADS - 1) / DS_THREADS;
  const uint32_t k0 = min(tid * kp, nkeys), k1 = min(k0 + kp, nkeys);
  uint32_t mine = 0;
  for (uint32_t k = k0; k < k1; k++) mine += (bucket_start[k + 1] - bucket_start[k] + S - 1) / S;
  uint32_t wtot;
  uint32_t base = wave_excl_scan(mine, wtot);
  if (lane == 63) sh_w[wv] = wtot;
  __syncthreads();
  uint32_t total = 0;
  for (uint32_t w = 0; w < DS_THREADS / 64; w++) {
    if (w == wv) base += total;
    total += sh_w[w];
  }
  __syncthreads();  // sh_w is reused below
  for (uint32_t k = k0, run = base; k < k1; k++) {
    seg_base[k] = run;
    run += (bucket_start[k + 1] - bucket_start[k] + S - 1) / S;
  }
  if (tid == 0) seg_base[nkeys] = total;
  const uint32_t live = min(total, ubound);
  for (uint32_t u = tid; u < live; u += DS_THREADS) unit_key[u] = 0u;
  const uint32_t M = bucket_start[nkeys];
  for (uint32_t g = tid; g <= M / KA + 1u && g < ncross; g += DS_THREADS) cross_key[g] = KEY_INVALID;
  __syncthreads();
  for (uint32_t k = k0, run = base; k < k1; k++) {
    const uint32_t segs = (bucket_start[k + 1] - bucket_start[k] + S - 1) / S;
    if (segs && run < live) unit_key[run] = k;
    run += segs;
  }
  __syncthreads();
  const uint32_t up = (live + DS_THREADS - 1) / DS_THREADS;
  const uint32_t u0 = min(tid * up, live), u1 = min(u0 + up, live);
  uint32_t m = 0;
  for (uint32_t u = u0; u < u1; u++) m = max(m, unit_key[u]);
  const uint32_t incl = wave_incl_max(m);
  if (lane == 63) sh_w[wv] = incl;
  uint32_t carry = (uint32_t)__shfl_up((int)incl, 1, 64);
  if (lane == 0) carry = 0;
  __syncthreads();
  for (uint32_t w = 0; w < wv; w++) carry = max(carry, sh_w[w]);
  for (uint32_t u = u0; u < u1; u++) {
    carry = max(carry, unit_key[u]);
    unit_key[u] = carry;
  }
}

// One tree level of a lane group through `x` ([word][lane], so a level's reads and writes walk
// consecutive banks): lanes [d, 2 d) hand their points to lanes [0, d).  `sync` orders the writes
// before the reads, and the reads before the next level's writes.
template <uint32_t LANES, typename SYNC>
__device__ __forceinline__ void dense_tree_level(uint32_t (*x)[LANES], uint32_t l, uint32_t d, xyzt& acc, SYNC&& sync) {
  if (l >= d && l < 2 * d) {
#pragma unroll
    for (int k = 0; k < NL; k++) {
      x[k][l - d] = acc.X.v[k];
      x[NL + k][l - d] = acc.Y.v[k];
      x[2 * NL + k][l - d] = acc.T.v[k];
      x[3 * NL + k][l - d] = acc.Z.v[k];
    }
  }
  sync();
  if (l < d) {
    xyzt o;
#pragma unroll
    for (int k = 0; k < NL; k++) {
      o.X.v[k] = x[k][l];
      o.Y.v[k] = x[NL + k][l];
      o.T.v[k] = x[2 * NL + k][l];
      o.Z.v[k] = x[3 * NL + k][l];
    }
    acc = pt_add(acc, o);
  }
  sync();
}

// (four waves per SIMD asked of the compiler, k_accumulate's occupancy: 132 VGPRs without the bound)
extern "C" __global__ void __launch_bounds__(DU_THREADS, 4) k_dense_units(const uint32_t* __restrict__ pts,
                                                                       const uint32_t* __restrict__ sorted_entry,
                                                                       const uint32_t* __restrict__ bucket_start,
                                                                       const uint32_t* __restrict__ seg_base,
                                                                       const uint32_t* __restrict__ unit_key,
                                                                       uint32_t E, uint32_t nkeys, uint32_t ubound,
                                                                       uint32_t* __restrict__ buckets,
                                                                       uint32_t* __restrict__ partials) {
  __shared__ uint32_t sh_x[DU_THREADS / 64][PT_WORDS][32];
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t u = blockIdx.x * (DU_THREADS / 64) + wv;
  // (no workgroup barrier below: a wave past the live units just leaves)
  if (u >= ubound || u >= seg_base[nkeys]) return;
  const uint32_t key = min((uint32_t)__builtin_amdgcn_readfirstlane((int)unit_key[u]), nkeys - 1);
  const uint32_t sb = seg_base[key], nseg = seg_base[key + 1] - sb;
  const uint32_t S = 64u * E;
  const uint32_t bend = bucket_start[key + 1];
  const uint32_t beg = min(bucket_start[key] + (u - sb) * S, bend), end = min(beg + S, bend);
  xyzt acc = pt_identity();
  if (end - beg == S) {
    // a whole segment: E entries per lane, nothing to test
    const uint32_t* ep = sorted_entry + beg + lane;
    uint32_t ent = ep[0];
#pragma unroll 1
    for (uint32_t j = 1; j <= E; j++) {
      const pre q = load_pre_signed(pts, ent);
      if (j < E) ent = ep[64u * j];  // the next entry's load beside this one's add
      acc = pt_madd(acc, q);
    }
  } else {
    // the bucket's last segment: lanes past its end keep the identity
#pragma unroll 1
    for (uint32_t pos = beg + lane; pos < end; pos += 64u) acc = pt_madd(acc, load_pre_signed(pts, sorted_entry[pos]));
  }
  // wave-synchronous: the exchange is private to the wave, so its LDS writes and reads need only
  // keep their program order (the fences hold the compiler to it, the hardware runs a wave's LDS
  // operations in order)
  auto sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
#pragma unroll 1
  for (uint32_t d = 32; d >= 1; d >>= 1) dense_tree_level<32>(sh_x[wv], lane, d, acc, sync);
  if (lane == 0) store_pt(nseg == 1 ? buckets + (size_t)key * PT_WORDS : partials + (size_t)u * PT_WORDS, acc);
}

// The buckets of more than one segment: one workgroup per bucket adds its partials, lane l those
// at l, l + 256, ... (one bucket may hold the whole list: all-equal scalars), then a tree of as
// many levels as the bucket has live lanes.
extern "C" __global__ void __launch_bounds__(DF_THREADS) k_dense_fold(const uint32_t* __restrict__ seg_base,
                                                                      const uint32_t* __restrict__ partials,
                                                                      uint32_t ubound,
                                                                      uint32_t* __restrict__ buckets) {
  __shared__ uint32_t sh_x[PT_WORDS][DF_THREADS / 2];
  const uint32_t key = blockIdx.x, lt = threadIdx.x;
  const uint32_t sb = seg_base[key];
  const uint32_t ns = min(seg_base[key + 1], ubound) - min(sb, ubound);
  if (ns < 2) return;  // uniform: the bucket is empty, or its one unit stored it
  xyzt acc = pt_identity();
  if (lt < ns) acc = load_pt(partials + (size_t)(sb + lt) * PT_WORDS);
  for (uint32_t i = lt + DF_THREADS; i < ns; i += DF_THREADS)
    acc = pt_add(acc, load_pt(partials + (size_t)(sb + i) * PT_WORDS));
  uint32_t top = DF_THREADS / 2;
  while (top >= ns) top >>= 1;  // the first level that still moves a live lane: top < ns <= 2 top
#pragma unroll 1
  for (uint32_t d = top; d >= 1; d >>= 1) dense_tree_level<DF_THREADS / 2>(sh_x, lt, d, acc, [] { __syncthreads(); });
  if (lt == 0) store_pt(buckets + (size_t)key * PT_WORDS, acc);
}

// ---------------------------------------------------------------------------------------------
// bucket reduction:  G_w = sum_{b} (b+1) B_{w,b}
//   chunk c (L buckets): U_c = sum_i (i+1) B_{cL+i}, T_c = sum_i B_{cL+i}   (running sums)
//   G_w = sum_c U_c + L * sum_c c T_c = R_{w,V} + sum_k L 2^k R_{w,k},  R_{w,k} = sum_{c: bit k} T_c
// L need not be a power of two: the host Horner places R_{w,k} once per set bit of L.
// ---------------------------------------------------------------------------------------------
// L = buckets per k_bucket_reduce_1 lane.  Each lane's running sums are a chain of ~2L dependent
// adds and one wave per SIMD already keeps its VALU ~82% busy, so the kernel takes ~one chain per
// SIMD -- as long as the live lanes fit in one wave per SIMD.  The host picks the smallest L
// (of RED1_LS) for which they do (bucket_reduce_L): at c = 15 two MSMs have 540,672 live buckets,
// so L = 8 would need 1,056 waves on 1,024 SIMDs (two chains on some) and L = 9 needs 939.
#ifndef MSM_RED1_THREADS
#define MSM_RED1_THREADS 256
#endif
constexpr uint32_t RED1_THREADS = MSM_RED1_THREADS;

// Chunks of a window that a digit can reach (its "live" chunks; the others hold no entry): a main
// window of the table's full width fills every chunk, a (q)-bit window in a (q+1)-bit table its
// lower half, and the overflow window (|digit| <= 4, buckets 0..3) is counted dead altogether (it
// is empty for canonical scalars).  `a` is the window's index in its MSM.
__host__ __device__ __forceinline__ uint32_t red1_live_chunks(const MsmDims& d, uint32_t L, uint32_t nchunks,
                                                              uint32_t a) {
  if (a + 1 == d.Wm) return 0;
  if (d.nhi == 0 || a < d.nhi) return nchunks;
  return (d.B / 2 + L - 1) / L;
}

// Lane -> (window, chunk) of k_bucket_reduce_1.  Live chunks of every MSM's windows come first, so
// real work is whole waves at the front of the grid; then the dead ones (empty unless the scalars
// are non-canonical), which exit early.
__host__ __device__ __forceinline__ bool red1_lane(const MsmDims& d, uint32_t L, uint32_t nchunks, uint32_t gd, uint32_t& w,
                                          uint32_t& c) {
  uint32_t live = 0;  // per MSM
  for (uint32_t l = 0; l < d.Wr; l++) live += red1_live_chunks(d, L, nchunks, d.w0 + l);
  const uint32_t dead = d.Wr * nchunks - live;
  uint32_t r, m;
  bool in_live;
  if (gd < d.nm * live) {
    m = gd / live;
    r = gd % live;
    in_live = true;
  } else {
    const uint32_t r0 = gd - d.nm * live;
    if (r0 >= d.nm * dead) return false;
    m = r0 / dead;
    r = r0 % dead;
    in_live = false;
  }
  for (uint32_t l = 0; l < d.Wr; l++) {
    const uint32_t lc = red1_live_chunks(d, L, nchunks, d.w0 + l);
    const uint32_t span = in_live ? lc : nchunks - lc;
    if (r < span) {
      w = m * d.Wr + l;
      c = in_live ? r : lc + r;
      return true;
    }
    r -= span;
  }
  return false;
}

// Running sums of chunk c of window w (one lane): U = sum_i (i+1) B_i and T = sum_i B_i over the
// chunk's buckets, i counted within the chunk.
template <uint32_t RL>
__device__ __forceinline__ void red1_chunk(const uint32_t* __restrict__ buckets, const uint32_t* __restrict__ bucket_start,
                                           const MsmDims& d, uint32_t K, uint32_t w, uint32_t c,
                                           const uint32_t* __restrict__ cross_key, const uint32_t* __restrict__ lead_val,
                                           xyzt& U, xyzt& T) {
  const uint32_t key0 = w * d.B + c * RL;
  const uint32_t nb = min(RL, d.B - c * RL);  // buckets of this chunk inside the window (last chunk: fewer)
  // bucket metadata up front (independent loads): which buckets are non-empty, and which left
  // their accumulation workgroup and need the continuation from lead_val
  uint32_t bs[RL + 1];
#pragma unroll
  for (uint32_t i = 0; i <= RL; i++) bs[i] = i <= nb ? bucket_start[key0 + i] : 0u;
  uint32_t live = 0, cross = 0;
  const double ginv = 1.0 / ((double)K * ACC_THREADS);  // (bs / K) / ACC_THREADS = bs / (K ACC_THREADS)
#pragma unroll
  for (uint32_t i = 0; i < RL; i++) {
    if (i < nb && bs[i + 1] != bs[i]) {
      live |= 1u << i;
      if (cross_key[div_by_inv(bs[i], ginv)] == key0 + i) cross |= 1u << i;
    }
  }
  if (!live) {  // whole chunk empty (e.g. the windows above the scalars' top bit)
    U = T = pt_identity();
    return;
  }
  xyzt carry = pt_identity(), acc = pt_identity();
  bool carry_live = false, acc_live = false;
  // running sums from the top bucket down; the next live bucket's load is issued before the
  // current bucket's adds.  (Software-pipelining the two adds of a step -- both read the previous
  // carry -- measured 159 -> 184 us at 2^17: the compiler keeps 242 VGPRs and serialises them.)
  int i = 31 - __builtin_clz(live);
  xyzt nb_pt = load_pt(buckets + (size_t)(key0 + i) * PT_WORDS);
#pragma unroll 1
  for (; i >= 0; i--) {
    if ((live >> i) & 1u) {
      xyzt b = nb_pt;
      const uint32_t below = live & ((1u << i) - 1u);
      if (below) nb_pt = load_pt(buckets + (size_t)(key0 + 31 - __builtin_clz(below)) * PT_WORDS);
      if ((cross >> i) & 1u) {  // rare: reload the bucket's start rather than index bs[] dynamically
        const uint32_t g0 = (bucket_start[key0 + i] / K) / ACC_THREADS;
        b = pt_add(b, load_pt(lead_val + (size_t)(g0 + 1) * PT_WORDS));
      }
      carry = carry_live ? pt_add(carry, b) : b;
      carry_live = true;
    }
    if (carry_live) {
      acc = acc_live ? pt_add(acc, carry) : carry;
      acc_live = true;
    }
  }
  U = acc;
  T = carry;
}

template <uint32_t RL>
__global__ void __launch_bounds__(RED1_THREADS) k_bucket_reduce_1(const uint32_t* __restrict__ buckets,
                                                         const uint32_t* __restrict__ bucket_start, MsmDims d,
                                                         uint32_t K, uint32_t nchunks,
                                                         const uint32_t* __restrict__ cross_key,
                                                         const uint32_t* __restrict__ lead_val,
                                                         uint32_t* __restrict__ out_U, uint32_t* __restrict__ out_T) {
  uint32_t w, c;
  if (!red1_lane(d, RL, nchunks, blockIdx.x * blockDim.x + threadIdx.x, w, c)) return;
  const uint32_t g = w * nchunks + c;
  xyzt U, T;
  red1_chunk<RL>(buckets, bucket_start, d, K, w, c, cross_key, lead_val, U, T);
  store_pt(out_U + (size_t)g * PT_WORDS, U);
  store_pt(out_T + (size_t)g * PT_WORDS, T);
}

// The same running sums on lane pairs (MSM_RED1_PAIRS=1; measured no faster, kept off): a chunk's two chains run on two
// lanes in lock step -- the even lane the bucket chain T (carry += B_i, top bucket down), the odd
// lane the weighted chain U (acc += the carry after the even lane's previous step, taken with a
// DPP quad permute) -- so every lane holds one running point instead of two plus the prefetched
// bucket: half the registers (more waves per SIMD to hide the adds' latency) for L + 1 steps of
// one add instead of 2L adds.  Identity adds (empty buckets, the chains' ends) are harmless: the
// formulas are complete.
__device__ __forceinline__ fe fe_from_even(const fe& a) {
  fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)a.v[i], 0xA0, 0xF, 0xF, false);
  return r;
}

#ifndef MSM_RED1P_WAVES
#define MSM_RED1P_WAVES 3  // waves per SIMD asked of the compiler (4: <= 128 VGPRs, 17 spilled)
#endif
template <uint32_t RL>
__global__ void __launch_bounds__(RED1_THREADS, MSM_RED1P_WAVES) k_bucket_reduce_1p(const uint32_t* __restrict__ buckets,
                                                          const uint32_t* __restrict__ bucket_start, MsmDims d,
                                                          uint32_t K, uint32_t nchunks,
                                                          const uint32_t* __restrict__ cross_key,
                                                          const uint32_t* __restrict__ lead_val,
                                                          uint32_t* __restrict__ out_U, uint32_t* __restrict__ out_T) {
  const bool u_lane = (threadIdx.x & 1u) != 0;
  uint32_t w, c;
  // both lanes of a pair map to the same chunk, so a pair leaves (or stays) together
  if (!red1_lane(d, RL, nchunks, (blockIdx.x * blockDim.x + threadIdx.x) >> 1, w, c)) return;
  const uint32_t g = w * nchunks + c;
  const uint32_t key0 = w * d.B + c * RL;
  const uint32_t nb = min(RL, d.B - c * RL);
  uint32_t live = 0, cross = 0;
  {
    uint32_t bs[RL + 1];
#pragma unroll
    for (uint32_t i = 0; i <= RL; i++) bs[i] = i <= nb ? bucket_start[key0 + i] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < RL; i++) {
      if (i < nb && bs[i + 1] != bs[i]) {
        live |= 1u << i;
        if (!u_lane && cross_key[(bs[i] / K) / ACC_THREADS] == key0 + i) cross |= 1u << i;
      }
    }
  }
  uint32_t* out = (u_lane ? out_U : out_T) + (size_t)g * PT_WORDS;
  if (!live) {  // whole chunk empty (e.g. the windows above the scalars' top bit)
    store_pt(out, pt_identity());
    return;
  }
  const int top = 31 - __builtin_clz(live);
  xyzt run = pt_identity();
#pragma unroll 1
  for (int i = top; i >= -1; i--) {
    // the odd lane's operand: its even lane's carry as it stands before this step's add
    xyzt q;
    q.X = fe_from_even(run.X);
    q.Y = fe_from_even(run.Y);
    q.T = fe_from_even(run.T);
    q.Z = fe_from_even(run.Z);
    if (u_lane) {
      // q as permuted (identity at the first step: the even lane's carry starts there)
    } else if (i >= 0 && ((live >> i) & 1u)) {
      q = load_pt(buckets + (size_t)(key0 + i) * PT_WORDS);
      if ((cross >> i) & 1u) {  // rare: the bucket continues past its accumulation workgroup
        const uint32_t g0 = (bucket_start[key0 + i] / K) / ACC_THREADS;
        q = pt_add(q, load_pt(lead_val + (size_t)(g0 + 1) * PT_WORDS));
      }
    } else {
      q = pt_identity();
    }
    run = pt_add(run, q);
  }
  store_pt(out, run);
}

// One workgroup per (window, term).  Terms 0..nv-1: R_{V,v} = sum of U_c over the v-th slice of
// chunks; term nv+k: R_k = sum_{c: bit k of c} T_c.  Every workgroup sums at most
// pow2ceil(nchunks)/2 points.
// Output: X, Y, T, Z in the host's Montgomery form (a * 2^256 mod p, 8 LE words each), written
// straight into coherent pinned host memory (no readback copy), so the host Horner
// (hostfield.h) uses them without conversion.  Block 0 also forwards the error flags, the entry
// count and whether the joins of skewed buckets are still due.
#ifndef MSM_RED2_THREADS
#define MSM_RED2_THREADS 512
#endif
constexpr int RED2_THREADS = MSM_RED2_THREADS;
#ifndef MSM_RED2_QUAD
#define MSM_RED2_QUAD 256
#endif
constexpr uint32_t RED2_QUAD = MSM_RED2_QUAD;  // tree levels below this many points use quad-cooperative adds
extern "C" __global__ void __launch_bounds__(RED2_THREADS) k_bucket_reduce_2(const uint32_t* __restrict__ in_U,
                                                                             const uint32_t* __restrict__ in_T,
                                                                             uint32_t nchunks, uint32_t nv,
                                                                             uint32_t nterms,
                                                                             uint32_t* __restrict__ err,
                                                                             uint32_t* __restrict__ lead_flag,
                                                                             uint32_t* __restrict__ skew_list,
                                                                             const uint32_t* __restrict__ total,
                                                                             uint32_t final_pass,
                                                                             const uint32_t* __restrict__ bucket_start,
                                                                             uint32_t B,
                                                                             uint32_t* __restrict__ out_host) {
  __shared__ uint32_t sh[RED2_THREADS / 2][PT_WORDS];
  const uint32_t w = blockIdx.x / nterms, term = blockIdx.x % nterms;
  // a window without entries (the overflow window of canonical scalars, a window range's empty
  // windows) has identity terms: skip its loads and latency-bound tree
  const bool empty = bucket_start[(size_t)w * B] == bucket_start[(size_t)(w + 1) * B];
  if (empty) {
    if (threadIdx.x == 0) store_pt_lds(sh[0], pt_identity());
    __syncthreads();
  } else {
    const bool vterm = term < nv;
    const uint32_t* src = vterm ? in_U : in_T;
    const uint32_t kbit = term - nv;
    // A V slice is ceil(nchunks/nv) consecutive chunks; a bit term enumerates its j-th chunk with
    // bit k set directly (j < pow2ceil(nchunks)/2, chunks past the end skipped), so every lane
    // loads about the same number of points (a stride-and-skip loop over all chunks would give half
    // the lanes all the work for k < 10).
    const uint32_t vslice = (nchunks + nv - 1) / nv;
    uint32_t half_n = 1;
    while (2 * half_n < nchunks) half_n <<= 1;
    xyzt acc = pt_identity();
    bool live = false;
    for (uint32_t j = threadIdx.x; j < (vterm ? vslice : half_n); j += RED2_THREADS) {
      const uint32_t c = vterm ? term * vslice + j : (((j >> kbit) << (kbit + 1)) | (1u << kbit) | (j & ((1u << kbit) - 1u)));
      if (c >= nchunks) continue;
      xyzt p = load_pt(src + ((size_t)w * nchunks + c) * PT_WORDS);
      acc = live ? pt_add(acc, p) : p;
      live = true;
    }
    // tree reduce through LDS: upper half hands its point to the lower half each round.  The wide
    // levels add one point per lane; from RED2_QUAD points down, each add is spread over a quad of
    // lanes (pt_add_quad: 3 multiply latencies instead of 9) since those levels are latency-bound.
    for (uint32_t half = RED2_THREADS / 2; half >= RED2_QUAD; half >>= 1) {
      if (threadIdx.x >= half && threadIdx.x < 2 * half) store_pt_lds(sh[threadIdx.x - half], acc);
      __syncthreads();
      if (threadIdx.x < half) acc = pt_add(acc, load_pt_lds(sh[threadIdx.x]));
      __syncthreads();
    }
    if (threadIdx.x < RED2_QUAD) store_pt_lds(sh[threadIdx.x], acc);
    __syncthreads();
    {
      const uint32_t j = threadIdx.x >> 2, q = threadIdx.x & 3;
      for (uint32_t half = RED2_QUAD / 2; half >= 1; half >>= 1) {
        const bool act = j < half;  // uniform across a quad
        fe res;
        if (act) res = pt_add_quad(load_fe_lds(&sh[j][q * NL]), load_fe_lds(&sh[j + half][q * NL]));
        __syncthreads();
        if (act) store_fe_lds(&sh[j][q * NL], res);
        __syncthreads();
      }
    }
  }
  if (threadIdx.x < 4) {  // one lane per coordinate (X, Y, T, Z): the conversions run side by side
    const uint32_t q = threadIdx.x;
    uint32_t* o = out_host + (size_t)blockIdx.x * 32 + 8 * q;
    uint32_t wd[8];
    fe_to_words_le(fe_to_host_mont(load_fe_lds(&sh[0][q * NL])), wd);
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = wd[k];
  }
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) {
      // Without the joins in the sequence (final_pass 0), skewed buckets make the terms invalid:
      // the host then runs the joins and this reduction again (msm_host.hip PART_JOIN), so the
      // skew flags stay set for them.
      const size_t tail = (size_t)gridDim.x * 32;
      const bool skew = skew_list[0] != 0 || *lead_flag != 0;
      out_host[tail] = *err;
      out_host[tail + 1] = *total;
      // (nonzero: run the joins; the skewed workgroups' count where there is one, for msm_test_acc_state)
      out_host[tail + 2] = (skew && !final_pass) ? max(skew_list[0], 1u) : 0u;
      *err = 0;  // flags start the next MSM cleared (no memset node in the graph)
      if (final_pass || !skew) {
        *lead_flag = 0;
        skew_list[0] = 0;
      }
    }
    __threadfence_system();
  }
}

// ---- bucket reduction, second stage in two kernels (k_red2_groups + k_red2_terms) ------------
// k_bucket_reduce_2 sums, per window, every chunk's U_c once and its T_c once per set bit of c
// (~6.5 adds per chunk at 2,048 chunks), in trees whose wide levels make it VALU-bound.  Here
// the chunks of a window go in groups of RG_CH = 2^RG_LOG: k_red2_groups reduces a group in LDS
// to 2 + RG_LOG points,
//   V_g = sum U_c,  S_g = sum T_c,  R_{g,k} = sum_{c: bit k of (c - RG_CH g)} T_c  (k < RG_LOG),
// with ~3 adds per chunk: one tree over U, one over T whose odd operands at level j are exactly
// R_{g,j}'s points (kept in place, lowest set bit of the index = 2^j), and the R trees run in
// the same steps as the main trees (RG_LOG steps of <= 2 RG_CH quad-cooperative adds).
// k_red2_terms then forms the same terms as k_bucket_reduce_2 from <= 64 group points each:
//   V slices = sum V_g,  R_k = sum_g R_{g,k} (k < RG_LOG),  R_k = sum_{g: bit k-RG_LOG of g} S_g,
// since sum_c c T_c = sum_g (RG_CH g S_g + sum_k 2^k R_{g,k}).
#ifndef MSM_RG_LOG
#define MSM_RG_LOG 7
#endif
constexpr uint32_t RG_LOG = MSM_RG_LOG;      // log2 chunks per group
constexpr uint32_t RG_CH = 1u << RG_LOG;     // chunks per group
constexpr uint32_t RG_OUT = 2 + RG_LOG;      // points per group: V, S, R_0..R_{RG_LOG-1}
constexpr uint32_t RG_MAXG = 64;             // groups per window k_red2_terms takes
#ifndef MSM_RED2_SYSFENCE
#define MSM_RED2_SYSFENCE 0
#endif

// Coordinate q (0 X, 1 Y, 2 T, 3 Z) of the identity (0, 1, 0, 1).
__device__ __forceinline__ fe identity_coord(uint32_t q) { return fe_sel((q & 1u) != 0, fe_zero(), fe_one()); }
__device__ __forceinline__ fe load_fe_g(const uint32_t* __restrict__ src) {
  fe a;
#pragma unroll
  for (int k = 0; k < NL; k++) a.v[k] = src[k];
  return a;
}

// The RG_LOG steps of one group's reduction over its chunk points in LDS (T in shA, U in shB):
// leaves V at shB[0], S at shA[0] and R_k at shA[2^k].  Quad Q of the block's quads takes tasks
// Q, Q + nquads, ... of each step (no task of a step reads another's destination).
__device__ __forceinline__ void red2_tree_steps(uint32_t (*shA)[PT_WORDS], uint32_t (*shB)[PT_WORDS]) {
  const uint32_t q = threadIdx.x & 3, nquads = blockDim.x >> 2;
#pragma unroll 1
  for (uint32_t s = 0; s < RG_LOG; s++) {
    const uint32_t lp = RG_LOG - 1 - s;  // log2 of the pairs per list at this step
    const uint32_t ntask = (2 + s) << lp;
#pragma unroll 1
    for (uint32_t Q = threadIdx.x >> 2; Q < ntask; Q += nquads) {
      const uint32_t kind = Q >> lp, i = Q & ((1u << lp) - 1u);
      uint32_t(*arr)[PT_WORDS] = kind == 1 ? shB : shA;
      uint32_t dst, srcx;
      if (kind < 2) {  // the T and U trees: pairs (i 2^(s+1), i 2^(s+1) + 2^s)
        dst = i << (s + 1);
        srcx = dst + (1u << s);
      } else {  // R_j's tree, level s - j - 1, over its list at indices (2 m + 1) 2^j
        const uint32_t j = kind - 2, l = s - j - 1;
        const uint32_t md = i << (l + 1), ms = md + (1u << l);
        dst = (2 * md + 1) << j;
        srcx = (2 * ms + 1) << j;
      }
      const fe r = pt_add_quad(load_fe_lds(&arr[dst][q * NL]), load_fe_lds(&arr[srcx][q * NL]));
      store_fe_lds(&arr[dst][q * NL], r);  // no other task of this step reads dst or srcx
    }
    __syncthreads();
  }
}

// One group's reduction (k_red2_groups): chunks g RG_CH .. of window w from in_U / in_T into
// shA (T) / shB (U), then the steps.  Every thread of the block takes part (4 RG_CH threads,
// quad Q = chunk).
__device__ __forceinline__ void red2_group_tree(const uint32_t* __restrict__ in_U, const uint32_t* __restrict__ in_T,
                                                uint32_t nchunks, uint32_t w, uint32_t g,
                                                uint32_t (*shA)[PT_WORDS], uint32_t (*shB)[PT_WORDS]) {
  const uint32_t Q = threadIdx.x >> 2, q = threadIdx.x & 3;
  const uint32_t c = g * RG_CH + Q;
  fe u, t;
  if (c < nchunks) {
    const size_t off = ((size_t)w * nchunks + c) * PT_WORDS + q * NL;
    u = load_fe_g(in_U + off);
    t = load_fe_g(in_T + off);
  } else {
    u = t = identity_coord(q);
  }
  store_fe_lds(&shB[Q][q * NL], u);
  store_fe_lds(&shA[Q][q * NL], t);
  __syncthreads();
  red2_tree_steps(shA, shB);
}

// Group point idx (0 V, 1 S, 2 + k R_k) of the tree left in shA / shB.
__device__ __forceinline__ const uint32_t* red2_group_point(uint32_t (*shA)[PT_WORDS], uint32_t (*shB)[PT_WORDS],
                                                            uint32_t idx) {
  return idx == 0 ? shB[0] : idx == 1 ? shA[0] : shA[1u << (idx - 2)];
}

// Which group points make term `term` of a window: point idx of groups g0 + j (or, for the bit
// terms past RG_LOG, of the j-th group with bit kbit set), j < npts.
struct Red2Term {
  uint32_t idx, g0, g1, kbit, npts;
  bool bitsel;
};
__host__ __device__ __forceinline__ Red2Term red2_term(uint32_t term, uint32_t nv, uint32_t ngroups) {
  Red2Term r{0, 0, 0, 0, 0, false};
  if (term < nv) {
    const uint32_t sl = (ngroups + nv - 1) / nv;
    r.g0 = min(ngroups, term * sl);
    r.g1 = min(ngroups, r.g0 + sl);
    r.npts = r.g1 - r.g0;
  } else if (term - nv < RG_LOG) {
    r.idx = 2 + (term - nv);
    r.g1 = ngroups;
    r.npts = ngroups;
  } else {
    r.idx = 1;
    r.kbit = term - nv - RG_LOG;
    r.bitsel = true;
    r.npts = 1;  // g = ((j >> kbit) << (kbit + 1)) | (1 << kbit) | (j & (2^kbit - 1)), j < pow2ceil(ngroups) / 2
    while (2 * r.npts < ngroups) r.npts <<= 1;
  }
  return r;
}
__host__ __device__ __forceinline__ uint32_t red2_term_group(const Red2Term& t, uint32_t j) {
  return t.bitsel ? (((j >> t.kbit) << (t.kbit + 1)) | (1u << t.kbit) | (j & ((1u << t.kbit) - 1u))) : t.g0 + j;
}

// Block 0 of k_red2_terms: the MSM's flags beside the terms (as k_bucket_reduce_2).
__device__ __forceinline__ void red2_flags(uint32_t nwindows_terms, uint32_t* __restrict__ err,
                                           uint32_t* __restrict__ lead_flag, uint32_t* __restrict__ skew_list,
                                           const uint32_t* __restrict__ total, uint32_t final_pass,
                                           uint32_t* __restrict__ out_host) {
  const size_t tail = (size_t)nwindows_terms * 32;
  const bool skew = skew_list[0] != 0 || *lead_flag != 0;
  out_host[tail] = *err;
  out_host[tail + 1] = *total;
  out_host[tail + 2] = (skew && !final_pass) ? max(skew_list[0], 1u) : 0u;
  *err = 0;
  if (final_pass || !skew) {
    *lead_flag = 0;
    skew_list[0] = 0;
  }
}

extern "C" __global__ void __launch_bounds__(4 * RG_CH) k_red2_groups(const uint32_t* __restrict__ in_U,
                                                                     const uint32_t* __restrict__ in_T,
                                                                     uint32_t nchunks, uint32_t ngroups,
                                                                     const uint32_t* __restrict__ bucket_start,
                                                                     uint32_t B, uint32_t* __restrict__ out) {
  __shared__ uint32_t shA[RG_CH][PT_WORDS];  // T, then its partial sums and the R lists in place
  __shared__ uint32_t shB[RG_CH][PT_WORDS];  // U
  const uint32_t w = blockIdx.x / ngroups, g = blockIdx.x % ngroups;
  if (bucket_start[(size_t)w * B] == bucket_start[(size_t)(w + 1) * B]) return;  // empty window: unread
  red2_group_tree(in_U, in_T, nchunks, w, g, shA, shB);
  const uint32_t Q = threadIdx.x >> 2, q = threadIdx.x & 3;
  if (Q < RG_OUT) {
    const fe v = load_fe_lds(red2_group_point(shA, shB, Q) + q * NL);
    uint32_t* o = out + (((size_t)w * ngroups + g) * RG_OUT + Q) * PT_WORDS + q * NL;
#pragma unroll
    for (int k = 0; k < NL; k++) o[k] = v.v[k];
  }
}

// The first stage and the group trees in one launch (MSM_RED_FOLD=1; measured slower, kept off:
// the tree runs at the first stage's occupancy, two 226-VGPR waves per group): a workgroup of RG_CH
// lanes takes one group of RG_CH consecutive chunks of a window -- each lane its chunk's running
// sums (red1_chunk), straight into LDS, then the group's tree (red2_tree_steps, 32 quads) -- and
// writes the group's V, S and R_0..R_{RG_LOG-1}: the chunk sums never go to memory and the second
// launch of the stage (k_red2_groups) is gone.  Live groups first (red1_group), then the dead ones
// (chunks a canonical scalar's digit cannot reach); a group without entries writes identities, and
// an empty window's groups are not read.
__host__ __device__ __forceinline__ bool red1_group(const MsmDims& d, uint32_t L, uint32_t nchunks, uint32_t G, uint32_t gd,
                                           uint32_t& w, uint32_t& g, bool& live) {
  uint32_t lg = 0;  // live groups per MSM
  for (uint32_t l = 0; l < d.Wr; l++) lg += (red1_live_chunks(d, L, nchunks, d.w0 + l) + RG_CH - 1) / RG_CH;
  const uint32_t dg = d.Wr * G - lg;
  uint32_t r, m;
  if (gd < d.nm * lg) {
    m = gd / lg;
    r = gd % lg;
    live = true;
  } else {
    const uint32_t r0 = gd - d.nm * lg;
    if (r0 >= d.nm * dg) return false;
    m = r0 / dg;
    r = r0 % dg;
    live = false;
  }
  for (uint32_t l = 0; l < d.Wr; l++) {
    const uint32_t lgl = (red1_live_chunks(d, L, nchunks, d.w0 + l) + RG_CH - 1) / RG_CH;
    const uint32_t span = live ? lgl : G - lgl;
    if (r < span) {
      w = m * d.Wr + l;
      g = live ? r : lgl + r;
      return true;
    }
    r -= span;
  }
  return false;
}

template <uint32_t RL>
__global__ void __launch_bounds__(RG_CH) k_bucket_reduce_1g(const uint32_t* __restrict__ buckets,
                                                          const uint32_t* __restrict__ bucket_start, MsmDims d,
                                                          uint32_t K, uint32_t nchunks, uint32_t ngroups,
                                                          const uint32_t* __restrict__ cross_key,
                                                          const uint32_t* __restrict__ lead_val,
                                                          uint32_t* __restrict__ out) {
  __shared__ uint32_t shA[RG_CH][PT_WORDS];  // T
  __shared__ uint32_t shB[RG_CH][PT_WORDS];  // U
  uint32_t w, g;
  bool live;  // (order only: a dead group with entries is reduced like any other)
  if (!red1_group(d, RL, nchunks, ngroups, blockIdx.x, w, g, live)) return;
  if (bucket_start[(size_t)w * d.B] == bucket_start[(size_t)(w + 1) * d.B]) return;  // empty window: unread
  uint32_t* o = out + ((size_t)w * ngroups + g) * RG_OUT * PT_WORDS;
  // a group without entries (the dead groups, unless the scalars are non-canonical) is identities
  const uint32_t kb0 = w * d.B + min(d.B, g * RG_CH * RL), kb1 = w * d.B + min(d.B, (g + 1) * RG_CH * RL);
  if (bucket_start[kb0] == bucket_start[kb1]) {
    for (uint32_t k = threadIdx.x; k < RG_OUT * 4; k += RG_CH) {
      const fe id = identity_coord(k & 3);
#pragma unroll
      for (int j = 0; j < NL; j++) o[(k >> 2) * PT_WORDS + (k & 3) * NL + j] = id.v[j];
    }
    return;
  }
  const uint32_t c = g * RG_CH + threadIdx.x;
  xyzt U = pt_identity(), T = pt_identity();
  if (c < nchunks) red1_chunk<RL>(buckets, bucket_start, d, K, w, c, cross_key, lead_val, U, T);
  store_pt_lds(shB[threadIdx.x], U);
  store_pt_lds(shA[threadIdx.x], T);
  __syncthreads();
  red2_tree_steps(shA, shB);
  const uint32_t Q = threadIdx.x >> 2, q = threadIdx.x & 3;
  if (Q < RG_OUT) {
    const fe v = load_fe_lds(red2_group_point(shA, shB, Q) + q * NL);
#pragma unroll
    for (int k = 0; k < NL; k++) o[Q * PT_WORDS + q * NL + k] = v.v[k];
  }
}

extern "C" __global__ void __launch_bounds__(4 * RG_MAXG) k_red2_terms(const uint32_t* __restrict__ grp,
                                                                      uint32_t ngroups, uint32_t nv,
                                                                      uint32_t nterms, uint32_t* __restrict__ err,
                                                                      uint32_t* __restrict__ lead_flag,
                                                                      uint32_t* __restrict__ skew_list,
                                                                      const uint32_t* __restrict__ total,
                                                                      uint32_t final_pass,
                                                                      const uint32_t* __restrict__ bucket_start,
                                                                      uint32_t B, uint32_t* __restrict__ out_host) {
  __shared__ uint32_t sh[RG_MAXG][PT_WORDS];
  const uint32_t w = blockIdx.x / nterms, term = blockIdx.x % nterms;
  const uint32_t Q = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool empty = bucket_start[(size_t)w * B] == bucket_start[(size_t)(w + 1) * B];
  const Red2Term rt = red2_term(term, nv, ngroups);
  fe v = identity_coord(q);
  if (!empty && Q < rt.npts) {
    const uint32_t g = red2_term_group(rt, Q);
    if (g < ngroups) v = load_fe_g(grp + (((size_t)w * ngroups + g) * RG_OUT + rt.idx) * PT_WORDS + q * NL);
  }
  store_fe_lds(&sh[Q][q * NL], v);
  __syncthreads();
  uint32_t half = 1;
  while (2 * half < rt.npts) half <<= 1;
  if (empty || rt.npts <= 1) half = 0;
#pragma unroll 1
  for (; half >= 1; half >>= 1) {
    if (Q < half) {
      const fe r = pt_add_quad(load_fe_lds(&sh[Q][q * NL]), load_fe_lds(&sh[Q + half][q * NL]));
      store_fe_lds(&sh[Q][q * NL], r);
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) {  // as k_bucket_reduce_2: host Montgomery form, straight into pinned memory
    uint32_t* o = out_host + (size_t)blockIdx.x * 32 + 8 * q;
    uint32_t wd[8];
    fe_to_words_le(fe_to_host_mont(load_fe_lds(&sh[0][q * NL])), wd);
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = wd[k];
  }
#if MSM_RED2_SYSFENCE
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) red2_flags(gridDim.x, err, lead_flag, skew_list, total, final_pass, out_host);
    __threadfence_system();
  }
#else
  // no system-scope fence per workgroup: the host reads the terms only after the launch's event,
  // whose completion makes the kernel's writes to pinned memory visible
  if (threadIdx.x == 0 && blockIdx.x == 0) red2_flags(gridDim.x, err, lead_flag, skew_list, total, final_pass, out_host);
#endif
}

// Small utility kernels used by tests: batch field ops / point ops on canonical inputs.
// op 0: field mul, 1: add, 2: sub, 3: 2d * a (fe_mul_2d); inputs LE standard words [n][8] x2, output [n][8].
extern "C" __global__ void k_test_field(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                        uint32_t* __restrict__ out, uint32_t n, uint32_t op) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t aw[8], bw[8], ow[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    aw[k] = a[(size_t)i * 8 + k];
    bw[k] = b[(size_t)i * 8 + k];
  }
  fe x = fe_to_mont(fe_from_words_le(aw)), y = fe_to_mont(fe_from_words_le(bw));
  // ops 4, 5: pt_madd's signed-difference multiply, (x - y)(y - x) and (x - y)(x + y)
  fe r = op == 0   ? fe_mul(x, y)
         : op == 1 ? fe_add_n(x, y)
         : op == 2 ? fe_sub(x, y)
         : op == 3 ? fe_mul_2d(x)
         : op == 4 ? fe_mul_sd<WIDE_ALL, true>(fe_sub_s(x, y), fe_sub_s(y, x))
                   : fe_mul_sd<WIDE_ALL, false>(fe_sub_s(x, y), fe_add(x, y));
  fe_to_words_le(fe_to_std(r), ow);
#pragma unroll
  for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = ow[k];
}

// op 0: P + Q via pt_add, 1: P + Q via pt_madd (Q affine from its x,y), 2: 2P via pt_dbl.
// Inputs: affine points as LE words [n][16] (x, y); output affine-projective X,Y,T,Z std LE words [n][32].
template <int OP>
__global__ void k_test_point(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
                             uint32_t* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4][8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    w[0][k] = p[(size_t)i * 16 + k];
    w[1][k] = p[(size_t)i * 16 + 8 + k];
    w[2][k] = q[(size_t)i * 16 + k];
    w[3][k] = q[(size_t)i * 16 + 8 + k];
  }
  xyzt P;
  P.X = fe_to_mont(fe_from_words_le(w[0]));
  P.Y = fe_to_mont(fe_from_words_le(w[1]));
  P.T = fe_mul(P.X, P.Y);
  P.Z = fe_one();
  xyzt Q;
  Q.X = fe_to_mont(fe_from_words_le(w[2]));
  Q.Y = fe_to_mont(fe_from_words_le(w[3]));
  Q.T = fe_mul(Q.X, Q.Y);
  Q.Z = fe_one();
  xyzt R;
  if constexpr (OP == 0) {
    R = pt_add(P, Q);
  } else if constexpr (OP == 1) {
    pre qq;  // halved, as k_prepare_points writes it
    qq.ymx = fe_mul(fe_sub(Q.Y, Q.X), fe_const(HALF29));
    qq.ypx = fe_mul(fe_add_n(Q.Y, Q.X), fe_const(HALF29));
    qq.kt = fe_mul(Q.T, fe_const(KD29));
    R = pt_madd(P, qq);
  } else {
    R = pt_dbl(P);
  }
  fe c4[4] = {fe_to_std(R.X), fe_to_std(R.Y), fe_to_std(R.T), fe_to_std(R.Z)};
  uint32_t ow[8];
#pragma unroll
  for (int qd = 0; qd < 4; qd++) {
    fe_to_words_le(c4[qd], ow);
#pragma unroll
    for (int k = 0; k < 8; k++) out[(size_t)i * 32 + qd * 8 + k] = ow[k];
  }
}

// Quad-cooperative add check: pair i is handled by lanes 4i..4i+3.  Inputs as k_test_point
// (affine LE words), output X,Y,T,Z std LE words [n][32].
extern "C" __global__ void k_test_quad(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
                                       uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2, c = threadIdx.x & 3;
  const bool live = i < n;
  const uint32_t ii = live ? i : 0;
  uint32_t w[4][8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    w[0][k] = p[(size_t)ii * 16 + k];
    w[1][k] = p[(size_t)ii * 16 + 8 + k];
    w[2][k] = q[(size_t)ii * 16 + k];
    w[3][k] = q[(size_t)ii * 16 + 8 + k];
  }
  const fe px = fe_to_mont(fe_from_words_le(w[0])), py = fe_to_mont(fe_from_words_le(w[1]));
  const fe qx = fe_to_mont(fe_from_words_le(w[2])), qy = fe_to_mont(fe_from_words_le(w[3]));
  const fe pc[4] = {px, py, fe_mul(px, py), fe_one()};
  const fe qc[4] = {qx, qy, fe_mul(qx, qy), fe_one()};
  fe a = pc[0], b = qc[0];
#pragma unroll
  for (uint32_t k = 1; k < 4; k++) {
    a = fe_sel(c == k, a, pc[k]);
    b = fe_sel(c == k, b, qc[k]);
  }
  const fe r = pt_add_quad(a, b);
  uint32_t ow[8];
  fe_to_words_le(fe_to_std(r), ow);
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[(size_t)i * 32 + c * 8 + k] = ow[k];
  }
}

// ---- raw-limb hooks (tests/test_gpu_limbs.py) ---------------------------------------------------
// The kernels above convert canonical words on the way in and reduce on the way out, so they see
// fresh fe_mul outputs only and compare mod p.  These take the 9 u32 limbs of each operand as they
// are and return every output limb as it is, for a limb-for-limb comparison with the bit-exact
// model (tests/_fp29_model.py) at operands no conversion produces: the unnormalised forms at
// their limb maxima, signed differences, values in [p, 2p).  One instantiation per op.
enum LimbOp : int {
  LOP_MUL_ALL = 0, LOP_MUL_GH, LOP_MUL_EH, LOP_MUL_EF, LOP_MUL_GHEH,  // fe_mul_w<mask>
  LOP_MUL_SD_U, LOP_MUL_SD_S,                                         // fe_mul_sd<WIDE_ALL, false | true>
  LOP_MUL_2D, LOP_MUL_D, LOP_SUB, LOP_NEG, LOP_ADD_N, LOP_DBL_N, LOP_TO_STD, LOP_TO_HOST_MONT, LOP_INV,
  LOP_FROM_WORDS, LOP_TO_WORDS, LOP_WORDS_LT_P,                       // [n][8] LE words on one side
  LOP_PT_ADD, LOP_PT_DBL, LOP_PT_MADD, LOP_PT_QUAD,                   // [n][36] X|Y|T|Z limbs
  // the per-lane point kernels' functions (k_test_limbs_lane, tests/test_gpu_lanes.py)
  LOP_SQR, LOP_STD_NEG, LOP_IS_ONE, LOP_SQRT_TS,                      // [n][9] limbs (is_one: one word out)
  LOP_FROM_RECORD, LOP_MUL_ORDER, LOP_SHIFT_LANE,                     // record -> point, point -> point, record -> record
  LOP_COUNT
};
constexpr uint32_t LOP_SHIFT_MAX = 255;  // LOP_SHIFT_LANE's doublings per record: a handle's chunk bits S never pass it
__host__ __device__ constexpr bool limb_op_is_point(int op) { return op >= LOP_PT_ADD && op <= LOP_PT_QUAD; }
__host__ __device__ constexpr uint32_t limb_op_in_words(int op) {
  return limb_op_is_point(op) || op == LOP_MUL_ORDER ? PT_WORDS
         : (op == LOP_FROM_RECORD || op == LOP_SHIFT_LANE) ? PRE_WORDS
         : (op == LOP_FROM_WORDS || op == LOP_WORDS_LT_P) ? 8u : (uint32_t)NL;
}
__host__ __device__ constexpr uint32_t limb_op_b_words(int op) {  // 0: no second operand
  return op == LOP_PT_MADD ? 3u * NL : (op == LOP_PT_ADD || op == LOP_PT_QUAD) ? PT_WORDS
         : op == LOP_SHIFT_LANE ? 1u  // the record's number of doublings
         : (op <= LOP_MUL_SD_S || op == LOP_SUB || op == LOP_ADD_N) ? (uint32_t)NL : 0u;
}
__host__ __device__ constexpr uint32_t limb_op_out_words(int op) {
  return limb_op_is_point(op) || op == LOP_FROM_RECORD || op == LOP_MUL_ORDER ? PT_WORDS
         : op == LOP_SHIFT_LANE ? PRE_WORDS : op == LOP_TO_WORDS ? 8u
         : (op == LOP_WORDS_LT_P || op == LOP_IS_ONE) ? 1u : (uint32_t)NL;
}

template <int OP>
__global__ void k_test_limbs(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                             uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (OP == LOP_FROM_WORDS || OP == LOP_WORDS_LT_P) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = a[(size_t)i * 8 + k];
    if constexpr (OP == LOP_FROM_WORDS)
      store_fe(out + (size_t)i * NL, fe_from_words_le(w));
    else
      out[i] = words_lt_p(w) ? 1u : 0u;
  } else if constexpr (OP == LOP_TO_WORDS) {
    uint32_t w[8];
    fe_to_words_le(load_fe(a + (size_t)i * NL), w);
#pragma unroll
    for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = w[k];
  } else {
    const fe x = load_fe(a + (size_t)i * NL);
    fe y = fe_zero();
    if constexpr (limb_op_b_words(OP) != 0) y = load_fe(b + (size_t)i * NL);
    fe r;
    if constexpr (OP == LOP_MUL_ALL) r = fe_mul_w<WIDE_ALL>(x, y);
    else if constexpr (OP == LOP_MUL_GH) r = fe_mul_w<WIDE_GH>(x, y);
    else if constexpr (OP == LOP_MUL_EH) r = fe_mul_w<WIDE_EH>(x, y);
    else if constexpr (OP == LOP_MUL_EF) r = fe_mul_w<WIDE_EF>(x, y);
    else if constexpr (OP == LOP_MUL_GHEH) r = fe_mul_w<WIDE_GH & WIDE_EH>(x, y);
    else if constexpr (OP == LOP_MUL_SD_U) r = fe_mul_sd<WIDE_ALL, false>(x, y);
    else if constexpr (OP == LOP_MUL_SD_S) r = fe_mul_sd<WIDE_ALL, true>(x, y);
    else if constexpr (OP == LOP_MUL_2D) r = fe_mul_2d(x);
    else if constexpr (OP == LOP_MUL_D) r = fe_mul_d(x);
    else if constexpr (OP == LOP_SUB) r = fe_sub(x, y);
    else if constexpr (OP == LOP_NEG) r = fe_neg(x);
    else if constexpr (OP == LOP_ADD_N) r = fe_add_n(x, y);
    else if constexpr (OP == LOP_DBL_N) r = fe_dbl_n(x);
    else if constexpr (OP == LOP_TO_STD) r = fe_to_std(x);
    else if constexpr (OP == LOP_TO_HOST_MONT) r = fe_to_host_mont(x);
    else r = fe_inv(x);
    store_fe(out + (size_t)i * NL, r);
  }
}

// pt_add / pt_dbl / pt_madd on raw extended coordinates.  pt_madd's q is a raw record
// (ymx | ypx | kt, 27 limbs) and neg[i] != 0 negates it as k_accumulate's gather does: the halves
// swapped, then kt_neg_if.
template <int OP>
__global__ void k_test_limbs_point(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
                                   const uint32_t* __restrict__ neg, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xyzt P = load_pt(p + (size_t)i * PT_WORDS);
  xyzt R;
  if constexpr (OP == LOP_PT_ADD) {
    R = pt_add(P, load_pt(q + (size_t)i * PT_WORDS));
  } else if constexpr (OP == LOP_PT_DBL) {
    R = pt_dbl(P);
  } else {
    const uint32_t* qs = q + (size_t)i * 3 * NL;
    const bool ng = neg[i] != 0;
    pre qq;
    qq.ymx = load_fe(qs + (ng ? NL : 0));
    qq.ypx = load_fe(qs + (ng ? 0 : NL));
    qq.kt = kt_neg_if(load_fe(qs + 2 * NL), ng);
    R = pt_madd(P, qq);
  }
  store_pt(out + (size_t)i * PT_WORDS, R);
}

// pt_add_quad on raw coordinates: pair i on lanes 4i..4i+3, lane c holding coordinate c, as
// k_test_quad deals them (dead quads of the last wave run on pair 0 and store nothing).
__global__ void k_test_limbs_quad(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
                                  uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 2, c = threadIdx.x & 3;
  const bool live = i < n;
  const uint32_t ii = live ? i : 0;
  const fe a = load_fe(p + (size_t)ii * PT_WORDS + c * NL), b = load_fe(q + (size_t)ii * PT_WORDS + c * NL);
  const fe r = pt_add_quad(a, b);
  if (live) store_fe(out + (size_t)i * PT_WORDS + c * NL, r);
}

// The gather and add of k_accumulate on prepared records: out[j] = acc[j] + record(ents[j]),
// ents[j] = point index << 1 | sign (load_pre_signed).  The host checks every index < n.
__global__ void k_test_limbs_gather(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ents,
                                    const uint32_t* __restrict__ acc, uint32_t* __restrict__ out, uint32_t m) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const pre q = load_pre_signed(pts, ents[j]);
  store_pt(out + (size_t)j * PT_WORDS, pt_madd(load_pt(acc + (size_t)j * PT_WORDS), q));
}

// The functions the per-lane point kernels run (k_shift_bases, k_decompress_x, k_scale_points,
// k_fixed_build) on raw limbs, one element per lane, 64 lanes per workgroup as those kernels have.
// LOP_SHIFT_LANE is k_shift_bases' lane: the record's point rebuilt (pt_from_record), doubled
// b[i] times, and made a record again (record_from_halved) -- the functions the kernel calls.
// Every loop is bounded whatever the operands hold: fe_sqrt_ts' m strictly decreases from 47 and
// its inner loops stop at m, pt_mul_order runs the constant's 251 bits, fe_inv the exponent's 256,
// and the host refuses a LOP_SHIFT_LANE count above LOP_SHIFT_MAX before it launches.
template <int OP>
__global__ void __launch_bounds__(64) k_test_limbs_lane(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                        uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (OP == LOP_SQR) {
    store_fe(out + (size_t)i * NL, fe_sqr(load_fe(a + (size_t)i * NL)));
  } else if constexpr (OP == LOP_STD_NEG) {
    store_fe(out + (size_t)i * NL, fe_std_neg(load_fe(a + (size_t)i * NL)));
  } else if constexpr (OP == LOP_IS_ONE) {
    const fe one = fe_one();
    const fe one_p = fe_add_n(one, fe_const(P29));  // as fe_sqrt_ts makes it
    out[i] = fe_mul_out_is_one(load_fe(a + (size_t)i * NL), one, one_p) ? 1u : 0u;
  } else if constexpr (OP == LOP_SQRT_TS) {
    store_fe(out + (size_t)i * NL, fe_sqrt_ts(load_fe(a + (size_t)i * NL)));
  } else if constexpr (OP == LOP_MUL_ORDER) {
    store_pt(out + (size_t)i * PT_WORDS, pt_mul_order(load_pt(a + (size_t)i * PT_WORDS)));
  } else {
    uint32_t rec[32];
#pragma unroll
    for (int k = 0; k < 32; k++) rec[k] = a[(size_t)i * PRE_WORDS + k];
    xyzt p = pt_from_record(rec);
    if constexpr (OP == LOP_FROM_RECORD) {
      store_pt(out + (size_t)i * PT_WORDS, p);
    } else {
      const uint32_t S = min(b[i], LOP_SHIFT_MAX);
#pragma unroll 1
      for (uint32_t s = 0; s < S; s++) p = pt_dbl(p);
      // x/2 and y/2, as k_shift_bases makes them
      const fe zh = fe_mul(fe_inv(p.Z), fe_const(HALF29));
      record_from_halved(fe_mul(p.X, zh), fe_mul(p.Y, zh), rec);
#pragma unroll
      for (int k = 0; k < 32; k++) out[(size_t)i * PRE_WORDS + k] = rec[k];
    }
  }
}

}  // namespace msm

#include "fr_kernels.cuh"
#include "fr_scan_kernels.cuh"
