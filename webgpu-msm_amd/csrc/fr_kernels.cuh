// The Fr vector kernels (include/msm.h msm_fr_*): elementwise x_i a_i +- y_i b_i, powers c g^i and inner
// products mod r, on fr.cuh's word arithmetic.  Included by msm_kernels.hip; the host side is host_fr.h.
//
// Elements are 32 bytes in one of two forms (FR_FORM_*, the header's MSM_FR_*): wire -- 8 big-endian u32
// words, any integer < 2^256 read as its residue -- and mont -- the little-endian memory of an arkworks
// Fr, a 2^256 mod r, which must be canonical (a >= r raises MSM_DEV_ERR_SCALAR_RANGE, the launch runs to
// its end and never reads out of range).  A lane holds an element as 8 little-endian words and moves it
// with two 16-byte loads or stores.  Everything kept or stored is canonical.
//
// Forms cost no multiply of their own.  Write e = 0 for wire and 1 for mont, so a value v in form e is
// v R^e (R = 2^256); fr_mont_mul adds its operands' exponents and takes 1 off.  A term x a therefore
// becomes mont_mul(a, mont_mul(x, R^k)) with k = e_out - 2 e_in + 2, and a term without a multiplier
// mont_mul(a, R^k) with k = e_out - e_in + 1: the first operand of fr_mont_mul may be any 256-bit integer,
// so wire inputs are reduced on the way, and the second is a constant or a product, canonical either way.
// k = 1 is a product by R, the identity on canonical values, and is skipped.
#pragma once

namespace msm {

constexpr uint32_t FR_FORM_WIRE = 0, FR_FORM_MONT = 1;
constexpr uint32_t FR_THREADS = 256;
// k_fr_combine's grid cap (lanes stride over the rest), k_fr_dot_partial's -- the most partials the
// second stage sums --, and the elements one lane of k_fr_powers steps through.
constexpr uint32_t FR_COMBINE_CAP = 4096, FR_DOT_CAP = 1024, FR_POW_STEPS = 16;
// k_fr_combine's operand modes, two bits each in `shape`: x at bit 0, y at bit 2; then the flags.
constexpr uint32_t FR_OP_NONE = 0, FR_OP_BCAST = 1, FR_OP_EACH = 2;
constexpr uint32_t FR_SHAPE_B = 16, FR_SHAPE_SUB = 32;

struct FrElem {
  uint32_t v[8];  // little-endian words
};

__device__ __forceinline__ FrElem fr_const(int k) {
  const FrWords c = k == 0 ? fr_r_power(0) : k == 1 ? fr_r_power(1) : k == 2 ? fr_r_power(2) : fr_r_power(3);
  FrElem e;
#pragma unroll
  for (int j = 0; j < 8; j++) e.v[j] = c.v[j];
  return e;
}
// Element i of a vector, as two 16-byte loads; and its store.  Wire: word 0 is the most significant.
__device__ __forceinline__ FrElem fr_load(const uint32_t* __restrict__ p, size_t i, uint32_t form) {
  const uint4 lo = reinterpret_cast<const uint4*>(p)[2 * i], hi = reinterpret_cast<const uint4*>(p)[2 * i + 1];
  FrElem e;
  if (form == FR_FORM_WIRE) {
    e.v[7] = lo.x, e.v[6] = lo.y, e.v[5] = lo.z, e.v[4] = lo.w;
    e.v[3] = hi.x, e.v[2] = hi.y, e.v[1] = hi.z, e.v[0] = hi.w;
  } else {
    e.v[0] = lo.x, e.v[1] = lo.y, e.v[2] = lo.z, e.v[3] = lo.w;
    e.v[4] = hi.x, e.v[5] = hi.y, e.v[6] = hi.z, e.v[7] = hi.w;
  }
  return e;
}
__device__ __forceinline__ void fr_store(uint32_t* __restrict__ p, size_t i, uint32_t form, const FrElem& e) {
  uint4 lo, hi;
  if (form == FR_FORM_WIRE) {
    lo = make_uint4(e.v[7], e.v[6], e.v[5], e.v[4]);
    hi = make_uint4(e.v[3], e.v[2], e.v[1], e.v[0]);
  } else {
    lo = make_uint4(e.v[0], e.v[1], e.v[2], e.v[3]);
    hi = make_uint4(e.v[4], e.v[5], e.v[6], e.v[7]);
  }
  reinterpret_cast<uint4*>(p)[2 * i] = lo;
  reinterpret_cast<uint4*>(p)[2 * i + 1] = hi;
}
__device__ __forceinline__ FrElem fr_mul(const FrElem& a, const FrElem& b) {
  FrElem o;
  fr_mont_mul(a.v, b.v, o.v);
  return o;
}
// A mont-form input that is not canonical.
__device__ __forceinline__ bool fr_bad(const FrElem& e, uint32_t form) { return form == FR_FORM_MONT && !fr_is_canonical(e.v); }
// a R^(k-1): one product by the constant R^k, none for k = 1.  k is wave-uniform.
__device__ __forceinline__ FrElem fr_fix_power(const FrElem& a, int k) {
  return k == 1 ? a : fr_mul(a, k == 0 ? fr_const(0) : k == 2 ? fr_const(2) : fr_const(3));
}

// out_i = x_i a_i +- y_i b_i mod r for i < m.  `shape` says which operands there are (FR_OP_* of x and
// of y, FR_SHAPE_B, FR_SHAPE_SUB) and is the same for every lane, so each branch on it is wave-uniform;
// a broadcast multiplier is fixed up once per lane, ahead of the loop.  A lane loads every operand of
// its element before the first multiply and stores after the last, so `out` may be `a` or `b`.
// The grid is at most FR_COMBINE_CAP workgroups; lanes stride over the rest.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_combine(const uint32_t* a, const uint32_t* b, const uint32_t* __restrict__ x,
                 const uint32_t* __restrict__ y, uint32_t* out, size_t m, uint32_t shape, uint32_t in_form,
                 uint32_t out_form, uint32_t* __restrict__ err) {
  const uint32_t xm = shape & 3u, ym = (shape >> 2) & 3u;
  const bool has_b = shape & FR_SHAPE_B, sub = shape & FR_SHAPE_SUB;
  const int k_mul = (int)out_form - 2 * (int)in_form + 2, k_one = (int)out_form - (int)in_form + 1;
  // mont to mont without a multiplier: the product by R is the identity on a canonical value (a wire
  // value may be any 256-bit integer, and the same product reduces it)
  const bool copy = in_form == FR_FORM_MONT && out_form == FR_FORM_MONT;
  bool bad = false;
  // the second operand of each term's product when it is the same for every element
  FrElem fx = fr_const(k_one), fy = fx;
  if (xm == FR_OP_BCAST) {
    const FrElem v = fr_load(x, 0, in_form);
    bad = bad || fr_bad(v, in_form);
    fx = fr_fix_power(v, k_mul);
  }
  if (ym == FR_OP_BCAST) {
    const FrElem v = fr_load(y, 0, in_form);
    bad = bad || fr_bad(v, in_form);
    fy = fr_fix_power(v, k_mul);
  }
  const size_t stride = (size_t)gridDim.x * FR_THREADS;
  for (size_t i = (size_t)blockIdx.x * FR_THREADS + threadIdx.x; i < m; i += stride) {
    // every load of the element ahead of the multiplies
    const FrElem av = fr_load(a, i, in_form);
    FrElem bv = av, xv = fx, yv = fy;
    if (has_b) bv = fr_load(b, i, in_form);
    if (xm == FR_OP_EACH) xv = fr_load(x, i, in_form);
    if (ym == FR_OP_EACH) yv = fr_load(y, i, in_form);
    bad = bad || fr_bad(av, in_form) || fr_bad(bv, in_form);
    if (xm == FR_OP_EACH) {
      bad = bad || fr_bad(xv, in_form);
      xv = fr_fix_power(xv, k_mul);
    }
    if (ym == FR_OP_EACH) {
      bad = bad || fr_bad(yv, in_form);
      yv = fr_fix_power(yv, k_mul);
    }
    FrElem r = xm == FR_OP_NONE && copy ? av : fr_mul(av, xv);
    if (has_b) {
      const FrElem t = ym == FR_OP_NONE && copy ? bv : fr_mul(bv, yv);
      if (sub) fr_sub(r.v, t.v, r.v);
      else fr_add(r.v, t.v, r.v);
    }
    fr_store(out, i, out_form, r);
  }
  if (bad) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
}

// out_i = c g^i mod r for i < n.  Lane t of the T = gridDim.x FR_THREADS lanes reaches g^t by
// square-and-multiply over the bits of t below `tbits` (T <= 2^tbits), takes c in with one product and
// then steps by g^T: elements t, t + T, ..., at most FR_POW_STEPS of them (the host sizes the grid), so a
// lane's chain of dependent products is 2 tbits + 1 + FR_POW_STEPS long and a wave's stores are 64
// consecutive elements.  g and gT are in Montgomery form, cf is c R^e_out; the running value carries
// the output's form, so a step is one product and the store converts nothing.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_powers(FrElem g, FrElem gT, FrElem cf, uint32_t tbits, uint32_t* __restrict__ out, size_t n, uint32_t out_form) {
  const uint32_t t = blockIdx.x * FR_THREADS + threadIdx.x;
  FrElem p = fr_const(1);  // 1 in Montgomery form
#pragma unroll 1
  for (int bit = (int)tbits - 1; bit >= 0; bit--) {
    p = fr_mul(p, p);
    const FrElem pg = fr_mul(p, g);
    const bool take = (t >> bit) & 1u;
#pragma unroll
    for (int j = 0; j < 8; j++) p.v[j] = take ? pg.v[j] : p.v[j];
  }
  FrElem v = fr_mul(p, cf);
  const size_t T = (size_t)gridDim.x * FR_THREADS;
#pragma unroll 1
  for (size_t i = t; i < n; i += T) {
    fr_store(out, i, out_form, v);
    v = fr_mul(v, gT);
  }
}

// The workgroup's sum of one element per lane, through LDS (word-major rows of FR_THREADS, so a step's
// reads are conflict-free): eight halving steps of fr_add.  Lane 0 returns the sum.
__device__ __forceinline__ FrElem fr_block_sum(FrElem acc, uint32_t (*lds)[FR_THREADS]) {
  const uint32_t l = threadIdx.x;
#pragma unroll 1
  for (uint32_t s = FR_THREADS / 2; s >= 1; s >>= 1) {
    if (l >= s && l < 2 * s) {
#pragma unroll
      for (int j = 0; j < 8; j++) lds[j][l - s] = acc.v[j];
    }
    __syncthreads();
    if (l < s) {
      FrElem o;
#pragma unroll
      for (int j = 0; j < 8; j++) o.v[j] = lds[j][l];
      fr_add(acc.v, o.v, acc.v);
    }
    __syncthreads();
  }
  return acc;
}

// The inner product's first stage: part[blockIdx.x] = sum over the workgroup's lanes of sum_i a_i b_i (b
// null: a_i), the lanes striding over n; at most FR_DOT_CAP workgroups.  The sums carry the input's form:
// a wire product is a_i (b_i R) / R, a mont one (a_i R)(b_i R) / R, and a lone wire a_i is reduced by a
// product by R.  Partials are 8 little-endian words each.  No atomics: the sum is exact, so its order is free.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_dot_partial(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t n, uint32_t in_form,
                     uint32_t* __restrict__ part, uint32_t* __restrict__ err) {
  __shared__ uint32_t lds[8][FR_THREADS];
  FrElem acc;
#pragma unroll
  for (int j = 0; j < 8; j++) acc.v[j] = 0;
  bool bad = false;
  const size_t stride = (size_t)gridDim.x * FR_THREADS;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * FR_THREADS + threadIdx.x; i < n; i += stride) {
    FrElem av = fr_load(a, i, in_form);
    bad = bad || fr_bad(av, in_form);
    if (b) {
      FrElem bv = fr_load(b, i, in_form);
      bad = bad || fr_bad(bv, in_form);
      if (in_form == FR_FORM_WIRE) bv = fr_mul(bv, fr_const(2));
      av = fr_mul(av, bv);
    } else if (in_form == FR_FORM_WIRE) {
      av = fr_mul(av, fr_const(1));
    }
    fr_add(acc.v, av.v, acc.v);
  }
  acc = fr_block_sum(acc, lds);
  if (threadIdx.x == 0) fr_store(part, blockIdx.x, FR_FORM_MONT, acc);
  if (bad) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
}

// The second stage, one workgroup: the sum of the `count` partials, moved from the input's form to the
// output's (fr_fix_power) and stored as element `count` of the same buffer, in the output's layout.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_dot_final(uint32_t* __restrict__ part, uint32_t count, uint32_t in_form, uint32_t out_form) {
  __shared__ uint32_t lds[8][FR_THREADS];
  FrElem acc;
#pragma unroll
  for (int j = 0; j < 8; j++) acc.v[j] = 0;
#pragma unroll 1
  for (uint32_t i = threadIdx.x; i < count; i += FR_THREADS) {
    const FrElem v = fr_load(part, i, FR_FORM_MONT);
    fr_add(acc.v, v.v, acc.v);
  }
  acc = fr_block_sum(acc, lds);
  if (threadIdx.x == 0) fr_store(part, count, out_form, fr_fix_power(acc, (int)out_form - (int)in_form + 1));
}

}  // namespace msm
