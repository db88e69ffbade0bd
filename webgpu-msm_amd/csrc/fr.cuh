// The scalar field Fr of ark-ed-on-bls12-377 (the order r of the curve's prime subgroup): r, -r^-1 mod
// 2^32, the canonical test a < r and the conversion out of Montgomery form, v = a 2^-256 mod r, which
// the wide scalar types need (include/msm.h MSM_FIELD_FR_MONT); and below them the arithmetic mod r of
// the Fr vector entries (msm_fr_*): Montgomery product, sum, difference, conversion into Montgomery
// form, inverse.  Host and device run this one code: the host entries' range checks (host_bases.h,
// host_fr.h), the kernels (k_recode_wide, fr_kernels.cuh, fr_scan_kernels.cuh) and the test hooks.
// Values are 8 x uint32, LITTLE-endian words (index 0 least significant): the memory of an arkworks
// Fr -- four little-endian u64 limbs -- read as words on a little-endian machine.
#pragma once
#include <stdint.h>

namespace msm {

struct FrWords {
  uint32_t v[8];
};
// r = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff, 251 bits
constexpr FrWords fr_modulus() {
  return FrWords{{0xc33fd9ffu, 0xb95aee9au, 0xc43c8afeu, 0x5293a3afu, 0x970dec00u, 0x982d1347u, 0xa68b2955u,
                  0x04aad957u}};
}
constexpr uint32_t FR_BITS = 251;
constexpr uint32_t FR_NINV32 = 0x70e3da01u;  // -r^-1 mod 2^32
static_assert((uint32_t)(fr_modulus().v[0] * FR_NINV32) == 0xffffffffu, "r * (-r^-1) = -1 mod 2^32");

// a < r
__host__ __device__ inline bool fr_is_canonical(const uint32_t a[8]) {
  constexpr FrWords R = fr_modulus();
  // the top word decides all but one value in 2^27 (the host's scan of 2^20 elements is then a
  // compare per element, bound by reading them)
  if (a[7] != R.v[7]) return a[7] < R.v[7];
  // the borrow out of a - r
  uint32_t borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)a[k] - R.v[k] - borrow;
    borrow = (uint32_t)(x >> 32) & 1u;
  }
  return borrow != 0;
}

// out = a 2^-256 mod r for any a < 2^256 (canonical output, out < r): eight rounds of word REDC -- m =
// t_0 (-r^-1) mod 2^32, t = (t + m r) / 2^32, each limb one 32 x 32 + 32 + 32 -> 64-bit multiply-add
// (v_mad_u64_u32 on the device) -- then one conditional subtract.  t stays below 2^256 throughout (t' <
// t / 2^32 + r), and after the eighth round t < a / 2^256 + r <= r, so one subtract reduces it.
// `out` may alias `a`.
__host__ __device__ inline void fr_from_mont(const uint32_t a[8], uint32_t out[8]) {
  constexpr FrWords R = fr_modulus();
  uint32_t t[8];
#pragma unroll
  for (int k = 0; k < 8; k++) t[k] = a[k];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t m = t[0] * FR_NINV32;
    uint64_t x = (uint64_t)m * R.v[0] + t[0];  // low word 0 by the choice of m
    uint32_t carry = (uint32_t)(x >> 32);
#pragma unroll
    for (int j = 1; j < 8; j++) {
      x = (uint64_t)m * R.v[j] + t[j] + carry;
      t[j - 1] = (uint32_t)x;
      carry = (uint32_t)(x >> 32);
    }
    t[7] = carry;
  }
  // t - r where t >= r
  uint32_t d[8], borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)t[k] - R.v[k] - borrow;
    d[k] = (uint32_t)x;
    borrow = (uint32_t)(x >> 32) & 1u;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = borrow ? t[k] : d[k];
}

// ---- arithmetic mod r (the Fr vector entries, include/msm.h msm_fr_*) -------------------------------
// 2^(256 k) mod r for k = 0..3: 1, R, R^2 (fr_to_mont's factor) and R^3.  A Montgomery product by R^k
// moves a value by k - 1 powers of R, which is how the kernels pass between the two element forms
// without a multiply of their own (fr_kernels.cuh fr_fix_power).  tests/test_fr_host.py recomputes the
// four from r.
constexpr FrWords fr_r_power(int k) {
  return k == 0   ? FrWords{{1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}}
         : k == 1 ? FrWords{{0xd0880436u, 0xe6d1ab5au, 0x9b3aae44u, 0x94db78ecu, 0x231037eeu, 0xe67deee6u, 0xdea547f1u,
                             0x03f62782u}}
         : k == 2 ? FrWords{{0x6a55d45eu, 0x375699cdu, 0x7a73da73u, 0xf639c3f5u, 0xcd027a21u, 0xca06049cu, 0xef02d841u,
                             0x047ada1eu}}
                  : FrWords{{0x28b07941u, 0x396270fbu, 0x026e0036u, 0x3b23b94bu, 0x19ca327fu, 0x4e5c47e5u, 0xb70a96c4u,
                             0x02b65b12u}};
}

// out = t - r where t >= r, else t: canonical for any t < 2 r.  `out` may alias `t`.
__host__ __device__ inline void fr_reduce_once(const uint32_t t[8], uint32_t out[8]) {
  constexpr FrWords R = fr_modulus();
  uint32_t d[8], borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)t[k] - R.v[k] - borrow;
    d[k] = (uint32_t)x;
    borrow = (uint32_t)(x >> 32) & 1u;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = borrow ? t[k] : d[k];
}

// out = a b 2^-256 mod r for any a < 2^256 and b < r (canonical output): eight rounds of word CIOS --
// t += a_i b, then m = t_0 (-r^-1) mod 2^32 and t = (t + m r) / 2^32, each limb one 32 x 32 + 32 + 32 ->
// 64-bit multiply-add (v_mad_u64_u32 on the device) -- then one conditional subtract.  With t < b + r
// before a round, t' = (t + a_i b + m r) / 2^32 < (b + r + (2^32 - 1)(b + r)) / 2^32 = b + r after it, so t
// stays below 2 r < 2^252 between rounds: the ninth word is zero there and holds only the carry of the
// first loop (t + a_i b < 2^32 (b + r) < 2^284).  After the eighth round t = (a b + m r) / 2^256 < b + r
// < 2 r, so one subtract reduces it.  `out` may alias `a` or `b`.
__host__ __device__ inline void fr_mont_mul(const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
  constexpr FrWords R = fr_modulus();
  uint32_t t[9];
#pragma unroll
  for (int k = 0; k < 9; k++) t[k] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t ai = a[i];
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t x = (uint64_t)ai * b[j] + t[j] + carry;
      t[j] = (uint32_t)x;
      carry = (uint32_t)(x >> 32);
    }
    t[8] = carry;
    const uint32_t m = t[0] * FR_NINV32;
    uint64_t x = (uint64_t)m * R.v[0] + t[0];  // low word 0 by the choice of m
    carry = (uint32_t)(x >> 32);
#pragma unroll
    for (int j = 1; j < 8; j++) {
      x = (uint64_t)m * R.v[j] + t[j] + carry;
      t[j - 1] = (uint32_t)x;
      carry = (uint32_t)(x >> 32);
    }
    t[7] = t[8] + carry;  // t' < 2^252: no carry out of this word
  }
  fr_reduce_once(t, out);
}

// out = a + b mod r and out = a - b mod r: canonical in, canonical out (a + b < 2 r < 2^252 carries out of
// no word; a - b + r where a < b).  `out` may alias either operand.
__host__ __device__ inline void fr_add(const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
  uint32_t s[8], carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)a[k] + b[k] + carry;
    s[k] = (uint32_t)x;
    carry = (uint32_t)(x >> 32);
  }
  fr_reduce_once(s, out);
}
__host__ __device__ inline void fr_sub(const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
  constexpr FrWords R = fr_modulus();
  uint32_t d[8], borrow = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)a[k] - b[k] - borrow;
    d[k] = (uint32_t)x;
    borrow = (uint32_t)(x >> 32) & 1u;
  }
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint64_t x = (uint64_t)d[k] + (borrow ? R.v[k] : 0u) + carry;
    out[k] = (uint32_t)x;
    carry = (uint32_t)(x >> 32);
  }
}

// out = a 2^256 mod r for any a < 2^256 (canonical output): the Montgomery form of a's residue, and with
// fr_from_mont after it the reduction of any 256-bit integer mod r.  `out` may alias `a`.
__host__ __device__ inline void fr_to_mont(const uint32_t a[8], uint32_t out[8]) {
  constexpr FrWords R2 = fr_r_power(2);
  fr_mont_mul(a, R2.v, out);
}

// Word k of the constant exponent r - 2, as selects on k (no table in memory: k is uniform in a kernel).
__host__ __device__ inline uint32_t fr_inv_exp_word(int k) {
  constexpr FrWords R = fr_modulus();
  static_assert(R.v[0] >= 2, "r - 2 borrows from no word");
  return k == 0 ? R.v[0] - 2u : k == 1 ? R.v[1] : k == 2 ? R.v[2] : k == 3 ? R.v[3] : k == 4 ? R.v[4] : k == 5 ? R.v[5]
         : k == 6 ? R.v[6] : R.v[7];
}
// The products of one fr_inv: 62 windows of four squarings and tab[2] = a^2; tab[3..15] and one product per
// non-zero window below the top one (three of the 62 nibbles of r - 2 are zero).
constexpr uint32_t FR_INV_SQUARINGS = 62 * 4 + 1, FR_INV_PRODUCTS = 13 + 59;

// tab[e] = a^e for e = 2 .. E from tab[1] = a, by recursion: every index is a constant, so the table of a
// kernel stays in registers whatever the unroller makes of a loop this large.
template <int E>
__host__ __device__ inline __attribute__((always_inline)) void fr_inv_table(uint32_t (&tab)[16][8]) {
  if constexpr (E > 2) fr_inv_table<E - 1>(tab);
  fr_mont_mul(tab[E - 1], tab[1], tab[E]);
}

// out = a^-1 for a < r in Montgomery form, in Montgomery form (a^-1 2^256 mod r), and 0 for a = 0: a^(r - 2)
// by a fixed 4-bit window over the constant exponent, top nibble first -- the table a^1 .. a^15, then per
// nibble four squarings and, where the nibble is not zero, one product by its table entry, which is read
// with selects (no indexed private memory).  The chain is FR_INV_SQUARINGS + FR_INV_PRODUCTS = 321
// dependent fr_mont_mul long; every branch is on the exponent, none on a, so lanes never diverge.
// `out` may alias `a`.
__host__ __device__ inline void fr_inv(const uint32_t a[8], uint32_t out[8]) {
  constexpr FrWords R = fr_modulus();
  constexpr uint32_t top = R.v[7] >> 24;  // nibble 62 of r - 2; nibble 63 is zero
  static_assert(top >= 1 && top < 16, "r has 63 nibbles");
  uint32_t tab[16][8];
#pragma unroll
  for (int j = 0; j < 8; j++) tab[1][j] = a[j];
  fr_inv_table<15>(tab);
  uint32_t acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j] = tab[top][j];
#pragma unroll 1
  for (int i = 61; i >= 0; i--) {
#pragma unroll 1
    for (int s = 0; s < 4; s++) fr_mont_mul(acc, acc, acc);
    const uint32_t w = (fr_inv_exp_word(i >> 3) >> (4 * (i & 7))) & 15u;
    if (w) {
      uint32_t x[8];
#pragma unroll
      for (int j = 0; j < 8; j++) x[j] = tab[1][j];
#pragma unroll
      for (int e = 2; e < 16; e++) {
        const bool take = w == (uint32_t)e;
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = take ? tab[e][j] : x[j];
      }
      fr_mont_mul(acc, x, acc);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = acc[j];
}

}  // namespace msm
