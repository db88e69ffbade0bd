// The scalar field Fr of ark-ed-on-bls12-377 (the order r of the curve's prime subgroup), as far as the
// wide scalar types need it (include/msm.h MSM_FIELD_FR_MONT): r, -r^-1 mod 2^32, the canonical test
// a < r and the conversion out of Montgomery form, v = a 2^-256 mod r.  Host and device run this one
// code: the host entries' range check (host_bases.h), the recode kernel (k_recode_wide) and the test hook.
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

}  // namespace msm
