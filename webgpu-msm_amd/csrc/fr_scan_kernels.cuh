// The second set of Fr vector kernels (include/msm.h msm_fr_inverse*, msm_fr_scan*, msm_fr_tensor*): batch
// inverses, running products and sums, tensor products of k pairs.  Included by msm_kernels.hip after
// fr_kernels.cuh, whose element forms, loads, stores and R-power rules (a value in form e is v R^e;
// fr_mont_mul adds exponents and takes 1 off) these kernels share; the host side is host_fr_scan.h.
//
// A tile is FR_TILE = FR_THREADS * FR_TILE_E elements, FR_TILE_E contiguous ones per lane.  No kernel here
// waits for another workgroup: a scan is three launches, and the tiles of an inverse are independent.
#pragma once

namespace msm {

// Elements per lane of a tile (k_fr_inverse, k_fr_scan_apply): eight elements of state per lane is 64
// VGPRs; and the most span totals k_fr_scan_totals turns into carries, FR_SCAN_TOTALS per lane.
constexpr uint32_t FR_TILE_E = 8, FR_TILE = FR_THREADS * FR_TILE_E;
constexpr uint32_t FR_SCAN_CAP = 1024, FR_SCAN_TOTALS = FR_SCAN_CAP / FR_THREADS;
// k_fr_scan_*'s operation.
constexpr uint32_t FR_SCAN_OP_SUM = 1, FR_SCAN_OP_EXCLUSIVE = 2;

// f(FrIdx<I>) for I = 0 .. N - 1 by recursion: a lane's FR_TILE_E elements are indexed by constants only, so
// they stay in registers (a `#pragma unroll` over bodies of several products is not always honoured).
template <int I>
struct FrIdx {
  static constexpr int value = I;
};
template <int I, int N, typename F>
__device__ __forceinline__ void fr_static_for(F&& f) {
  if constexpr (I < N) {
    f(FrIdx<I>{});
    fr_static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ FrElem fr_zero() {
  FrElem e;
#pragma unroll
  for (int j = 0; j < 8; j++) e.v[j] = 0;
  return e;
}
__device__ __forceinline__ bool fr_is_zero(const FrElem& e) {
  return (e.v[0] | e.v[1] | e.v[2] | e.v[3] | e.v[4] | e.v[5] | e.v[6] | e.v[7]) == 0;
}
__device__ __forceinline__ FrElem fr_select(bool take, const FrElem& a, const FrElem& b) {
  FrElem o;
#pragma unroll
  for (int j = 0; j < 8; j++) o.v[j] = take ? a.v[j] : b.v[j];
  return o;
}
// An element as the kernels below compute with it: the raw words times R^(k - 1) (k < 0: the words as they
// are, for a canonical Montgomery input).  The raw words are the first operand, so any 256-bit wire
// integer is reduced by the same product.  k is wave-uniform.
__device__ __forceinline__ FrElem fr_take(const FrElem& raw, int k) {
  return k < 0 ? raw : fr_mul(raw, k == 0 ? fr_const(0) : k == 1 ? fr_const(1) : fr_const(2));
}
__device__ __forceinline__ void fr_lds_put(uint32_t* lds, uint32_t stride, uint32_t at, const FrElem& e) {
#pragma unroll
  for (int j = 0; j < 8; j++) lds[j * stride + at] = e.v[j];
}
__device__ __forceinline__ FrElem fr_lds_get(const uint32_t* lds, uint32_t stride, uint32_t at) {
  FrElem e;
#pragma unroll
  for (int j = 0; j < 8; j++) e.v[j] = lds[j * stride + at];
  return e;
}

// ---- inverse -----------------------------------------------------------------------------------------
// out_i = c a_i^-1 mod r for i < m, and 0 where a_i = 0 mod r.  Workgroups stride over tiles; per tile:
//   1. lane t loads its FR_TILE_E elements, moves them to Montgomery form (wire: one product by R^2, which
//      also reduces them; then zero is eight zero words), replaces a zero by 1 with a select, and keeps the
//      running products p_j = a_0 .. a_j: one product per element;
//   2. the 256 lane totals go up a product tree in LDS (node i has children 2 i and 2 i + 1, leaves at
//      FR_THREADS + t, word-major rows): 255 products in eight steps;
//   3. one wave inverts the root -- every lane of it the same fr_inv, 321 dependent products, so no lane
//      diverges; wave tile mod 4, so that the inversions of the workgroups on one compute unit are not all
//      on the same SIMD -- and takes cf = c R^e_out in with one product: the root now holds c / (the tile's
//      product) in the output's form;
//   4. down the tree, inv(left) = inv(parent) right and inv(right) = inv(parent) left: 510 products in
//      eight steps, after which leaf t holds c / (lane t's total) in the output's form;
//   5. lane t walks back: out_j = inv p_(j-1), inv = inv a_j, with a_j read again (the tile was just read:
//      an L2 hit) and moved to Montgomery form again; out_0 = inv.  Two products per element.
// Every product keeps the exponent of `inv` (the other operand is in Montgomery form), so c and the
// output's form cost nothing per element.  A lane has loaded all its elements in step 1 before its first
// store, it stores only its own elements, and in step 5 it reads a_j before it stores out_j and a_(j-1)
// after: `out` may be exactly `a`.  An element past m takes part as 1 and is not stored.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_inverse(const uint32_t* a, uint32_t* out, size_t m, FrElem cf, uint32_t in_form, uint32_t out_form,
                 uint32_t* __restrict__ err) {
  static_assert(FR_THREADS == 4 * 64, "four waves: step 3 picks one by tile mod 4");
  __shared__ uint32_t tree[8 * 2 * FR_THREADS];
  constexpr uint32_t TS = 2 * FR_THREADS;
  const uint32_t l = threadIdx.x;
  const int k_in = in_form == FR_FORM_WIRE ? 2 : -1;
  const size_t ntiles = (m + FR_TILE - 1) / FR_TILE;
  bool bad = false;
#pragma unroll 1
  for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t base = tile * FR_TILE + (size_t)l * FR_TILE_E;
    FrElem p[FR_TILE_E];
    FrElem run = fr_const(1);
    fr_static_for<0, (int)FR_TILE_E>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      FrElem v = fr_const(1);
      if (base + j < m) {
        const FrElem raw = fr_load(a, base + j, in_form);
        bad = bad || fr_bad(raw, in_form);
        v = fr_take(raw, k_in);
        v = fr_select(fr_is_zero(v), fr_const(1), v);
      }
      if constexpr (j == 0) run = v;
      else run = fr_mul(run, v);
      p[j] = run;
    });
    fr_lds_put(tree, TS, FR_THREADS + l, run);
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = FR_THREADS / 2; s >= 1; s >>= 1) {
      if (l < s) {
        const uint32_t i = s + l;
        fr_lds_put(tree, TS, i, fr_mul(fr_lds_get(tree, TS, 2 * i), fr_lds_get(tree, TS, 2 * i + 1)));
      }
      __syncthreads();
    }
    if ((l >> 6) == (uint32_t)(tile & 3u)) {  // one wave, a different one from tile to tile
      FrElem root = fr_lds_get(tree, TS, 1), inv;
      fr_inv(root.v, inv.v);
      inv = fr_mul(inv, cf);
      if ((l & 63u) == 0) fr_lds_put(tree, TS, 1, inv);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 1; s < FR_THREADS; s <<= 1) {
      if (l < s) {
        const uint32_t i = s + l;
        const FrElem pi = fr_lds_get(tree, TS, i), lt = fr_lds_get(tree, TS, 2 * i), rt = fr_lds_get(tree, TS, 2 * i + 1);
        fr_lds_put(tree, TS, 2 * i, fr_mul(pi, rt));
        fr_lds_put(tree, TS, 2 * i + 1, fr_mul(pi, lt));
      }
      __syncthreads();
    }
    FrElem inv = fr_lds_get(tree, TS, FR_THREADS + l);
    __syncthreads();  // the next tile's leaves go where this one's were read
    fr_static_for<0, (int)FR_TILE_E>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = (int)FR_TILE_E - 1 - decltype(jc)::value;
      if (base + j < m) {
        const FrElem v = fr_take(fr_load(a, base + j, in_form), k_in);
        const bool zero = fr_is_zero(v);
        FrElem o = inv;
        if constexpr (j > 0) o = fr_mul(inv, p[j - 1]);
        fr_store(out, base + j, out_form, fr_select(zero, fr_zero(), o));
        if constexpr (j > 0) inv = fr_mul(inv, fr_select(zero, fr_const(1), v));
      }
    });
  }
  if (bad) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
}

// ---- scan --------------------------------------------------------------------------------------------
// The operation of a scan on two elements of one form: a sum, or a Montgomery product, whose second
// operand is in Montgomery form so that the first one's form is kept.
template <bool SUM>
__device__ __forceinline__ FrElem fr_scan_op(const FrElem& a, const FrElem& b) {
  if constexpr (SUM) {
    FrElem o;
    fr_add(a.v, b.v, o.v);
    return o;
  } else {
    return fr_mul(a, b);
  }
}
// The identity among the values lanes scan: 0, or 1 in Montgomery form.
template <bool SUM>
__device__ __forceinline__ FrElem fr_scan_identity() {
  return SUM ? fr_zero() : fr_const(1);
}

// The workgroup's scan of one element per lane through LDS (word-major rows of FR_THREADS, as
// fr_block_sum's): eight doubling steps.  Returns the exclusive prefix of the lane and, in *total, the whole
// workgroup's.  Every word read was written by this call.
template <bool SUM>
__device__ __forceinline__ FrElem fr_block_scan(FrElem v, uint32_t* lds, FrElem* total) {
  const uint32_t l = threadIdx.x;
  fr_lds_put(lds, FR_THREADS, l, v);
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < FR_THREADS; d <<= 1) {
    FrElem o = v;
    if (l >= d) o = fr_lds_get(lds, FR_THREADS, l - d);
    __syncthreads();
    if (l >= d) {
      v = fr_scan_op<SUM>(o, v);
      fr_lds_put(lds, FR_THREADS, l, v);
    }
    __syncthreads();
  }
  *total = fr_lds_get(lds, FR_THREADS, FR_THREADS - 1);
  const FrElem before = l ? fr_lds_get(lds, FR_THREADS, l - 1) : fr_scan_identity<SUM>();
  __syncthreads();  // the caller's next scan writes these rows
  return before;
}

// The workgroup's total of one element per lane, to lane 0: fr_block_sum's halving steps with the scan's
// operation.
template <bool SUM>
__device__ __forceinline__ FrElem fr_block_total(FrElem acc, uint32_t* lds) {
  const uint32_t l = threadIdx.x;
#pragma unroll 1
  for (uint32_t s = FR_THREADS / 2; s >= 1; s >>= 1) {
    if (l >= s && l < 2 * s) fr_lds_put(lds, FR_THREADS, l - s, acc);
    __syncthreads();
    if (l < s) acc = fr_scan_op<SUM>(acc, fr_lds_get(lds, FR_THREADS, l));
    __syncthreads();
  }
  return acc;
}

// A scan's first launch: workgroup b folds its span -- `span` elements from b * span on, a whole number of
// tiles, the last span ragged -- into part[b], the lanes striding over it (the fold's order is free: both
// operations commute and are exact).  Elements are taken with k_load (fr_take): Montgomery form for a
// product, the output's form for a sum.
template <bool SUM>
__device__ __forceinline__ void fr_scan_spans(const uint32_t* __restrict__ a, size_t m, size_t span, uint32_t in_form,
                                              int k_load, uint32_t* __restrict__ part, uint32_t* __restrict__ err,
                                              uint32_t* lds) {
  const size_t lo = (size_t)blockIdx.x * span, hi = lo + span < m ? lo + span : m;
  FrElem acc = fr_scan_identity<SUM>();
  bool bad = false;
#pragma unroll 1
  for (size_t i = lo + threadIdx.x; i < hi; i += FR_THREADS) {
    const FrElem raw = fr_load(a, i, in_form);
    bad = bad || fr_bad(raw, in_form);
    acc = fr_scan_op<SUM>(acc, fr_take(raw, k_load));
  }
  acc = fr_block_total<SUM>(acc, lds);
  if (threadIdx.x == 0) fr_store(part, blockIdx.x, FR_FORM_MONT, acc);
  if (bad) atomicOr(err, MSM_DEV_ERR_SCALAR_RANGE);
}
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_scan_spans(const uint32_t* __restrict__ a, size_t m, size_t span, uint32_t op, uint32_t in_form, int k_load,
                    uint32_t* __restrict__ part, uint32_t* __restrict__ err) {
  __shared__ uint32_t lds[8 * FR_THREADS];
  if (op & FR_SCAN_OP_SUM) fr_scan_spans<true>(a, m, span, in_form, k_load, part, err, lds);
  else fr_scan_spans<false>(a, m, span, in_form, k_load, part, err, lds);
}

// The second launch, one workgroup: the `count` <= FR_SCAN_CAP span totals of part become, in place, the
// carries into the spans -- carry_b = first (x) total_0 (x) .. (x) total_(b-1), with `first` the scan's
// starting value in the output's form (c R^e_out, or 0 for a sum).  Lane t owns totals t FR_SCAN_TOTALS
// .. + FR_SCAN_TOTALS - 1 and loads them all before it stores.
template <bool SUM>
__device__ __forceinline__ void fr_scan_totals(uint32_t* __restrict__ part, uint32_t count, const FrElem& first,
                                               uint32_t* lds) {
  const uint32_t at = threadIdx.x * FR_SCAN_TOTALS;
  FrElem t[FR_SCAN_TOTALS];
  FrElem all = fr_scan_identity<SUM>();
#pragma unroll
  for (int j = 0; j < (int)FR_SCAN_TOTALS; j++) {
    t[j] = at + j < count ? fr_load(part, at + j, FR_FORM_MONT) : fr_scan_identity<SUM>();
    all = j == 0 ? t[0] : fr_scan_op<SUM>(all, t[j]);
  }
  FrElem whole;
  const FrElem before = fr_block_scan<SUM>(all, lds, &whole);
  FrElem run = fr_scan_op<SUM>(first, before);
#pragma unroll
  for (int j = 0; j < (int)FR_SCAN_TOTALS; j++) {
    if (at + j < count) fr_store(part, at + j, FR_FORM_MONT, run);
    run = fr_scan_op<SUM>(run, t[j]);
  }
}
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_scan_totals(uint32_t* __restrict__ part, uint32_t count, uint32_t op, FrElem first) {
  __shared__ uint32_t lds[8 * FR_THREADS];
  if (op & FR_SCAN_OP_SUM) fr_scan_totals<true>(part, count, first, lds);
  else fr_scan_totals<false>(part, count, first, lds);
}

// The third launch: workgroup b goes over its span again tile by tile with the carry part[b].  Lane t loads
// its FR_TILE_E contiguous elements -- all of them before it stores any, and it stores only those, so `out`
// may be exactly `a` --, folds them, the block scan of the 256 lane totals gives what precedes the lane in
// the tile, and the lane runs over its elements once more from carry (x) that: inclusive stores after the
// step, exclusive before it.  The carry is in the output's form and every other operand of a product in
// Montgomery form, so a store converts nothing.  Two operations per element and one per lane.
template <bool SUM>
__device__ __forceinline__ void fr_scan_apply(const uint32_t* a, uint32_t* out, size_t m, size_t span, bool exclusive,
                                              uint32_t in_form, uint32_t out_form, int k_load,
                                              const uint32_t* __restrict__ part, uint32_t* lds) {
  const size_t lo = (size_t)blockIdx.x * span, hi = lo + span < m ? lo + span : m;
  FrElem carry = fr_load(part, blockIdx.x, FR_FORM_MONT);
#pragma unroll 1
  for (size_t tile = lo; tile < hi; tile += FR_TILE) {
    const size_t base = tile + (size_t)threadIdx.x * FR_TILE_E;
    FrElem v[FR_TILE_E];
    FrElem all = fr_scan_identity<SUM>();
    fr_static_for<0, (int)FR_TILE_E>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      v[j] = base + j < hi ? fr_take(fr_load(a, base + j, in_form), k_load) : fr_scan_identity<SUM>();
      if constexpr (j == 0) all = v[0];
      else all = fr_scan_op<SUM>(all, v[j]);
    });
    FrElem whole;
    const FrElem before = fr_block_scan<SUM>(all, lds, &whole);
    FrElem run = fr_scan_op<SUM>(carry, before);
    fr_static_for<0, (int)FR_TILE_E>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      // exclusive: the value before the step (wave-uniform select, one operation either way)
      const FrElem next = fr_scan_op<SUM>(run, v[j]);
      if (base + j < hi) fr_store(out, base + j, out_form, exclusive ? run : next);
      run = next;
    });
    carry = fr_scan_op<SUM>(carry, whole);
  }
}
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_scan_apply(const uint32_t* a, uint32_t* out, size_t m, size_t span, uint32_t op, uint32_t in_form,
                    uint32_t out_form, int k_load, const uint32_t* __restrict__ part) {
  const bool exclusive = op & FR_SCAN_OP_EXCLUSIVE;
  __shared__ uint32_t lds[8 * FR_THREADS];
  if (op & FR_SCAN_OP_SUM) fr_scan_apply<true>(a, out, m, span, exclusive, in_form, out_form, k_load, part, lds);
  else fr_scan_apply<false>(a, out, m, span, exclusive, in_form, out_form, k_load, part, lds);
}

// ---- tensor ------------------------------------------------------------------------------------------
// The arguments of k_fr_tensor: the pairs of the low `tb` bits in Montgomery form, and the products over
// the high k - tb <= 4 bits, which carry c and the output's form (host_fr_scan.h makes them with fr_mont_mul).
constexpr uint32_t FR_TENSOR_MAX_K = 31, FR_TENSOR_MAX_TB = FR_TENSOR_MAX_K - 4;
struct FrTensorArgs {
  FrElem lo[FR_TENSOR_MAX_TB], hi[FR_TENSOR_MAX_TB];
  FrElem high[FR_POW_STEPS];
};
static_assert(FR_POW_STEPS == 16, "the high part of a tensor product is four bits");
static_assert(sizeof(FrTensorArgs) <= 3072, "kernel arguments");

// out_i = c prod_(j<k) (bit_j(i) ? hi_j : lo_j) for i < 2^k, built like k_fr_powers: lane t of the T = 2^tb
// lanes forms the product over the low tb bits, one select and one product per bit (the selects are on the
// lane's bits, the pairs wave-uniform arguments), and stores elements t + u T for u < 2^(k - tb) <=
// FR_POW_STEPS, each one product by high[u].  A wave's stores are 64 consecutive elements.
extern "C" __global__ void __launch_bounds__(FR_THREADS)
    k_fr_tensor(FrTensorArgs ta, uint32_t tb, uint32_t steps, uint32_t* __restrict__ out, uint32_t out_form) {
  const size_t T = (size_t)1 << tb;
  const size_t t = (size_t)blockIdx.x * FR_THREADS + threadIdx.x;
  if (t >= T) return;
  FrElem p = fr_const(1);
#pragma unroll 1
  for (uint32_t j = 0; j < tb; j++) {
    const FrElem f = fr_select((t >> j) & 1u, ta.hi[j], ta.lo[j]);
    p = j == 0 ? f : fr_mul(p, f);
  }
#pragma unroll 1
  for (uint32_t u = 0; u < steps; u++) fr_store(out, t + (size_t)u * T, out_form, fr_mul(p, ta.high[u]));
}

}  // namespace msm
