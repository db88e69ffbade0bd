// Layer 12, the msm_test_* hooks (not in msm.h) and their helpers.  Included last: it may use every layer,
// and only msm_shutdown (stopping the hooks' pools) uses it.
#pragma once
namespace {

// Pools the CPU test hooks start (msm_test_pack, msm_test_pools), stopped by msm_shutdown too.
struct TestPools {
  PackPool* packer = nullptr;
  TailCrew* crew = nullptr;
  HornerPool* pool = nullptr;
  void stop() {
    delete packer;
    delete crew;
    delete pool;
    packer = nullptr;
    crew = nullptr;
    pool = nullptr;
  }
};
std::mutex g_test_mu;
TestPools g_test_pools;

// ---- helpers of the device test hooks (msm_test_field_op .. msm_test_records) -------------------
// A device buffer of one hook call: freed when the call returns, on its HIPCHECK exits too.
struct TestBuf {
  uint32_t* p = nullptr;
  TestBuf() = default;
  TestBuf(const TestBuf&) = delete;
  TestBuf& operator=(const TestBuf&) = delete;
  ~TestBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

// One k_test_limbs* instantiation per LimbOp (msm_kernels.hip), picked by the runtime op.
template <int OP>
void launch_limb_op(const uint32_t* a, const uint32_t* b, const uint32_t* neg, uint32_t* out, uint32_t n) {
  const dim3 g(grid_for(n, 256)), t(256);
  if constexpr (OP == LOP_PT_QUAD)
    hipLaunchKernelGGL(k_test_limbs_quad, dim3(grid_for(4 * (size_t)n, 256)), t, 0, 0, a, b, out, n);
  else if constexpr (OP >= LOP_SQR)
    hipLaunchKernelGGL(k_test_limbs_lane<OP>, dim3(grid_for(n, 64)), dim3(64), 0, 0, a, b, out, n);
  else if constexpr (OP >= LOP_PT_ADD)
    hipLaunchKernelGGL(k_test_limbs_point<OP>, g, t, 0, 0, a, b, neg, out, n);
  else
    hipLaunchKernelGGL(k_test_limbs<OP>, g, t, 0, 0, a, b, out, n);
}
template <int... OPS>
void dispatch_limb_op(int op, std::integer_sequence<int, OPS...>, const uint32_t* a, const uint32_t* b,
                      const uint32_t* neg, uint32_t* out, uint32_t n) {
  ((op == OPS ? launch_limb_op<OPS>(a, b, neg, out, n) : (void)0), ...);
}

// `fn(ctx)` on the context of `device`, or on every context there is for device < 0 (none is created),
// each under its lock, with its device current and its streams drained.
template <typename F>
int guard_each_ctx(int device, F&& fn) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (DevCtx* c : g_ctx) {
    if (!c || (device >= 0 && c->device != device)) continue;
    std::lock_guard<std::mutex> lk2(c->mu);
    DeviceGuard g(c->device);
    bool ok = true;
    c->each_stream([&](hipStream_t* s) { ok = ok && hipStreamSynchronize(*s) == hipSuccess; });
    if (!ok) return MSM_ERR_HIP;
    if (int rc = fn(c)) return rc;
  }
  return MSM_OK;
}

// A device field element's 9 limbs (value sum_k v_k 2^(29 k), whatever representative the kernel
// stored) as an Fq, by Horner over hostfield's loader and multiply.  The device's Montgomery factor
// 2^261 stays in: it cancels in an affine ratio.
msmh::Fq fq_from_limbs29(const uint32_t* v) {
  const uint64_t radix[4] = {1ull << 29, 0, 0, 0};
  const msmh::Fq r29 = msmh::fq_from_std(radix);
  msmh::Fq acc = msmh::fq_zero();
  for (int k = 8; k >= 0; k--) {
    const uint64_t limb[4] = {v[k], 0, 0, 0};
    acc = msmh::fq_add(msmh::fq_mul(acc, r29), msmh::fq_from_std(limb));
  }
  return acc;
}
// A stored extended point (store_pt: X | Y | T | Z, 9 limbs each) -> affine x | y, 8 BE words each,
// through the tail's inversion (pt_to_affine_std).
void limbs_point_to_xy_be(const uint32_t* rec, uint32_t* xy_be) {
  msmh::Pt p{fq_from_limbs29(rec), fq_from_limbs29(rec + 9), fq_from_limbs29(rec + 18), fq_from_limbs29(rec + 27)};
  uint64_t x[4], y[4];
  msmh::pt_to_affine_std(p, x, y);
  msmh::std_to_be_words(x, xy_be);
  msmh::std_to_be_words(y, xy_be + 8);
}

}  // namespace

extern "C" {

// ---- test hooks (not in msm.h) ----
// The device-list shard split (tests/test_host_logic.py checks it against msm_amd.dist).
int msm_test_shard_range(size_t n, size_t i, size_t D, size_t* lo, size_t* hi) {
  if (!lo || !hi || D == 0 || i >= D) return MSM_ERR_INVALID_ARG;
  shard_range(n, i, D, lo, hi);
  return MSM_OK;
}

// The sharded paths with a list that may repeat a device (the one-GPU box has no second device):
// mode 0 = msm_compute (host inputs), 1 = msm_compute_device; affine result.
int msm_test_sharded(int mode, const uint32_t* points, const uint32_t* scalars, size_t n, const msm_opts* opts,
                     const int32_t* devices, uint32_t n_devices, void* hip_stream, uint32_t out_xy_be[16]) {
  if (!opts || !devices || !n_devices || n_devices > MSM_MAX_DEVICES || !out_xy_be) return MSM_ERR_INVALID_ARG;
  std::vector<int> devs(devices, devices + n_devices);
  for (int d : devs) {
    DevCtx* c;
    if (int rc = get_ctx(d, &c)) return rc;
  }
  Pt r;
  const int rc = mode == 0 ? sharded_host(points, scalars, n, opts, devs, &r)
                           : sharded_device(points, scalars, n, opts, hip_stream, devs, &r);
  if (rc != MSM_OK) return rc;
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

// Peer access of device `dev` to `owner` (enabled on first use, as peer_shard does): 1 enabled
// (or dev == owner), 0 unavailable, MSM_ERR_INVALID_ARG for a non-gfx950 ordinal.
int msm_test_peer_state(int dev, int owner) {
  DevCtx *a, *b;
  if (get_ctx(dev, &a) != MSM_OK || get_ctx(owner, &b) != MSM_OK) return MSM_ERR_INVALID_ARG;
  DeviceGuard g(dev);
  return enable_peer(dev, owner);
}

// The host tail of a lone MSM of n points (auto plan) on caller-supplied window terms (host
// Montgomery X|Y|T|Z words, the layout k_bucket_reduce_2 writes): helpers = 0 runs horner_tail,
// otherwise the TailCrew.  Affine result; *ms = the tail's wall time.
// helpers < 0: one crew of -helpers threads over 40 rounds (the persistent crew of a device
// context), every third round armed and disarmed without terms first (an error return); the
// result of the last round, MSM_ERR_INVALID_ARG if any round disagrees with the first.
int msm_test_tail(size_t n, const uint32_t* terms, int helpers, uint32_t out_xy_be[16], double* ms) {
  Plan pl;
  if (int rc = make_plan(n, nullptr, DevShape{}, &pl)) return rc;
  const int rounds = helpers < 0 ? 40 : 1;
  TailCrew crew(helpers < 0 ? -helpers : helpers);
  Pt first{}, r{};
  bool same = true;
  const auto t0 = clk::now();
  for (int k = 0; k < rounds; k++) {
    if (helpers < 0 && k % 3 == 1) {
      crew.arm();
      crew.disarm();
    }
    crew.arm();
    r = helpers ? crew.run(pl, terms) : horner_tail(pl, terms);
    crew.disarm();
    if (k == 0) first = r;
    same = same && fq_eq(fq_mul(r.X, first.Z), fq_mul(first.X, r.Z)) && fq_eq(fq_mul(r.Y, first.Z), fq_mul(first.Y, r.Z));
  }
  *ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count() / rounds;
  pt_to_be_affine(r, out_xy_be);
  return same ? MSM_OK : MSM_ERR_INVALID_ARG;
}

// Host field / curve timings (ns per operation, dependent chains): what 0 = fq_mul, 1 = one
// doubling of pt_dbl_n, 2 = pt_add, 3 = fq_inv.  For sizing the host tail.
int msm_test_host_timing(int what, size_t iters, double* ns) {
  if (!ns || iters == 0 || what < 0 || what > 4) return MSM_ERR_INVALID_ARG;
  if (what == 4) {  // self-check: binary-Euclid fq_inv against a^(p-2) on iters pseudo-random a
    uint64_t st = 0x9E3779B97F4A7C15ull, bad = 0;
    for (size_t i = 0; i < iters; i++) {
      uint64_t s[4];
      for (int j = 0; j < 4; j++) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        s[j] = st ^ (st >> 29);
      }
      s[3] &= (i & 1) ? 0x0fffffffffffffffull : 0x000000000000ffffull;  // full-width and short
      if (i == 0) s[0] = 1, s[1] = s[2] = s[3] = 0;
      if (i == 1) s[0] = P[0] - 1, s[1] = P[1], s[2] = P[2], s[3] = P[3];
      const Fq a = fq_from_std(s);
      const Fq x = fq_inv(a);
      bad += !fq_eq(x, fq_inv_pow(a)) || !fq_eq(fq_mul(x, a), fq_one());
    }
    bad += !fq_is_zero(fq_inv(fq_zero()));
    *ns = (double)bad;
    return MSM_OK;
  }
  Pt p = pt_identity();
  p.X = fq_one();
  p.Y = fq_add(fq_one(), fq_one());
  p.T = fq_add(p.Y, fq_one());
  p.Z = fq_add(p.T, fq_one());
  Fq a = p.Z;
  const auto t0 = clk::now();
  for (size_t i = 0; i < iters; i++) {
    if (what == 0) a = fq_mul(a, a);
    else if (what == 1) p = pt_dbl_n(p, 1);
    else if (what == 2) p = pt_add(p, p);
    else a = fq_inv(a);
  }
  *ns = std::chrono::duration<double, std::nano>(clk::now() - t0).count() / (double)iters;
  volatile uint64_t sink = a.l[0] ^ p.X.l[0];
  (void)sink;
  return MSM_OK;
}

// The number of window-term words msm_test_tail reads for n points.
// msm_test_tail over k MSMs' terms at once (k blocks of msm_test_tail_words(n) words), as the last
// launch of a pipelined run finishes: helpers > 0 runs TailCrew::run_batch on a crew of that many
// threads, helpers = 0 one horner_tail per MSM.  out_xy_be: k affine results (16 words each).
int msm_test_tail_batch(size_t n, uint32_t k, const uint32_t* terms, int helpers, uint32_t* out_xy_be, double* ms) {
  if (!terms || !out_xy_be || !ms || k < 1 || k > MSM_MAX_BATCH || helpers < 0) return MSM_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = make_plan(n, nullptr, DevShape{}, &pl)) return rc;
  TailCrew crew(helpers);
  Pt r[MSM_MAX_BATCH];
  const auto t0 = clk::now();
  if (helpers) {
    crew.arm();
    crew.run_batch(pl, terms, k, r);
  } else {
    for (uint32_t m = 0; m < k; m++) r[m] = horner_tail(pl, terms, m);
  }
  *ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  for (uint32_t m = 0; m < k; m++) pt_to_be_affine(r[m], out_xy_be + 16 * m);
  return MSM_OK;
}

// The launch plan make_plan builds for n points, nm MSMs per launch, pipelined or lone, with
// `opts` (window width / range; may be null): out = {c (widest window), windows in the launch per
// MSM (Wr), run length K, reduction chunk L, MSMs per launch, coarse bins per window, skew floor
// of K}, for the default device shape (256 CUs, 4 accumulation waves per SIMD).
int msm_test_plan(size_t n, uint32_t nm, int pipelined, const msm_opts* opts, uint32_t out[7]) {
  if (!out || nm < 1 || nm > MSM_MAX_BATCH) return MSM_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = make_plan(n, opts, DevShape{}, &pl, pipelined != 0, nm)) return rc;
  const uint32_t v[7] = {pl.d.c, pl.d.Wr, pl.K, pl.L, pl.d.nm, pl.d.nbc, run_length_skew_floor(pl.d)};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// The host packing of the packed uploads (pack_records over a pool of MSM_HOST_PACK_THREADS):
// n wire records -> out (16 words per point for fmt 1 = x|y, 24 for fmt 2 = x|y|z); *all_z_one =
// whether every z is 1, *t_bad = whether some t >= p.  Host code only (no device needed).
// The host thread pools a call over `ndev` devices runs per device context (CPU test hook,
// no device needed): out[0] the CPU budget (host_threads: hardware threads capped by the cgroup
// quota), out[1..3] packing threads (the caller included), lone-MSM tail helpers and pipelined-tail
// threads per device, out[4] the threads the library adds for the whole call -- per device its
// packing workers, helpers, tail threads and one uploader, plus a host thread per device but the
// first.  With `run` the three pools are started at those sizes (replacing the previous set), given
// one job each, and left parked until the next call or msm_shutdown.
int msm_test_pools(int ndev, int run, int* out) {
  if (ndev < 1 || ndev > 64 || !out) return MSM_ERR_INVALID_ARG;
  const int own = t_call_devices;
  t_call_devices = ndev;
  const int pk = pack_threads(), th = tail_helpers(), hn = horner_threads();
  t_call_devices = own;
  out[0] = (int)host_threads();
  out[1] = pk;
  out[2] = th;
  out[3] = hn;
  out[4] = ndev * ((pk - 1) + th + hn + 1) + (ndev - 1);
  if (!run) return MSM_OK;
  std::lock_guard<std::mutex> lk(g_test_mu);
  g_test_pools.stop();
  g_test_pools.packer = new PackPool(pk);
  g_test_pools.crew = new TailCrew(th);
  g_test_pools.pool = hn ? new HornerPool(hn) : nullptr;
  std::atomic<int> hits{0};
  g_test_pools.packer->run([&](int, int) { hits.fetch_add(1); });
  if (g_test_pools.pool) {
    for (int i = 0; i < 2 * hn; i++) g_test_pools.pool->push([&] { hits.fetch_add(1); });
    g_test_pools.pool->wait_all();
  }
  g_test_pools.crew->arm();  // the helpers wake and spin, then go back to sleep
  g_test_pools.crew->disarm();
  return hits.load() == pk + 2 * hn ? MSM_OK : MSM_ERR_HIP;
}

int msm_test_pack(const uint32_t* wire, size_t n, uint32_t fmt, uint32_t* out, int* all_z_one, int* t_bad) {
  if ((!wire || !out) && n) return MSM_ERR_INVALID_ARG;
  if (fmt != PT_FMT_XY && fmt != PT_FMT_XYZ) return MSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g_test_mu);
  PackPool*& pool = g_test_pools.packer;
  if (!pool) pool = new PackPool(pack_threads());
  const size_t bytes = n * pt_fmt_slots(fmt) * 16;
  void* tmp = aligned_alloc(64, (bytes + 63) / 64 * 64 + 64);  // the nontemporal stores want 32-B alignment
  if (!tmp) return MSM_ERR_OOM;
  bool tb = false;
  const bool z1 = pack_records(*pool, static_cast<uint32_t*>(tmp), wire, n, fmt, &tb);
  memcpy(out, tmp, bytes);
  free(tmp);
  if (all_z_one) *all_z_one = z1 ? 1 : 0;
  if (t_bad) *t_bad = tb ? 1 : 0;
  return MSM_OK;
}

size_t msm_test_tail_words(size_t n) {
  Plan pl;
  if (make_plan(n, nullptr, DevShape{}, &pl)) return 0;
  return (size_t)pl.d.W * pl.nterms * 32;
}

// Batch field / point ops on the device, canonical LE words.
int msm_test_field_op(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  TestBuf da, db, dout;  // freed on every return path
  HIPCHECK(da.alloc(n * 32 + 32));
  HIPCHECK(db.alloc(n * 32 + 32));
  HIPCHECK(dout.alloc(n * 32 + 32));
  HIPCHECK(hipMemcpy(da.p, a, n * 32, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(db.p, b, n * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_field, dim3(grid_for(n, 256)), dim3(256), 0, 0, da.p, db.p, dout.p, (uint32_t)n, op);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(out, dout.p, n * 32, hipMemcpyDeviceToHost));
  return MSM_OK;
}

int msm_test_point_op(uint32_t op, const uint32_t* p, const uint32_t* q, uint32_t* out, size_t n) {
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  TestBuf dp, dq, dout;
  HIPCHECK(dp.alloc(n * 64 + 64));
  HIPCHECK(dq.alloc(n * 64 + 64));
  HIPCHECK(dout.alloc(n * 128 + 128));
  HIPCHECK(hipMemcpy(dp.p, p, n * 64, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dq.p, q, n * 64, hipMemcpyHostToDevice));
  if (op == 3)
    hipLaunchKernelGGL(k_test_quad, dim3(grid_for(4 * n, 256)), dim3(256), 0, 0, dp.p, dq.p, dout.p, (uint32_t)n);
  else if (op == 0)
    hipLaunchKernelGGL(k_test_point<0>, dim3(grid_for(n, 256)), dim3(256), 0, 0, dp.p, dq.p, dout.p, (uint32_t)n);
  else if (op == 1)
    hipLaunchKernelGGL(k_test_point<1>, dim3(grid_for(n, 256)), dim3(256), 0, 0, dp.p, dq.p, dout.p, (uint32_t)n);
  else
    hipLaunchKernelGGL(k_test_point<2>, dim3(grid_for(n, 256)), dim3(256), 0, 0, dp.p, dq.p, dout.p, (uint32_t)n);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(out, dout.p, n * 128, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// ---- raw-limb hooks (msm_kernels.hip k_test_limbs*, tests/test_gpu_limbs.py) --------------------
// The four WIDE_* masks this library was built with (fp29.cuh; all 0 under MSM_NARROW_DIGITS).
int msm_test_wide_masks(uint32_t out[4]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  out[0] = WIDE_ALL;
  out[1] = WIDE_GH;
  out[2] = WIDE_EH;
  out[3] = WIDE_EF;
  return MSM_OK;
}

// k_decompress_x's constants as the kernel reads them (msm_kernels.hip dx_*; tests/test_sqrt_model.py
// recomputes each from p): out[0] the 2-adicity of p - 1, out[1] the words of the exponent the loop
// runs, out[2] the bits of the order the ladder runs, out[3..11] (q - 1) / 2 and out[11..19] r as
// little-endian words, out[19..28] omega's Montgomery limbs.
int msm_test_decompress_constants(uint32_t out[28]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  out[0] = DX_TWO_ADICITY;
  out[1] = DX_EXP_WORDS;
  out[2] = DX_ORDER_BITS;
  for (uint32_t i = 0; i < 8; i++) {
    out[3 + i] = dx_exp_word(i);
    out[11 + i] = dx_order_word(i);
  }
  for (uint32_t i = 0; i < NL; i++) out[19 + i] = dx_omega_limb(i);
  return MSM_OK;
}

// k_scale_points' own digit function on the host (msm_kernels.hip scale_digit, scale_windows): the
// windows of one b-bit scalar of sw big-endian words, least significant first, and their count -- the
// ladder's trip count (256 / w at b = 256 for windows of w bits).  digits holds 256 entries.
int msm_test_scale_digits(const uint32_t* scalar_be, uint32_t sw, uint32_t b, uint32_t* digits, uint32_t* count) {
  if (!scalar_be || !digits || !count || b < 1 || b > 256 || sw != (b + 31) / 32) return MSM_ERR_INVALID_ARG;
  *count = scale_windows(b);
  for (uint32_t j = 0; j < *count; j++) digits[j] = scale_digit(scalar_be, sw, b, j);
  return MSM_OK;
}

// k_combine_joint's own digit function on the host (msm_kernels.hip combine_digit): the joint ladder's
// digits of two b-bit scalars of sw big-endian words each, least significant first -- bit j of a + 2 * bit
// j of b -- and their count, the ladder's trip count b.  digits holds 256 entries.
int msm_test_combine_digits(const uint32_t* a_be, const uint32_t* b_be, uint32_t sw, uint32_t b, uint32_t* digits,
                            uint32_t* count) {
  if (!a_be || !b_be || !digits || !count || b < 1 || b > 256 || sw != (b + 31) / 32) return MSM_ERR_INVALID_ARG;
  *count = b;
  for (uint32_t j = 0; j < b; j++) digits[j] = combine_digit(a_be, b_be, sw, b, j);
  return MSM_OK;
}

// k_fixed_eval's own digit function on the host (msm_kernels.hip fixed_digit, fixed_windows): the
// signed digits of one b-bit scalar of sw big-endian words for windows of w bits, least significant
// first, their count, and the carry out of the last one (always 0).  digits holds 257 entries.
int msm_test_fixed_digits(const uint32_t* scalar_be, uint32_t sw, uint32_t b, uint32_t w, int32_t* digits,
                          uint32_t* count, uint32_t* carry_out) {
  if (!scalar_be || !digits || !count || !carry_out || b < 1 || b > 256 || sw != (b + 31) / 32 || w < 2 || w > 16)
    return MSM_ERR_INVALID_ARG;
  *count = fixed_windows(b, w);
  uint32_t carry = 0;
  for (uint32_t j = 0; j < *count; j++) digits[j] = fixed_digit(scalar_be, sw, b, w, j, carry);
  *carry_out = carry;
  return MSM_OK;
}

// The shape msm_fixed_create gives a table of k bases (host_fixed.h fixed_plan): out = window width,
// scalar width, windows per base, then records and bytes as two words each (low, high).  Its
// refusals are the creation's.  Needs no device.
int msm_test_fixed_plan(uint32_t k, uint32_t w, uint32_t b, uint32_t out[7]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  FixedPlan fp;
  if (int rc = fixed_plan(k, w, b, &fp)) return rc;
  out[0] = fp.w;
  out[1] = fp.b;
  out[2] = fp.Wn;
  out[3] = (uint32_t)fp.records;
  out[4] = (uint32_t)(fp.records >> 32);
  out[5] = (uint32_t)fp.bytes;
  out[6] = (uint32_t)(fp.bytes >> 32);
  return MSM_OK;
}

// The shape msm_fixed_create_vector gives a table of k bases (host_fixed.h vector_table_plan), laid out
// as msm_test_fixed_plan's, and with m > 0 how a call of m rows of sw-word scalars on it is cut
// (vector_plan): out[7..] = G, P, the fold's passes, then a slab's rows and the partial buffer's bytes as
// two words each.  Needs no device.
int msm_test_vector_plan(uint32_t k, uint32_t w, uint32_t b, uint64_t m, uint32_t sw, uint32_t out[14]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  FixedPlan fp;
  if (int rc = vector_table_plan(k, w, b, &fp)) return rc;
  out[0] = fp.w;
  out[1] = fp.b;
  out[2] = fp.Wn;
  out[3] = (uint32_t)fp.records;
  out[4] = (uint32_t)(fp.records >> 32);
  out[5] = (uint32_t)fp.bytes;
  out[6] = (uint32_t)(fp.bytes >> 32);
  for (int i = 7; i < 14; i++) out[i] = 0;
  if (!m) return MSM_OK;
  if (sw < 1 || sw > 8) return MSM_ERR_INVALID_ARG;
  const VectorPlan vp = vector_plan(k, m, sw);
  out[7] = vp.G;
  out[8] = vp.P;
  out[9] = vp.passes;
  out[10] = (uint32_t)vp.slab_rows;
  out[11] = (uint32_t)(vp.slab_rows >> 32);
  out[12] = (uint32_t)vp.part_bytes;
  out[13] = (uint32_t)(vp.part_bytes >> 32);
  return MSM_OK;
}
// The cap on the partial buffer of the calls that follow (0: VEC_PART_MAX_BYTES again), so that a test
// runs a small call as several slabs; and the G every plan takes (0: the rule's again), so that a
// test, or a sweep, meets parts of a chosen size.
void msm_test_vector_slab(uint64_t bytes) { g_vec_part_cap.store(bytes ? bytes : VEC_PART_MAX_BYTES); }
void msm_test_vector_group(uint32_t g) { g_vec_group.store(g); }

// out[i] = op(a[i], b[i]) on raw limbs, nothing converted or reduced (LimbOp and its word counts:
// msm_kernels.hip).  b is read only by the two-operand ops, neg (n flags) only by LOP_PT_MADD.
// The lane ops' loops are bounded whatever the operands hold: fe_sqrt_ts' m strictly decreases from
// 47 and its inner loops stop at m, pt_mul_order and fe_inv walk constants, and LOP_SHIFT_LANE's
// count (b, one word per record) is refused here above LOP_SHIFT_MAX.
int msm_test_limb_op(uint32_t op, const uint32_t* a, const uint32_t* b, const uint32_t* neg, uint32_t* out, size_t n) {
  if (op >= (uint32_t)LOP_COUNT || n == 0 || n > (1u << 24) || !a || !out) return MSM_ERR_INVALID_ARG;
  const size_t wa = limb_op_in_words((int)op), wb = limb_op_b_words((int)op), wo = limb_op_out_words((int)op);
  if ((wb && !b) || (op == (uint32_t)LOP_PT_MADD && !neg)) return MSM_ERR_INVALID_ARG;
  if (op == (uint32_t)LOP_SHIFT_LANE)  // the lane's loop is bounded before anything is launched
    for (size_t i = 0; i < n; i++)
      if (b[i] > LOP_SHIFT_MAX) return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  TestBuf da, db, dn, dout;
  HIPCHECK(da.alloc(n * wa * 4));
  HIPCHECK(db.alloc(n * (wb ? wb : 1) * 4));
  HIPCHECK(dn.alloc(n * 4));
  HIPCHECK(dout.alloc(n * wo * 4));
  HIPCHECK(hipMemcpy(da.p, a, n * wa * 4, hipMemcpyHostToDevice));
  if (wb) HIPCHECK(hipMemcpy(db.p, b, n * wb * 4, hipMemcpyHostToDevice));
  if (op == (uint32_t)LOP_PT_MADD) HIPCHECK(hipMemcpy(dn.p, neg, n * 4, hipMemcpyHostToDevice));
  dispatch_limb_op((int)op, std::make_integer_sequence<int, LOP_COUNT>{}, da.p, db.p, dn.p, dout.p, (uint32_t)n);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(out, dout.p, n * wo * 4, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// k_prepare_points on n input points (fmt: PT_FMT_WIRE 32, PT_FMT_XY 16 or PT_FMT_XYZ 24 BE words
// each) -> the n 32-word records and the device error word; then, for m > 0, the accumulation's
// gather and add on them: out[j] = acc[j] + record(ents[j]), ents[j] = index << 1 | sign.
int msm_test_records(uint32_t fmt, const uint32_t* in, size_t n, uint32_t* records, uint32_t* err,
                     const uint32_t* ents, const uint32_t* acc, uint32_t* out, size_t m) {
  if (fmt > PT_FMT_XYZ || !in || !records || !err || n == 0 || n > (1u << 24) || m > (1u << 24))
    return MSM_ERR_INVALID_ARG;
  if (m && (!ents || !acc || !out)) return MSM_ERR_INVALID_ARG;
  for (size_t j = 0; j < m; j++)
    if ((ents[j] >> 1) >= n) return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  const size_t in_bytes = n * pt_fmt_slots(fmt) * 16;
  TestBuf din, dpts, derr, dents, dacc, dout;
  HIPCHECK(din.alloc(in_bytes));
  HIPCHECK(dpts.alloc(n * PRE_WORDS * 4));
  HIPCHECK(derr.alloc(4));
  HIPCHECK(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(derr.p, 0, 4));
  launch_prepare(din.p, dpts.p, (uint32_t)n, derr.p, 0u, nullptr, fmt);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(records, dpts.p, n * PRE_WORDS * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(err, derr.p, 4, hipMemcpyDeviceToHost));
  if (!m) return MSM_OK;
  HIPCHECK(dents.alloc(m * 4));
  HIPCHECK(dacc.alloc(m * PT_WORDS * 4));
  HIPCHECK(dout.alloc(m * PT_WORDS * 4));
  HIPCHECK(hipMemcpy(dents.p, ents, m * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(dacc.p, acc, m * PT_WORDS * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_limbs_gather, dim3(grid_for(m, 256)), dim3(256), 0, 0, dpts.p, dents.p, dacc.p, dout.p,
                     (uint32_t)m);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(out, dout.p, m * PT_WORDS * 4, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// The fold geometry a handle of `levels` levels gets at width window_bits (0: the auto width for n
// points): out = {window_bits c, windows per folded MSM Wc, chunk bits S, points of the folded
// problem levels * n}.  Host code only (no device needed).
int msm_test_bases_plan(size_t n, uint32_t levels, uint32_t window_bits, uint32_t out[4]) {
  if (!out || levels < 1 || levels > 8) return MSM_ERR_INVALID_ARG;
  const uint32_t c = window_bits ? window_bits : levels > 1 ? bases_auto_window(n, levels) : msm_best_window(n);
  BasesGeo g;
  if (!bases_geometry(c, levels, &g)) return MSM_ERR_UNSUPPORTED_WINDOW;
  out[0] = g.c;
  out[1] = g.Wc;
  out[2] = g.S;
  out[3] = (uint32_t)(n * levels);
  return MSM_OK;
}

// The geometry of one narrow-scalar MSM (MSM_FLAG_SCALAR_BITS) of n terms at width window_bits (0:
// the lone launch's auto width for n): out = {widest window c, windows in the launch W', base width
// q, windows of q + 1 bits nhi, words per wire scalar, d.packed}.  254 bits and more report the plain
// launch (Wr counts its overflow window; 8 words).  Host code only.
int msm_test_narrow_plan(size_t n, uint32_t scalar_bits, uint32_t window_bits, uint32_t out[6]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  msm_opts op{};
  op.window_bits = window_bits;
  op.flags = MSM_FLAG_SCALAR_BITS;
  op.scalar_bits = scalar_bits;
  Plan pl;
  if (int rc = make_plan(n, &op, DevShape{}, &pl, false, 1, true)) return rc;
  const uint32_t v[6] = {pl.d.c, pl.d.Wr, pl.d.q, pl.d.nhi, pl.d.sw ? pl.d.sw : 8u, pl.d.packed};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// The plan of one native-type MSM (MSM_FLAG_SCALAR_TYPE with MSM_FLAG_SCALAR_BITS) of n terms:
// out = msm_test_narrow_plan's six fields for scalar_bits, then the bytes of one vector and of its
// region in a slot's wire buffer.  The entry's argument rules apply (unknown type, scalar_bits 0 or
// past the element's width, a bit vector wider than 1: MSM_ERR_INVALID_ARG).  Host code only.
int msm_test_native_plan(size_t n, uint32_t scalar_type, uint32_t scalar_bits, uint32_t window_bits, uint32_t out[8]) {
  if (!out || !typed_width(scalar_type, true, scalar_bits)) return MSM_ERR_INVALID_ARG;
  msm_opts_typed op{};
  op.opts.window_bits = window_bits;
  op.opts.flags = MSM_FLAG_SCALAR_BITS | MSM_FLAG_SCALAR_TYPE;
  op.opts.scalar_bits = scalar_bits;
  op.scalar_type = scalar_type;
  Plan pl;
  if (int rc = make_plan(n, &op.opts, DevShape{}, &pl, false, 1, true)) return rc;
  if (pl.stype != scalar_type) return MSM_ERR_INVALID_ARG;
  const uint32_t v[8] = {pl.d.c,  pl.d.Wr,     pl.d.q,
                         pl.d.nhi, pl.d.sw,    pl.d.packed,
                         (uint32_t)pl.sc_bytes, (uint32_t)typed_region_bytes(n, scalar_type)};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// The plan of one wide-type MSM (MSM_FLAG_SCALAR_FIELD with MSM_FLAG_SCALAR_BITS) of n terms, as the entry
// makes it: out = msm_test_narrow_plan's six fields for scalar_bits (254 bits and more of a 256-bit
// integer: the plain launch, 8 words), then the bytes of one vector and of its region in a slot's wire
// buffer.  The entry's argument rules apply (unknown field, scalar_bits 0 or past the element's width, a
// Montgomery-form Fr of any width but 251: MSM_ERR_INVALID_ARG).  Host code only.
int msm_test_wide_plan(size_t n, uint32_t field, uint32_t scalar_bits, uint32_t window_bits, uint32_t out[8]) {
  msm_opts_typed op{};
  op.opts.window_bits = window_bits;
  op.opts.flags = MSM_FLAG_SCALAR_FIELD | MSM_FLAG_SCALAR_BITS;
  op.opts.scalar_bits = scalar_bits;
  op.scalar_field = field;
  const uint32_t stype = opts_scalar_type(&op.opts);
  if (!out || !typed_width(stype, true, scalar_bits)) return MSM_ERR_INVALID_ARG;
  // (as bases_compute: the width is said to the planner only below 254 bits)
  if (scalar_bits >= MAIN_BITS) op.opts.flags = MSM_FLAG_SCALAR_FIELD;
  Plan pl;
  if (int rc = make_plan(n, &op.opts, DevShape{}, &pl, false, 1, true)) return rc;
  if (pl.stype != stype) return MSM_ERR_INVALID_ARG;
  const uint32_t v[8] = {pl.d.c,  pl.d.Wr,     pl.d.q,
                         pl.d.nhi, pl.d.sw ? pl.d.sw : 8u, pl.d.packed,
                         (uint32_t)pl.sc_bytes, (uint32_t)typed_region_bytes(n, stype)};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// fr.cuh on the host: n values of 8 little-endian words each; ok[i] = fr_is_canonical(in_i) and
// out_i = fr_from_mont(in_i) (computed whatever ok says, as the recode kernel does).
int msm_test_fr_from_mont(const uint32_t* in_le, size_t n, uint32_t* out_le, uint8_t* ok) {
  if ((!in_le || !out_le || !ok) && n) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++) {
    ok[i] = fr_is_canonical(in_le + 8 * i) ? 1 : 0;
    fr_from_mont(in_le + 8 * i, out_le + 8 * i);
  }
  return MSM_OK;
}

// fr.cuh's arithmetic on the host, the code the Fr vector kernels run: n pairs of 8 little-endian words
// each, out_i = op(a_i, b_i) -- 0 fr_mont_mul, 1 fr_add, 2 fr_sub, 3 fr_to_mont(a_i), 4 fr_from_mont of
// fr_to_mont(a_i).  The functions' preconditions are the hook's: b >= r for op 0, or either operand >= r for
// ops 1 and 2, is MSM_ERR_INVALID_ARG.  Op 5 reads nothing and writes the constants: out[0..32) = R^k mod r
// for k = 0..3 (fr_r_power), then FR_THREADS, FR_DOT_CAP, FR_COMBINE_CAP and FR_POW_STEPS (out holds 36 words).
int msm_test_fr_op(uint32_t op, const uint32_t* a_le, const uint32_t* b_le, uint32_t* out_le, size_t n) {
  if (op > 5 || !out_le) return MSM_ERR_INVALID_ARG;
  if (op == 5) {
    for (int k = 0; k < 4; k++) {
      const FrWords w = fr_r_power(k);
      memcpy(out_le + 8 * k, w.v, 32);
    }
    const uint32_t shape[4] = {FR_THREADS, FR_DOT_CAP, FR_COMBINE_CAP, FR_POW_STEPS};
    memcpy(out_le + 32, shape, sizeof(shape));
    return MSM_OK;
  }
  if ((!a_le || (op <= 2 && !b_le)) && n) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++) {
    const uint32_t *a = a_le + 8 * i, *b = b_le + 8 * i;
    uint32_t* o = out_le + 8 * i;
    if (op <= 2 && (!fr_is_canonical(b) || (op != 0 && !fr_is_canonical(a)))) return MSM_ERR_INVALID_ARG;
    if (op == 0) fr_mont_mul(a, b, o);
    else if (op == 1) fr_add(a, b, o);
    else if (op == 2) fr_sub(a, b, o);
    else fr_to_mont(a, o);
    if (op == 4) fr_from_mont(o, o);
  }
  return MSM_OK;
}

// fr.cuh's fr_inv on the host, the code k_fr_inverse runs once per tile: n values of 8 little-endian words
// each, canonical and in Montgomery form (a >= r: MSM_ERR_INVALID_ARG); out_i = a_i^-1 in Montgomery form,
// 0 for 0.
int msm_test_fr_inv(const uint32_t* a_le, uint32_t* out_le, size_t n) {
  if ((!a_le || !out_le) && n) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < n; i++) {
    if (!fr_is_canonical(a_le + 8 * i)) return MSM_ERR_INVALID_ARG;
    fr_inv(a_le + 8 * i, out_le + 8 * i);
  }
  return MSM_OK;
}

// The shape of the second set of Fr kernels: out = {FR_TILE_E, FR_TILE, FR_SCAN_CAP, k_fr_inverse's grid
// cap, fr_inv's squarings, fr_inv's products, MSM_FR_TENSOR_MAX_K, 0}.
int msm_test_fr_scan_constants(uint32_t out[8]) {
  if (!out) return MSM_ERR_INVALID_ARG;
  const uint32_t v[8] = {FR_TILE_E, FR_TILE, FR_SCAN_CAP, FR_COMBINE_CAP, FR_INV_SQUARINGS, FR_INV_PRODUCTS, FR_TENSOR_MAX_K, 0};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// The plan of a scan of m elements over at most grid_cap spans, as msm_fr_scan* makes it (fr_scan_plan):
// out = {elements per lane, elements per tile, workgroups, tiles per span}.  Host code only.
int msm_test_fr_scan_plan(size_t m, uint32_t grid_cap, uint32_t out[4]) {
  if (!out || !grid_cap || m >= (1ull << 32)) return MSM_ERR_INVALID_ARG;
  const FrScanPlan pl = fr_scan_plan(m, grid_cap);
  const uint32_t v[4] = {pl.e, pl.tile, pl.grid, pl.tiles_per_span};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// msm_fr_scan_device and msm_fr_inverse_device on the current device and the null stream with a
// caller-given grid cap (1 .. FR_SCAN_CAP for a scan), so that spans of several tiles and workgroups
// striding over tiles are reached at a few thousand elements.  Everything else is the entries' own path.
int msm_test_fr_scan_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t flags, uint32_t in_form,
                            uint32_t out_form, uint32_t grid_cap, uint32_t* d_out) {
  return fr_scan(d_a, c_be, m, flags, in_form, out_form, false, nullptr, (hipStream_t)MSM_STREAM_NULL, d_out, grid_cap);
}
int msm_test_fr_inverse_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t in_form, uint32_t out_form,
                               uint32_t grid_cap, uint32_t* d_out) {
  return fr_inverse(d_a, c_be, m, in_form, out_form, false, nullptr, (hipStream_t)MSM_STREAM_NULL, d_out, grid_cap);
}

// The dense-bucket part of the plan of a narrow launch (msm_bases_compute* with MSM_FLAG_SCALAR_BITS)
// of nm MSMs of n terms at width window_bits (0: auto), pipelined or lone: out = {dense (0 / 1),
// entries per unit lane E, keys W * B, the unit kernel's grid bound, run length K}, for the default
// device shape.  E and the bound are 0 for a launch that is not dense.  Host code only.
int msm_test_dense_plan(size_t n, uint32_t nm, int pipelined, uint32_t scalar_bits, uint32_t window_bits,
                        uint32_t out[5]) {
  if (!out || nm < 1 || nm > MSM_MAX_BATCH) return MSM_ERR_INVALID_ARG;
  msm_opts op{};
  op.window_bits = window_bits;
  op.flags = MSM_FLAG_SCALAR_BITS;
  op.scalar_bits = scalar_bits;
  Plan pl;
  if (int rc = make_plan(n, &op, DevShape{}, &pl, pipelined != 0, nm, true)) return rc;
  const uint32_t v[5] = {pl.dense, pl.dense_E, pl.d.W * pl.d.B, pl.dense_units, pl.K};
  memcpy(out, v, sizeof(v));
  return MSM_OK;
}

// k_dense_segments alone, on the device: bucket_start[0..nkeys] (non-decreasing) and the segment
// length S (a multiple of 64) -> seg_base[0..nkeys] and unit_key[0..bound), bound =
// bucket_start[nkeys] / S + nkeys, the grid bound a plan would hold; the words of unit_key past the
// live units come back as 0xffffffff (unwritten).
int msm_test_dense_segments(const uint32_t* bucket_start, uint32_t nkeys, uint32_t S, uint32_t* seg_base,
                            uint32_t* unit_key) {
  if (!bucket_start || !seg_base || !unit_key || nkeys < 1 || nkeys > DENSE_MAX_KEYS || S < 64 || (S & 63u))
    return MSM_ERR_INVALID_ARG;
  for (uint32_t k = 0; k < nkeys; k++)
    if (bucket_start[k + 1] < bucket_start[k]) return MSM_ERR_INVALID_ARG;
  if (bucket_start[nkeys] >= (1u << 31)) return MSM_ERR_INVALID_ARG;
  const uint32_t bound = bucket_start[nkeys] / S + nkeys;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  const uint32_t KA = DENSE_K * ACC_THREADS, ncross = bucket_start[nkeys] / KA + 2;
  TestBuf dbs, dseg, dunit, dcross;
  HIPCHECK(dbs.alloc(((size_t)nkeys + 1) * 4));
  HIPCHECK(dseg.alloc(((size_t)nkeys + 1) * 4));
  HIPCHECK(dunit.alloc((size_t)bound * 4));
  HIPCHECK(dcross.alloc((size_t)ncross * 4));
  HIPCHECK(hipMemcpy(dbs.p, bucket_start, ((size_t)nkeys + 1) * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(dunit.p, 0xff, (size_t)bound * 4));
  hipLaunchKernelGGL(k_dense_segments, dim3(1), dim3(DS_THREADS), 0, 0, dbs.p, nkeys, S, dseg.p, dunit.p, bound,
                     dcross.p, KA, ncross);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(seg_base, dseg.p, ((size_t)nkeys + 1) * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(unit_key, dunit.p, (size_t)bound * 4, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// The launch plan of one subset MSM (msm_bases_compute_subset*) of m terms on a handle of n_handle
// points and `levels` levels at width window_bits (0: the width such a handle or launch gets):
// out = {d.n, d.packed, the record stride d.rstride, d.fb, d.sub}.  The argument rules that need no
// device apply (MSM_ERR_INVALID_ARG); the range [0, m) of a levels = 1 handle reports the plain
// plan of m points (sub 0, stride 0).  Host code only.
int msm_test_subset_plan(size_t n_handle, uint32_t levels, uint32_t window_bits, uint64_t first, uint64_t m,
                         int indexed, uint32_t out[5]) {
  if (!out || levels < 1 || levels > 8) return MSM_ERR_INVALID_ARG;
  if ((uint64_t)levels * n_handle >= (1ull << 30)) return MSM_ERR_INVALID_ARG;  // no such handle
  if (int rc = subset_check(n_handle, levels, first, m, indexed != 0)) return rc;
  msm_opts op{};
  op.window_bits = window_bits;
  if (levels > 1) {
    BasesGeo g;
    op.window_bits = window_bits ? window_bits : bases_auto_window(n_handle, levels);
    if (!bases_geometry(op.window_bits, levels, &g)) return MSM_ERR_UNSUPPORTED_WINDOW;
    op.flags = MSM_FLAG_WINDOWS;
    op.window_hi = g.Wc;
  }
  SubsetGeo sg;
  sg.kind = subset_kind(levels, first, indexed != 0);
  sg.levels = levels;
  sg.rec_n = n_handle;
  sg.first = (size_t)first;
  Plan pl;
  if (int rc = make_plan((size_t)m * levels, &op, DevShape{}, &pl, false, 1, true, &sg)) return rc;
  out[0] = pl.d.n;
  out[1] = pl.d.packed;
  out[2] = pl.d.rstride;
  out[3] = pl.d.fb;
  out[4] = pl.d.sub;
  return MSM_OK;
}

// The records of one level of a handle, copied to the host (n * 32 words).
int msm_test_bases_records(const msm_bases* h, uint32_t level, uint32_t* records) {
  if (!h || !records) return MSM_ERR_INVALID_ARG;
  std::shared_ptr<Bases> b = find_bases(h);
  if (!b || level >= b->levels) return MSM_ERR_INVALID_ARG;
  msm_opts o{};
  o.device = b->device;
  return on_device(&o, [&](DevCtx*) -> int {
    if (!b->alive) return MSM_ERR_INVALID_ARG;
    if (!b->n) return MSM_OK;
    HIPCHECK(hipMemcpy(records, b->rec.as<uint32_t>() + (size_t)level * b->n * PRE_WORDS, b->n * PRE_WORDS * 4,
                       hipMemcpyDeviceToHost));
    return MSM_OK;
  });
}

// A fixed-base table's records as a handle of levels = 1 (a device-to-device copy the caller destroys):
// msm_test_bases_records then reads the records, and scaling by ones the points they hold.
int msm_test_fixed_bases(const msm_fixed* h, msm_bases** out) {
  if (!h || !out) return MSM_ERR_INVALID_ARG;
  *out = nullptr;
  std::shared_ptr<Fixed> t = find_fixed(h);
  if (!t) return MSM_ERR_INVALID_ARG;
  auto nb = std::make_shared<Bases>();
  if (int rc = bases_shape(nb.get(), t->records(), 1, 0)) return rc;
  msm_opts o{};
  o.device = t->device;
  int rc = on_device(&o, [&](DevCtx* c) -> int {
    if (!t->alive) return MSM_ERR_INVALID_ARG;
    nb->device = c->device;
    const size_t bytes = t->records() * PRE_WORDS * 4;
    if (int r = nb->rec.ensure(bytes)) return r;
    if (hipMemcpy(nb->rec.p, t->rec.p, bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
      nb->rec.release();
      return MSM_ERR_HIP;
    }
    return MSM_OK;
  });
  return rc != MSM_OK ? rc : register_bases(nb, out);
}

// What the last msm_fixed_mul* of m points left in slot 0's fx_proj on the default device, read back
// after the call as msm_test_acc_state reads its slot: nothing is launched.  out takes k_fixed_eval's
// whole blocks, ceil(m / 64) * 27 * 64 words in the kernel's own layout (limb q of X | Y | Z of point
// 64 g + l at (g * 27 + q) * 64 + l), the identities of the lanes past m included.
int msm_test_fixed_proj(uint32_t* out, size_t m) {
  if (!out || m == 0 || m >= (1ull << 30)) return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot& sl = c->slot[0];
  const Buf& b = sl.ws.fx_proj;
  const size_t bytes = fixed_proj_bytes(m);
  if (!b.p || bytes > b.cap || !sl.stream) return MSM_ERR_INVALID_ARG;
  HIPCHECK(hipStreamSynchronize(sl.stream));
  HIPCHECK(hipMemcpy(out, b.p, bytes, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// ---- the host field at operand level (hostfield.h, tests/test_host_field.py) ----------------------
// out[i] = op(a[i], b[i]) on raw representatives: an element is the four little-endian 64-bit limbs an
// Fq holds (its Montgomery form, R = 2^256), a point sixteen of them (X | Y | T | Z).  Nothing is
// converted on the way in or out, so the caller prices every operation on plain integers:
//   0 fq_mul   1, 2 fq_mul_n<3>, fq_mul_n<4> (element i on lane i mod N of its group; a last short
//   group is filled with the elements before it)   3 fq_add   4 fq_sub   5 fq_inv   6 fq_from_std
//   (a: a standard-form integer)   7 fq_to_std   8, 9, 10 div2k_mod at k = 1, 32, 63
//   11, 12 pt_add with and without want_t   13 pt_dbl   14, 15, 16 pt_dbl_n at k = 1, 2, 5
// b is read by ops 0..4, 11 and 12.  Every operand must be below p (the functions' precondition):
// MSM_ERR_INVALID_ARG otherwise.  Needs no device.
int msm_test_host_field(uint32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (op > 16 || !a || !out || n == 0) return MSM_ERR_INVALID_ARG;
  const bool pts = op >= 11;
  const bool two = op <= 4 || op == 11 || op == 12;
  const size_t w = pts ? 16 : 4;
  if (two && !b) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < n * w / 4; i++)
    if (msmh::geq_p(a + 4 * i) || (two && msmh::geq_p(b + 4 * i))) return MSM_ERR_INVALID_ARG;
  auto fq_at = [](const uint64_t* v, size_t i) {
    Fq x;
    memcpy(x.l, v + 4 * i, 32);
    return x;
  };
  auto pt_at = [&](const uint64_t* v, size_t i) { return Pt{fq_at(v, 4 * i), fq_at(v, 4 * i + 1), fq_at(v, 4 * i + 2), fq_at(v, 4 * i + 3)}; };
  auto put = [&](size_t i, const Fq& x) { memcpy(out + 4 * i, x.l, 32); };
  auto put_pt = [&](size_t i, const Pt& p) {
    put(4 * i, p.X);
    put(4 * i + 1, p.Y);
    put(4 * i + 2, p.T);
    put(4 * i + 3, p.Z);
  };
  if (op == 1 || op == 2) {
    const size_t N = op == 1 ? 3 : 4;
    if (n < N) return MSM_ERR_INVALID_ARG;
    for (size_t g0 = 0; g0 < n; g0 += N) {
      const size_t g = g0 + N <= n ? g0 : n - N;  // the last group moves back to stay whole
      Fq x[4], y[4], r[4];
      for (size_t k = 0; k < N; k++) x[k] = fq_at(a, g + k), y[k] = fq_at(b, g + k);
      if (N == 3) msmh::fq_mul_n<3>(r, x, y);
      else msmh::fq_mul_n<4>(r, x, y);
      for (size_t k = 0; k < N; k++) put(g + k, r[k]);
    }
    return MSM_OK;
  }
  for (size_t i = 0; i < n; i++) {
    if (pts) {
      const Pt p = pt_at(a, i);
      Pt r;
      if (op == 11) r = msmh::pt_add(p, pt_at(b, i));
      else if (op == 12) r = msmh::pt_add(p, pt_at(b, i), false);
      else if (op == 13) r = msmh::pt_dbl(p);
      else r = msmh::pt_dbl_n(p, op == 14 ? 1 : op == 15 ? 2 : 5);
      put_pt(i, r);
      continue;
    }
    const Fq x = fq_at(a, i);
    Fq r = x;
    if (op == 0) r = msmh::fq_mul(x, fq_at(b, i));
    else if (op == 3) r = msmh::fq_add(x, fq_at(b, i));
    else if (op == 4) r = msmh::fq_sub(x, fq_at(b, i));
    else if (op == 5) r = msmh::fq_inv(x);
    else if (op == 6) r = msmh::fq_from_std(x.l);
    else if (op == 7) msmh::fq_to_std(x, r.l);
    else msmh::div2k_mod(r.l, op == 8 ? 1 : op == 9 ? 32 : 63);
    put(i, r);
  }
  return MSM_OK;
}

// k_split_scalars on n wire scalars: out = the k * n virtual scalars of S bits (8 words each,
// element j n + i).
int msm_test_split_scalars(const uint32_t* scalars, size_t n, uint32_t k, uint32_t S, uint32_t* out) {
  if (!scalars || !out || n == 0 || n > (1u << 24) || k < 2 || k > 8 || S < 1 || S > 255)
    return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  TestBuf din, dout;
  HIPCHECK(din.alloc(n * 32));
  HIPCHECK(dout.alloc((size_t)k * n * 32));
  HIPCHECK(hipMemcpy(din.p, scalars, n * 32, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_split_scalars, dim3(grid_for(n, 256), k, 1), dim3(256), 0, 0, splat(din.p), dout.p, (uint32_t)n, k,
                     S);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpy(out, dout.p, (size_t)k * n * 32, hipMemcpyDeviceToHost));
  return MSM_OK;
}

// ---- the run accumulation's state (tests/test_gpu_acc_chains.py, tests/_acc_model.py) -------------
// What the last MSM of the default device's lone-MSM slot (slot 0) left in that slot's workspace, read
// back after the call: nothing is launched.  info = {M, K, nkeys, runs, workgroups, the skewed
// workgroups' count, whether the launch took the second (PART_JOIN) pass, c}; the count is wait_slot's
// latch of the flag word, taken before the final reduction clears skew_list[0] (profiling mode 1 runs
// the joins in line: no second pass, and the count stays 0).  Every array pointer
// may be null (call once for info, then with buffers): bucket_start [nkeys + 1], run_key [runs],
// sorted_entry [M], cross_key and lead_open [workgroups], skewed [count] (the list's order is the
// launch's own).  key_xy [nk][16] and wg_xy [nw][16] receive the affine x | y (BE words) of
// buckets[keys[i]] and lead_val[wgs[i]], converted on the host (limbs_point_to_xy_be); a slot the
// launch did not write comes back as whatever it holds.  MSM_ERR_INVALID_ARG unless the slot's last
// launch was one MSM through k_accumulate.
int msm_test_acc_state(uint32_t info[8], uint32_t* bucket_start, uint32_t* run_key, uint32_t* sorted_entry,
                       uint32_t* cross_key, uint32_t* lead_open, uint32_t* skewed, const uint32_t* keys, size_t nk,
                       uint32_t* key_xy, const uint32_t* wgs, size_t nw, uint32_t* wg_xy) {
  if (!info || (nk && (!keys || !key_xy)) || (nw && (!wgs || !wg_xy))) return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot& sl = c->slot[0];
  const Plan& pl = sl.pl;
  Workspace& w = sl.ws;
  if (pl.d.nm != 1 || pl.dense || !pl.K || !sl.h_out.p || !w.bucket_start.p || !sl.stream) return MSM_ERR_INVALID_ARG;
  HIPCHECK(hipStreamSynchronize(sl.stream));
  const size_t outb = (size_t)pl.d.W * pl.nterms * 32 * 4;
  const uint32_t M = reinterpret_cast<const uint32_t*>(sl.h_out.p)[outb / 4 + 1];
  const uint32_t nkeys = pl.d.W * pl.d.B;
  const uint32_t runs = (M + pl.K - 1) / pl.K, nwg = (runs + ACC_THREADS - 1) / ACC_THREADS;
  if (M > pl.Mmax || runs > pl.runs_max || sl.skew_seen > nwg) return MSM_ERR_INVALID_ARG;
  const uint32_t v[8] = {M, pl.K, nkeys, runs, nwg, sl.skew_seen, sl.skew_seen ? 1u : 0u, pl.d.c};
  memcpy(info, v, sizeof v);
  auto fetch = [](uint32_t* dst, const Buf& b, size_t first, size_t words) -> hipError_t {
    if (!dst || !words) return hipSuccess;
    if (!b.p || (first + words) * 4 > b.cap) return hipErrorInvalidValue;
    return hipMemcpy(dst, static_cast<const uint32_t*>(b.p) + first, words * 4, hipMemcpyDeviceToHost);
  };
  HIPCHECK(fetch(bucket_start, w.bucket_start, 0, (size_t)nkeys + 1));
  HIPCHECK(fetch(run_key, w.run_key, 0, runs));
  HIPCHECK(fetch(sorted_entry, w.sorted_entry, 0, M));
  HIPCHECK(fetch(cross_key, w.cross_key, 0, nwg));
  HIPCHECK(fetch(lead_open, w.lead_open, 0, nwg));
  HIPCHECK(fetch(skewed, w.skew_list, 1, sl.skew_seen));
  uint32_t rec[PT_WORDS];
  for (size_t i = 0; i < nk; i++) {
    if (keys[i] >= nkeys) return MSM_ERR_INVALID_ARG;
    HIPCHECK(fetch(rec, w.buckets, (size_t)keys[i] * PT_WORDS, PT_WORDS));
    limbs_point_to_xy_be(rec, key_xy + i * 16);
  }
  for (size_t i = 0; i < nw; i++) {
    if (wgs[i] >= nwg) return MSM_ERR_INVALID_ARG;
    HIPCHECK(fetch(rec, w.lead_val, (size_t)wgs[i] * PT_WORDS, PT_WORDS));
    limbs_point_to_xy_be(rec, wg_xy + i * 16);
  }
  return MSM_OK;
}

// ---- the bucket reduction's state and maps (tests/test_gpu_red_state.py, tests/_red_model.py) ------
// What the reduction of the last lone MSM of the default device's slot 0 left behind, read back after
// the call as msm_test_acc_state does: nothing is launched, and every array may be null (with its
// count 0).  info = {L, nchunks, ngroups, nv, nterms, W, B, the second stage that ran (0: k_red2_groups
// + k_red2_terms, 1: k_bucket_reduce_2, 2: k_bucket_reduce_1g + k_red2_terms), whether the first stage
// ran on lane pairs, RG_OUT, c, the widest window, then three words of a bit mask of the empty
// windows (bit w of word w / 32), 0, 0}.  chunks[i] = w * nchunks + c -> u_xy / t_xy [i][16], the affine
// x | y (BE words, limbs_point_to_xy_be) of red_U / red_T; gpts[i] = (w * ngroups + g) * RG_OUT + idx
// -> g_xy [i][16] of red_G; terms[i] = w * nterms + t -> term_xy [i][16] of the terms in h_out (host
// Montgomery X | Y | T | Z).  The identity comes back as (0, 1).  MSM_ERR_INVALID_ARG for an index past
// its table, for red_G where no launch of this plan writes it (k_bucket_reduce_2) or of an empty
// window (k_red2_groups leaves it as the previous launch wrote it), and for red_U / red_T after
// k_bucket_reduce_1g (never written).  A dense plan is read like any other.
int msm_test_red_state(uint32_t info[16], const uint32_t* chunks, size_t nc, uint32_t* u_xy, uint32_t* t_xy,
                       const uint32_t* gpts, size_t ng, uint32_t* g_xy, const uint32_t* terms, size_t nt,
                       uint32_t* term_xy) {
  if (!info || (nc && (!chunks || !u_xy || !t_xy)) || (ng && (!gpts || !g_xy)) || (nt && (!terms || !term_xy)))
    return MSM_ERR_INVALID_ARG;
  DevCtx* c;
  int rc = get_ctx(-1, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  Slot& sl = c->slot[0];
  const Plan& pl = sl.pl;
  Workspace& w = sl.ws;
  const MsmDims& d = pl.d;
  if (d.nm != 1 || !pl.L || !sl.h_out.p || !w.bucket_start.p || !sl.stream || d.W > 96) return MSM_ERR_INVALID_ARG;
  HIPCHECK(hipStreamSynchronize(sl.stream));
  const uint32_t G = red2_groups(pl);
  const bool tree = red2_tree(pl), fold = tree && red_fold();
  uint32_t v[16] = {pl.L, pl.nchunks, G, pl.nv, pl.nterms, d.W, d.B, tree ? (fold ? 2u : 0u) : 1u,
                    (!fold && red1_pairs()) ? 1u : 0u, RG_OUT, d.c};
  auto fetch = [](uint32_t* dst, const Buf& b, size_t first, size_t words) -> hipError_t {
    if (!b.p || (first + words) * 4 > b.cap) return hipErrorInvalidValue;
    return hipMemcpy(dst, static_cast<const uint32_t*>(b.p) + first, words * 4, hipMemcpyDeviceToHost);
  };
  std::vector<bool> empty(d.W);
  for (uint32_t i = 0; i < d.W; i++) {
    uint32_t a, b;
    HIPCHECK(fetch(&a, w.bucket_start, (size_t)i * d.B, 1));
    HIPCHECK(fetch(&b, w.bucket_start, (size_t)(i + 1) * d.B, 1));
    empty[i] = a == b;
    if (empty[i]) v[11 + i / 32] |= 1u << (i % 32);
  }
  memcpy(info, v, sizeof v);
  uint32_t rec[PT_WORDS];
  if (nc && fold) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < nc; i++) {
    if (chunks[i] >= d.W * pl.nchunks) return MSM_ERR_INVALID_ARG;
    HIPCHECK(fetch(rec, w.red_U, (size_t)chunks[i] * PT_WORDS, PT_WORDS));
    limbs_point_to_xy_be(rec, u_xy + i * 16);
    HIPCHECK(fetch(rec, w.red_T, (size_t)chunks[i] * PT_WORDS, PT_WORDS));
    limbs_point_to_xy_be(rec, t_xy + i * 16);
  }
  if (ng && !tree) return MSM_ERR_INVALID_ARG;
  for (size_t i = 0; i < ng; i++) {
    if (gpts[i] >= d.W * G * RG_OUT || empty[gpts[i] / (G * RG_OUT)]) return MSM_ERR_INVALID_ARG;
    HIPCHECK(fetch(rec, w.red_G, (size_t)gpts[i] * PT_WORDS, PT_WORDS));
    limbs_point_to_xy_be(rec, g_xy + i * 16);
  }
  for (size_t i = 0; i < nt; i++) {
    if (terms[i] >= d.W * pl.nterms) return MSM_ERR_INVALID_ARG;
    pt_to_be_affine(term_at(reinterpret_cast<const uint32_t*>(sl.h_out.p) + (size_t)terms[i] * 32), term_xy + i * 16);
  }
  return MSM_OK;
}

// The first stage's grid maps of the plan of nm MSMs of n points with `opts` (window width and range,
// narrow scalars; may be null) and chunks of L buckets (0: the plan's own), on the host: the very
// red1_lane / red1_group the kernels call.  info = {L, nchunks, ngroups, W, Wr, B, Wm, w0}.  lanes
// [nlanes][2] = the (window, chunk) of lane index 0 .. nlanes - 1, groups [ngrid][3] = the (window,
// group, live) of workgroup index 0 .. ngrid - 1; 0xffffffff in every word where the map returns
// false.  No device needed.
int msm_test_red_map(size_t n, uint32_t nm, const msm_opts* opts, uint32_t L, uint32_t info[8], uint32_t* lanes,
                     size_t nlanes, uint32_t* groups, size_t ngrid) {
  if (!info || nm < 1 || nm > MSM_MAX_BATCH || (nlanes && !lanes) || (ngrid && !groups) || (L && !red_l_known(L)))
    return MSM_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = make_plan(n, opts, DevShape{}, &pl, false, nm, true)) return rc;
  if (L) plan_chunks(&pl, L);
  const MsmDims& d = pl.d;
  const uint32_t G = red2_groups(pl);
  const uint32_t v[8] = {pl.L, pl.nchunks, G, d.W, d.Wr, d.B, d.Wm, d.w0};
  memcpy(info, v, sizeof v);
  for (size_t i = 0; i < nlanes; i++) {
    uint32_t w = ~0u, c = ~0u;
    if (!red1_lane(d, pl.L, pl.nchunks, (uint32_t)i, w, c)) w = c = ~0u;
    lanes[2 * i] = w;
    lanes[2 * i + 1] = c;
  }
  for (size_t i = 0; i < ngrid; i++) {
    uint32_t w = ~0u, g = ~0u;
    bool live = false;
    const bool ok = red1_group(d, pl.L, pl.nchunks, G, (uint32_t)i, w, g, live);
    groups[3 * i] = ok ? w : ~0u;
    groups[3 * i + 1] = ok ? g : ~0u;
    groups[3 * i + 2] = ok ? (live ? 1u : 0u) : ~0u;
  }
  return MSM_OK;
}

// k_red2_terms' map on the host: red2_term(term, nv, ngroups) as out = {idx, g0, g1, kbit, npts,
// bitsel}, and groups[j] = red2_term_group(j) for j < min(npts, cap).  No device needed.
int msm_test_red_map_term(uint32_t nv, uint32_t ngroups, uint32_t term, uint32_t out[6], uint32_t* groups, size_t cap) {
  if (!out || nv < 1 || ngroups < 1 || (cap && !groups)) return MSM_ERR_INVALID_ARG;
  const Red2Term t = red2_term(term, nv, ngroups);
  const uint32_t v[6] = {t.idx, t.g0, t.g1, t.kbit, t.npts, t.bitsel ? 1u : 0u};
  memcpy(out, v, sizeof v);
  for (uint32_t j = 0; j < t.npts && j < cap; j++) groups[j] = red2_term_group(t, j);
  return MSM_OK;
}

// msm_test_tail for a plan of the caller's: one MSM of n points with `opts` (window width and range;
// may be null) and chunks of L buckets (0: the plan's own).  info = {Wr, nterms, nv, L, w0, Wm}; with
// terms (Wr * nterms * 32 words, as msm_test_tail reads them) the tail's affine result: helpers = 0
// runs horner_tail, otherwise a TailCrew of that many threads.  No device needed.
int msm_test_tail_plan(size_t n, const msm_opts* opts, uint32_t L, const uint32_t* terms, int helpers,
                       uint32_t info[6], uint32_t out_xy_be[16]) {
  if (!info || helpers < 0 || helpers > 16 || (terms && !out_xy_be) || (L && !red_l_known(L))) return MSM_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = make_plan(n, opts, DevShape{}, &pl)) return rc;
  if (L) plan_chunks(&pl, L);
  const uint32_t v[6] = {pl.d.Wr, pl.nterms, pl.nv, pl.L, pl.d.w0, pl.d.Wm};
  memcpy(info, v, sizeof v);
  if (!terms) return MSM_OK;
  TailCrew crew(helpers);
  crew.arm();
  const Pt r = helpers ? crew.run(pl, terms) : horner_tail(pl, terms);
  crew.disarm();
  pt_to_be_affine(r, out_xy_be);
  return MSM_OK;
}

// ---- guarded workspaces (host_ctx.h g_guard, host_guard.h; tests/test_gpu_guard.py) ---------------
// The name of buffer index `id` in the guard reports (null past the table's end).  No device needed.
const char* msm_test_guard_name(uint32_t id) {
  const auto& v = guard_names();
  return id < v.size() ? v[id] : nullptr;
}

// Sets the guard switch and returns its previous value (0 / 1).  MSM_ERR_INVALID_ARG while a device
// context or a handle holds an allocation made in the other mode (run msm_shutdown first): one process
// never mixes the two layouts.
int msm_test_guard(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  const bool prev = g_guard.load();
  if ((on != 0) == prev) return prev ? 1 : 0;
  bool held = false;
  auto seen = [&](const char*, Buf& b) { held = held || b.p; };
  for (DevCtx* c : g_ctx) {
    if (!c) continue;
    std::lock_guard<std::mutex> lk2(c->mu);
    c->each_buf(seen);
    for (Slot& sl : c->slot) {
      sl.ws.each_buf(seen);
      held = held || sl.h_out.p;
    }
  }
  for (auto& kv : g_bases) kv.second->each_buf(seen);
  for (auto& kv : g_fixed) kv.second->each_buf(seen);
  if (held) return MSM_ERR_INVALID_ARG;
  g_guard.store(on != 0);
  return prev ? 1 : 0;
}

// Frees every slot's workspace and result buffer and the context's own buffers, with the captured
// graphs that point into them; handles stay.  The next call allocates every buffer at exactly its own
// plan's size (guarded or not).
int msm_test_guard_release(int device) {
  return guard_each_ctx(device, [](DevCtx* c) -> int {
    g_alloc_gen.fetch_add(1);
    c->each_buf([](const char*, Buf& b) { b.release(); });
    for (Slot& sl : c->slot) {
      sl.ws.release();
      for (Segment& sg : sl.seg) sg.drop();
      sl.h_out.release();
      sl.h_out_dev = nullptr;
    }
    return MSM_OK;
  });
}

// Reads every guard band back, and the payload of the five buffers the kernels keep all-zero between
// MSMs (err, lead_flag, skew_list[0], colsum, bin_cur): one GuardHit per touched band or broken
// invariant, over the slots, the contexts' own buffers and the live handles' records, and what a
// handle's preparation left behind.  What is reported is repaired (guards refilled, words cleared), so
// the next check reports it no more.  Writes at most `cap` records; *count is the number found.
int msm_test_guard_check(int device, GuardHit* report, size_t cap, size_t* count) {
  if (!count || (!report && cap)) return MSM_ERR_INVALID_ARG;
  std::vector<GuardHit> hits;
  int rc = guard_each_ctx(device, [&](DevCtx* c) -> int {
    const int dev = c->device;
    int r = MSM_OK;
    for (int si = 0; si < NSLOT; si++) {
      Slot& sl = c->slot[si];
      Workspace& w = sl.ws;
      uint32_t id = 0;
      w.each_buf([&](const char*, Buf& b) {
        if (r == MSM_OK) r = guard_scan(b, id, dev, si, &hits);
        id++;
      });
      guard_scan_host(sl.h_out, guard_id("h_out"), dev, si, &hits);
      struct Zero {
        const char* name;
        Buf* b;
        size_t bytes;
      } zeros[] = {{"err", &w.err, w.err.cap},
                   {"lead_flag", &w.lead_flag, w.lead_flag.cap},
                   {"skew_list", &w.skew_list, 4},
                   {"colsum", &w.colsum, w.colsum.cap},
                   {"bin_cur", &w.bin_cur, w.bin_cur.cap}};
      for (const Zero& z : zeros)
        if (r == MSM_OK) r = guard_scan_zero(*z.b, z.bytes, guard_id(z.name), dev, si, &hits);
    }
    c->each_buf([&](const char* n, Buf& b) {
      if (r == MSM_OK) r = guard_scan(b, guard_id(n), dev, -1, &hits);
    });
    for (auto& kv : g_bases)
      if (kv.second->device == dev)
        kv.second->each_buf([&](const char* n, Buf& b) {
          if (r == MSM_OK) r = guard_scan(b, guard_id(n), dev, -1, &hits);
        });
    for (auto& kv : g_fixed)
      if (kv.second->device == dev)
        kv.second->each_buf([&](const char* n, Buf& b) {
          if (r == MSM_OK) r = guard_scan(b, guard_id(n), dev, -1, &hits);
        });
    return r;
  });
  if (rc != MSM_OK) return rc;
  {
    std::lock_guard<std::mutex> gl(g_guard_mu);
    for (auto it = g_guard_pending.begin(); it != g_guard_pending.end();)
      if (device < 0 || it->device == device) {
        hits.push_back(*it);
        it = g_guard_pending.erase(it);
      } else {
        ++it;
      }
  }
  *count = hits.size();
  for (size_t i = 0; i < hits.size() && i < cap; i++) report[i] = hits[i];
  return MSM_OK;
}

// The check's self-test: one byte written with hipMemset (no kernel runs) into buffer `buffer` (an
// index of msm_test_guard_name's table) of slot `slot` -- where 0: the first byte of the back guard,
// 1: its last byte, 2: the last byte of the front guard, 3: the second payload word.  Every place
// lies inside the allocation.  MSM_ERR_INVALID_ARG for a buffer that is not allocated, for a guard of
// one that is not guarded, and for a payload shorter than two words.
int msm_test_guard_plant(int device, int slot, uint32_t buffer, int where) {
  if (slot < 0 || slot >= NSLOT || where < 0 || where > 3) return MSM_ERR_INVALID_ARG;
  bool found = false;
  int rc = guard_each_ctx(device, [&](DevCtx* c) -> int {
    int r = MSM_ERR_INVALID_ARG;
    uint32_t id = 0;
    c->slot[slot].ws.each_buf([&](const char*, Buf& b) {
      if (id++ != buffer || found) return;
      found = true;
      if (!b.p || (where < 3 && !b.base) || (where == 3 && b.cap < 8)) return;
      char* p = static_cast<char*>(b.p);
      char* at = where == 0 ? p + b.cap : where == 1 ? p + b.cap + GUARD_BACK - 1 : where == 2 ? p - 1 : p + 4;
      r = hipMemset(at, 0x5A, 1) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess ? MSM_OK : MSM_ERR_HIP;
    });
    return r;
  });
  return found ? rc : MSM_ERR_INVALID_ARG;
}

// ---- poisoned payloads (host_ctx.h g_guard_word; tests/test_gpu_poison.py) -------------------------
// Sets the word guarded allocations write over their payload and returns the previous one; the reasoning
// that bounds it is host_ctx.h's.  MSM_ERR_INVALID_ARG for a word above GUARD_WORD_MAX.  It changes
// allocations made after the call, and nothing while the guard switch is off.  No device needed.
int msm_test_guard_fill(uint32_t word) {
  if (word > GUARD_WORD_MAX) return MSM_ERR_INVALID_ARG;
  return (int)g_guard_word.exchange(word);
}

// Overwrites, at quiescence, the payload of every guarded buffer of the device's context (every context
// for device < 0) with the current fill word: every slot's workspace, its h_out, and the context's
// shared_pts, host_sc and host_pts.  Nothing is freed and no graph is dropped, so the next call replays
// its cached graph onto a workspace that holds nothing of the launch before it.  Left out, by name:
//   err, lead_flag, colsum, bin_cur (whole) and skew_list[0] -- the five regions the kernels keep all-zero
//     between MSMs (ensure_workspace starts that invariant only after a reallocation, so these do carry
//     state from call to call: msm_test_guard_check's zero scan is what watches them);
//   a handle's and a table's records (bases_rec) -- live state, the inputs of the calls to come.
// No other buffer carries anything across calls: shared_pts is prepared again by every
// msm_compute_shared* call (ManyRun::setup), host_sc and host_pts are uploaded whole by every split call,
// and the preparation's error word (bases_prep_err) does not outlive its call.  Nothing while the guard
// switch is off.
int msm_test_guard_poison(int device) {
  if (!g_guard.load()) return MSM_OK;
  const uint32_t word = g_guard_word.load();
  return guard_each_ctx(device, [&](DevCtx* c) -> int {
    int r = MSM_OK;
    for (Slot& sl : c->slot) {
      Workspace& w = sl.ws;
      w.each_buf([&](const char*, Buf& b) {
        if (&b == &w.err || &b == &w.lead_flag || &b == &w.colsum || &b == &w.bin_cur) return;
        if (r == MSM_OK) r = guard_poison(b, &b == &w.skew_list ? 4 : 0, word);
      });
      guard_poison_host(sl.h_out, word);
    }
    c->each_buf([&](const char*, Buf& b) {
      if (r == MSM_OK) r = guard_poison(b, 0, word);
    });
    if (r == MSM_OK && hipStreamSynchronize(nullptr) != hipSuccess) r = MSM_ERR_HIP;
    return r;
  });
}

// Copies `words` payload words of buffer `buffer` (an index of msm_test_guard_name's table) from word
// `first_word` on into out: a workspace buffer or the h_out of slot `slot`, or one of the context's own
// buffers (the slot is not looked at).  Nothing is launched.  MSM_ERR_INVALID_ARG for a range that is
// empty or not inside the payload, a buffer that is not allocated, a handle's buffers (there may be
// many), an id past the table, and where the device has no context.
int msm_test_guard_peek(int device, int slot, uint32_t buffer, size_t first_word, size_t words, uint32_t* out) {
  const size_t nws = guard_id("h_out");
  if (!out || !words || buffer >= guard_names().size() || (buffer <= nws && (slot < 0 || slot >= NSLOT)))
    return MSM_ERR_INVALID_ARG;
  if (first_word > (SIZE_MAX / 4) - words) return MSM_ERR_INVALID_ARG;
  bool found = false;
  int rc = guard_each_ctx(device, [&](DevCtx* c) -> int {
    if (found) return MSM_OK;
    found = true;
    const void* p = nullptr;
    size_t cap = 0;
    bool host = false;
    uint32_t id = 0;
    auto pick = [&](const char*, Buf& b) {
      if (id++ == buffer) p = b.p, cap = b.cap;
    };
    if (buffer < nws) {
      c->slot[slot].ws.each_buf(pick);
    } else if (buffer == nws) {
      p = c->slot[slot].h_out.p, cap = c->slot[slot].h_out.cap, host = true;
    } else {
      id = (uint32_t)nws + 1;
      c->each_buf(pick);
    }
    if (!p || (first_word + words) * 4 > cap) return MSM_ERR_INVALID_ARG;
    const uint32_t* src = static_cast<const uint32_t*>(p) + first_word;
    if (host) {
      memcpy(out, src, words * 4);
      return MSM_OK;
    }
    HIPCHECK(hipMemcpy(out, src, words * 4, hipMemcpyDeviceToHost));
    return MSM_OK;
  });
  return found ? rc : MSM_ERR_INVALID_ARG;
}

#ifdef MSM_PHASE_PROBE
// Tuning builds only: writes the sort kernels' phase stamps of the last launch (g_probe) to `path`.
int msm_test_probe_dump(const char* path) {
  static std::vector<uint64_t> buf(sizeof(g_probe) / 8);
  if (hipDeviceSynchronize() != hipSuccess) return MSM_ERR_HIP;
  if (hipMemcpyFromSymbol(buf.data(), HIP_SYMBOL(g_probe), sizeof(g_probe), 0, hipMemcpyDeviceToHost) != hipSuccess)
    return MSM_ERR_HIP;
  FILE* f = fopen(path, "wb");
  if (!f) return MSM_ERR_INVALID_ARG;
  fwrite(buf.data(), 8, buf.size(), f);
  fclose(f);
  return MSM_OK;
}
#endif

}  // extern "C"
