// Layer 5, one launch: workspaces, the kernel tables (recode_kernel, scatter_kernel, RED1_TABLE), the arguments
// of the repointable kernels (PrepareArgs, RecodeArgs), the launch sequence (enqueue_msm over LaunchCtx's stages), its
// captured graphs, waiting for a slot and finishing its MSMs.  Depends on the layers above it (knobs, ctx, plan, tail).
#pragma once
// (`own_pts` false: the launch reads a handle's resident records, the slot needs no record buffer.)
int ensure_workspace(DevCtx* c, const Plan& pl, int si, bool own_pts = true) {
  Slot& sl0 = c->slot[si];
  Workspace& w = sl0.ws;
  const MsmDims& d = pl.d;
  const size_t nb = (size_t)d.W * d.B;
  int rc;
  const uint64_t gen0 = g_alloc_gen.load();
#define ENS(buf, bytes) \
  if ((rc = w.buf.ensure(bytes)) != MSM_OK) return rc
  ENS(pts, own_pts ? (size_t)(d.shared ? 1 : d.nm) * d.n * PRE_WORDS * 4 : 0);
  ENS(err, 16);
  ENS(digits, (size_t)d.W * d.n * 4);
  ENS(colsum, ((size_t)d.nbins + d.W) * 4);  // bin totals, then window totals
  ENS(bin_base, ((size_t)d.nbins + 1) * 4);
  ENS(bin_cur, (size_t)d.nbins * 4);
  ENS(part_entry, pl.Mmax * 4);
  ENS(part_fine, pl.Mmax * 2);
  ENS(sorted_entry, pl.Mmax * 4 + 16);  // + a 16-B tail for k_accumulate's vector entry loads
  ENS(bucket_start, (nb + 2) * 4);
  ENS(run_key, pl.runs_max * 4);
#ifdef MSM_DUMMY_ALLOC
  ENS(dummy_tiles, (pl.Mmax / FS_CAP + d.nbins + 1) * 8 + 8);
  ENS(dummy_cursor, nb * 4);
#endif
  ENS(buckets, nb * PT_WORDS * 4);
  const size_t nwg = pl.runs_max / ACC_THREADS + 2;
  ENS(lead_val, nwg * PT_WORDS * 4);
  ENS(lead_open, nwg * 4);
  ENS(cross_key, nwg * 4);
  ENS(lead_flag, 16);
  ENS(skew_list, (nwg + 1) * 4);
  ENS(g_head, pl.runs_max * PT_WORDS * 4);  // touched only by skewed workgroups
  ENS(g_hkey, pl.runs_max * 4);
  ENS(g_tkey, pl.runs_max * 4);
  ENS(red_U, (size_t)d.W * pl.nchunks * PT_WORDS * 4);
  ENS(red_T, (size_t)d.W * pl.nchunks * PT_WORDS * 4);
  if (red2_tree(pl)) ENS(red_G, (size_t)d.W * red2_groups(pl) * RG_OUT * PT_WORDS * 4);
  if (pl.dense) {
    ENS(seg_base, (nb + 1) * 4);
    ENS(unit_key, (size_t)pl.dense_units * 4);
    ENS(partials, (size_t)pl.dense_units * PT_WORDS * 4);
  }
#undef ENS
  if (g_alloc_gen.load() != gen0) {
    // err, lead_flag, colsum and bin_cur are kept all-zero between MSMs by the kernels themselves
    // (k_bucket_reduce_2 clears the flags, k_fine_sort the bin totals and cursors), so a
    // replayed graph needs no memset nodes; fresh allocations start that invariant here.
    hipStream_t st = sl0.stream;
    if (hipMemsetAsync(w.err.p, 0, w.err.cap, st) != hipSuccess ||
        hipMemsetAsync(w.lead_flag.p, 0, w.lead_flag.cap, st) != hipSuccess ||
        hipMemsetAsync(w.skew_list.p, 0, 4, st) != hipSuccess ||
        hipMemsetAsync(w.colsum.p, 0, w.colsum.cap, st) != hipSuccess ||
        hipMemsetAsync(w.bin_cur.p, 0, w.bin_cur.cap, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return MSM_ERR_HIP;
  }
  const size_t hbytes = (size_t)d.W * pl.nterms * 32 * 4 + 64;
  if (hbytes > sl0.h_out.cap || !sl0.h_out_dev) {
    if ((rc = sl0.h_out.ensure(hbytes, true)) != MSM_OK) return rc;
    if (hipHostGetDevicePointer(&sl0.h_out_dev, sl0.h_out.p, 0) != hipSuccess) return MSM_ERR_HIP;
  }
  return MSM_OK;
}

inline unsigned grid_for(size_t threads, unsigned block) { return (unsigned)((threads + block - 1) / block); }
template <typename F>  // a kernel as hipLaunchKernel and a graph's kernel node name it
const void* kfn(F* kernel) { return reinterpret_cast<const void*>(kernel); }

bool slot_forks(const Slot& sl) { return sl.pipelined ? fork_prepare() && fork_prepare_pipelined() : fork_prepare(); }

// Whether k_prepare_points writes `records` point records with nontemporal stores: only when they
// outgrow the Infinity Cache (>= 128 MiB, i.e. 2^20 records; MSM_PP_NT=0/1 forces it).
uint32_t prep_nt(size_t records) {
  if (knob_pp_nt() >= 0) return knob_pp_nt() ? 1u : 0u;
  return records * 128 >= (size_t(1) << 27) ? 1u : 0u;
}

// k_prepare_points' arguments and launch, assembled here alone.  argv is the array hipLaunchKernel and
// hipKernelNodeParams take; it points into the struct, which therefore does not copy.
struct PrepareArgs {
  BatchPtrs wires;
  uint32_t* pts;
  uint32_t n;
  uint32_t* err;
  uint32_t nt, fmt;
  unsigned ny;  // wire buffers read: the grid's y
  void* argv[6] = {&wires, &pts, &n, &err, &nt, &fmt};
  PrepareArgs(const BatchPtrs& wires, uint32_t* pts, uint32_t n, uint32_t* err, uint32_t nt, uint32_t fmt, unsigned ny)
      : wires(wires), pts(pts), n(n), err(err), nt(nt), fmt(fmt), ny(ny) {}
  // a launch's own preparation: every MSM's points (one vector where they share it) into `pts`
  PrepareArgs(const Plan& pl, Slot& sl, const BatchPtrs& points, uint32_t* pts)
      : PrepareArgs(points, pts, pl.d.n, sl.ws.err.as<uint32_t>(),
                    prep_nt((size_t)(pl.d.shared ? 1 : pl.d.nm) * pl.d.n), pl.pfmt, pl.d.shared ? 1 : pl.d.nm) {}
  PrepareArgs(const PrepareArgs&) = delete;
  void launch(hipStream_t s) {
    (void)hipLaunchKernel(kfn(k_prepare_points), dim3(grid_for(n, PP_THREADS), ny), dim3(PP_THREADS), argv, 0, s);
  }
};

// k_prepare_points over `cnt` points of one wire buffer into `pts_out` (one MSM, or one uploaded
// chunk of it); `nt` from prep_nt of the whole record buffer.
void launch_prepare(const uint32_t* wire, uint32_t* pts_out, uint32_t cnt, uint32_t* err, uint32_t nt,
                    hipStream_t s, uint32_t fmt = PT_FMT_WIRE) {
  PrepareArgs(BatchPtrs{{wire}}, pts_out, cnt, err, nt, fmt, 1).launch(s);
}

// The bias C = sum_w (2^(b_w - 1) - 1) 2^off_w of the narrow, native and wide recodes over the
// launch's windows (the sum stays below 2^(T - 1), so it fits the scalar's own words).
NarrowBias narrow_bias(const MsmDims& d) {
  NarrowBias nb{};
  for (uint32_t w = 0; w < d.Wr; w++) {
    const uint64_t h = (1ull << (win_bits(d, w) - 1)) - 1ull;  // < 2^20: spans at most two words
    const uint32_t o = win_off(d, w), k = o / 32, sh = o % 32;
    uint64_t carry = h << sh;
    for (uint32_t j = k; j < 8 && carry; j++) {
      const uint64_t x = (uint64_t)nb.v[j] + (carry & 0xffffffffull);
      nb.v[j] = (uint32_t)x;
      carry = (carry >> 32) + (x >> 32);
    }
  }
  return nb;
}

// The biased recode kernels (all take k_recode_narrow's six arguments): a row per scalar format -- the
// narrow word counts (Plan::stype 0, MsmDims::sw), the native types and the wide kinds (Plan::stype) --
// and a column per code width.  MSM_SCALAR_U32 has the bytes of the one-word narrow format.
struct RecodeRow {
  uint32_t stype, sw;
  const void* fn[2];  // 16-bit codes, 32-bit codes (c > 16)
};
#define RECODE_ROW(stype, sw, K, ...) {stype, sw, {kfn(K<uint16_t, __VA_ARGS__>), kfn(K<uint32_t, __VA_ARGS__>)}}
const RecodeRow RECODE_TABLE[] = {
    RECODE_ROW(0, 1, k_recode_narrow, 1),
    RECODE_ROW(0, 2, k_recode_narrow, 2),
    RECODE_ROW(0, 3, k_recode_narrow, 3),
    RECODE_ROW(0, 4, k_recode_narrow, 4),
    RECODE_ROW(0, 5, k_recode_narrow, 5),
    RECODE_ROW(0, 6, k_recode_narrow, 6),
    RECODE_ROW(0, 7, k_recode_narrow, 7),
    RECODE_ROW(0, 8, k_recode_narrow, 8),
    RECODE_ROW(MSM_SCALAR_BIT, 0, k_recode_native, 1, false),
    RECODE_ROW(MSM_SCALAR_U8, 0, k_recode_native, 8, false),
    RECODE_ROW(MSM_SCALAR_I8, 0, k_recode_native, 8, true),
    RECODE_ROW(MSM_SCALAR_U16, 0, k_recode_native, 16, false),
    RECODE_ROW(MSM_SCALAR_I16, 0, k_recode_native, 16, true),
    RECODE_ROW(MSM_SCALAR_U32, 0, k_recode_narrow, 1),
    RECODE_ROW(MSM_SCALAR_I32, 0, k_recode_native, 32, true),
    RECODE_ROW(MSM_SCALAR_U64, 0, k_recode_native, 64, false),
    RECODE_ROW(MSM_SCALAR_I64, 0, k_recode_native, 64, true),
    RECODE_ROW(STYPE_U128, 0, k_recode_wide, 4, WIDE_U),
    RECODE_ROW(STYPE_I128, 0, k_recode_wide, 4, WIDE_I),
    RECODE_ROW(STYPE_U256, 0, k_recode_wide, 8, WIDE_U),
    RECODE_ROW(STYPE_FR_MONT, 0, k_recode_wide, 8, WIDE_MONT),
};
#undef RECODE_ROW
// The four-argument recodes of 8-word scalars: k_recode_hist (wire words; [1]: k_recode_hist_le, little-endian
// words) by code width, and the geometries k_recode_fixed is unrolled for, [1] with FULL (every window whole).
const void* const RECODE_HIST[2][2] = {{kfn(k_recode_hist<uint16_t>), kfn(k_recode_hist<uint32_t>)},
                                       {kfn(k_recode_hist_le<uint16_t>), kfn(k_recode_hist_le<uint32_t>)}};
struct RecodeFixedRow {
  uint32_t q, nhi;
  const void* fn[2];
};
#define RECODE_FIXED_ROW(Q, NHI) {Q, NHI, {kfn(k_recode_fixed<Q, NHI, false>), kfn(k_recode_fixed<Q, NHI, true>)}}
const RecodeFixedRow RECODE_FIXED[] = {RECODE_FIXED_ROW(15, 14), RECODE_FIXED_ROW(14, 16), RECODE_FIXED_ROW(13, 7),
                                       RECODE_FIXED_ROW(12, 14)};
#undef RECODE_FIXED_ROW

// The recode kernel of a plan, and how many arguments it takes: four, or RECODE_TABLE's six.
struct RecodeKernel {
  const void* fn;
  unsigned nargs;
};
RecodeKernel recode_kernel(const Plan& pl) {
  const MsmDims& d = pl.d;
  const bool wide = d.c > 16;  // 32-bit codes
  if (d.sw) {
    for (const RecodeRow& r : RECODE_TABLE)
      if (r.stype == pl.stype && (pl.stype || r.sw == d.sw)) return {r.fn[wide], 6};
    return {nullptr, 6};  // (make_plan admits no other type)
  }
  // (a typed plan here is a 256-bit integer of 254 bits and more: the full-width geometry)
  if (pl.stype) return {RECODE_HIST[1][wide], 4};
  if (!wide && recode_fixed_on()) {
    const bool full = d.w0 == 0 && d.Wr == d.Wm && !d.half_lo && !d.half_hi;
    for (const RecodeFixedRow& r : RECODE_FIXED)
      if (r.q == d.q && r.nhi == d.nhi) return {r.fn[full], 4};
  }
  return {RECODE_HIST[0][wide], 4};
}
// Every recode kernel, from the tables recode_kernel picks from: a replayed graph must not read the
// previous call's scalars, whatever their format.
bool is_recode_kernel(const void* f) {
  for (const auto& pair : RECODE_HIST)
    if (f == pair[0] || f == pair[1]) return true;
  for (const RecodeFixedRow& r : RECODE_FIXED)
    if (f == r.fn[0] || f == r.fn[1]) return true;
  for (const RecodeRow& r : RECODE_TABLE)
    if (f == r.fn[0] || f == r.fn[1]) return true;
  return false;
}

// A recode kernel's arguments and launch: argv holds as many entries as the plan's kernel has
// parameters (it points into the struct, which therefore does not copy).
struct RecodeArgs {
  RecodeKernel k;
  BatchPtrs scalars;
  MsmDims d;
  void* digits;
  uint32_t* colsum;
  NarrowBias nb;
  uint32_t* err;
  void* argv[6] = {&scalars, &d, &digits, &colsum, &nb, &err};
  RecodeArgs(const Plan& pl, Slot& sl, const BatchPtrs& scalars)
      : k(recode_kernel(pl)), scalars(scalars), d(pl.d), digits(sl.ws.digits.p), colsum(sl.ws.colsum.as<uint32_t>()),
        nb(k.nargs == 6 ? narrow_bias(pl.d) : NarrowBias{}), err(sl.ws.err.as<uint32_t>()) {
    if (k.nargs == 4) argv[4] = argv[5] = nullptr;
  }
  RecodeArgs(const RecodeArgs&) = delete;
  void launch(hipStream_t s) {
    const size_t lds = ((size_t)d.Wr * d.nbc + d.Wr) * 4;  // histogram + window totals
    (void)hipLaunchKernel(k.fn, dim3(grid_for(d.n, RC_SPAN), d.nm), dim3(RC_THREADS), argv, lds, s);
  }
};

// k_part_scatter's instantiation for a plan's code width and subset kind (MsmDims::sub); the subset
// variants take one more argument, the index buffer.
const void* scatter_kernel(const MsmDims& d) {
  using I = const uint32_t*;
#define SCATTER_ROW(T) \
  {kfn(k_part_scatter<T>), kfn(k_part_scatter<T, MSM_SUB_RANGE, I>), kfn(k_part_scatter<T, MSM_SUB_INDEXED, I>)}
  static const void* const K[2][3] = {SCATTER_ROW(uint16_t), SCATTER_ROW(uint32_t)};
#undef SCATTER_ROW
  static_assert(MSM_SUB_NONE == 0 && MSM_SUB_RANGE == 1 && MSM_SUB_INDEXED == 2, "K's columns");
  return K[d.c > 16][d.sub];
}

// The first reduction stage's kernels, a row per chunk length of RED1_LENGTHS (host_plan.h).
struct Red1Row {
  uint32_t L;
  decltype(&k_bucket_reduce_1<8>) lanes, pairs;  // one lane per chunk; lane pairs (MSM_RED1_PAIRS)
  decltype(&k_bucket_reduce_1g<8>) fold;         // with the second stage's group trees (MSM_RED_FOLD)
};
#define RED1_ROW(L) {L, k_bucket_reduce_1<L>, k_bucket_reduce_1p<L>, k_bucket_reduce_1g<L>}
const Red1Row RED1_TABLE[] = {RED1_LENGTHS(RED1_ROW)};
#undef RED1_ROW
const Red1Row* red1_row(uint32_t L) {
  for (const Red1Row& r : RED1_TABLE)
    if (r.L == L) return &r;
  return nullptr;
}

// The stages of one launch sequence (enqueue_msm puts them in order), over what they share: the plan,
// the slot whose workspace they work in, their stream and the point-record buffer.
struct LaunchCtx {
  const Plan& pl;
  const MsmDims& d;
  Slot& sl;
  Workspace& w;
  hipStream_t s;
  uint32_t* pts;
  static uint32_t* u32(const Buf& b) { return b.as<uint32_t>(); }
  const uint32_t* total() const { return u32(w.bin_base) + d.nbins; }  // the launch's entry count
  // The preparation, on `ps`: the launch's stream, or the slot's aux stream where it forks.
  void launch_prepare(const BatchPtrs& in, hipStream_t ps) const { PrepareArgs(pl, sl, in, pts).launch(ps); }
  // The sort: recode (digits and bin counts), coarse scatter, fine sort.
  void launch_recode(const BatchPtrs& d_scalars) const { RecodeArgs(pl, sl, d_scalars).launch(s); }
  void launch_scatter() const {
    MsmDims dd = d;
    void* digits = w.digits.p;
    uint32_t *colsum = u32(w.colsum), *bin_cur = u32(w.bin_cur), *bin_base = u32(w.bin_base);
    uint32_t* part_entry = u32(w.part_entry);
    uint16_t* part_fine = w.part_fine.as<uint16_t>();
    // a subset launch on a handle's records: the record-mapping variants read the slot's own index
    // buffer (a fixed address: the captured node never holds a caller's pointer)
    const uint32_t* sub_idx = w.sub_idx.as<uint32_t>();
    void* args[8] = {&digits, &dd, &colsum, &bin_cur, &bin_base, &part_entry, &part_fine};
    if (d.sub != MSM_SUB_NONE) args[7] = &sub_idx;
    (void)hipLaunchKernel(scatter_kernel(d), dim3(d.nch, d.W), dim3(PT_THREADS), args, (size_t)d.nbc * 12, s);
  }
  void launch_fine_sort() const {
    hipLaunchKernelGGL(k_fine_sort, dim3(d.nbins), dim3(FS_THREADS), 0, s, u32(w.part_entry),
                       w.part_fine.as<uint16_t>(), u32(w.bin_base), d, pl.K, u32(w.sorted_entry),
                       u32(w.bucket_start), u32(w.run_key), u32(w.colsum), u32(w.bin_cur));
#ifdef MSM_GAP_KERNEL
    hipLaunchKernelGGL(k_gap, dim3(MSM_GAP_KERNEL), dim3(64), 0, s, u32(w.err));
#endif
  }
  // The accumulation: k_accumulate, or a dense plan's k_dense_segments, k_dense_units and k_dense_fold.
  void launch_accumulation() const {
    if (!pl.dense) {
      hipLaunchKernelGGL(k_accumulate, dim3(grid_for(pl.runs_max, ACC_THREADS)), dim3(ACC_THREADS), 0, s, pts,
                         u32(w.sorted_entry), u32(w.bucket_start), u32(w.run_key), total(), pl.K, d.W * d.B,
                         u32(w.buckets), u32(w.lead_val), u32(w.lead_open), u32(w.cross_key), u32(w.skew_list),
                         u32(w.g_head), u32(w.g_hkey), u32(w.g_tkey));
      return;
    }
    // The segment map is data: k_dense_segments rebuilds it from this launch's bucket_start, so a
    // replayed graph holds nothing of any launch's bucket sizes, only the plan's grid bound.
    const uint32_t nkeys = d.W * d.B;
    const uint32_t ncross = (uint32_t)(pl.runs_max / ACC_THREADS + 2);  // ensure_workspace's cross_key words
    hipLaunchKernelGGL(k_dense_segments, dim3(1), dim3(DS_THREADS), 0, s, u32(w.bucket_start), nkeys, 64u * pl.dense_E,
                       u32(w.seg_base), u32(w.unit_key), pl.dense_units, u32(w.cross_key), pl.K * ACC_THREADS, ncross);
    hipLaunchKernelGGL(k_dense_units, dim3(grid_for(pl.dense_units, DU_THREADS / 64)), dim3(DU_THREADS), 0, s, pts,
                       u32(w.sorted_entry), u32(w.bucket_start), u32(w.seg_base), u32(w.unit_key), pl.dense_E, nkeys,
                       pl.dense_units, u32(w.buckets), u32(w.partials));
    hipLaunchKernelGGL(k_dense_fold, dim3(nkeys), dim3(DF_THREADS), 0, s, u32(w.seg_base), u32(w.partials),
                       pl.dense_units, u32(w.buckets));
  }
  // The bucket joins of skewed launches.
  void launch_joins() const {
    hipLaunchKernelGGL(k_chain_join, dim3(CJ_GRID), dim3(ACC_THREADS), 0, s, u32(w.skew_list), total(), pl.K,
                       u32(w.g_head), u32(w.g_hkey), u32(w.g_tkey), u32(w.buckets), u32(w.lead_val), u32(w.lead_open),
                       u32(w.lead_flag));
    hipLaunchKernelGGL(k_lead_scan, dim3(1), dim3(LS_THREADS), 0, s, u32(w.lead_val), u32(w.lead_open),
                       u32(w.lead_flag), total(), pl.K);
  }
  // The reduction.  Its first stage, from the plan's row of RED1_TABLE: folded with the second stage's
  // group trees (red_fold), on lane pairs (red1_pairs), or one lane per chunk.
  bool folds() const { return red_fold() && red2_tree(pl); }
  void launch_reduce_1(const Red1Row& row) const {
    const uint32_t G = red2_groups(pl);
    const bool pairs = red1_pairs();
    if (folds())
      hipLaunchKernelGGL(row.fold, dim3(d.W * G), dim3(RG_CH), 0, s, u32(w.buckets), u32(w.bucket_start), d, pl.K,
                         pl.nchunks, G, u32(w.cross_key), u32(w.lead_val), u32(w.red_G));
    else
      hipLaunchKernelGGL(pairs ? row.pairs : row.lanes,
                         dim3(grid_for((size_t)d.W * pl.nchunks * (pairs ? 2 : 1), RED1_THREADS)), dim3(RED1_THREADS),
                         0, s, u32(w.buckets), u32(w.bucket_start), d, pl.K, pl.nchunks, u32(w.cross_key),
                         u32(w.lead_val), u32(w.red_U), u32(w.red_T));
  }
  // Its second stage; the terms land in the slot's h_out.  `joins`: the bucket joins ran before it.
  void launch_reduce_2(bool joins) const {
    uint32_t* out = reinterpret_cast<uint32_t*>(sl.h_out_dev);
    if (!red2_tree(pl)) {
      hipLaunchKernelGGL(k_bucket_reduce_2, dim3(d.W * pl.nterms), dim3(RED2_THREADS), 0, s, u32(w.red_U),
                         u32(w.red_T), pl.nchunks, pl.nv, pl.nterms, u32(w.err), u32(w.lead_flag), u32(w.skew_list),
                         total(), joins ? 1u : 0u, u32(w.bucket_start), d.B, out);
      return;
    }
    const uint32_t G = red2_groups(pl);
    if (!folds())
      hipLaunchKernelGGL(k_red2_groups, dim3(d.W * G), dim3(4 * RG_CH), 0, s, u32(w.red_U), u32(w.red_T), pl.nchunks,
                         G, u32(w.bucket_start), d.B, u32(w.red_G));
    // one lane quad per group point of the widest term (a wave at least): 2^16 pipelined
    // 0.117-0.120 against 0.125-0.131 ms per MSM with 64 quads throughout
    uint32_t gp = 16;
    while (gp < G) gp <<= 1;
    hipLaunchKernelGGL(k_red2_terms, dim3(d.W * pl.nterms), dim3(4 * gp), 0, s, u32(w.red_G), G, pl.nv, pl.nterms,
                       u32(w.err), u32(w.lead_flag), u32(w.skew_list), total(), joins ? 1u : 0u, u32(w.bucket_start),
                       d.B, out);
  }
};

// Enqueue parts of the device pipeline on `s`; the reduced per-window terms land in the slot's
// h_out.  `pts` is the point-record buffer (the slot's own, or a shared base vector's).
// With `acc_events` (eager launches only), the accumulation runs between the slot's ev_acc0 /
// ev_acc1 (2), or is followed by ev_acc1 alone (1);
// captured graphs get the same events as record nodes (add_acc_event_nodes).
int enqueue_msm(DevCtx* c, const Plan& pl, const BatchPtrs& d_points, const BatchPtrs& d_scalars, int si,
                hipStream_t s, int parts, uint32_t* pts, int acc_events = 0) {
  Slot& sl = c->slot[si];
  const LaunchCtx x{pl, pl.d, sl, sl.ws, s, pts};
  const bool prof = c->profiling == 1;
  auto mark = [&](int ph) {
    if (prof) hipEventRecord(c->ev[ph], s);
  };
  const Red1Row* red1 = red1_row(pl.L);
  if ((parts & PART_POST) && !red1) return MSM_ERR_INVALID_ARG;  // (make_plan gives no such L)
  // The preparation reads only the points and the sort only the scalars: with both in this
  // sequence the preparation forks onto the slot's aux stream (a parallel branch of the captured
  // graph) and rejoins before the accumulation, so a lone MSM's sort no longer waits behind it.
  // (Profiling mode 1 keeps them in order, one event between every phase.)
  const bool fork = (parts & PART_PREP) && (parts & PART_SORT) && !prof && slot_forks(sl);
  if (parts & PART_PREP) {
    mark(PH_START);
    if (fork) {
      HIPCHECK(hipEventRecord(sl.ev_fork, s));
      HIPCHECK(hipStreamWaitEvent(sl.aux, sl.ev_fork, 0));
    }
    x.launch_prepare(d_points, fork ? sl.aux : s);
    if (fork) HIPCHECK(hipEventRecord(sl.ev_join, sl.aux));
    mark(PH_PREPARE);
  }
  if (parts & PART_SORT) {
    if (!(parts & PART_PREP)) {
      mark(PH_START);
      mark(PH_PREPARE);
    }
    x.launch_recode(d_scalars);
    mark(PH_RECODE);
    mark(PH_SCAN);
    x.launch_scatter();
    mark(PH_SCATTER);
    x.launch_fine_sort();
    mark(PH_FINE);
  }
  if (fork) HIPCHECK(hipStreamWaitEvent(s, sl.ev_join, 0));
  if ((parts & PART_ACC) && acc_events == 2) HIPCHECK(hipEventRecord(sl.ev_acc0, s));
  if (parts & PART_ACC) {
    x.launch_accumulation();
    mark(PH_ACCUM);
  }
  if ((parts & PART_ACC) && acc_events) HIPCHECK(hipEventRecord(sl.ev_acc1, s));
  // profiling mode 1 keeps the joins in line (its per-phase timings include them)
  // (a dense launch has none: no bucket continues in another lane's run, skew_list and lead_flag stay clear)
  const bool joins = ((parts & PART_JOIN) || prof) && !pl.dense;
  if ((parts & PART_POST) && joins) x.launch_joins();
  if (parts & PART_POST) {
    mark(PH_FIXUP);
    x.launch_reduce_1(*red1);
    mark(PH_RED1);
    x.launch_reduce_2(joins);
    mark(PH_RED2);
    mark(PH_READBACK);
  }
  HIPCHECK(hipGetLastError());
  return MSM_OK;
}

// Bracket the captured accumulation with event-record nodes (the slot's ev_acc0 / ev_acc1): every
// replay of the graph then times the accumulation, with no extra launches.  The accumulation is the
// k_accumulate node, or a dense plan's chain k_dense_segments -> k_dense_units -> k_dense_fold:
// ev_acc0 goes before the first of them, ev_acc1 after the last.
int add_acc_event_nodes(hipGraph_t g, Slot& sl, bool both) {
  size_t num = 0;
  if (hipGraphGetNodes(g, nullptr, &num) != hipSuccess || num == 0) return MSM_ERR_HIP;
  std::vector<hipGraphNode_t> nodes(num);
  if (hipGraphGetNodes(g, nodes.data(), &num) != hipSuccess) return MSM_ERR_HIP;
  hipGraphNode_t acc = nullptr, acc_end = nullptr;  // the accumulation's first and last node
  for (hipGraphNode_t nd : nodes) {
    hipGraphNodeType ty;
    hipKernelNodeParams kp{};
    if (hipGraphNodeGetType(nd, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel ||
        hipGraphKernelNodeGetParams(nd, &kp) != hipSuccess)
      continue;
    if (kp.func == kfn(k_accumulate)) acc = acc_end = nd;
    if (kp.func == kfn(k_dense_segments)) acc = nd;
    if (kp.func == kfn(k_dense_fold)) acc_end = nd;
  }
  if (!acc || !acc_end) return MSM_ERR_HIP;
  size_t nd = 0, nx = 0;
  if (hipGraphNodeGetDependencies(acc, nullptr, &nd) != hipSuccess ||
      hipGraphNodeGetDependentNodes(acc_end, nullptr, &nx) != hipSuccess)
    return MSM_ERR_HIP;
  std::vector<hipGraphNode_t> deps(nd), outs(nx);
  if ((nd && hipGraphNodeGetDependencies(acc, deps.data(), &nd) != hipSuccess) ||
      (nx && hipGraphNodeGetDependentNodes(acc_end, outs.data(), &nx) != hipSuccess))
    return MSM_ERR_HIP;
  hipGraphNode_t r0 = nullptr, r1 = nullptr;
  if (both) {
    for (hipGraphNode_t d : deps)
      if (hipGraphRemoveDependencies(g, &d, &acc, 1) != hipSuccess) return MSM_ERR_HIP;
    if (hipGraphAddEventRecordNode(&r0, g, deps.data(), deps.size(), sl.ev_acc0) != hipSuccess ||
        hipGraphAddDependencies(g, &r0, &acc, 1) != hipSuccess)
      return MSM_ERR_HIP;
  }
  for (hipGraphNode_t o : outs)
    if (hipGraphRemoveDependencies(g, &acc_end, &o, 1) != hipSuccess) return MSM_ERR_HIP;
  if (hipGraphAddEventRecordNode(&r1, g, &acc_end, 1, sl.ev_acc1) != hipSuccess) return MSM_ERR_HIP;
  for (hipGraphNode_t o : outs)
    if (hipGraphAddDependencies(g, &r1, &o, 1) != hipSuccess) return MSM_ERR_HIP;
  return MSM_OK;
}

int capture(DevCtx* c, const Plan& pl, const BatchPtrs& d_points, const BatchPtrs& d_scalars, int si, hipStream_t s,
            int parts, uint32_t* pts, int acc_events, hipGraph_t* gout, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return MSM_ERR_HIP;
  int rc = enqueue_msm(c, pl, d_points, d_scalars, si, s, parts, pts);
  hipError_t e = hipStreamEndCapture(s, &g);
  if (rc != MSM_OK || e != hipSuccess || !g) {
    if (g) hipGraphDestroy(g);
    (void)hipGetLastError();
    return MSM_ERR_HIP;
  }
  if (acc_events && (parts & PART_ACC) && add_acc_event_nodes(g, c->slot[si], acc_events == 2) != MSM_OK) {
    hipGraphDestroy(g);
    (void)hipGetLastError();
    return MSM_ERR_HIP;
  }
  e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    hipGraphDestroy(g);
    *out = nullptr;
    (void)hipGetLastError();
    return MSM_ERR_HIP;
  }
  *gout = g;
  return MSM_OK;
}

// Find the input-reading kernel nodes of a segment so later launches can repoint them.
int find_input_nodes(Segment& sg) {
  size_t num = 0;
  if (hipGraphGetNodes(sg.graph, nullptr, &num) != hipSuccess || num == 0) return MSM_ERR_HIP;
  std::vector<hipGraphNode_t> nodes(num);
  if (hipGraphGetNodes(sg.graph, nodes.data(), &num) != hipSuccess) return MSM_ERR_HIP;
  for (hipGraphNode_t nd : nodes) {
    hipGraphNodeType ty;
    if (hipGraphNodeGetType(nd, &ty) != hipSuccess || ty != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams kp{};
    if (hipGraphKernelNodeGetParams(nd, &kp) != hipSuccess) continue;
    if (kp.func == kfn(k_prepare_points)) {
      sg.n_prep = nd;
      sg.p_prep = kp;
    } else if (is_recode_kernel(kp.func)) {
      sg.n_recode = nd;
      sg.p_recode = kp;
    }
  }
  const bool ok = (!(sg.parts & PART_PREP) || sg.n_prep) && (!(sg.parts & PART_SORT) || sg.n_recode);
  return ok ? MSM_OK : MSM_ERR_HIP;
}

bool same_ptrs(const BatchPtrs& a, const BatchPtrs& b) { return memcmp(&a, &b, sizeof(BatchPtrs)) == 0; }

// Point an instantiated segment at new input buffers (kernel-node argument update, no
// re-capture).
int repoint_inputs(const Plan& pl, Slot& sl, Segment& sg, const BatchPtrs& d_points, const BatchPtrs& d_scalars) {
  auto set_args = [&](hipGraphNode_t nd, hipKernelNodeParams kp, void** argv) {
    kp.kernelParams = argv;
    kp.extra = nullptr;
    return hipGraphExecKernelNodeSetParams(sg.exec, nd, &kp) == hipSuccess;
  };
  if (sg.n_prep && !same_ptrs(sg.in_pts, d_points)) {
    PrepareArgs a(pl, sl, d_points, const_cast<uint32_t*>(sg.pts_buf));
    if (!set_args(sg.n_prep, sg.p_prep, a.argv)) return MSM_ERR_HIP;
    sg.in_pts = d_points;
  }
  if (sg.n_recode && !same_ptrs(sg.in_sc, d_scalars)) {
    RecodeArgs a(pl, sl, d_scalars);
    if (!set_args(sg.n_recode, sg.p_recode, a.argv)) return MSM_ERR_HIP;
    sg.in_sc = d_scalars;
  }
  return MSM_OK;
}

// The cached graph of `parts` for this plan (captured on first use, least recently used segment
// evicted), repointed at the launch's inputs; nullptr when graphs are unavailable.
Segment* get_segment(DevCtx* c, const Plan& pl, const BatchPtrs& d_points, const BatchPtrs& d_scalars, int si,
                     int parts, uint32_t* pts, int acc_events) {
  Slot& sl = c->slot[si];
  const uint64_t gen = g_alloc_gen.load();
  Segment* hit = nullptr;
  for (Segment& sg : sl.seg)
    if (sg.exec && sg.parts == parts && sg.pts_buf == pts && sg.acc_events == acc_events && sg.gen == gen &&
        sg.fork == slot_forks(sl) && plan_eq(sg.pl, pl))
      hit = &sg;
  if (!hit) {
    Segment* victim = &sl.seg[0];
    for (Segment& sg : sl.seg) {
      if (!sg.exec || sg.gen != gen) {
        victim = &sg;
        break;
      }
      if (sg.used < victim->used) victim = &sg;
    }
    victim->drop();
    victim->pl = pl;
    victim->parts = parts;
    victim->pts_buf = pts;
    victim->acc_events = acc_events;
    victim->fork = slot_forks(sl);
    victim->gen = gen;
    int rc = capture(c, pl, d_points, d_scalars, si, sl.stream, parts, pts, acc_events, &victim->graph,
                     &victim->exec);
    if (rc == MSM_OK) rc = find_input_nodes(*victim);
    if (rc != MSM_OK) {
      victim->drop();
      // event-record nodes unsupported: time k_accumulate eagerly between graph segments;
      // otherwise capture itself is unsupported here: stay eager
      if (acc_events) c->graph_events_ok = false;
      else c->graphs_ok = false;
      return nullptr;
    }
    victim->in_pts = d_points;
    victim->in_sc = d_scalars;
    hit = victim;
  }
  if (repoint_inputs(pl, sl, *hit, d_points, d_scalars) != MSM_OK) {
    hit->drop();
    (void)hipGetLastError();
    c->graphs_ok = false;
    return nullptr;
  }
  hit->used = ++sl.seg_clock;
  return hit;
}

// Enqueue `parts` of one launch in slot `si` (on the slot's stream) by replaying the captured
// graph of those parts; k_accumulate runs between the slot's two timing events on every launch
// (event-record nodes inside the graph), so the production path is the timed one.  Where the
// runtime cannot capture event records, the accumulation is launched eagerly between a graph of
// the parts before it and one of the parts after it.  Profiling mode 1 launches everything
// eagerly with an event between every phase.
int launch_on(DevCtx* c, const Plan& pl, const BatchPtrs& d_points, const BatchPtrs& d_scalars, int si, int parts,
              uint32_t* pts, hipStream_t s) {
  // k_accumulate's bracketing events only when profiling mode 2 reads them: each event-record
  // node adds ~6 us to the launch sequence's critical path (profiles/r3/latency_timeline.txt)
  // (a staggered slot's graphs also record ev_acc1 after k_accumulate: the next launch waits on it)
  const int acc = (parts & PART_ACC) == 0 ? 0 : c->profiling == 2 ? 2 : c->slot[si].stagger ? 1 : 0;
  if (parts & PART_ACC) c->slot[si].acc_timed = acc == 2;
  if (c->profiling == 1) {
    c->slot[si].acc_timed = false;
    if (int rc = enqueue_msm(c, pl, d_points, d_scalars, si, s, parts, pts)) return rc;
  } else if (c->graphs_ok && graphs_enabled()) {
    Segment* sg = (!acc || c->graph_events_ok) ? get_segment(c, pl, d_points, d_scalars, si, parts, pts, acc) : nullptr;
    if (sg) {
      HIPCHECK(hipGraphLaunch(sg->exec, s));
    } else {
      auto run = [&](int p) -> int {
        if (!p) return MSM_OK;
        Segment* g = c->graphs_ok ? get_segment(c, pl, d_points, d_scalars, si, p, pts, false) : nullptr;
        if (g) {
          HIPCHECK(hipGraphLaunch(g->exec, s));
          return MSM_OK;
        }
        return enqueue_msm(c, pl, d_points, d_scalars, si, s, p, pts);
      };
      if (int rc = run(parts & (PART_PREP | PART_SORT))) return rc;
      if (parts & PART_ACC)
        if (int rc = enqueue_msm(c, pl, d_points, d_scalars, si, s, PART_ACC, pts, acc)) return rc;
      if (int rc = run(parts & (PART_POST | PART_JOIN))) return rc;
    }
  } else if (int rc = enqueue_msm(c, pl, d_points, d_scalars, si, s, parts, pts, acc)) {
    return rc;
  }
  return MSM_OK;
}

int launch_parts(DevCtx* c, const Plan& pl, const BatchPtrs& d_points, const BatchPtrs& d_scalars, int si,
                 int parts, uint32_t* pts) {
  Slot& sl = c->slot[si];
  hipStream_t s = sl.stream;
  if (c->profiling && (parts & (PART_PREP | PART_SORT))) HIPCHECK(hipEventRecord(sl.ev_start, s));
  if (int rc = launch_on(c, pl, d_points, d_scalars, si, parts, pts, s)) return rc;
  if (parts & PART_POST) {
    if (c->profiling) HIPCHECK(hipEventRecord(sl.ev_end, s));
    HIPCHECK(hipEventRecord(sl.ev_done, s));
  }
  return MSM_OK;
}

// Wait for the launch in slot `si` (spinning briefly: the result is usually due within a couple of
// milliseconds, and a blocking wait adds a wake-up latency) and check its flags; its window terms
// are then in the slot's h_out.  Skewed scalars: the sequence ran without the bucket joins
// (PART_JOIN), so they and the reduction run again here (the slot's stream is idle: its next launch
// is enqueued afterwards).
int wait_slot(DevCtx* c, int si, uint32_t* total_out = nullptr) {
  Slot& sl = c->slot[si];
  const Plan& pl = sl.pl;
  const auto spin_until = clk::now() + std::chrono::milliseconds(50);
  hipError_t q;
  while ((q = hipEventQuery(sl.ev_done)) == hipErrorNotReady && clk::now() < spin_until) _mm_pause();
  if (q == hipErrorNotReady) q = hipEventSynchronize(sl.ev_done);
  HIPCHECK(q);
  const size_t outb = (size_t)pl.d.W * pl.nterms * 32 * 4;
  const uint32_t* h = reinterpret_cast<const uint32_t*>(sl.h_out.p);
  const uint32_t err = h[outb / 4];
  if (total_out) *total_out = h[outb / 4 + 1];
  sl.skew_seen = h[outb / 4 + 2];
  if (h[outb / 4 + 2]) {
    // only the second k_bucket_reduce_2 clears the skew list and the lead flag: if the re-run
    // cannot be enqueued or does not complete, clear them here, or the slot's next MSM would append
    // to a stale skew list and rejoin stale workgroups without any error
    int rc = enqueue_msm(c, pl, BatchPtrs{}, BatchPtrs{}, si, sl.stream, PART_JOIN | PART_POST, nullptr);
    if (rc == MSM_OK && (hipEventRecord(sl.ev_done, sl.stream) != hipSuccess ||
                         hipEventSynchronize(sl.ev_done) != hipSuccess))
      rc = MSM_ERR_HIP;
    if (rc != MSM_OK) {
      (void)hipGetLastError();
      hipMemsetAsync(sl.ws.skew_list.p, 0, 4, sl.stream);
      hipMemsetAsync(sl.ws.lead_flag.p, 0, sl.ws.lead_flag.cap, sl.stream);
      hipStreamSynchronize(sl.stream);
      return rc;
    }
  }
  if (err & MSM_DEV_ERR_COORD_RANGE) return MSM_ERR_COORD_RANGE;
  if (err & MSM_DEV_ERR_BAD_POINT) return MSM_ERR_BAD_POINT;
  if (err & MSM_DEV_ERR_BAD_INDEX) return MSM_ERR_INVALID_ARG;  // a device-entry subset's index >= n
  if (err & MSM_DEV_ERR_SCALAR_RANGE) return MSM_ERR_INVALID_ARG;  // a narrow scalar's bit at or above scalar_bits
  return MSM_OK;
}

int finish_msm(DevCtx* c, int si, Pt* result, std::vector<uint32_t>* terms = nullptr, TailCrew* crew = nullptr) {
  Slot& sl = c->slot[si];
  const Plan& pl = sl.pl;
  uint32_t total = 0;
  if (int rc = wait_slot(c, si, &total)) return rc;
  const size_t outb = (size_t)pl.d.W * pl.nterms * 32 * 4;
  const uint32_t* h = reinterpret_cast<const uint32_t*>(sl.h_out.p);
  auto t0 = clk::now();
  if (terms)
    terms->assign(h, h + outb / 4);
  else if (crew && crew->active())
    *result = crew->run(pl, h);
  else
    *result = horner_tail(pl, h);
  auto t1 = clk::now();
  if (c->profiling == 1 || (c->profiling == 2 && sl.acc_timed)) {
    float ms[PH_COUNT] = {};
    msm_profile_t& P = c->last;
    if (c->profiling == 1) {
      for (int i = 1; i < PH_COUNT; i++) hipEventElapsedTime(&ms[i], c->ev[i - 1], c->ev[i]);
      hipEventElapsedTime(&P.device_total, c->ev[PH_START], c->ev[PH_READBACK]);
    } else {
      hipEventElapsedTime(&ms[PH_ACCUM], sl.ev_acc0, sl.ev_acc1);
      hipEventElapsedTime(&P.device_total, sl.ev_start, sl.ev_end);
    }
    P.prepare_points = ms[PH_PREPARE];
    P.recode_count = ms[PH_RECODE];
    P.coarse_scan = ms[PH_SCAN];
    P.coarse_scatter = ms[PH_SCATTER];
    P.fine_sort = ms[PH_FINE];
    P.accumulate = ms[PH_ACCUM];
    P.fixup = ms[PH_FIXUP];
    P.bucket_reduce_1 = ms[PH_RED1];
    P.bucket_reduce_2 = ms[PH_RED2];
    P.readback = ms[PH_READBACK];
    P.host_tail = std::chrono::duration<float, std::milli>(t1 - t0).count();
    P.entries = total;
    P.window_bits = pl.d.c;
    P.windows = pl.d.Wr;
    P.run_length = pl.dense ? pl.dense_E : pl.K;  // a dense launch: entries per unit lane
    P.chunk_len = pl.L;
    P.msms_per_launch = pl.d.nm;
    P.accumulate_sum += P.accumulate;
    P.device_total_sum += P.device_total;
    P.profiled++;
    if (c->profiling == 2) {
      float a = 0, b = 0;
      if (hipEventElapsedTime(&a, c->ev_base, sl.ev_acc0) == hipSuccess &&
          hipEventElapsedTime(&b, c->ev_base, sl.ev_acc1) == hipSuccess)
        c->acc_ivals.emplace_back(a, b);
    }
  }
  return MSM_OK;
}

BatchPtrs splat(const uint32_t* p) {
  BatchPtrs b{};
  for (uint32_t m = 0; m < MSM_MAX_BATCH; m++) b.p[m] = p;
  return b;
}

// The caller's stream (if any) -> every slot stream about to be used waits for its work so far.
int order_after_user(DevCtx* c, hipStream_t user, int nslot) {
  if (!user) return MSM_OK;
  HIPCHECK(hipEventRecord(c->ev_user, user == (hipStream_t)MSM_STREAM_NULL ? nullptr : user));
  for (int si = 0; si < nslot; si++) HIPCHECK(hipStreamWaitEvent(c->slot[si].stream, c->ev_user, 0));
  return MSM_OK;
}

// Before an error return once something is queued: wait for the copy stream and the streams of slots
// [0, nslot), then hand back `code`.  The copies read the caller's arrays, which msm.h promises are
// not read after the call returns.
int drain_streams(DevCtx* c, int nslot, int code) {
  hipStreamSynchronize(c->copy_stream);
  for (int si = 0; si < nslot; si++) hipStreamSynchronize(c->slot[si].stream);
  return code;
}

// The host tail of a lone MSM in slot `si`, over the device context's persistent helpers: armed
// right after the launch (they spin while the device works), handed the terms when they land.
int finish_lone(DevCtx* c, int si, Pt* result) {
  TailCrew* crew = ctx_crew(c);
  crew->arm();
  const int rc = finish_msm(c, si, result, nullptr, crew);
  if (rc != MSM_OK) crew->disarm();  // no terms will come
  return rc;
}
