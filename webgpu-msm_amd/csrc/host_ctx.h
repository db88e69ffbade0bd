// Layer 2, the device context: error macro, buffers, plan and slot records, DevCtx and its creation and
// teardown, the per-call device guard.  Depends on host_knobs.h and the kernels' headers only.
#pragma once
#define HIPCHECK(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      fprintf(stderr, "libmsm: HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); \
      return _e == hipErrorOutOfMemory ? MSM_ERR_OOM : MSM_ERR_HIP;                            \
    }                                                                                          \
  } while (0)

enum Phase {
  PH_START = 0,
  PH_PREPARE,
  PH_RECODE,
  PH_SCAN,
  PH_SCATTER,
  PH_FINE,
  PH_ACCUM,
  PH_FIXUP,
  PH_RED1,
  PH_RED2,
  PH_READBACK,
  PH_COUNT
};

// Bumped on every (re)allocation anywhere: captured graphs hold raw pointers, so a graph is
// replayed only while the generation it was captured under is current.
std::atomic<uint64_t> g_alloc_gen{0};

// Guarded workspaces, a test mode (msm_test_guard, host_guard.h; off in production, no environment
// knob): every allocation made while the switch is on is front guard | payload | back guard, with
// `cap` the requested bytes exactly -- no 256-B floor, so nothing hides in slack --, the guards filled
// with GUARD_FILL and the payload with g_guard_word (below; zero by default, a defined value: read as an
// index it stays in range).  The back guard is one whole partition chunk of 32-bit entries, the largest
// unit any one lane group writes; the front guard keeps `p` 256-B aligned.  msm_test_guard_check reads the guards
// back.  The switch changes only while nothing is allocated, so one process never mixes the layouts.
std::atomic<bool> g_guard{false};
constexpr size_t GUARD_FRONT = 4096, GUARD_BACK = 65536;
constexpr int GUARD_FILL = 0xA5;

// The payload's fill is a 32-bit word of the tests' choosing (msm_test_guard_fill; 0 unless a test says
// otherwise): a poison, so that a kernel reading a word its launch never wrote computes with something
// other than zero -- the neutral value of nearly all the integer state the kernels keep (no entry, an
// empty count, a clear flag, key 0, the additive identity of an Fr sum), which is why a zero fill cannot
// show such a read.  Only words <= GUARD_WORD_MAX = 3 are accepted.  Read as an index, a count, a key, an
// entry word (index << 1 | sign), a run's workgroup or a shift, such a word addresses at most record 3 of
// a table -- 4 point records of 144 B, 4 prepared records of 128 B, 4 Fr elements of 32 B, words 0..5 of
// an integer table -- and every one of those lies inside the payload or the 64 KiB back guard of its
// buffer: a kernel that does read poison computes a wrong value or touches a guard band
// (msm_test_guard_check names it), it does not leave the allocation.  Read as the halves of a 16-bit
// table (digits, part_fine) the word is {word, 0}; as limbs of a point or of a field element it is a
// small residue, and the arithmetic forms no address from it.  (The per-point kernels -- k_scale_points,
// the k_combine_* -- compare every index they gather by with n before they use it.)  What the kernels
// multiply into an address (n, K, B, nbc, ch, rstride, the plan's counts) comes by value in the launch's
// arguments, never from a workspace word.  The differences the kernels take of two workspace words -- bin_base[bin + 1] -
// bin_base[bin] (k_fine_sort), bucket_start[k + 1] - bucket_start[k] (k_dense_segments, the reductions'
// emptiness tests compare only), seg_base[key + 1] - seg_base[key] (k_dense_units, k_dense_fold) --
// would wrap if one side were poison and the other a smaller true value; both sides of each are stored
// by the launch's own sort (k_part_scatter writes bin_base[0 .. nbins], k_fine_sort bucket_start[0 ..
// W B + 1], k_dense_segments seg_base[0 .. nkeys]) in a kernel that ends before the reader starts, and
// a zero fill wraps the same way with the sides exchanged, so the poison adds no way out there.  No
// buffer is excluded for its indexing.
constexpr uint32_t GUARD_WORD_MAX = 3;
std::atomic<uint32_t> g_guard_word{0};

// `bytes` at device address p filled with `word`, whole words then the word's low bytes (null stream;
// the caller synchronises).
inline hipError_t guard_fill_dev(void* p, size_t bytes, uint32_t word) {
  char* b = static_cast<char*>(p);
  const size_t words = bytes / 4;
  if (words)
    if (hipError_t e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b), (int)word, words); e != hipSuccess) return e;
  for (size_t k = 4 * words; k < bytes; k++)
    if (hipError_t e = hipMemset(b + k, (int)((word >> (8 * (k & 3))) & 0xffu), 1); e != hipSuccess) return e;
  return hipSuccess;
}
// The same on the host, for a pinned buffer.
inline void guard_fill_host(void* p, size_t bytes, uint32_t word) {
  uint8_t* b = static_cast<uint8_t*>(p);
  for (size_t k = 0; k < bytes; k++) b[k] = (uint8_t)(word >> (8 * (k & 3)));
}

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  void* base = nullptr;  // a guarded allocation's own start (p = base + GUARD_FRONT), null otherwise
  int ensure(size_t bytes) {
    if (bytes <= cap) return MSM_OK;
    g_alloc_gen.fetch_add(1);
    release();
    if (g_guard.load(std::memory_order_relaxed)) return ensure_guarded(bytes);
    size_t want = std::max<size_t>(bytes, 256);
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;
      return MSM_ERR_OOM;
    }
    cap = want;
    return MSM_OK;
  }
  int ensure_guarded(size_t bytes) {
    if (hipMalloc(&base, GUARD_FRONT + bytes + GUARD_BACK) != hipSuccess) {
      base = nullptr;
      return MSM_ERR_OOM;
    }
    char* b = static_cast<char*>(base);
    // (the fills are complete before any of the library's streams, which do not wait for the null
    // stream, can touch the buffer)
    if (hipMemset(b, GUARD_FILL, GUARD_FRONT) != hipSuccess ||
        guard_fill_dev(b + GUARD_FRONT, bytes, g_guard_word.load(std::memory_order_relaxed)) != hipSuccess ||
        hipMemset(b + GUARD_FRONT + bytes, GUARD_FILL, GUARD_BACK) != hipSuccess ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      hipFree(base);
      base = nullptr;
      return MSM_ERR_HIP;
    }
    p = b + GUARD_FRONT;
    cap = bytes;
    return MSM_OK;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  void release() {
    if (p) hipFree(base ? base : p);
    p = base = nullptr;
    cap = 0;
  }
};

struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  void* base = nullptr;  // as Buf::base
  // `guardable`: a buffer kernels write into (a slot's h_out) takes the guarded layout in the test
  // mode; the pinned upload ring, which only the host writes, never does.
  int ensure(size_t bytes, bool guardable = false) {
    if (bytes <= cap) return MSM_OK;
    g_alloc_gen.fetch_add(1);
    release();
    if (guardable && g_guard.load(std::memory_order_relaxed)) return ensure_guarded(bytes);
    // pinned, host-cacheable memory; k_red2_terms (or k_bucket_reduce_2) writes its results
    // straight into it, visible to the host once the launch's event completes (a coherent /
    // uncached mapping would make the host Horner's reads ~4x slower)
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      return MSM_ERR_OOM;
    }
    cap = bytes;
    return MSM_OK;
  }
  int ensure_guarded(size_t bytes) {
    if (hipHostMalloc(&base, GUARD_FRONT + bytes + GUARD_BACK, hipHostMallocDefault) != hipSuccess) {
      base = nullptr;
      return MSM_ERR_OOM;
    }
    char* b = static_cast<char*>(base);
    memset(b, GUARD_FILL, GUARD_FRONT);
    guard_fill_host(b + GUARD_FRONT, bytes, g_guard_word.load(std::memory_order_relaxed));
    memset(b + GUARD_FRONT + bytes, GUARD_FILL, GUARD_BACK);
    p = b + GUARD_FRONT;
    cap = bytes;
    return MSM_OK;
  }
  void release() {
    if (p) hipHostFree(base ? base : p);
    p = base = nullptr;
    cap = 0;
  }
};

struct Plan {
  MsmDims d;
  uint32_t K;       // run length
  uint32_t L;       // bucket-reduce chunk length (any of RED1_LS; not necessarily a power of two)
  uint32_t nchunks; // ceil(B / L)
  uint32_t nv;      // V-slices: R_V = sum_c U_c is split into nv equal partial sums
  uint32_t nterms;  // nv + bits of the largest chunk index
  size_t Mmax;      // W * n upper bound on sorted entries
  size_t runs_max;
  uint32_t pfmt;    // input point format of k_prepare_points (PT_FMT_*: wire records or a compact upload)
  // The dense-bucket accumulation (finish_plan; k_dense_* in the place of k_accumulate): entries per
  // unit lane E (a unit's segment is 64 E entries) and the unit kernel's grid bound.  Zero otherwise.
  uint32_t dense, dense_E, dense_units;
  // Native scalar types (msm_opts_typed): MSM_SCALAR_* of the launch's vectors -- or STYPE_WIDE | MSM_FIELD_*
  // of a wide type's (host_plan.h) -- 0 for word formats, and the bytes of one vector, ceil(n e / 8).  The
  // geometry in `d` is the narrow one of d.sbits (a 256-bit integer of 254 bits and more: the full-width
  // one) and knows nothing of the type: only the recode kernel's choice and the upload's length follow it.
  uint32_t stype;
  size_t sc_bytes;
};

// Every field that shapes a launch (grids, buffer offsets, the h_out layout): a captured graph is
// replayed only for an identical plan.
bool plan_eq(const Plan& a, const Plan& b) {
  const MsmDims &x = a.d, &y = b.d;
  return x.n == y.n && x.c == y.c && x.B == y.B && x.W == y.W && x.Wm == y.Wm && x.w0 == y.w0 && x.Wr == y.Wr &&
         x.half_lo == y.half_lo && x.half_hi == y.half_hi &&
         x.nm == y.nm && x.q == y.q &&
         x.nhi == y.nhi && x.fb == y.fb && x.nbc == y.nbc && x.nbins == y.nbins && x.ch == y.ch && x.nch == y.nch &&
         x.packed == y.packed && x.shared == y.shared && x.sub == y.sub && x.rstride == y.rstride &&
         x.first == y.first && x.sm == y.sm && x.sw == y.sw && x.sbits == y.sbits && a.K == b.K && a.L == b.L &&
         a.nchunks == b.nchunks && a.nv == b.nv && a.nterms == b.nterms && a.Mmax == b.Mmax &&
         a.runs_max == b.runs_max && a.pfmt == b.pfmt && a.dense == b.dense && a.dense_E == b.dense_E &&
         a.dense_units == b.dense_units && a.stype == b.stype && a.sc_bytes == b.sc_bytes;
}

// Device workspace of one MSM (all sizes from Plan; grown on demand, never shrunk).
struct Workspace {
  Buf pts, err, digits, colsum, bin_base, bin_cur;
  Buf part_entry, part_fine, sorted_entry, bucket_start, run_key, buckets;
  Buf lead_val, lead_open, cross_key, lead_flag, skew_list, g_head, g_hkey, g_tkey, red_U, red_T;
  Buf wire_pts, wire_sc;  // device copies of host-resident inputs (msm_compute*, host entries)
  Buf red_G;               // k_red2_groups' points per (window, group of RG_CH chunks)
  Buf split_sc;            // k_split_scalars' virtual scalars of a folded launch (msm_bases_*, levels > 1)
  Buf sub_idx;             // base indices [nm][m] of an indexed subset launch (msm_bases_compute_subset*)
  Buf seg_base, unit_key, partials;  // the dense-bucket accumulation's segment map and per-unit sums (Plan::dense)
  Buf dx_pts;              // k_decompress_x's output: x|y of a compressed creation, wire records of msm_decompress_points
  Buf fx_proj;             // k_fixed_eval's points (X : Y : Z) in blocks of 64, read by k_fixed_normalise (msm_fixed_mul*)
  Buf vx_part;             // k_vector_eval's partial sums (X : Y : Z : T) per part and block, and k_vector_fold's two halves
  Buf fr_part;             // k_fr_dot_partial's sums, one element per workgroup, and k_fr_dot_final's result after them (msm_fr_dot*);
                           // k_fr_scan_spans' totals, one per span, which k_fr_scan_totals turns into carries (msm_fr_scan*)
#ifdef MSM_DUMMY_ALLOC
  Buf dummy_tiles, dummy_cursor;  // tuning builds: the round-5 allocation layout
#endif
  // Every buffer with its name: release() and the guard check (host_guard.h) both go through this, so
  // neither can miss one.
  template <typename F>
  void each_buf(F&& f) {
#define WS_BUF(b) f(#b, b)
    WS_BUF(pts), WS_BUF(err), WS_BUF(digits), WS_BUF(colsum), WS_BUF(bin_base), WS_BUF(bin_cur);
    WS_BUF(part_entry), WS_BUF(part_fine), WS_BUF(sorted_entry), WS_BUF(bucket_start), WS_BUF(run_key), WS_BUF(buckets);
    WS_BUF(lead_val), WS_BUF(lead_open), WS_BUF(cross_key), WS_BUF(lead_flag), WS_BUF(skew_list);
    WS_BUF(g_head), WS_BUF(g_hkey), WS_BUF(g_tkey), WS_BUF(red_U), WS_BUF(red_T);
    WS_BUF(wire_pts), WS_BUF(wire_sc), WS_BUF(red_G), WS_BUF(split_sc), WS_BUF(sub_idx);
    WS_BUF(seg_base), WS_BUF(unit_key), WS_BUF(partials), WS_BUF(dx_pts), WS_BUF(fx_proj), WS_BUF(vx_part);
    WS_BUF(fr_part);
#ifdef MSM_DUMMY_ALLOC
    WS_BUF(dummy_tiles), WS_BUF(dummy_cursor);
#endif
#undef WS_BUF
  }
  void release() {
    each_buf([](const char*, Buf& b) { b.release(); });
  }
};

// Launch-sequence parts.  PREP: wire points -> precomputed records; SORT: scalar recoding and the
// bucket sort; ACC: bucket accumulation; POST: the bucket reduction; JOIN: the joins of skewed
// buckets (k_chain_join, k_lead_scan).  The regular sequence (PART_ALL) leaves JOIN out: with
// unskewed scalars both kernels would do nothing, yet each costs ~5 us of the critical path.
// k_accumulate flags skew, k_bucket_reduce_2 reports it with the terms, and finish_msm then runs
// JOIN + POST again on the slot (the order of the original sequence; nothing they read was
// changed by the first reduction).
constexpr int PART_PREP = 1, PART_SORT = 2, PART_ACC = 4, PART_POST = 8, PART_ALL = 15, PART_JOIN = 16;

// One captured graph of a slot: a contiguous part of the launch sequence for one plan.
struct Segment {
  Plan pl{};
  int parts = 0;
  const uint32_t* pts_buf = nullptr;  // the point-record buffer the captured kernels use
  int acc_events = 0;                 // event-record nodes: 2 around k_accumulate, 1 after it only
  bool fork = false;                  // the preparation forked beside the sort (slot_forks)
  uint64_t gen = 0;
  uint64_t used = 0;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // the kernel nodes that take the MSM's input buffers: repointed per launch
  hipGraphNode_t n_prep = nullptr, n_recode = nullptr;
  hipKernelNodeParams p_prep{}, p_recode{};
  BatchPtrs in_pts{}, in_sc{};
  void drop() {
    if (exec) hipGraphExecDestroy(exec);
    if (graph) hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
    n_prep = n_recode = nullptr;
    parts = 0;
  }
};
constexpr int NSEG = 6;

// One in-flight launch (one or a batch of MSMs): its own stream, device workspace, result buffer,
// captured graph segments and events.  Several slots let the pipelined entries keep launches
// j+1.. on the device while launch j is still there (the latency-bound tails of one overlap the
// others' kernels) and while the host finishes launch j (window Horner).
struct Slot {
  hipStream_t stream = nullptr;
  // k_prepare_points forks onto aux (ev_fork) and rejoins before the accumulation (ev_join): the
  // point preparation (HBM streaming) runs beside the bucket sort (the scalars' kernels)
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  Workspace ws;
  HostBuf h_out;  // k_bucket_reduce_2 writes the window terms, err and total here
  void* h_out_dev = nullptr;
  Segment seg[NSEG];
  uint64_t seg_clock = 0;
  hipEvent_t ev_start = nullptr, ev_acc0 = nullptr, ev_acc1 = nullptr, ev_end = nullptr, ev_done = nullptr;
  hipEvent_t ev_in = nullptr;  // inputs of the slot's next launch are in place (uploads, caller's stream)
  hipEvent_t ev_sc = nullptr;  // the scalars of the slot's next launch are in place (host uploads)
  Plan pl{};
  bool acc_timed = false;
  bool stagger = false;  // this slot's pipelined launches are staggered (stagger_launches)
  bool pipelined = false;  // a launch of a pipelined run (another launch in flight beside it)
  uint32_t skew_seen = 0;  // wait_slot's latch: the skewed workgroups of the slot's last launch (msm_test_acc_state)
};
constexpr int NSLOT = 4;      // at most this many launches in flight (one HIP stream each)
constexpr int NCHUNK_EV = 8;  // events marking uploaded point chunks

// What a device context owns of the later layers, and how DevCtx::destroy gives it back (the one
// place this header names what is defined after it).
class TailCrew;
class HornerPool;
class PackPool;
struct DevCtx;
void ctx_drop_pools(DevCtx* c);     // host_tail.h: stops and deletes the context's three pools
void release_bases_on(int device);  // host_bases.h: frees the records of every handle on the device
void release_fixed_on(int device);  // host_fixed.h: and of every fixed-base table
using clk = std::chrono::steady_clock;

// Pinned staging buffers of the packed host upload (run_host_split with host_pack()): the
// library's own threads write compacted points (and the scalars) into them, the copy engine
// reads them (a DMA from pinned memory needs no staging by the runtime), each buffer reused once
// the copy out of it has completed (ev).
constexpr int NPIN = 3;
struct PinRing {
  HostBuf buf[NPIN];
  hipEvent_t ev[NPIN] = {};
  bool used[NPIN] = {};
};

// What the launch plans take from the device: compute units, and k_accumulate's and k_dense_units'
// waves per SIMD (the occupancy queries at context creation; run_length_for and dense_entries fill
// whole rounds of them).  The test hooks plan for the defaults, so their plans do not depend on
// which device was used first.
struct DevShape {
  int n_cu = 256;
  int acc_waves = 4;
  int dense_waves = 4;
};

struct DevCtx {
  int device = -1;
  DevShape shape;
  std::mutex mu;
  Slot slot[NSLOT];
  hipStream_t copy_stream = nullptr;  // host->device uploads (overlap the slots' kernels)
  hipEvent_t ev_chunk[NCHUNK_EV] = {};
  hipEvent_t ev_user = nullptr;  // recorded on a caller's stream: the library's streams wait on it
  hipEvent_t ev_shared = nullptr;
  Buf shared_pts;  // point records of a shared base vector (msm_compute_shared*)
  Buf host_sc;     // all the scalars of a split host-input MSM (run_host_split), uploaded first
  Buf host_pts;    // and all its points, slice by slice (no slot buffer reused within the call)
  PinRing pin;     // pinned staging of the packed host upload
  PackPool* packer = nullptr;  // its packing threads (persistent, created on first use)
  hipEvent_t ev[PH_COUNT] = {};  // per-phase events (profiling mode 1)
  int profiling = 0;  // 0 off, 1 every phase (eager launches), 2 k_accumulate + device total per launch
  // The launch sequence of each slot is captured into HIP graphs and replayed: one
  // hipGraphLaunch instead of ~14 enqueues per launch.
  bool graphs_ok = true;
  bool graph_events_ok = true;  // event-record nodes can be added to captured graphs here
  hipEvent_t ev_base = nullptr;  // per-call time origin of the accumulation intervals (profiling 2)
  std::vector<std::pair<float, float>> acc_ivals;
  msm_profile_t last{};
  TailCrew* crew = nullptr;  // a lone MSM's host-tail helpers (persistent, created on first use)
  HornerPool* pool = nullptr;  // the pipelined entries' host tails, off the launching thread
  // per-launch upload events of a host-input pipelined run (launch j: up_ev[2 j] its scalars,
  // up_ev[2 j + 1] all its inputs), grown on demand
  std::vector<hipEvent_t> up_ev;

  // Every stream of the context, in creation order, and every event made with it, with whether it is
  // timed: create() and destroy() both go through these two, so neither can miss one.
  template <typename F>
  void each_stream(F&& f) {
    f(&copy_stream);
    for (Slot& sl : slot) f(&sl.stream);
    for (Slot& sl : slot) f(&sl.aux);
  }
  template <typename F>
  void each_event(F&& f) {
    for (hipEvent_t& e : ev) f(&e, true);
    for (hipEvent_t& e : ev_chunk) f(&e, false);
    f(&ev_user, false);
    f(&ev_shared, false);
    f(&ev_base, true);
    for (Slot& sl : slot) {
      for (hipEvent_t* e : {&sl.ev_start, &sl.ev_acc0, &sl.ev_acc1, &sl.ev_end}) f(e, true);
      for (hipEvent_t* e : {&sl.ev_done, &sl.ev_in, &sl.ev_sc, &sl.ev_fork, &sl.ev_join}) f(e, false);
    }
  }
  // The context's own device buffers with their names (the slots' are Workspace::each_buf's).
  template <typename F>
  void each_buf(F&& f) {
    f("shared_pts", shared_pts);
    f("host_sc", host_sc);
    f("host_pts", host_pts);
  }
  // No context without its streams and events (a null event would fail every call later): on an error
  // the caller destroys what was made.
  int create(int dev) {
    device = dev;
    int prev = 0;
    hipGetDevice(&prev);
    if (hipSetDevice(dev) != hipSuccess) return MSM_ERR_HIP;
    // Streams in this order because the runtime deals them round-robin over its hardware queues
    // (GPU_MAX_HW_QUEUES, 4 by default) and two streams on one queue run in order: the slots'
    // streams first, so the launches in flight never share a queue (three slots for host inputs
    // beside the copy stream), then the aux streams of the preparation fork.
    bool ok = true;
    each_stream([&](hipStream_t* s) { ok = ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess; });
    each_event([&](hipEvent_t* e, bool timed) {
      ok = ok && (timed ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming)) == hipSuccess;
    });
    hipDeviceProp_t prop;
    if (ok && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      shape.n_cu = prop.multiProcessorCount;
    int acc_blocks = 0;  // k_accumulate workgroups per CU -> waves per SIMD (run_length_for)
    if (ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&acc_blocks, reinterpret_cast<const void*>(&k_accumulate),
                                                           ACC_THREADS, 0) == hipSuccess &&
        acc_blocks > 0)
      shape.acc_waves = std::max(1, acc_blocks * (int)(ACC_THREADS / 64) / 4);
    int du_blocks = 0;
    if (ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&du_blocks, reinterpret_cast<const void*>(&k_dense_units),
                                                           DU_THREADS, 0) == hipSuccess &&
        du_blocks > 0)
      shape.dense_waves = std::max(1, du_blocks * (int)(DU_THREADS / 64) / 4);
    hipSetDevice(prev);
    return ok ? MSM_OK : MSM_ERR_HIP;
  }
  // Everything the context holds, idle streams first (called under g_mu and the context's own lock).
  void destroy() {
    int prev = 0;
    hipGetDevice(&prev);
    hipSetDevice(device);
    hipStreamSynchronize(copy_stream);
    for (Slot& sl : slot) hipStreamSynchronize(sl.stream);
    each_buf([](const char*, Buf& b) { b.release(); });
    release_bases_on(device);
    release_fixed_on(device);
    for (Slot& sl : slot) {
      sl.ws.release();
      for (Segment& sg : sl.seg) sg.drop();
      sl.h_out.release();
      sl.h_out_dev = nullptr;
    }
    each_event([](hipEvent_t* e, bool) {
      if (*e) hipEventDestroy(*e);
      *e = nullptr;
    });
    each_stream([](hipStream_t* s) {
      if (*s) hipStreamDestroy(*s);
      *s = nullptr;
    });
    ctx_drop_pools(this);
    for (int k = 0; k < NPIN; k++) {
      pin.buf[k].release();
      if (pin.ev[k]) hipEventDestroy(pin.ev[k]);
      pin.ev[k] = nullptr;
      pin.used[k] = false;
    }
    for (hipEvent_t e : up_ev) hipEventDestroy(e);
    up_ev.clear();
    hipSetDevice(prev);
  }
};

std::mutex g_mu;
std::vector<DevCtx*> g_ctx;   // indexed by HIP ordinal
std::vector<int> g_gfx950;    // HIP ordinals of the gfx950 devices
int g_nhip = -1;              // HIP devices visible (any architecture)
std::atomic<int> g_profiling{0};  // read by calls on other devices' threads

int probe_devices() {
  if (g_nhip >= 0) return (int)g_gfx950.size();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  g_nhip = n;
  for (int i = 0; i < n; i++) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0)
      g_gfx950.push_back(i);
  }
  return (int)g_gfx950.size();
}

bool is_gfx950(int device) { return std::find(g_gfx950.begin(), g_gfx950.end(), device) != g_gfx950.end(); }

int get_ctx(int device, DevCtx** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (probe_devices() <= 0) return MSM_ERR_NO_DEVICE;
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) return MSM_ERR_HIP;
  }
  // opts.device is a HIP ordinal; only gfx950 ordinals are accepted (a mixed node keeps its
  // numbering)
  if (device >= g_nhip || !is_gfx950(device)) return MSM_ERR_INVALID_ARG;
  if ((int)g_ctx.size() < g_nhip) g_ctx.resize(g_nhip, nullptr);
  if (!g_ctx[device]) {
    DevCtx* c = new DevCtx();
    if (int rc = c->create(device)) {
      c->destroy();
      delete c;
      return rc;
    }
    g_ctx[device] = c;
  }
  *out = g_ctx[device];
  return MSM_OK;
}

// Profiling mode 2: the call's accumulation intervals start from ev_base; at the end their union
// (wall time with at least one k_accumulate in flight) is added to accumulate_union_sum.  With
// several launches in flight accumulations may overlap each other, so the union, not the sum of
// brackets, is the kernel's share of the device time.
void begin_call(DevCtx* c) {
  c->acc_ivals.clear();
  if (c->profiling == 2) hipEventRecord(c->ev_base, c->slot[0].stream);
}
void end_call(DevCtx* c) {
  if (c->profiling != 2 || c->acc_ivals.empty()) return;
  std::sort(c->acc_ivals.begin(), c->acc_ivals.end());
  double total = 0, lo = c->acc_ivals[0].first, hi = c->acc_ivals[0].second;
  for (const auto& iv : c->acc_ivals) {
    if (iv.first > hi) {
      total += hi - lo;
      lo = iv.first;
      hi = iv.second;
    } else {
      hi = std::max<double>(hi, iv.second);
    }
  }
  total += hi - lo;
  c->last.accumulate_union_sum += total;
  c->acc_ivals.clear();
}

// A caller's options, copied field by field (null: all zero): a caller built against the original
// 16-byte msm_opts owns no fields past `flags`, and the later ones are read only under the flags that
// announce them (msm.h).
msm_opts copy_opts(const msm_opts* o) {
  msm_opts r;
  memset(&r, 0, sizeof(r));
  if (!o) return r;
  r.window_bits = o->window_bits;
  r.run_length = o->run_length;
  r.device = o->device;
  r.flags = o->flags;
  if (o->flags & MSM_FLAG_DEVICES) {
    r.devices = o->devices;
    r.n_devices = o->n_devices;
  }
  if (o->flags & MSM_FLAG_WINDOWS) {
    r.window_lo = o->window_lo;
    r.window_hi = o->window_hi;
  }
  return r;
}

int with_device(const msm_opts* o, DevCtx** c) {
  int dev = o ? o->device : -1;
  return get_ctx(dev, c);
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) hipSetDevice(prev);
  }
};

// Lock the device context of `opts` and run `fn(ctx)` with its device current.
template <typename F>
int on_device(const msm_opts* opts, F&& fn) {
  DevCtx* c;
  int rc = with_device(opts, &c);
  if (rc != MSM_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  c->profiling = g_profiling.load();
  begin_call(c);
  rc = fn(c);
  end_call(c);
  return rc;
}
