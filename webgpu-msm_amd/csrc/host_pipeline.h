// Layer 8, the pipelined run: `count` MSMs in batched launches over several slots (run_many).
// Depends on the layers above it (knobs .. upload).
#pragma once
// Where the inputs of one pipelined run come from.
struct ManyInputs {
  enum Kind { DEVICE, HOST } kind = DEVICE;
  const uint32_t* const* points = nullptr;  // per MSM (ignored when shared_points is set)
  const uint32_t* const* scalars = nullptr;
  const uint32_t* shared_points = nullptr;  // one base vector for every MSM (prover batch)
  uint32_t batch = 0;                        // MSMs per launch (0: pipeline_batch's choice)
  const size_t* lens = nullptr;  // host inputs: real points per MSM (<= n; the rest is padded on
                                 // the device with identity points and zero scalars); null: all n
  const uint32_t* const* dev_points = nullptr;  // host inputs: per MSM, the device buffer (n points,
                                                // its own, never reused in the call) their points are
                                                // uploaded into instead of the slot's wire buffer
  bool packed = false;  // host points packed by the library's threads into pinned staging (x|y, or
                        // x|y|z for a launch with some z != 1) and copied into dev_points (24 words
                        // of room per point) or the slots' wire buffers; the launch's
                        // k_prepare_points reads that format
  const uint32_t* const* dev_scalars = nullptr;  // host inputs whose scalars are already on the
                                                 // device (n + padding words per MSM): no scalar upload
  // Records already prepared (a msm_bases handle's, device memory): they stand where the shared
  // base vector's records stand, and nothing is prepared.  With levels > 1 they are `levels`
  // copies of n records (level j = 2^(j chunk_bits) P_i) and every MSM runs folded: its scalars
  // are cut into levels * n virtual scalars of chunk_bits bits (k_split_scalars, into the slot's
  // split_sc) and the plan is the one of levels * n points (the caller's opts carry the window
  // width and the window range [0, Wc)).
  const uint32_t* prepared = nullptr;
  uint32_t levels = 1, chunk_bits = 0;
  // A subset of the handle's bases (msm_bases_compute_subset*; `prepared` set): run_many's n is then
  // the subset's m terms and everything is planned for levels * m, while the entries index the
  // handle's levels * rec_n records -- bases [first, first + m) of every level (MSM_SUB_RANGE) or
  // bases indices[b][0..m) for MSM b (MSM_SUB_INDEXED: host arrays, validated by the caller, or
  // device pointers, by `kind`).  The range [0, m) of a levels = 1 handle is not a subset launch
  // but the plain one on the first m records (sub = MSM_SUB_NONE).
  uint32_t sub = MSM_SUB_NONE;
  size_t sub_first = 0, rec_n = 0;
  const uint32_t* const* indices = nullptr;
};

// `count` MSMs of n points each, pipelined over pipeline_slots slots, each with its own stream and
// workspace, in launches of pipeline_batch MSMs (the last launch is padded by repeating its last
// MSM, whose extra results are dropped): later launches are enqueued before the host finishes
// launch j, so the host tail (window Horner) of one overlaps the device work of the next, and
// the launches' kernels overlap on the device (the latency-bound reduction of one beside
// another's sort and accumulation).  Host inputs are uploaded on the copy stream into the
// slot's wire buffers, overlapping the other slots' kernels.  A shared base vector is prepared
// once, before the first launch, and every launch reads its records.  Results go out affine (16
// words each) or, with `projective`, as X|Y|T|Z partials (32 words).
// One such run: run_many's arguments, what setup derives from them, and the steps in run_many's order.
struct ManyRun {
  DevCtx* c;
  const ManyInputs& in;
  const size_t n, count;
  const msm_opts* o;
  hipStream_t user_stream;
  uint32_t* out_be;
  bool projective;
  Pt* out_pts;
  bool prepared = false, shared = false, host = false, indexed = false, narrow = false, stagger = false;
  uint32_t kf = 1, nm = 1;    // levels of a folded launch; MSMs per launch
  size_t np = 0, nbatch = 0;  // points the plan sees per MSM; launches
  size_t sw = 8, scs = 0;     // words per wire scalar, and between the MSMs' scalars in a slot's wire buffer
  size_t sc_bytes = 0;        // bytes of one MSM's scalar vector: n sw words, or ceil(n e / 8) of a native type
  int nslot = 1;
  Plan pl;
  uint32_t* pts_shared = nullptr;
  // host inputs: how they go up, the packed launches' point formats, a packed t >= p
  // (MSM_ERR_COORD_RANGE), and the uploader thread with its progress
  bool packed = false, uploader = false, own_buffers = false;
  std::vector<uint32_t> launch_fmt;
  std::atomic<bool> t_bad{false}, up_stop{false};
  std::atomic<size_t> sc_ready{0}, up_ready{0}, enqueued{0};
  std::atomic<int> up_rc{MSM_OK};
  std::thread up_th;
  // the host tails: the device context's tail helpers take the last launch's (armed once it is
  // enqueued), the pool the earlier launches' (their terms copied out per launch)
  TailCrew* crew = nullptr;
  HornerPool* pool = nullptr;
  bool crew_armed = false;
  std::vector<std::vector<uint32_t>> launch_terms;
  std::vector<uint32_t> terms;
  size_t finished = 0;  // launches waited for (finish_msm returned, with or without an error)

  void emit(const Pt& r, size_t b) const {
    if (out_pts)
      out_pts[b] = r;
    else if (projective)
      pt_to_be_xyzt(r, out_be + 32 * b);
    else
      pt_to_be_affine(r, out_be + 16 * b);
  }
  size_t len_of(size_t b) const { return in.lens ? std::min(in.lens[b], n) : n; }

  // Validation, the plan, the slots' workspaces, and a shared base vector's preparation.
  int setup() {
    prepared = in.prepared != nullptr;
    shared = in.shared_points != nullptr || prepared;
    host = in.kind == ManyInputs::HOST;
    kf = prepared ? std::max(1u, in.levels) : 1u;
    np = n * kf;
    for (size_t b = 0; b < count; b++)
      if ((!shared && !in.points[b]) || !in.scalars[b]) return MSM_ERR_INVALID_ARG;
    // the batch's BatchPtrs hold MSM_MAX_BATCH entries: never more MSMs per launch than that
    nm = (uint32_t)std::min<size_t>(in.batch ? std::min<size_t>(in.batch, count) : pipeline_batch(n, count),
                                    MSM_MAX_BATCH);
    nbatch = (count + nm - 1) / nm;
    SubsetGeo sg;
    sg.kind = prepared ? in.sub : MSM_SUB_NONE;
    sg.levels = kf;
    sg.rec_n = in.rec_n;
    sg.first = in.sub_first;
    indexed = sg.kind == MSM_SUB_INDEXED;
    if (indexed)
      for (size_t b = 0; b < count; b++)
        if (!in.indices || !in.indices[b]) return MSM_ERR_INVALID_ARG;
    int rc = make_plan(np, o, c->shape, &pl, count > 1, nm, shared, &sg);
    if (rc != MSM_OK) return rc;
    // Words per wire scalar (a narrow launch on a handle: pl.d.sw, else 8) and the words between the
    // MSMs' scalars in a slot's wire buffer: a narrow MSM's vector is padded to whole 16-B units so
    // that every MSM's scalars start aligned for k_recode_narrow's vector loads.
    // A native type's vector (pl.stype) is counted in bytes, ceil(n e / 8), and padded the same way.
    narrow = pl.d.sw != 0;
    sw = narrow ? pl.d.sw : 8;
    sc_bytes = pl.stype ? pl.sc_bytes : n * sw * 4;
    scs = pl.stype ? typed_region_bytes(n, pl.stype) / 4 : narrow ? (n * sw + 3) & ~(size_t)3 : n * 8;
    // host inputs: one more launch in flight, so its upload queues behind the running ones
    // (2^20 msm_compute 4.21 -> 4.05 ms with three, profiles/r2t_*; device inputs are best with two)
    const int want = pipeline_slots(n, o) + (host && !(o && (o->flags & MSM_FLAG_SERIAL)) && !knob_slots_set() ? 1 : 0);
    nslot = nbatch > 1 ? (int)std::min<size_t>(nbatch, (size_t)std::min(want, NSLOT)) : 1;
    for (int si = 0; si < nslot; si++) {
      c->slot[si].pipelined = nslot > 1;
      if ((rc = ensure_workspace(c, pl, si, !prepared)) != MSM_OK) return rc;
      if (kf > 1 && (rc = c->slot[si].ws.split_sc.ensure((size_t)nm * np * 32)) != MSM_OK) return rc;
      if (indexed && (rc = c->slot[si].ws.sub_idx.ensure((size_t)nm * n * 4)) != MSM_OK) return rc;
      if (host) {
        Workspace& w = c->slot[si].ws;
        if ((!shared && (rc = w.wire_pts.ensure((size_t)nm * n * 128)) != MSM_OK) ||
            (rc = w.wire_sc.ensure((size_t)nm * scs * 4)) != MSM_OK)
          return rc;
      }
    }
    if ((rc = order_after_user(c, user_stream, nslot)) != MSM_OK) return rc;
    pts_shared = prepared ? const_cast<uint32_t*>(in.prepared) : nullptr;
    if (!shared || prepared) return MSM_OK;
    // the base vector's records, prepared once on slot 0's stream; the other slots wait for them
    if ((rc = c->shared_pts.ensure(n * PRE_WORDS * 4)) != MSM_OK) return rc;
    pts_shared = c->shared_pts.as<uint32_t>();
    Slot& s0 = c->slot[0];
    if (host) {
      if ((rc = s0.ws.wire_pts.ensure(n * 128)) != MSM_OK) return rc;
      rc = upload_points(c, in.shared_points, n, s0.ws.wire_pts.as<uint32_t>(), pts_shared, s0.ws.err.as<uint32_t>(),
                         s0.stream);
      if (rc != MSM_OK) return drain_streams(c, nslot, rc);
    } else {
      launch_prepare(in.shared_points, pts_shared, (uint32_t)n, s0.ws.err.as<uint32_t>(), prep_nt(n), s0.stream);
      if (hipGetLastError() != hipSuccess) return drain_streams(c, nslot, MSM_ERR_HIP);
    }
    if (hipEventRecord(c->ev_shared, s0.stream) != hipSuccess) return drain_streams(c, nslot, MSM_ERR_HIP);
    for (int si = 1; si < nslot; si++)
      if (hipStreamWaitEvent(c->slot[si].stream, c->ev_shared, 0) != hipSuccess)
        return drain_streams(c, nslot, MSM_ERR_HIP);
    return MSM_OK;
  }

  // How host inputs go up (packed or plain, through the uploader or not), the upload events, the host
  // tails' threads, and whether the launches are staggered.
  int setup_host_side() {
    packed = host && in.packed && !shared && pin_ring_ready(c, (size_t)nm * n * 128);
    // run_host_split sized its own point buffers (in.dev_points) for packed records: no unpacked
    // fallback into them (it checked the ring itself; only a failure since then lands here)
    if (host && in.packed && !shared && !packed && in.dev_points) return MSM_ERR_HIP;
    launch_fmt = std::vector<uint32_t>(nbatch, PT_FMT_WIRE);
    if (packed) ctx_packer(c);
    uploader = host && nbatch > 1;
    // Inputs uploaded into buffers of their own (dev_points / dev_scalars, never reused within the
    // call) need no wait for a slot's previous launch: the copies then run back to back.
    own_buffers = (shared || in.dev_points) && in.dev_scalars;
    while (host && c->up_ev.size() < 2 * nbatch) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return MSM_ERR_HIP;
      c->up_ev.push_back(e);
    }
    crew = tail_helpers() > 0 ? ctx_crew(c) : nullptr;
    pool = ctx_pool(c);
    launch_terms = std::vector<std::vector<uint32_t>>(pool ? nbatch : 0);
    stagger = nslot > 1 && c->profiling != 1 && stagger_launches() > (host ? 1 : 0);
    for (int si = 0; si < NSLOT; si++) c->slot[si].stagger = stagger && si < nslot;
    return MSM_OK;
  }

  // The inputs of launch j (per-MSM pointers, or the slot's wire buffers for host inputs) and the
  // number of real (not padding) MSMs in it.
  uint32_t launch_inputs(size_t j, BatchPtrs* bp, BatchPtrs* bs) const {
    Slot& sl = c->slot[j % nslot];
    const uint32_t nreal = (uint32_t)std::min<size_t>(nm, count - j * nm);
    *bp = BatchPtrs{};
    *bs = BatchPtrs{};
    for (uint32_t m = 0; m < MSM_MAX_BATCH; m++) {
      const size_t b = std::min(j * nm + std::min<uint32_t>(m, nm - 1), count - 1);
      bp->p[m] = shared ? in.shared_points : in.points[b];
      bs->p[m] = in.scalars[b];
      if (host) {  // padding MSMs of a short last launch read the last real MSM's wire buffers
        const uint32_t mr = std::min<uint32_t>(m, nreal - 1);
        bs->p[m] = in.dev_scalars ? in.dev_scalars[j * nm + mr] : sl.ws.wire_sc.as<uint32_t>() + (size_t)mr * scs;
        if (!shared)
          bp->p[m] = in.dev_points ? in.dev_points[j * nm + mr] : sl.ws.wire_pts.as<uint32_t>() + (size_t)mr * n * 32;
      }
    }
    return nreal;
  }

  // Host inputs of launch j into its slot's wire buffers, on the copy stream: the scalars, the
  // device padding of short MSMs, an event on the scalars (up_ev[2 j]), the points, an event on all
  // of them (up_ev[2 j + 1]).  MSMs whose host arrays are adjacent (the slices of run_host_split) go
  // up in one copy per array (upload_runs).  The padding MSMs of a short last launch upload nothing;
  // a short MSM (in.lens) goes up alone and its tail is padded on the device.
  int upload_launch(size_t j) {
    BatchPtrs bp, bs;
    const uint32_t nreal = launch_inputs(j, &bp, &bs);
    return packed ? upload_packed(j, nreal, bp, bs) : upload_plain(j, nreal, bp, bs);
  }

  // Packed: the launch's scalars, then its points, through pinned staging buffer j % NPIN (points at
  // [0, 24 nm n) words, scalars after them): the scalars first, each slice's into its dev_scalars
  // region, so the sort can start; the points as x|y if every z is 1, else x|y|z, one copy per slice
  // into its dev_points region; a short slice's padding in that format.
  int upload_packed(size_t j, uint32_t nreal, const BatchPtrs& bp, const BatchPtrs& bs) {
    const int k = (int)(j % NPIN);
    void* buf;
    if (int rc = pin_take(c, k, (size_t)nm * n * 128, &buf)) return rc;
    uint32_t* pb = static_cast<uint32_t*>(buf);
    uint32_t* psc = pb + (size_t)nm * n * 24;
    for (uint32_t m = 0; m < nreal; m++) {
      const size_t b = j * nm + m, len = len_of(b);
      if (!len) continue;
      pack_copy(*c->packer, psc + (size_t)m * n * 8, in.scalars[b], len * 32);
      if (hipMemcpyAsync(const_cast<uint32_t*>(bs.p[m]), psc + (size_t)m * n * 8, len * 32, hipMemcpyHostToDevice,
                         c->copy_stream) != hipSuccess)
        return MSM_ERR_HIP;
      // a short slice's scalar tail is zero before the sort may start (k_pad_identity below
      // pads its points)
      if (len < n && hipMemsetAsync(const_cast<uint32_t*>(bs.p[m]) + len * 8, 0, (n - len) * 32, c->copy_stream) !=
                         hipSuccess)
        return MSM_ERR_HIP;
    }
    HIPCHECK(hipEventRecord(c->up_ev[2 * j], c->copy_stream));
    if (uploader) sc_ready.store(j + 1, std::memory_order_release);  // its sort may be enqueued
    // each slice's x|y goes up as soon as it is packed; a z != 1 anywhere in the launch repacks
    // every slice as x|y|z and sends it again over the same regions (stream order)
    uint32_t fmt;
    bool tb = false;
    auto src = [&](uint32_t m) { return std::make_pair(in.points[j * nm + m], len_of(j * nm + m)); };
    auto send = [&](uint32_t m, uint32_t f) -> int {
      const size_t len = len_of(j * nm + m), pw = pt_fmt_slots(f) * 4;
      return !len || hipMemcpyAsync(const_cast<uint32_t*>(bp.p[m]), pb + (size_t)m * n * pw, len * pw * 4,
                                    hipMemcpyHostToDevice, c->copy_stream) == hipSuccess
                 ? MSM_OK
                 : MSM_ERR_HIP;
    };
    if (int rc = pack_and_send(*c->packer, pb, n, nreal, src, &fmt, &tb, send)) return rc;
    if (tb) t_bad.store(true);
    for (uint32_t m = 0; m < nreal; m++) {
      const size_t len = len_of(j * nm + m);
      if (len < n) {
        hipLaunchKernelGGL(k_pad_identity, dim3(grid_for((n - len) * (pt_fmt_slots(fmt) + 2), 256)), dim3(256), 0,
                           c->copy_stream, const_cast<uint32_t*>(bp.p[m]) + len * pt_fmt_slots(fmt) * 4,
                           const_cast<uint32_t*>(bs.p[m]) + len * 8, (uint32_t)(n - len), fmt);
        if (hipGetLastError() != hipSuccess) return MSM_ERR_HIP;
      }
    }
    if (int rc = pin_give(c, k, c->copy_stream)) return rc;
    launch_fmt[j] = fmt;
    HIPCHECK(hipEventRecord(c->up_ev[2 * j + 1], c->copy_stream));
    return MSM_OK;
  }

  int upload_plain(size_t j, uint32_t nreal, const BatchPtrs& bp, const BatchPtrs& bs) {
    auto up = [&](const uint32_t* const* src, const BatchPtrs& dst, size_t per) {
      return upload_runs(
          c, nreal, n, per, [&](uint32_t m) { return src[j * nm + m]; }, [&](uint32_t m) { return len_of(j * nm + m); },
          [&](uint32_t m) { return const_cast<uint32_t*>(dst.p[m]); });
    };
    if (pl.stype) {
      // a native type's vectors are bytes, not whole words per scalar: one copy each (the padding
      // MSMs of a short last launch read the last real MSM's region, launch_inputs)
      for (uint32_t m = 0; m < nreal; m++)
        if (hipMemcpyAsync(const_cast<uint32_t*>(bs.p[m]), in.scalars[j * nm + m], sc_bytes, hipMemcpyHostToDevice,
                           c->copy_stream) != hipSuccess)
          return MSM_ERR_HIP;
    } else if (!in.dev_scalars && !up(in.scalars, bs, sw)) {
      return MSM_ERR_HIP;
    }
    if (indexed) {
      // the launch's index vectors into the slot's own buffer (validated by the entry: no kernel);
      // the padding MSMs of a short last launch repeat the last real MSM's, as they do its scalars
      uint32_t* ib = c->slot[j % nslot].ws.sub_idx.as<uint32_t>();
      for (uint32_t m = 0; m < nm; m++)
        if (hipMemcpyAsync(ib + (size_t)m * n, in.indices[j * nm + std::min(m, nreal - 1)], n * 4,
                           hipMemcpyHostToDevice, c->copy_stream) != hipSuccess)
          return MSM_ERR_HIP;
    }
    for (uint32_t m = 0; m < nreal && !shared; m++) {
      const size_t len = len_of(std::min(j * nm + m, count - 1));
      if (len < n) {
        hipLaunchKernelGGL(k_pad_identity, dim3(grid_for((n - len) * 10, 256)), dim3(256), 0, c->copy_stream,
                           const_cast<uint32_t*>(bp.p[m]) + len * 32, const_cast<uint32_t*>(bs.p[m]) + len * 8,
                           (uint32_t)(n - len), PT_FMT_WIRE);
        if (hipGetLastError() != hipSuccess) return MSM_ERR_HIP;
      }
    }
    HIPCHECK(hipEventRecord(c->up_ev[2 * j], c->copy_stream));
    if (uploader) sc_ready.store(j + 1, std::memory_order_release);  // its sort may be enqueued
    if (!shared && !up(in.points, bp, 32)) return MSM_ERR_HIP;
    HIPCHECK(hipEventRecord(c->up_ev[2 * j + 1], c->copy_stream));
    return MSM_OK;
  }

  // With host inputs and more than one launch, a helper thread (the uploader) issues every
  // launch's copies back to back while this thread enqueues the launches and runs the host tails:
  // a pageable hipMemcpyAsync returns only once its data is staged, so copies issued from the
  // launching thread left the copy engine idle for every graph launch and host tail between them
  // (~120 us per launch, profiles/r4/e2e_timeline_before.txt).  A slot's wire buffers are rewritten
  // only after its previous launch is done with them: the copy stream waits for that launch's
  // ev_done, recorded once this thread has enqueued it (`enqueued`).
  void start_uploader() {
    if (!uploader) return;
    up_th = std::thread([this] {
      hipSetDevice(c->device);
      for (size_t j = 0; j < nbatch && !up_stop.load(); j++) {
        int urc = MSM_OK;
        if (j >= (size_t)nslot && !own_buffers) {
          // launch j - nslot (the slot's previous one) must have been enqueued before its
          // ev_done can be waited for
          while (enqueued.load(std::memory_order_acquire) < j - nslot + 1 && !up_stop.load()) std::this_thread::yield();
          if (up_stop.load()) break;
          if (hipStreamWaitEvent(c->copy_stream, c->slot[j % nslot].ev_done, 0) != hipSuccess) urc = MSM_ERR_HIP;
        }
        if (urc == MSM_OK) urc = upload_launch(j);
        if (urc != MSM_OK) {
          up_rc.store(urc);
          break;
        }
        up_ready.store(j + 1, std::memory_order_release);
      }
    });
  }
  bool wait_for(std::atomic<size_t>& v, size_t want) {  // false: the uploader failed
    for (uint32_t spins = 0; v.load(std::memory_order_acquire) < want; spins++) {
      if (up_rc.load() != MSM_OK) return false;
      if (spins > 256) std::this_thread::yield();
      else _mm_pause();
    }
    return true;
  }
  void stop_uploader() {
    up_stop.store(true);
    if (up_th.joinable()) up_th.join();
  }

  int fail(int code) {
    if (crew_armed) crew->disarm();  // no terms will come
    crew_armed = false;
    if (pool) pool->wait_all();  // its jobs read launch_terms
    stop_uploader();
    drain_streams(c, nslot, code);
    // An indexed subset fails at run time (MSM_DEV_ERR_BAD_INDEX) with other launches in flight:
    // each of those is waited for as usual, so that a skewed one still gets its second reduction,
    // which is what clears its slot's skew flags for the next call.
    // (and so does a narrow launch whose scalars had excess bits, MSM_DEV_ERR_SCALAR_RANGE)
    if ((indexed || narrow) && !host)
      for (size_t j = finished; j < enqueued.load(); j++) (void)wait_slot(c, (int)(j % nslot));
    return code;
  }

  // Launch f is waited for and its window terms copied out: the last launch's stay in `terms` (its
  // tails run here, over the crew); the pool's jobs read their launch's own copy.
  int collect(size_t f) {
    std::vector<uint32_t>* tdst = pool && f + 1 < nbatch ? &launch_terms[f] : &terms;
    finished = f + 1;
    if (int rc = finish_msm(c, (int)(f % nslot), nullptr, tdst)) return fail(rc);
    return MSM_OK;
  }

  // Launch j into slot j % nslot (its previous occupant, launch j - nslot, was collected just before).
  int enqueue(size_t j) {
    const int si = (int)(j % nslot);
    Slot& sl = c->slot[si];
    BatchPtrs bp, bs;
    launch_inputs(j, &bp, &bs);
    const int parts = shared ? (PART_SORT | PART_ACC | PART_POST) : PART_ALL;
    uint32_t* pts = shared ? pts_shared : sl.ws.pts.as<uint32_t>();
    // The last launch's bucket sort starts on its scalars while its points upload: the sort then
    // leaves the call's tail (earlier launches overlap the next uploads anyway).
    const bool sort_early = host && !shared && j + 1 == nbatch && nbatch > 1 && host_sort_early();
    int rc;
    if (host) {
      if (!uploader && (rc = upload_launch(j)) != MSM_OK) return fail(rc);
      if (sort_early) {
        if (uploader && !wait_for(sc_ready, j + 1)) return fail(up_rc.load());
        if (hipStreamWaitEvent(sl.stream, c->up_ev[2 * j], 0) != hipSuccess) return fail(MSM_ERR_HIP);
        sl.pl = pl;
        if ((rc = launch_parts(c, pl, bp, bs, si, PART_SORT, pts)) != MSM_OK) return fail(rc);
      }
      if (uploader && !wait_for(up_ready, j + 1)) return fail(up_rc.load());
      if (hipStreamWaitEvent(sl.stream, c->up_ev[2 * j + 1], 0) != hipSuccess) return fail(MSM_ERR_HIP);
    }
    if (kf > 1) {
      // the launch's scalars cut into its virtual scalars, on the slot's stream ahead of the sort
      uint32_t* vs = sl.ws.split_sc.as<uint32_t>();
      hipLaunchKernelGGL(k_split_scalars, dim3(grid_for(n, 256), kf, nm), dim3(256), 0, sl.stream, bs, vs,
                         (uint32_t)n, kf, in.chunk_bits);
      if (hipGetLastError() != hipSuccess) return fail(MSM_ERR_HIP);
      for (uint32_t m = 0; m < MSM_MAX_BATCH; m++) bs.p[m] = vs + (size_t)std::min(m, nm - 1) * np * 8;
    }
    if (indexed && !host) {
      // the caller's index vectors checked into the slot's buffer, on the slot's stream ahead of
      // the (captured) sort; padding MSMs repeat the last real MSM's (launch_inputs' rule)
      BatchPtrs bi{};
      for (uint32_t m = 0; m < MSM_MAX_BATCH; m++)
        bi.p[m] = in.indices[std::min(j * nm + std::min<uint32_t>(m, nm - 1), count - 1)];
      hipLaunchKernelGGL(k_stage_indices, dim3(grid_for(n, 256), nm), dim3(256), 0, sl.stream, bi,
                         sl.ws.sub_idx.as<uint32_t>(), (uint32_t)n, (uint32_t)in.rec_n, sl.ws.err.as<uint32_t>());
      if (hipGetLastError() != hipSuccess) return fail(MSM_ERR_HIP);
    }
    Plan plj = pl;
    plj.pfmt = packed ? launch_fmt[j] : PT_FMT_WIRE;  // set by the uploader before up_ready
    sl.pl = plj;
    const int lp = sort_early ? parts & ~PART_SORT : parts;
    // staggered: launch j's preparation and sort after launch j-1's accumulation
    if (stagger && j > 0 && hipStreamWaitEvent(sl.stream, c->slot[(j - 1) % nslot].ev_acc1, 0) != hipSuccess)
      return fail(MSM_ERR_HIP);
    if ((rc = launch_parts(c, plj, bp, bs, si, lp, pts)) != MSM_OK) return fail(rc);
    enqueued.store(j + 1, std::memory_order_release);
    if (crew && j + 1 == nbatch) {
      crew->arm();  // spins while the device runs the last launch
      crew_armed = true;
    }
    return MSM_OK;
  }

  // The host tails (window Horner) of launch f, whose terms collect() copied out.
  void drain(size_t f) {
    const uint32_t k = (uint32_t)std::min<size_t>(nm, count - f * nm);
    Pt res[MSM_MAX_BATCH];
    if (pool && f + 1 < nbatch) {
      // off this thread: the next launch's enqueue must not wait for these tails
      const uint32_t* tp = launch_terms[f].data();
      for (uint32_t m = 0; m < k; m++) pool->push([this, tp, f, m] { emit(horner_tail(pl, tp, m), f * nm + m); });
      return;
    }
    if (crew_armed && f + 1 == nbatch) {
      // the last launch's tails are the pipeline's drain, on the critical path of the call: their
      // window sums over the device context's helpers, the k outer Horners side by side
      crew->run_batch(pl, terms.data(), k, res);
      crew_armed = false;
    } else {
      // earlier launches' tails overlap the device's next launches: one host thread per MSM
      std::thread th[MSM_MAX_BATCH];
      for (uint32_t m = 1; m < k; m++) th[m] = std::thread([&, m] { res[m] = horner_tail(pl, terms.data(), m); });
      res[0] = horner_tail(pl, terms.data(), 0);
      for (uint32_t m = 1; m < k; m++) th[m].join();
    }
    for (uint32_t m = 0; m < k; m++) emit(res[m], f * nm + m);
  }
};

int run_many(DevCtx* c, const ManyInputs& in, size_t n, size_t count, const msm_opts* o, hipStream_t user_stream,
             uint32_t* out_be, bool projective, Pt* out_pts = nullptr) {
  ManyRun r{c, in, n, count, o, user_stream, out_be, projective, out_pts};
  if (n == 0) {
    for (size_t b = 0; b < count; b++) r.emit(pt_identity(), b);
    return MSM_OK;
  }
  int rc = r.setup();
  if (rc == MSM_OK) rc = r.setup_host_side();
  if (rc != MSM_OK) return rc;
  r.start_uploader();
  // Launch j goes to slot j % nslot.  Its previous occupant, launch j - nslot, is waited for and
  // its window terms copied out just before; the host tail (window Horner) of launch j - nslot
  // runs after j is enqueued, so the device holds nslot launches while the host works
  // (otherwise launches that finish together leave the device idle for a Horner each).
  for (size_t j = 0; j < r.nbatch + r.nslot; j++) {
    const bool have = j >= (size_t)r.nslot;
    if (have && (rc = r.collect(j - r.nslot)) != MSM_OK) return rc;
    if (j < r.nbatch && (rc = r.enqueue(j)) != MSM_OK) return rc;
    if (have) r.drain(j - r.nslot);
  }
  if (r.pool) r.pool->wait_all();
  r.stop_uploader();  // its last copies were waited for by the last launch
  return r.t_bad.load() ? MSM_ERR_COORD_RANGE : MSM_OK;
}
