// Layer 9, the single-device entries: the split of one large host-input MSM into pipelined slices, and the
// host / device / many entries that lock a device context.  Depends on the layers above it (knobs .. pipeline).
#pragma once
// One large MSM of host-resident inputs as G point-slices (G <= 16, slices of ~2^17 points):
// MSM = sum_g MSM(slice g), the reference's own shard/join identity (submission.ts:116-154,
// lib.rs:240-253) inside one GPU.  The slices go through the pipelined entry: slice g+1 uploads
// on the copy stream while slice g runs, so the PCIe transfer -- the bulk of a host-input MSM --
// overlaps all the compute but the last launch's; the partials are joined with G - 1 adds.  When
// G does not divide n the last slice is short: it is padded on the device (identity points, zero
// scalars) rather than run as a separate remainder MSM after the others.
int run_host_split(DevCtx* c, const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* o,
                   Pt* result) {
  // G <= 16 balanced slices of s points, a whole number of launches of nmb slices (every slice
  // is an MSM of s points to the pipelined entry; in.lens: a short slice is padded on the device
  // with identity points and zero scalars, which add no bucket entries).  (Short tail slices for
  // the last launch -- its compute is what is left after the last upload -- measured slower: one
  // more launch costs more than the shorter tail saves)
  // With MSM_HOST_TAIL_LOG = k the last launch instead holds nmb short slices of 2^k points (the
  // body then n - nmb 2^k points in Gb balanced slices): its compute after the last upload shrinks.
  const uint32_t nmb = host_batch();
  size_t t = host_tail();
  if (t * nmb * 8 > n) t = 0;  // small MSMs: no tail launch
  size_t body, Gb, s;
  for (;;) {
    body = n - t * nmb;
    Gb = std::max<size_t>(1, std::min<size_t>(16, body / host_piece()));
    Gb = (Gb + nmb - 1) / nmb * nmb;
    s = (body + Gb - 1) / Gb;
    // every slice runs as an MSM of s points (run_many sizes its buffers and clamps lengths by s):
    // a tail slice longer than a body slice would lose points, so then there is no tail launch
    if (t <= s) break;
    t = 0;
  }
  std::vector<size_t> offs, lens;
  for (size_t g = 0; g < Gb; g++) {
    offs.push_back(std::min(g * s, body));
    lens.push_back(g * s < body ? std::min(s, body - g * s) : 0);  // 0 only for tiny MSM_HOST_PIECE_LOG overrides
  }
  for (size_t g = 0; t && g < nmb; g++) {
    offs.push_back(body + g * t);
    lens.push_back(t);
  }
  const size_t G = offs.size();
  std::vector<const uint32_t*> pp(G), ss(G);
  for (size_t g = 0; g < G; g++) {
    pp[g] = points_be + offs[g] * 32;
    ss[g] = scalars_be + offs[g] * 8;
  }
  ManyInputs in;
  in.kind = ManyInputs::HOST;
  in.points = pp.data();
  in.scalars = ss.data();
  in.batch = nmb;
  in.lens = lens.data();
  std::vector<const uint32_t*> dsc(G);
  const bool pack =
      host_scalars_first() && host_own_points() && host_pack() && pin_ring_ready(c, (size_t)nmb * s * 128);
  if (pack) {
    // packed: every launch's scalars and points go up through the pinned ring from the uploader,
    // scalars first (run_many), into these device regions (slice g at g s)
    if (int rc = c->host_sc.ensure(G * s * 32)) return rc;
    ctx_packer(c);
    for (size_t g = 0; g < G; g++) dsc[g] = c->host_sc.as<uint32_t>() + g * s * 8;
    in.dev_scalars = dsc.data();
  } else if (host_scalars_first()) {
    // slice g's scalars at g s in one device buffer (s words each, the tail of a short slice is
    // its device padding): the run of full slices at the front goes up in one copy, every other
    // slice in its own
    if (int rc = c->host_sc.ensure(G * s * 32)) return rc;
    for (size_t g = 0; g < G; g++) dsc[g] = c->host_sc.as<uint32_t>() + g * s * 8;
    if (!upload_runs(c, (uint32_t)G, s, 8, [&](uint32_t g) { return ss[g]; }, [&](uint32_t g) { return lens[g]; },
                     [&](uint32_t g) { return const_cast<uint32_t*>(dsc[g]); }))
      return drain_streams(c, 0, MSM_ERR_HIP);
    in.dev_scalars = dsc.data();
  }
  // the points into a buffer of the call's own as well (slice g at g s, with room for its device
  // padding): the uploader then never waits for a slot's previous launch before a copy, so the
  // copy engine runs the whole upload back to back (MSM_HOST_OWN_PTS=0: the slots' wire buffers)
  std::vector<const uint32_t*> dpt(G);
  if (host_scalars_first() && host_own_points()) {
    // packed: room for the widest packed form, x|y|z (24 words per point)
    const size_t pw = pack ? 24 : 32;
    // (an error return waits for the scalar copy: it reads the caller's array)
    if (int rc = c->host_pts.ensure(G * s * pw * 4)) return drain_streams(c, 0, rc);
    for (size_t g = 0; g < G; g++) dpt[g] = c->host_pts.as<uint32_t>() + g * s * pw;
    in.dev_points = dpt.data();
    in.packed = pack;
  }
  // The slices' window: that of a 2^17 slice (c = 15) whatever their length.  n not a multiple of
  // 2^18 makes slices a little short of 2^17 (2^20 - 524 points: 131,007), where pipelined_window
  // would pick c = 14 -- two more windows' sort and accumulation for a 2% shorter slice
  // (msm_compute 4.3-4.4 against 3.7 ms; tools/e2e_align_probe.py).
  msm_opts oc = copy_opts(o);
  if (!oc.window_bits) oc.window_bits = pipelined_window(std::max(s, host_piece()));
  std::vector<Pt> part(G, pt_identity());
  if (int rc = run_many(c, in, s, G, &oc, nullptr, nullptr, true, part.data())) return drain_streams(c, 0, rc);
  *result = join_partials(part);
  return MSM_OK;
}

int host_entry(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts, Pt* r) {
  if ((!points_be || !scalars_be) && n) return MSM_ERR_INVALID_ARG;
  return on_device(opts, [&](DevCtx* c) {
    // the split from 3 slices' worth: at 2^18 and 2.5 x 2^17 points one launch with its points in
    // 8 MiB pieces measured 5-10% faster, from 3 x 2^17 the split (tools/e2e_size_probe.py)
    if (!host_split_off() && n >= 3 * host_piece())
      return run_host_split(c, points_be, scalars_be, n, opts, r);
    return run_host(c, points_be, scalars_be, n, opts, r);
  });
}

int device_entry(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, const msm_opts* opts,
                 void* hip_stream, Pt* r) {
  if ((!d_points_be || !d_scalars_be) && n) return MSM_ERR_INVALID_ARG;
  return on_device(opts, [&](DevCtx* c) {
    return run_device(c, d_points_be, d_scalars_be, n, opts, (hipStream_t)hip_stream, r);
  });
}

int many_entry(const ManyInputs& in, size_t n, size_t count, const msm_opts* opts, void* hip_stream, uint32_t* out,
               bool projective) {
  if (!out || (!in.scalars && count) || (!in.points && !in.shared_points && !in.prepared && count))
    return MSM_ERR_INVALID_ARG;
  if (count == 0) return MSM_OK;
  return on_device(opts, [&](DevCtx* c) {
    return run_many(c, in, n, count, opts, (hipStream_t)hip_stream, out, projective);
  });
}
