// Layer 7, one lone MSM: device inputs (run_device) and host inputs in one launch (run_host).
// Depends on the layers above it (knobs .. upload).
#pragma once
// Run one MSM with device inputs; result as a projective host point.
int run_device(DevCtx* c, const uint32_t* d_points, const uint32_t* d_scalars, size_t n, const msm_opts* o,
               hipStream_t user_stream, Pt* result) {
  if (n == 0) {
    *result = pt_identity();
    return MSM_OK;
  }
  Plan pl;
  int rc = make_plan(n, o, c->shape, &pl);
  if (rc != MSM_OK) return rc;
  const int si = 0;  // a lone MSM always uses slot 0 (the other workspaces only for pipelining)
  c->slot[si].pipelined = false;
  c->slot[si].stagger = false;
  if ((rc = ensure_workspace(c, pl, si)) != MSM_OK) return rc;
  if ((rc = order_after_user(c, user_stream, 1)) != MSM_OK) return rc;
  c->slot[si].pl = pl;
  if ((rc = launch_parts(c, pl, splat(d_points), splat(d_scalars), si, PART_ALL, c->slot[si].ws.pts.as<uint32_t>())))
    return rc;
  return finish_lone(c, si, result);
}

// One MSM of host-resident inputs: the scalars go up first and the bucket sort starts on them
// while the points upload piece by piece, each piece prepared as it lands; accumulation starts
// after the last piece.  The end-to-end time is then ~ PCIe transfer + the post-upload tail.
int run_host(DevCtx* c, const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* o,
             Pt* result) {
  if (n == 0) {
    *result = pt_identity();
    return MSM_OK;
  }
  Plan pl;
  int rc = make_plan(n, o, c->shape, &pl);
  if (rc != MSM_OK) return rc;
  const int si = 0;
  Slot& sl = c->slot[si];
  sl.pipelined = false;
  sl.stagger = false;
  Workspace& w = sl.ws;
  if ((rc = ensure_workspace(c, pl, si)) != MSM_OK) return rc;
  if ((rc = w.wire_pts.ensure(n * 128)) != MSM_OK || (rc = w.wire_sc.ensure(n * 32)) != MSM_OK) return rc;
  sl.pl = pl;
  uint32_t* pts = w.pts.as<uint32_t>();
  const BatchPtrs bp = splat(w.wire_pts.as<uint32_t>()), bs = splat(w.wire_sc.as<uint32_t>());
  auto fail = [&](int code) { return drain_streams(c, 1, code); };  // once an upload is queued
  bool t_bad = false;  // some t >= p, checked on the host (t is not uploaded): reported once the
                       // MSM has run, so the device's flags end cleared as after any call
  if (host_pack() && pin_ring_ready(c, std::min(n, UPLOAD_PTS_PIECE) * 96)) {
    // packed (as the split, §2.6): the scalars through the pinned ring, then each 8 MiB piece of
    // points as x|y (x|y|z for a piece with some z != 1), prepared in its own format as it lands
    ctx_packer(c);
    int k = 0;
    uint32_t* wsc = w.wire_sc.as<uint32_t>();
    for (size_t off = 0; off < n; off += UPLOAD_PTS_PIECE, k++) {
      const size_t cnt = std::min(UPLOAD_PTS_PIECE, n - off);
      void* buf;
      if ((rc = pin_take(c, k % NPIN, cnt * 32, &buf)) != MSM_OK) return fail(rc);
      pack_copy(*c->packer, buf, scalars_be + off * 8, cnt * 32);
      if (hipMemcpyAsync(wsc + off * 8, buf, cnt * 32, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess)
        return fail(MSM_ERR_HIP);
      if ((rc = pin_give(c, k % NPIN, c->copy_stream)) != MSM_OK) return fail(rc);
    }
    if (hipEventRecord(sl.ev_in, c->copy_stream) != hipSuccess || hipStreamWaitEvent(sl.stream, sl.ev_in, 0) != hipSuccess)
      return fail(MSM_ERR_HIP);
    if ((rc = launch_parts(c, pl, bp, bs, si, PART_SORT, pts)) != MSM_OK) return fail(rc);
    uint32_t* wp = w.wire_pts.as<uint32_t>();
    for (size_t p0 = 0; p0 < n; p0 += UPLOAD_PTS_PIECE, k++) {
      const size_t cnt = std::min(UPLOAD_PTS_PIECE, n - p0);
      void* buf;
      if ((rc = pin_take(c, k % NPIN, cnt * 96, &buf)) != MSM_OK) return fail(rc);
      // one slice: sent once, in the format it ends up with, and prepared in that format as it lands
      auto send = [&](uint32_t, uint32_t fmt) -> int {
        const size_t pw = pt_fmt_slots(fmt) * 4;
        if (hipMemcpyAsync(wp + p0 * 24, buf, cnt * pw * 4, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess)
          return MSM_ERR_HIP;
        if (int prc = pin_give(c, k % NPIN, c->copy_stream)) return prc;
        hipEvent_t e = c->ev_chunk[k % NCHUNK_EV];
        if (hipEventRecord(e, c->copy_stream) != hipSuccess || hipStreamWaitEvent(sl.stream, e, 0) != hipSuccess)
          return MSM_ERR_HIP;
        launch_prepare(wp + p0 * 24, pts + p0 * PRE_WORDS, (uint32_t)cnt, w.err.as<uint32_t>(), prep_nt(n), sl.stream, fmt);
        return hipGetLastError() != hipSuccess ? MSM_ERR_HIP : MSM_OK;
      };
      uint32_t fmt;
      rc = pack_and_send(*c->packer, static_cast<uint32_t*>(buf), 0, 1,
                         [&](uint32_t) { return std::make_pair(points_be + p0 * 32, cnt); }, &fmt, &t_bad, send);
      if (rc != MSM_OK) return fail(rc);
    }
  } else {
    if ((rc = upload_scalars(c, scalars_be, n, w.wire_sc.as<uint32_t>(), sl.stream, sl.ev_in)) != MSM_OK)
      return fail(rc);
    if ((rc = launch_parts(c, pl, bp, bs, si, PART_SORT, pts)) != MSM_OK) return fail(rc);
    if ((rc = upload_points(c, points_be, n, w.wire_pts.as<uint32_t>(), pts, w.err.as<uint32_t>(), sl.stream)) !=
        MSM_OK)
      return fail(rc);
  }
  if ((rc = launch_parts(c, pl, bp, bs, si, PART_ACC | PART_POST, pts)) != MSM_OK) return fail(rc);
  rc = finish_lone(c, si, result);
  return rc == MSM_OK && t_bad ? MSM_ERR_COORD_RANGE : rc;
}
