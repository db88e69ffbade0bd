// Layer 6, host inputs on their way to the device: the pinned staging ring and the copies on the copy
// stream.  Depends on the layers above it (knobs .. launch).
#pragma once
// The next staging buffer of the ring, at least `bytes` long, once the copy out of it is done.
int pin_take(DevCtx* c, int k, size_t bytes, void** out) {
  PinRing& r = c->pin;
  if (!r.ev[k] && hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming) != hipSuccess) return MSM_ERR_HIP;
  if (r.used[k] && hipEventSynchronize(r.ev[k]) != hipSuccess) return MSM_ERR_HIP;
  r.used[k] = false;
  if (int rc = r.buf[k].ensure(bytes)) return rc;
  *out = r.buf[k].p;
  return MSM_OK;
}
// The copy out of buffer k is enqueued on `s`: it is reusable once that completes.
int pin_give(DevCtx* c, int k, hipStream_t s) {
  if (hipEventRecord(c->pin.ev[k], s) != hipSuccess) return MSM_ERR_HIP;
  c->pin.used[k] = true;
  return MSM_OK;
}

// Every staging buffer of the ring at `bytes` before a packed call enqueues anything (a growth
// bumps the allocation generation).  False -- the call then uploads unpacked -- for buffers over
// 512 MiB (a launch of more than ~2^22 points: that much pinned memory per buffer costs more to
// allocate than packing saves) or when the pinned allocation fails.
bool pin_ring_ready(DevCtx* c, size_t bytes) {
  if (bytes > pin_max_bytes()) return false;
  for (int k = 0; k < NPIN; k++) {
    void* b;
    if (pin_take(c, k, bytes, &b) != MSM_OK) {
      (void)hipGetLastError();
      return false;
    }
  }
  return true;
}

// The points of a packed upload: slices [0, k) of src(m) = (records, count) packed into staging `pb` as
// x|y (slice m at record m * stride) and handed to send(m, fmt) one by one; a z != 1 in any of them packs
// every slice again as x|y|z and sends it again (over the same regions, in stream order).  *fmt is the
// format the device ends up with, *t_bad is set when some t >= p.
template <typename Src, typename Send>
int pack_and_send(PackPool& pool, uint32_t* pb, size_t stride, uint32_t k, Src&& src, uint32_t* fmt, bool* t_bad,
                  Send&& send) {
  *fmt = PT_FMT_XY;
  for (uint32_t m = 0; m < k && *fmt == PT_FMT_XY; m++) {
    if (!pack_records(pool, pb + (size_t)m * stride * 16, src(m).first, src(m).second, PT_FMT_XY, t_bad))
      *fmt = PT_FMT_XYZ;
    else if (int rc = send(m, PT_FMT_XY))
      return rc;
  }
  for (uint32_t m = 0; m < k && *fmt == PT_FMT_XYZ; m++) {
    pack_records(pool, pb + (size_t)m * stride * 24, src(m).first, src(m).second, PT_FMT_XYZ, t_bad);
    if (int rc = send(m, PT_FMT_XYZ)) return rc;
  }
  return MSM_OK;
}

// Host arrays src(i), i in [0, k), of len(i) <= n items of `per` words, each to its device region dst(i)
// on the copy stream.  Full arrays adjacent on the host whose regions are adjacent too go up in one
// copy: each pageable hipMemcpyAsync costs ~20 us of copy-engine idle time between transfers.
template <typename Src, typename Len, typename Dst>
bool upload_runs(DevCtx* c, uint32_t k, size_t n, size_t per, Src&& src, Len&& len, Dst&& dst) {
  for (uint32_t i = 0; i < k;) {
    uint32_t e = i + 1;
    if (len(i) == n)
      while (e < k && len(e) == n && src(e) == src(i) + (size_t)(e - i) * n * per &&
             dst(e) == dst(i) + (size_t)(e - i) * n * per)
        e++;
    const size_t words = (e - i == 1 ? len(i) : (size_t)(e - i) * n) * per;
    if (words && hipMemcpyAsync(dst(i), src(i), words * 4, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess)
      return false;
    i = e;
  }
  return true;
}

// Host -> device copy of one input array on the copy stream, in pieces of `piece` bytes; after
// each piece `on_piece(off, bytes)` may hand the uploaded range to the device (an event on the
// copy stream marks it).  hipMemcpyAsync stages pageable memory itself at the PCIe rate
// (tools/ubench/h2d_bench.cpp: 56 GB/s pageable or pinned), so no extra host copy is made.
template <typename F>
int upload(DevCtx* c, void* dst, const void* src, size_t bytes, size_t piece, F&& on_piece) {
  for (size_t off = 0; off < bytes; off += piece) {
    const size_t b = std::min(piece, bytes - off);
    HIPCHECK(hipMemcpyAsync(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, b,
                            hipMemcpyHostToDevice, c->copy_stream));
    if (int rc = on_piece(off, b)) return rc;
  }
  return MSM_OK;
}

constexpr size_t UPLOAD_PTS_PIECE = 65536;  // points per uploaded piece (8 MiB; a multiple of PP_THREADS)

// Upload n host points into `wire` and prepare them into `pts` piece by piece on stream `s`: the
// preparation of piece k overlaps the upload of piece k+1 (the reference's staging ring,
// gpu.ts:146-155, without its 128 MiB cap).
int upload_points(DevCtx* c, const uint32_t* points_be, size_t n, uint32_t* wire, uint32_t* pts, uint32_t* err,
                  hipStream_t s) {
  int k = 0;
  return upload(c, wire, points_be, n * 128, UPLOAD_PTS_PIECE * 128, [&](size_t off, size_t b) -> int {
    hipEvent_t e = c->ev_chunk[k++ % NCHUNK_EV];
    HIPCHECK(hipEventRecord(e, c->copy_stream));
    HIPCHECK(hipStreamWaitEvent(s, e, 0));
    const size_t p0 = off / 128;
    launch_prepare(wire + p0 * 32, pts + p0 * PRE_WORDS, (uint32_t)(b / 128), err, prep_nt(n), s);
    HIPCHECK(hipGetLastError());
    return MSM_OK;
  });
}

// Upload a scalar vector into `wire` and make stream `s` wait for it.
int upload_scalars(DevCtx* c, const uint32_t* scalars_be, size_t n, uint32_t* wire, hipStream_t s, hipEvent_t e) {
  int rc = upload(c, wire, scalars_be, n * 32, n * 32, [](size_t, size_t) { return MSM_OK; });
  if (rc != MSM_OK) return rc;
  HIPCHECK(hipEventRecord(e, c->copy_stream));
  HIPCHECK(hipStreamWaitEvent(s, e, 0));
  return MSM_OK;
}
