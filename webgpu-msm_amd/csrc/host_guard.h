// Layer 2b, guarded workspaces (the test mode of host_ctx.h's g_guard): the table of buffer names and the
// scans of one buffer's guard bands and of a zero invariant.  The hooks that drive them are
// msm_test_guard* (host_test_hooks.h).  Depends on host_ctx.h only.
#pragma once
// One finding of msm_test_guard_check (C layout: the Python binding mirrors it).  Offsets are in
// bytes: a front guard's relative to the payload's start (negative: -1 is the byte just before it), a
// back guard's relative to the payload's end (0 is the first byte past it), a zero invariant's
// relative to the payload's start (of the first and last non-zero word; count in words).
enum GuardSide : uint32_t { GUARD_SIDE_FRONT = 0, GUARD_SIDE_BACK = 1, GUARD_SIDE_ZERO = 2 };
struct GuardHit {
  uint32_t buffer;  // index into guard_names()
  int32_t device;
  int32_t slot;     // -1: not a slot's buffer (context-level, a handle's)
  uint32_t side;    // GuardSide
  int64_t first, last;
  uint64_t count;
};

// Names by buffer index: a slot's workspace in Workspace::each_buf order, its h_out, the context's own
// buffers in DevCtx::each_buf order, then a handle's records (a fixed-base table's go by the same name)
// and its preparation's error word.
const std::vector<const char*>& guard_names() {
  static const std::vector<const char*> names = [] {
    std::vector<const char*> v;
    Workspace w;
    w.each_buf([&](const char* n, Buf&) { v.push_back(n); });
    v.push_back("h_out");
    auto c = std::make_unique<DevCtx>();
    c->each_buf([&](const char* n, Buf&) { v.push_back(n); });
    v.push_back("bases_rec");
    v.push_back("bases_prep_err");
    return v;
  }();
  return names;
}
uint32_t guard_id(const char* name) {
  const auto& v = guard_names();
  for (size_t i = 0; i < v.size(); i++)
    if (!strcmp(v[i], name)) return (uint32_t)i;
  return (uint32_t)v.size();
}

// Bytes of [p, p + n) that differ from `fill`: their number, and the first and last one's index.
struct GuardSpan {
  size_t first = 0, last = 0, count = 0;
};
GuardSpan guard_span(const uint8_t* p, size_t n, uint8_t fill) {
  GuardSpan s;
  for (size_t i = 0; i < n; i++)
    if (p[i] != fill) {
      if (!s.count) s.first = i;
      s.last = i;
      s.count++;
    }
  return s;
}

// The two guard bands of one device buffer, copied back (the caller has drained the streams); a touched
// band is reported and filled again, so one violation is reported once.  Nothing for a buffer that is
// not guarded.
int guard_scan(const Buf& b, uint32_t id, int device, int slot, std::vector<GuardHit>* out) {
  if (!b.base) return MSM_OK;
  std::vector<uint8_t> tmp(GUARD_BACK);
  char* base = static_cast<char*>(b.base);
  struct Band {
    char* at;
    size_t len;
    uint32_t side;
  } bands[2] = {{base, GUARD_FRONT, GUARD_SIDE_FRONT}, {base + GUARD_FRONT + b.cap, GUARD_BACK, GUARD_SIDE_BACK}};
  for (const Band& g : bands) {
    HIPCHECK(hipMemcpy(tmp.data(), g.at, g.len, hipMemcpyDeviceToHost));
    const GuardSpan s = guard_span(tmp.data(), g.len, (uint8_t)GUARD_FILL);
    if (!s.count) continue;
    const int64_t org = g.side == GUARD_SIDE_FRONT ? -(int64_t)GUARD_FRONT : 0;
    out->push_back({id, device, slot, g.side, org + (int64_t)s.first, org + (int64_t)s.last, s.count});
    HIPCHECK(hipMemset(g.at, GUARD_FILL, g.len));
    HIPCHECK(hipStreamSynchronize(nullptr));
  }
  return MSM_OK;
}
// The same for a pinned host buffer kernels write into (read in place).
void guard_scan_host(const HostBuf& b, uint32_t id, int device, int slot, std::vector<GuardHit>* out) {
  if (!b.base) return;
  uint8_t* base = static_cast<uint8_t*>(b.base);
  const GuardSpan f = guard_span(base, GUARD_FRONT, (uint8_t)GUARD_FILL);
  if (f.count) {
    out->push_back({id, device, slot, GUARD_SIDE_FRONT, (int64_t)f.first - (int64_t)GUARD_FRONT,
                    (int64_t)f.last - (int64_t)GUARD_FRONT, f.count});
    memset(base, GUARD_FILL, GUARD_FRONT);
  }
  uint8_t* back = base + GUARD_FRONT + b.cap;
  const GuardSpan k = guard_span(back, GUARD_BACK, (uint8_t)GUARD_FILL);
  if (k.count) {
    out->push_back({id, device, slot, GUARD_SIDE_BACK, (int64_t)k.first, (int64_t)k.last, k.count});
    memset(back, GUARD_FILL, GUARD_BACK);
  }
}

// A zero invariant at quiescence: the first `bytes` of the payload (whole words) hold nothing but
// zeros.  Guarded or not.  A broken one is reported and cleared, as the guards are refilled.
int guard_scan_zero(const Buf& b, size_t bytes, uint32_t id, int device, int slot, std::vector<GuardHit>* out) {
  bytes = std::min(bytes, b.cap) & ~size_t(3);
  if (!b.p || !bytes) return MSM_OK;
  std::vector<uint32_t> tmp(bytes / 4);
  HIPCHECK(hipMemcpy(tmp.data(), b.p, bytes, hipMemcpyDeviceToHost));
  GuardHit h{id, device, slot, GUARD_SIDE_ZERO, 0, 0, 0};
  for (size_t i = 0; i < tmp.size(); i++)
    if (tmp[i]) {
      if (!h.count) h.first = (int64_t)(4 * i);
      h.last = (int64_t)(4 * i);
      h.count++;
    }
  if (!h.count) return MSM_OK;
  out->push_back(h);
  HIPCHECK(hipMemset(b.p, 0, bytes));
  HIPCHECK(hipStreamSynchronize(nullptr));
  return MSM_OK;
}

// The poison pass of msm_test_guard_poison: a guarded buffer's payload from byte `skip` on overwritten
// with the fill word (the caller has drained the streams, and synchronises the null stream after the
// last buffer).  Nothing for a buffer that is not guarded.
int guard_poison(const Buf& b, size_t skip, uint32_t word) {
  if (!b.base || skip >= b.cap) return MSM_OK;
  HIPCHECK(guard_fill_dev(static_cast<char*>(b.p) + skip, b.cap - skip, word));
  return MSM_OK;
}
void guard_poison_host(const HostBuf& b, uint32_t word) {
  if (b.base) guard_fill_host(b.p, b.cap, word);
}

// Findings on buffers that do not outlive their call (the error word of a handle's preparation),
// kept for the next msm_test_guard_check.
std::mutex g_guard_mu;
std::vector<GuardHit> g_guard_pending;
