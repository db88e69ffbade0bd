// Layer 4, the host side of an MSM: the Horner tail, the thread pools (tail crew, tail pool, packers), the
// record packing and the result formats.  No HIP call; depends on host_knobs.h, host_ctx.h, host_plan.h.
#pragma once
// Host tail: MSM = sum_w 2^(c w) [ sum_v R_{w,v} + sum_k L 2^k R_{w,k} ]  (Horner over bit
// positions).  Follows reduce_last (lib.rs:88-104) in role: doublings between windows, then
// into_affine.  The device already emitted the terms in this file's Montgomery form
// (fe_to_host_mont).  Runs of doublings skip T (pt_dbl_proj) except the one feeding an add.

Pt term_at(const uint32_t* o) {
  Pt p;
  memcpy(p.X.l, o, 32);
  memcpy(p.Y.l, o + 8, 32);
  memcpy(p.T.l, o + 16, 32);
  memcpy(p.Z.l, o + 24, 32);
  return p;
}

// (bit position - base, term) pairs of the launch's local windows [w0, w1) of MSM terms block
// `terms` (local window l is window d.w0 + l of the MSM): V slices at the window's offset, R_k once
// per set bit b of L at offset + k + b; identity terms skipped.
void collect_terms(const Plan& pl, const uint32_t* terms, uint32_t w0, uint32_t w1, uint32_t base,
                   std::vector<std::pair<uint32_t, const uint32_t*>>* at) {
  const MsmDims& d = pl.d;
  for (uint32_t w = w0; w < w1; w++)
    for (uint32_t t = 0; t < pl.nterms; t++) {
      const uint32_t* o = terms + (size_t)(w * pl.nterms + t) * 32;
      Fq X;
      memcpy(X.l, o, 32);
      if (fq_is_zero(X) && !memcmp(o + 8, o + 24, 32)) continue;  // identity: X = 0, Y = Z
      const uint32_t off = win_off(d, d.w0 + w) - base;
      if (t < pl.nv) {
        at->emplace_back(off, o);
      } else {
        for (uint32_t b = 0; (pl.L >> b) != 0; b++)
          if ((pl.L >> b) & 1u) at->emplace_back(off + (t - pl.nv) + b, o);
      }
    }
}

// sum_j 2^(pos_j) P_j by Horner in descending position; get(j) gives P_j.
template <typename Get>
Pt horner_run(std::vector<std::pair<uint32_t, const uint32_t*>>& at, Get&& get) {
  std::stable_sort(at.begin(), at.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
  Pt acc = pt_identity();
  for (size_t j = 0; j < at.size(); j++) {
    const Pt p = get(at[j].second);
    // T of the sum is needed when another add follows at the same position, and for the final
    // result (msm_compute_partial returns X|Y|T|Z); a doubling next never reads it
    const bool want_t = j + 1 == at.size() || at[j + 1].first == at[j].first;
    acc = j == 0 ? p : pt_add(acc, p, want_t);
    const uint32_t next = j + 1 < at.size() ? at[j + 1].first : 0u;
    if (at[j].first > next) acc = pt_dbl_n(acc, (int)(at[j].first - next));
  }
  return acc;
}

Pt horner_tail(const Plan& pl, const uint32_t* terms, uint32_t m = 0) {
  const MsmDims& d = pl.d;
  terms += (size_t)m * d.Wr * pl.nterms * 32;  // MSM m's windows
  std::vector<std::pair<uint32_t, const uint32_t*>> at;
  at.reserve((size_t)d.Wr * pl.nterms * 2);
  collect_terms(pl, terms, 0, d.Wr, 0, &at);
  return horner_run(at, term_at);
}

// The tail of a lone MSM (its latency, not a pipeline's throughput, is what counts), spread over
// helper threads started right after the launch, while the device works (thread start-up before
// the launch measured +15 us of latency; after it, it overlaps the device; they spin, yielding,
// until the terms land).  The helpers compute the window sums
// W_w = sum 2^(pos - off_w) term top window first, while the calling thread runs the outer Horner
// MSM = sum_w 2^(off_w) W_w, taking each W_w as it becomes ready: ~254 doublings and ~W adds on the
// critical path instead of ~254 doublings and ~W * nterms adds.  MSM_TAIL_THREADS sets the helper
// count (default 3; 0 = the one-thread horner_tail).
// The library's host threads are sized from the process's CPU budget (host_threads(): the
// hardware threads capped by the cgroup quota -- 16 on the GPU boxes, whose nproc says 256), shared
// among the devices of the running call (a device list runs one host thread per device, and each
// device context keeps its own pools): per device b = max(2, budget / devices); packing threads
// (the caller included) b / 2 up to 8, lone-MSM tail helpers b / 4 up to 3, pipelined-tail threads
// b / 8 up to 2, plus one uploader during a host-array call.  At one device on a 16-CPU quota that
// is the measured 8 / 3 / 2; a call over 8 devices gets 1 / 0 / 0 per device, so
// its 7 device threads and 8 uploaders stay within the quota.  The MSM_*_THREADS variables fix a
// count instead.
thread_local int t_call_devices = 1;  // devices of the call running on this thread (for_each_device)
int per_device_budget() { return std::max(2, (int)host_threads() / std::max(1, t_call_devices)); }

int tail_helpers() {
  const int env = knob_tail_threads();
  return env >= 0 ? env : std::min(3, per_device_budget() / 4);
}

class TailCrew {
 public:
  // The helpers are started once (per device context) and sleep between MSMs; arm() wakes them
  // right after a launch so they spin (yielding) while the device works, and run() hands them the
  // terms.  disarm() sends them back to sleep when no terms will come (an error return).
  explicit TailCrew(int helpers) {
    for (int i = 0; i < helpers; i++) th_.emplace_back([this] { work(); });
  }
  ~TailCrew() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_.store(true);
    }
    cv_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  bool active() const { return !th_.empty(); }
  int helpers() const { return (int)th_.size(); }
  void arm() {
    if (th_.empty()) return;
    wait_idle();  // the previous round is over (run() and disarm() wait for it too)
    {
      std::lock_guard<std::mutex> lk(mu_);
      idle_.store(0);
      armed_.store(true);
      gen_++;
    }
    cv_.notify_all();
  }
  void disarm() {
    armed_.store(false);
    wait_idle();
  }
  // The terms are on the host: the helpers start on the window sums, the caller on the outer
  // Horner, taking each window sum as it becomes ready (and computing one itself when none is).
  Pt run(const Plan& pl, const uint32_t* terms) {
    Pt r;
    run_batch(pl, terms, 1, &r);
    return r;
  }
  // The same for the k MSMs of one launch (terms block m at m * Wr * nterms * 32 words): the window
  // sums of all k, top windows first, over every thread; the outer Horner of MSM 0 on the caller,
  // those of MSMs 1.. on the first helpers free (the caller runs any no helper took).
  void run_batch(const Plan& pl, const uint32_t* terms, uint32_t k, Pt* out) {
    pl_ = &pl;
    terms_ = terms;
    k_ = k;
    out_ = out;
    const uint32_t n = k * pl.d.Wr;
    sums_.assign(n, pt_identity());
    ready_.reset(new std::atomic<int>[n]);
    for (uint32_t i = 0; i < n; i++) ready_[i].store(0);
    odone_.reset(new std::atomic<int>[k]);
    for (uint32_t m = 0; m < k; m++) odone_[m].store(0);
    next_.store(0);
    next_outer_.store(1);
    go_.store(true, std::memory_order_release);
    out[0] = outer(0);
    for (uint32_t m; (m = next_outer_.fetch_add(1)) < k;) {
      out[m] = outer(m);
      odone_[m].store(1, std::memory_order_release);
    }
    for (uint32_t m = 1; m < k; m++)
      while (!odone_[m].load(std::memory_order_acquire))
        if (!take_one()) _mm_pause();
    // every helper is out of this job before its state is reset by the next one
    armed_.store(false);
    wait_idle();
    go_.store(false);
  }

 private:
  void wait_idle() {
    while (idle_.load(std::memory_order_acquire) < (int)th_.size()) _mm_pause();
  }
  // MSM m = sum_w 2^(off_w) W_w by Horner over its windows, top first, each window sum taken as it
  // becomes ready (computing others meanwhile).
  Pt outer(uint32_t m) {
    const Plan& pl = *pl_;
    const uint32_t Wr = pl.d.Wr, w0 = pl.d.w0;  // local window w is window w0 + w of the MSM
    Pt acc = pt_identity();
    bool any = false;
    for (uint32_t kk = 0; kk < Wr; kk++) {
      const uint32_t w = Wr - 1 - kk;
      while (!ready_[m * Wr + w].load(std::memory_order_acquire))
        if (!take_one()) _mm_pause();
      const Pt& p = sums_[m * Wr + w];
      const bool ident = fq_is_zero(p.X) && fq_eq(p.Y, p.Z);
      if (!ident) acc = any ? pt_add(acc, p) : p;
      any = any || !ident;
      const uint32_t next = w ? win_off(pl.d, w0 + w - 1) : 0u;
      if (any && win_off(pl.d, w0 + w) > next) acc = pt_dbl_n(acc, (int)(win_off(pl.d, w0 + w) - next));
    }
    return acc;
  }
  // One window sum, top windows (of every MSM) first; false when none is left.
  bool take_one() {
    const uint32_t Wr = pl_->d.Wr;
    const uint32_t job = next_.fetch_add(1);
    if (job >= k_ * Wr) return false;
    const uint32_t m = job % k_, w = Wr - 1 - job / k_;
    std::vector<std::pair<uint32_t, const uint32_t*>> at;
    collect_terms(*pl_, terms_ + (size_t)m * Wr * pl_->nterms * 32, w, w + 1, win_off(pl_->d, pl_->d.w0 + w), &at);
    sums_[m * Wr + w] = horner_run(at, term_at);
    ready_[m * Wr + w].store(1, std::memory_order_release);
    return true;
  }
  void work() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return quit_.load() || gen_ != seen; });
        if (quit_.load()) return;
        seen = gen_;
      }
      // armed: spin (a long device wait: stay cheap) until the terms are posted or the call ends
      uint64_t spins = 0;
      while (!go_.load(std::memory_order_acquire) && armed_.load() && !quit_.load()) {
        if (++spins > 4096) std::this_thread::yield();
        else _mm_pause();
      }
      if (go_.load(std::memory_order_acquire)) {
        for (uint32_t m; (m = next_outer_.fetch_add(1)) < k_;) {
          out_[m] = outer(m);
          odone_[m].store(1, std::memory_order_release);
        }
        while (take_one()) {
        }
      }
      idle_.fetch_add(1, std::memory_order_release);
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  uint64_t gen_ = 0;
  std::atomic<bool> go_{false}, armed_{false}, quit_{false};
  std::atomic<int> idle_{1 << 30};  // helpers done with the current round (all idle at start)
  std::atomic<uint32_t> next_{0}, next_outer_{1};
  const Plan* pl_ = nullptr;
  const uint32_t* terms_ = nullptr;
  uint32_t k_ = 1;
  Pt* out_ = nullptr;
  std::vector<Pt> sums_;
  std::unique_ptr<std::atomic<int>[]> ready_, odone_;
};

// Host tails of a pipelined run's launches (all but the last, whose tails are the run's drain and
// go over the TailCrew), on persistent worker threads: the launching thread only waits for a
// launch, copies its terms and enqueues the next one.  With the tails on the launching thread, a
// slot whose launch finished while that thread was busy with another launch's Horner waited for
// it: a kernel trace of the 2^20 bench showed one slot's next launch 300 us behind the other's
// while the device ran only that other's sort (profiles/r5/pipeline_gap.txt).
class HornerPool {
 public:
  explicit HornerPool(int threads) {
    for (int i = 0; i < threads; i++) th_.emplace_back([this] { work(); });
  }
  ~HornerPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  void push(std::function<void()> fn) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      q_.push_back(std::move(fn));
      pending_++;
    }
    cv_.notify_one();
  }
  int size() const { return (int)th_.size(); }
  // every job pushed so far has run
  void wait_all() {
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return pending_ == 0; });
  }

 private:
  void work() {
    for (;;) {
      std::function<void()> fn;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return quit_ || !q_.empty(); });
        if (q_.empty()) return;  // quit with nothing left
        fn = std::move(q_.front());
        q_.pop_front();
      }
      fn();
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (--pending_ == 0) done_cv_.notify_all();
      }
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::deque<std::function<void()>> q_;
  int pending_ = 0;
  bool quit_ = false;
};

// The packed host upload's threads: run(fn) calls fn(k, K) on K threads (the caller is k = 0) and
// returns when all are done.  Workers sleep on a condition variable between jobs; the caller spins
// (pausing) until they are done.
class PackPool {
 public:
  explicit PackPool(int threads) : k_(std::max(1, threads)) {
    for (int i = 1; i < k_; i++) th_.emplace_back([this, i] { work(i); });
  }
  ~PackPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
      gen_++;
    }
    cv_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  int size() const { return k_; }
  void run(const std::function<void(int, int)>& fn) {
    fn_ = &fn;
    done_.store(0);
    {
      std::lock_guard<std::mutex> lk(mu_);
      gen_++;
    }
    cv_.notify_all();
    fn(0, k_);
    while (done_.load(std::memory_order_acquire) < k_ - 1) _mm_pause();
  }

 private:
  void work(int i) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (quit_) return;
      }
      (*fn_)(i, k_);
      done_.fetch_add(1, std::memory_order_release);
    }
  }
  int k_;
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  uint64_t gen_ = 0;
  bool quit_ = false;
  const std::function<void(int, int)>* fn_ = nullptr;
  std::atomic<int> done_{0};
};

int pack_threads() {
  const int env = knob_pack_threads();
  return env >= 0 ? env : std::max(1, std::min(8, per_device_budget() / 2));
}

// t < p for a coordinate in BE words (t is not uploaded by the packed path, so its range is
// checked here: the reference panics on any coordinate >= p, bytes.rs:19).
inline bool be_lt_p(const uint32_t* w) {
  static const uint32_t PBE[8] = {0x12ab655eu, 0x9a2ca556u, 0x60b44d1eu, 0x5c37b001u,
                                  0x59aa76feu, 0xd0000001u, 0x0a118000u, 0x00000001u};
  for (int k = 0; k < 8; k++)
    if (w[k] != PBE[k]) return w[k] < PBE[k];
  return false;
}

// One thread's share of pack_records: records [lo, hi).  32-B loads from the caller's array and
// nontemporal 32-B stores into the pinned staging (no read-for-ownership of the lines written;
// the staging is only read again by the copy engine; cached stores measured the same,
// profiles/r5/e2e_pack.jsonl).  dst is 32-B aligned (a pinned buffer at a
// multiple of 64 B).
__attribute__((target("avx2"))) void pack_range(uint32_t* dst, const uint32_t* src, size_t lo, size_t hi, uint32_t fmt,
                                                bool* z_other, bool* t_bad) {
  const size_t pw = pt_fmt_slots(fmt) * 4;
  bool zo = false, bad = false;
  for (size_t i = lo; i < hi; i++) {
    const uint32_t* r = src + i * 32;
    __m256i* d = reinterpret_cast<__m256i*>(dst + i * pw);
    _mm256_stream_si256(d, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(r)));
    _mm256_stream_si256(d + 1, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(r + 8)));
    if (fmt == PT_FMT_XYZ) _mm256_stream_si256(d + 2, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(r + 24)));
    zo = zo || r[31] != 1u || (r[24] | r[25] | r[26] | r[27] | r[28] | r[29] | r[30]) != 0u;
    bad = bad || (r[16] >= 0x12ab655eu && !be_lt_p(r + 16));
  }
  _mm_sfence();
  *z_other = zo;
  *t_bad = bad;
}

// Pack cnt wire records (x|y|t|z, 32 BE words) into dst in format fmt (PT_FMT_XY: x|y, 16 words;
// PT_FMT_XYZ: x|y|z, 24 words) over the pool; returns whether every z is 1 (XY is then exact)
// and sets *t_bad when some t >= p.
bool pack_records(PackPool& pool, uint32_t* dst, const uint32_t* src, size_t cnt, uint32_t fmt, bool* t_bad) {
  std::atomic<bool> z_other{false}, tb{false};
  pool.run([&](int k, int K) {
    const size_t lo = cnt * k / K, hi = cnt * (k + 1) / K;
    bool zo = false, bad = false;
    pack_range(dst, src, lo, hi, fmt, &zo, &bad);
    if (zo) z_other.store(true, std::memory_order_relaxed);
    if (bad) tb.store(true, std::memory_order_relaxed);
  });
  if (tb.load()) *t_bad = true;
  return !z_other.load();
}

// Plain parallel copy into pinned staging (the packed path's scalars).
void pack_copy(PackPool& pool, void* dst, const void* src, size_t bytes) {
  pool.run([&](int k, int K) {
    const size_t lo = (bytes * k / K) & ~size_t(63), hi = k + 1 == K ? bytes : (bytes * (k + 1) / K) & ~size_t(63);
    if (hi > lo) memcpy(static_cast<char*>(dst) + lo, static_cast<const char*>(src) + lo, hi - lo);
  });
}

// Worker threads of the pool (MSM_HORNER_THREADS; 0 = the launching thread runs the tails itself).
int horner_threads() {
  const int env = knob_horner_threads();
  return env >= 0 ? env : std::min(2, per_device_budget() / 8);
}

// A device context's pools at the sizes above for the running call (re-created when the call's
// share differs from the one they were made for; calls on a context hold its mutex).
PackPool* ctx_packer(DevCtx* c) {
  const int k = pack_threads();
  if (!c->packer || c->packer->size() != k) {
    delete c->packer;
    c->packer = new PackPool(k);
  }
  return c->packer;
}
TailCrew* ctx_crew(DevCtx* c) {
  const int h = tail_helpers();
  if (!c->crew || c->crew->helpers() != h) {
    delete c->crew;
    c->crew = new TailCrew(h);
  }
  return c->crew;
}
HornerPool* ctx_pool(DevCtx* c) {
  const int h = horner_threads();
  if (h == 0) return nullptr;
  if (!c->pool || c->pool->size() != h) {
    delete c->pool;
    c->pool = new HornerPool(h);
  }
  return c->pool;
}
// Their end (DevCtx::destroy declares it: the pool classes are complete only here).
void ctx_drop_pools(DevCtx* c) {
  delete c->crew;
  delete c->pool;
  delete c->packer;
  c->crew = nullptr;
  c->pool = nullptr;
  c->packer = nullptr;
}

void pt_to_be_affine(const Pt& p, uint32_t out[16]) {
  uint64_t x[4], y[4];
  pt_to_affine_std(p, x, y);
  std_to_be_words(x, out);
  std_to_be_words(y, out + 8);
}
void pt_to_be_xyzt(const Pt& p, uint32_t out[32]) {
  uint64_t s[4];
  const Fq* f[4] = {&p.X, &p.Y, &p.T, &p.Z};
  for (int i = 0; i < 4; i++) {
    fq_to_std(*f[i], s);
    std_to_be_words(s, out + 8 * i);
  }
}
int pt_from_be_xyzt(const uint32_t in[32], Pt* p) {
  uint64_t s[4];
  Fq* f[4] = {&p->X, &p->Y, &p->T, &p->Z};
  for (int i = 0; i < 4; i++) {
    be_words_to_std(in + 8 * i, s);
    if (!std_lt_p(s)) return MSM_ERR_COORD_RANGE;
    *f[i] = fq_from_std(s);
  }
  return MSM_OK;
}

// The sum of a call's partial results (shards of a device list, slices of a split host MSM).
Pt join_partials(const std::vector<Pt>& part) {
  Pt acc = part[0];
  for (size_t i = 1; i < part.size(); i++) acc = pt_add(acc, part[i]);
  return acc;
}
