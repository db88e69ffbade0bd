// Layer 1, the environment knobs: every MSM_* variable the library reads, one accessor each, read once per
// process.  Depends on nothing but the kernels' constants (MSM_MAX_BATCH).
#pragma once
// A variable as a switch (unset: dflt; set: nonzero), as an integer, and as a clamped thread count (-1 unset).
bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : dflt;
}
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
int env_threads(const char* name, int lo, int hi) {
  const char* e = getenv(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : -1;
}

// MSM_RED_L overrides bucket_reduce_L's chunk length (any of RED1_LS, or 4; 0: unset).
uint32_t knob_red_l() { static const uint32_t v = (uint32_t)env_int("MSM_RED_L", 0); return v; }

// The first bucket-reduction stage and the second's group trees in one launch (k_bucket_reduce_1g,
// MSM_RED_FOLD=1, where the tree form of the second stage applies; default k_bucket_reduce_1 then
// k_red2_groups).  Measured slower: 287 against 157 + 31 us per two-MSM 2^20 launch -- a group's
// tree then runs on two waves of 226-VGPR lanes (the first stage's occupancy) instead of eight
// light ones.
bool red_fold() { static const bool on = env_flag("MSM_RED_FOLD", false); return on; }

// The first bucket-reduction stage on lane pairs (k_bucket_reduce_1p, MSM_RED1_PAIRS=1; default one
// lane per chunk, k_bucket_reduce_1).  Measured equal: 159-162 against 160 us per two-MSM 2^20
// launch at three or four waves per SIMD, 154 at L = 8 but with the second stage then 51 against
// 31 us -- the chains' adds are issue-bound, not latency-bound.
bool red1_pairs() { static const bool on = env_flag("MSM_RED1_PAIRS", false); return on; }

// The second bucket-reduction stage as k_red2_groups + k_red2_terms (default; MSM_RED2_TREE=0:
// k_bucket_reduce_2): see red2_tree.
bool knob_red2_tree() { static const bool on = env_flag("MSM_RED2_TREE", true); return on; }

// Whether a launch sequence holding both the point preparation and the sort runs the two side by
// side (MSM_FORK_PREP=0 keeps them in order on one stream, for A/B runs).
bool fork_prepare() { static const bool on = env_flag("MSM_FORK_PREP", true); return on; }
// The same for the launches of a pipelined run (MSM_FORK_PREP_PIPE=1; default off).  There the fork
// measured slower: 2^20 at 20 steps 1.010 against 1.044 ms per MSM, three interleaved rounds each
// (and 1.022 against 1.035 in another session, profiles/r5/pipeline_ab.jsonl) -- a captured graph's
// forked branch runs on a hardware queue of the runtime's choosing, which the other slot's launch
// may be using (kernel traces show both slots' kernels on the same queues).
bool fork_prepare_pipelined() { static const bool on = env_flag("MSM_FORK_PREP_PIPE", false); return on; }

// MSM_PP_NT=0/1 forces prep_nt's choice of nontemporal record stores (-1: unset).
int knob_pp_nt() { static const int v = env_int("MSM_PP_NT", -1); return v; }

// The scalar recoding: the fixed-geometry kernel for the common window widths (c = 13..16,
// recode_fixed), the generic loop for the others (MSM_RECODE_FIXED=0 forces it everywhere).
bool recode_fixed_on() { static const bool on = env_flag("MSM_RECODE_FIXED", true); return on; }

// MSM_TAIL_THREADS, MSM_HOST_PACK_THREADS, MSM_HORNER_THREADS fix a pool's size (host_tail.h; -1: unset).
int knob_tail_threads() { static const int v = env_threads("MSM_TAIL_THREADS", 0, 16); return v; }
int knob_pack_threads() { static const int v = env_threads("MSM_HOST_PACK_THREADS", 1, 32); return v; }
int knob_horner_threads() { static const int v = env_threads("MSM_HORNER_THREADS", 0, 16); return v; }

// Whether run_host_split packs its points (MSM_HOST_PACK, default on): the library's threads copy
// only x|y of every 128-B record (or x|y|z when some point of a launch has z != 1) into pinned
// staging, and t is derived from x and y on the device -- half the PCIe bytes of the points.
// pack_range uses AVX2 stores: a host without AVX2 uploads unpacked instead of faulting.
bool host_pack() {
  static const bool on = env_flag("MSM_HOST_PACK", true) && __builtin_cpu_supports("avx2");
  return on;
}

// The largest pinned staging buffer of the ring (pin_ring_ready): 512 MiB.
size_t pin_max_bytes() {  // MSM_PIN_MAX_MB overrides (tests force the fallback with a small cap)
  static const long mb = getenv("MSM_PIN_MAX_MB") ? atol(getenv("MSM_PIN_MAX_MB")) : 512;
  static const size_t v = mb >= 0 && mb < (1l << 30) ? (size_t)mb << 20 : size_t(512) << 20;
  return v;
}

// MSM_DENSE_MIN overrides DENSE_MIN, the entries per bucket from which a narrow launch takes the
// dense-bucket accumulation (host_plan.h; 0: unset).  1 forces the path wherever it applies, a huge
// value turns it off: for A/B runs.
uint32_t knob_dense_min() { static const uint32_t v = (uint32_t)std::max(0, env_int("MSM_DENSE_MIN", 0)); return v; }

// MSM_NO_GRAPH (set to anything): every launch sequence is enqueued eagerly, none captured.
bool graphs_enabled() { static const bool on = !getenv("MSM_NO_GRAPH"); return on; }

// MSM_SLOTS overrides pipeline_slots (0: unset or not a count); set at all, a host-input run takes no extra slot.
int knob_slots() { static const int v = env_int("MSM_SLOTS", 0); return v; }
bool knob_slots_set() { static const bool on = getenv("MSM_SLOTS") != nullptr; return on; }
// MSM_BATCH overrides pipeline_batch (1..MSM_MAX_BATCH; 0: unset).
int knob_batch() { static const int v = env_int("MSM_BATCH", 0); return v; }

// Whether a host-input pipelined run starts its last launch's sort before that launch's points
// upload (MSM_HOST_SORT_EARLY=0 disables, for A/B runs).
bool host_sort_early() { static const bool on = env_flag("MSM_HOST_SORT_EARLY", true); return on; }

// Staggered pipelined launches (default; MSM_STAGGER=0 turns them off): launch j's preparation and
// sort wait for launch j-1's accumulation -- the stream waits on the previous slot's ev_acc1,
// recorded by an event node right after k_accumulate inside that launch's graph -- so they run
// beside j-1's bucket reduction (one wave per SIMD, no LDS) instead of being dispatched into the
// accumulation that holds every CU.  Unstaggered, the two slots drifted into running their
// accumulations side by side and their sorts and reductions side by side (kernel traces t11,
// t19); staggered, 2^20 pipelined 0.966-0.973 against 0.985-1.013 ms per MSM (sessions t20-t23,
// DESIGN.md §4.1).  Device-resident inputs only: host-input launches are paced by their uploads.
// (MSM_STAGGER=2 staggers host-input launches too, for A/B runs.)
int stagger_launches() {
  static const int v = env_int("MSM_STAGGER", 1);
  return v < 0 ? 0 : v > 2 ? 2 : v;
}

// Host-input points per slice of a split MSM (run_host_split), and MSMs per launch there.
size_t host_piece() {
  static const int lg = env_int("MSM_HOST_PIECE_LOG", 17);
  static const size_t v = (size_t)1 << (lg >= 10 && lg <= 24 ? lg : 17);
  return v;
}
uint32_t host_batch() {  // two slices per launch: measured best for 2^17 slices
  static const int env = env_int("MSM_HOST_NM", 2);
  return (uint32_t)std::min(std::max(env, 1), (int)MSM_MAX_BATCH);
}

// Whether the split uploads all the scalars in one copy before the first launch's points
// (MSM_HOST_SC_FIRST=0: per launch, beside its points): one copy instead of one per launch, so
// fewer ~20-us gaps between copies, and every launch's sort can start as soon as it is enqueued.
bool host_scalars_first() { static const bool on = env_flag("MSM_HOST_SC_FIRST", true); return on; }

// Points per slice of the split's last launch (MSM_HOST_TAIL_LOG; 0 = none): round 4 measured
// such tails slower (one more launch, and the copies waited for slots); re-measured with the
// call's own upload buffers.
size_t host_tail() {
  static const int lg = env_int("MSM_HOST_TAIL_LOG", 0);
  static const size_t v = lg > 0 && lg <= 24 ? (size_t)1 << lg : 0;
  return v;
}

// The split's points into a device buffer of the call's own (default; MSM_HOST_OWN_PTS=0: the slots' wire buffers).
bool host_own_points() { static const bool on = env_flag("MSM_HOST_OWN_PTS", true); return on; }

// MSM_HOST_SPLIT=0: a large host-input MSM runs as one launch (run_host), never as pipelined slices.
bool host_split_off() { static const bool off = !env_flag("MSM_HOST_SPLIT", true); return off; }
