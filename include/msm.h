/*
 * libmsm — MI355X (gfx950) multi-scalar multiplication over Edwards-BLS12
 * (ark-ed-on-bls12-377: -x^2 + y^2 = 1 + 3021 x^2 y^2 over the 253-bit BLS12-377 scalar field).
 *
 * C ABI that replaces the compute path under the reference's
 *   compute_msm(baseAffinePoints, scalars) -> Promise<{x, y}>      src/submission/submission.ts:25-157
 * i.e. the WebGPU intra-bucket reduction + Rust/wasm split / bucket-sum / window combine.
 * Plain pointers and sizes only; every entry point is re-entrant (calls on one device serialise).
 *
 * Wire formats (identical to the reference's, src/submission/consts.ts:1-4, bytes.rs:11-71):
 *   field element : 8 x uint32, BIG-endian word order (index 0 = most significant), standard form
 *   point         : x | y | t | z  = 32 x uint32 = 128 B   (t = x*y/z, z usually 1); every
 *                   coordinate must be < p (MSM_ERR_COORD_RANGE otherwise), but the MSM itself
 *                   uses only x, y and z -- d t is recomputed from the affine x y, as the oracle
 *                   (Aleo's msm over affine points) does, so an inconsistent t does not change it
 *   scalar        : 8 x uint32 big-endian = full 256-bit integer (not reduced mod r); the
 *                   msm_bases_compute* entries also take narrow scalars of ceil(b / 32) words
 *                   (MSM_FLAG_SCALAR_BITS below), native integer arrays, signed ones included
 *                   (MSM_FLAG_SCALAR_TYPE below), and little-endian 128- and 256-bit integers and
 *                   Montgomery-form field elements (MSM_FLAG_SCALAR_FIELD below)
 *   result        : x | y affine = 16 x uint32; identity = (0, 1)
 */
#ifndef MSM_MI355X_H
#define MSM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  The reference panics where these are returned (cited). */
#define MSM_OK 0
#define MSM_ERR_INVALID_ARG (-1)        /* null pointer / bad option                          */
#define MSM_ERR_UNSUPPORTED_WINDOW (-2) /* lib.rs:200,208,223,231 `Unsupported window size`  */
#define MSM_ERR_COORD_RANGE (-3)        /* bytes.rs:19 Fq::from_bigint(..).unwrap() (coord >= p) */
#define MSM_ERR_BAD_POINT (-4)          /* z == 0 (not a projective point); a compressed x of no such point */
#define MSM_ERR_HIP (-5)                /* HIP runtime failure                                */
#define MSM_ERR_NO_DEVICE (-6)          /* no gfx950 device visible: there is no CPU fallback */
#define MSM_ERR_OOM (-7)                /* device allocation failed                           */

/* hip_stream argument of the *_device entries: order after the null (legacy default) stream,
 * e.g. torch's default stream (whose handle is 0, i.e. indistinguishable from "no stream"). */
#define MSM_STREAM_NULL ((void*)1)

/* msm_opts.flags */
#define MSM_FLAG_SERIAL 1u  /* pipelined entries: one launch in flight at a time (no overlap)     */
#define MSM_FLAG_DEVICES 2u /* the device-list fields (devices, n_devices) are set: see below     */
#define MSM_FLAG_WINDOWS 4u /* the window-range fields (window_lo, window_hi) are set: see below  */
#define MSM_FLAG_HALF_WINDOWS 8u /* with MSM_FLAG_WINDOWS: window_lo / window_hi count half windows */
#define MSM_FLAG_SCALAR_BITS 16u /* scalar_bits is set: narrow scalars (msm_bases_compute* only, below) */
#define MSM_FLAG_SCALAR_TYPE 32u /* the options are a msm_opts_typed: native integer scalars (msm_bases_compute* only) */
#define MSM_FLAG_SCALAR_FIELD 64u /* msm_opts_typed.scalar_field is set: wide native scalars (msm_bases_compute* only) */

#define MSM_MAX_DEVICES 16

/* Options.  The struct is versioned by its flags: the first four fields are the original
 * (16-byte) layout, and a caller that never sets MSM_FLAG_DEVICES may pass that shorter struct --
 * the library reads `devices` / `n_devices` only when the flag is set.
 *
 * Device list (MSM_FLAG_DEVICES; SURVEY.md §8b's "device mask, n_gpus"): the MSM runs on the
 * `n_devices` listed gfx950 HIP ordinals (distinct, 1..MSM_MAX_DEVICES; `device` is ignored).  It
 * generalises the reference's only sharding precedent, the CPU/GPU split inside one compute_msm
 * call (submission.ts:116-154 + gpu_worker.ts:9-18, joined by point_add_affine lib.rs:240-253):
 *   - msm_compute / msm_compute_partial: the point vector is cut into n_devices contiguous shards
 *     (shard d = [n d / D, n (d+1) / D)), each device uploads and reduces its own shard on its own
 *     host thread (its own PCIe link), and the shards' partials are joined with one EC add each;
 *   - msm_compute_device / msm_compute_device_partial: the inputs live on one device (where the
 *     pointers were allocated, which must be listed); the other listed devices copy their shard
 *     from it over xGMI (peer copies) and reduce it, and the partials are joined the same way;
 *   - msm_compute_many / msm_compute_shared (host batches): each device takes a contiguous block
 *     of the `count` MSMs (no join: whole MSMs per device, the prover-batch replicas).
 * The result is the same group element whatever the list (tests/test_gpu_multidev.py).  A
 * repeated, negative or non-gfx950 ordinal, an empty list or more than MSM_MAX_DEVICES entries
 * give MSM_ERR_INVALID_ARG; the list is checked before any work is enqueued. */
typedef struct msm_opts {
  uint32_t window_bits; /* 0 = auto (msm_best_window); else 4..20. Replaces ?windowSize (submission.ts:29-33) */
  uint32_t run_length;  /* sorted-list entries per accumulation lane; 0 = auto                     */
  int32_t device;       /* HIP device ordinal (a gfx950 one), -1 = the calling thread's current device */
  uint32_t flags;       /* MSM_FLAG_* (0 = defaults)                                              */
  /* --- read only when flags & MSM_FLAG_DEVICES --- */
  const int32_t* devices; /* n_devices HIP ordinals                                                */
  uint32_t n_devices;
  /* --- read only when flags & MSM_FLAG_SCALAR_BITS --- */
  uint32_t scalar_bits; /* b, 1..256: every scalar is ceil(b / 32) words and below 2^b (below)        */
  /* --- read only when flags & MSM_FLAG_WINDOWS --- */
  uint32_t window_lo, window_hi; /* the MSM's windows [window_lo, window_hi) only (below)             */
} msm_opts;

/* Window range (MSM_FLAG_WINDOWS): with an explicit window_bits c, the scalars are recoded into
 * msm_window_count(c) signed-digit windows (counted from the least significant; the last is the
 * overflow window for bits 254..255 and the carry) and only windows [window_lo, window_hi) are
 * sorted, accumulated and reduced: the result is sum over those windows w of 2^(offset w) G_w.
 * The ranges of a partition of [0, msm_window_count(c)) sum (as group elements) to the whole MSM,
 * so the window ranges are a second way to shard one MSM over devices besides the point vector:
 * every device then reads all n points and scalars but does 1/D of the bucket work and of the
 * reduction.  Meant for the *_partial entries (the affine entries return the
 * range's sum in affine form, which joins by msm_point_add_affine); window_bits 0, an empty range
 * or one past the last window give MSM_ERR_INVALID_ARG, and so does the flag on
 * msm_compute_cocompute (its host share always covers every window).
 * msm_profile_t.windows reports the launch's range (its window count), not the MSM's layout:
 * msm_window_count(window_bits) gives that.
 * With MSM_FLAG_HALF_WINDOWS the range is counted in half windows, [0, 2 msm_window_count(c)):
 * half window 2w is window w's buckets of the lower half of its digit magnitudes, 2w + 1 the upper
 * half, so a range may start or end in the middle of a window (an odd number of windows can be
 * cut into equal shares). */
uint32_t msm_window_count(uint32_t window_bits);

/* Narrow scalars (MSM_FLAG_SCALAR_BITS, b = scalar_bits, 1 <= b <= 256): a prover's witness and
 * lookup columns hold booleans, bytes and 16/32/64-bit limbs, its folding challenges 128 bits.  With
 * the flag every scalar vector of the call holds words = ceil(b / 32) u32 words per scalar, big-endian
 * word order (index 0 most significant) as the 8-word format; the scalar is that integer, and its bits
 * at and above b must be zero.  The result is the group element the same entry gives for those scalars
 * zero-extended to 8 words.  The upload is `words` words per scalar, and for b <= 253 the launch runs
 * windows balanced over the scalar's own bits: with the width c (window_bits; 0 = the size's usual
 * choice, or 17 where that choice would put 64 entries or more into every bucket of so short a
 * scalar) and T = max(b + 1, 4), W' = ceil(T / c) windows of floor(T / W') bits, the
 * lowest T mod W' of them one bit wider -- 5 windows for b = 64 at c = 16 against the 17 of a 256-bit
 * scalar.  For b >= 254 the call is the 8-word one as it is.
 *
 * Dense buckets: a narrow launch of n terms whose widest window has 2^(c' - 1) buckets of n >> (c' - 1)
 * >= 128 entries each, with at most 8,192 buckets over all its windows and MSMs, accumulates by
 * bucket segment -- a wave per 256..4,096 entries of one bucket, then a fold -- instead of by runs of
 * the sorted list.  So b <= 8 needs no special care: booleans and bytes at any n are
 * faster than the same scalars zero-extended to 8 words.  Results are bit-identical either way; with
 * profiling on, msm_profile_t.accumulate covers the path's three kernels and run_length reports its
 * entries per lane.
 *
 * Honoured by the eight msm_bases_compute* entries (the subset forms included: a subset picks the
 * records, the width the digits; neither knows of the other).  Every other entry that takes msm_opts,
 * msm_bases_create* included, returns MSM_ERR_INVALID_ARG when the flag is set, before any device work.
 * b = 0 or b > 256 gives MSM_ERR_INVALID_ARG.  A caller of the 16-byte struct never sets the flag.
 *
 * A scalar with a bit set at or above b (possible only when b is not a multiple of 32) gives
 * MSM_ERR_INVALID_ARG, by the rule of the subset indices: the host entries check every vector before
 * anything is uploaded or enqueued; the device entries check on the device (b <= 253: the recode
 * kernel masks the excess bits, so the launch runs to its end, and the entry then returns the error
 * with its results unspecified; b = 254 and 255 run the 8-word launch, which takes the whole 256-bit
 * integer and checks nothing).
 *
 * On a handle of levels > 1 a narrow call (b <= 253) runs UNFOLDED on the level-0 records -- they are
 * plain prepared records -- so any window_bits is accepted, as on a levels = 1 handle.
 * msm_profile_t.windows reports the launch's W'.
 *
 * Alignment: device scalar pointers (every *_device entry, 8-word and narrow alike) must be 16-byte
 * aligned -- the kernels read scalars with 16-byte vector loads.  The narrow recode reads a vector
 * that is only 4-byte aligned (a slice of a larger tensor at b <= 32, say) word by word instead, at
 * a lower rate; host arrays need only their natural 4-byte alignment. */

/* Native scalar types (MSM_FLAG_SCALAR_TYPE): a column that already is an array of int8 / uint8 / ..
 * / int64 / uint64 elements, or a bitmap, goes to the msm_bases_compute* entries as it is -- no
 * rewrite into big-endian words, and an upload of ceil(m e / 8) bytes per vector of m scalars.
 *
 *   MSM_SCALAR_BIT                e = 1: scalar i is bit (i & 7) of byte (i >> 3), value 0 or 1
 *                                 (numpy's packbits(bitorder="little")); a vector of m scalars is
 *                                 ceil(m / 8) bytes and the pad bits of its last byte are ignored
 *   MSM_SCALAR_U8 / U16 / U32 / U64   e = 8 / 16 / 32 / 64 bits, contiguous, the host's (little-
 *                                 endian) byte order, unsigned
 *   MSM_SCALAR_I8 / I16 / I32 / I64   the same, two's complement
 *
 * The field is appended to the options: the caller fills a msm_opts_typed (a msm_opts followed by
 * scalar_type, so the bytes of every shorter struct in use keep their meaning), sets the flag and
 * passes &typed.opts; the library reads scalar_type only when the flag is set.
 *
 * Result: sum v_i P_i over the integers v_i; a negative v contributes |v| (-P_i).  It is the group
 * element the narrow call gives for the magnitudes |v_i| on bases with P_i negated where v_i < 0.
 * The signed-digit recode flips the digit's sign per scalar; nothing after it knows of the type.
 *
 * Width: with MSM_FLAG_SCALAR_BITS also set, scalar_bits = b bounds the magnitude, |v| < 2^b with
 * 1 <= b <= e; without it b = e (which covers -2^(e-1)).  For MSM_SCALAR_BIT b must be 1 or unset.
 * b = 0, b > e or an unknown scalar_type give MSM_ERR_INVALID_ARG.  The launch geometry is exactly the
 * narrow geometry of b -- the same windows, the same auto width, the same dense-bucket rule.
 *
 * A magnitude of 2^b or more (possible only when b < e) gives MSM_ERR_INVALID_ARG by the rule of the
 * narrow scalars: the host entries check every vector before anything is uploaded or enqueued; the
 * device entries mask the magnitude in the recode kernel, so the launch runs to its end, and then
 * return the error with their results unspecified.
 *
 * Honoured by the eight msm_bases_compute* entries (subsets compose unchanged); every other entry that
 * takes msm_opts, msm_bases_create* included, returns MSM_ERR_INVALID_ARG when the flag is set, before
 * any device work.  The pointer parameters keep their const uint32_t* type: callers cast.  On a
 * handle of levels > 1 a typed call runs unfolded on the level-0 records, as a narrow call does.
 *
 * Alignment: host vectors need their element's natural alignment; device vectors must be 4-byte
 * aligned (MSM_ERR_INVALID_ARG otherwise, checked on the host from the pointer value before anything
 * is enqueued).  16-byte alignment gets the 32- and 64-bit types their vector loads; a vector that is
 * only 4-byte aligned is read word by word at a lower rate, as in the narrow recode. */
#define MSM_SCALAR_BIT 1u
#define MSM_SCALAR_U8 2u
#define MSM_SCALAR_U16 3u
#define MSM_SCALAR_U32 4u
#define MSM_SCALAR_U64 5u
#define MSM_SCALAR_I8 6u
#define MSM_SCALAR_I16 7u
#define MSM_SCALAR_I32 8u
#define MSM_SCALAR_I64 9u
/* Wide scalar types (MSM_FLAG_SCALAR_FIELD): a column of 128-bit integers or of 256-bit field elements,
 * as an arkworks / snarkVM prover holds them, goes to the msm_bases_compute* entries as it is -- no
 * into_bigint() per element, no limb reversal, no zero extension.  Every element is little-endian (the
 * least significant byte first: u64 limbs of a little-endian host, least significant limb first).
 *
 *   MSM_FIELD_U128      16 B: the unsigned integer v
 *   MSM_FIELD_I128      16 B, two's complement: v; a negative v contributes |v| (-P_i), and -2^127 has
 *                       magnitude 2^127, as MSM_SCALAR_I64 treats -2^63
 *   MSM_FIELD_U256      32 B (arkworks BigInt<4>): the full 256-bit integer v, not reduced, as the wire
 *                       format's
 *   MSM_FIELD_FR_MONT   32 B (the memory of an arkworks Fr of ark-ed-on-bls12-377): a < r, and the scalar
 *                       is v = a 2^-256 mod r, with
 *                       r = 0x04aad957a68b2955982d1347970dec005293a3afc43c8afeb95aee9ac33fd9ff (251 bits)
 *
 * The field is msm_opts_typed.scalar_field, in what was the struct's tail padding (offset 44; the
 * struct stays 48 bytes and scalar_type stays at offset 40); the caller sets the flag and passes
 * &typed.opts, and the library reads scalar_field only when the flag is set.  MSM_FLAG_SCALAR_FIELD
 * together with MSM_FLAG_SCALAR_TYPE, or an unknown value, gives MSM_ERR_INVALID_ARG.
 *
 * Width, by the rule of the native types: with MSM_FLAG_SCALAR_BITS, scalar_bits = b bounds the
 * magnitude, 1 <= b <= e (e = 128 or 256); without it b = e.  For MSM_FIELD_FR_MONT b is 251 (v < r <
 * 2^251): MSM_FLAG_SCALAR_BITS must be unset or say 251.  For b <= 253 the launch geometry is exactly
 * the narrow geometry of b -- so a column of Fr runs 16 balanced windows at c = 16, without the overflow
 * window of the 8-word call.  MSM_FIELD_U256 with b = 254..256 runs the full-width geometry on the
 * little-endian words.  The result is bit-identical to the 8-word call on the same integers (for
 * MSM_FIELD_I128: on the magnitudes, with P_i negated where v_i < 0).  On a handle of levels > 1 a wide
 * call always runs unfolded on the level-0 records, b >= 254 included.
 *
 * Range errors, by the rule of the narrow and native scalars: a magnitude of 2^b or more, or for
 * MSM_FIELD_FR_MONT an a >= r, gives MSM_ERR_INVALID_ARG.  The host entries check every vector before
 * anything is uploaded or enqueued; the device entries check in the recode kernel, which masks the
 * value to b bits so that the launch runs to its end, and then return the error with their results
 * unspecified.  The handle stays usable.  MSM_FIELD_U256 at b >= 254 checks nothing.
 *
 * Alignment: host vectors need 8-byte alignment; device vectors 4-byte alignment (MSM_ERR_INVALID_ARG
 * otherwise, from the pointer value, before anything is enqueued).  A 16-byte-aligned device vector is
 * read with 16-byte vector loads, a 4-byte-aligned one word by word.  A vector of m scalars is m e / 8
 * bytes; nothing past them is touched, and that is the upload of a host entry.
 *
 * Honoured by the eight msm_bases_compute* entries (subsets, the `many` forms, MSM_FLAG_SERIAL,
 * run_length and window_bits compose unchanged); every other entry that takes msm_opts, msm_bases_create*
 * included, returns MSM_ERR_INVALID_ARG when the flag is set, before any device work. */
#define MSM_FIELD_U128 1u
#define MSM_FIELD_I128 2u
#define MSM_FIELD_U256 3u
#define MSM_FIELD_FR_MONT 4u
typedef struct msm_opts_typed {
  msm_opts opts;         /* flags has MSM_FLAG_SCALAR_TYPE or MSM_FLAG_SCALAR_FIELD                 */
  uint32_t scalar_type;  /* MSM_SCALAR_*: read only when opts.flags & MSM_FLAG_SCALAR_TYPE          */
  uint32_t scalar_field; /* MSM_FIELD_*: read only when opts.flags & MSM_FLAG_SCALAR_FIELD          */
} msm_opts_typed;

/* Per-phase device times (ms) of the most recent MSM on the calling thread's device when
 * profiling is enabled (hipEvents on the library's stream). */
typedef struct msm_profile_t {
  float prepare_points, recode_count, coarse_scan, coarse_scatter, fine_sort;
  float accumulate, fixup, bucket_reduce_1, bucket_reduce_2, readback;
  float device_total; /* first kernel start -> readback end */
  float host_tail;    /* host Horner + affine conversion (wall) */
  uint64_t entries;   /* nonzero digits sorted (= accumulation adds) */
  uint32_t window_bits, windows, run_length, chunk_len;
  double accumulate_sum; /* sum of `accumulate` over every launch profiled since msm_set_profiling */
  double device_total_sum;
  uint32_t profiled;     /* number of launches in those sums */
  uint32_t msms_per_launch; /* MSMs one launch (and one k_accumulate) covers */
  double accumulate_union_sum; /* wall time with >= 1 k_accumulate in flight, summed over the calls
                                  since msm_set_profiling (launches in flight may overlap) */
} msm_profile_t;

/* Library lifetime.  msm_init replaces the wasm init()/initThreadPool (submission.ts:89-93);
 * it probes the devices and fails with MSM_ERR_NO_DEVICE when no gfx950 is present. */
int msm_init(void);
void msm_shutdown(void);
/* Number of gfx950 devices visible, and the HIP ordinal of the index-th of them (0-based; -1 when
 * out of range).  On a node that mixes GPU types the gfx950 ordinals need not be contiguous, so
 * callers mapping a rank or a list index to opts.device / opts.devices should go through it. */
int msm_device_count(void);
int msm_device_ordinal(int index);
const char* msm_strerror(int code);

/* getBestWindowSize (submission.ts:18-23), re-tuned for signed digits on MI355X. */
uint32_t msm_best_window(size_t n);

/* compute_msm: host-resident inputs, result on the host.  n = 0 gives the identity (0, 1),
 * like the oracle's empty `Address.msm`.  Uploads overlap compute (generalises the reference's
 * staging ring, gpu.ts:146-155 / 244-271): from n = 3 * 2^17 the MSM runs as point slices of ~2^17
 * through the pipelined launches, slice g+1 uploading on a copy stream while slice g computes,
 * and the slices' partials are joined (the shard/join identity of submission.ts:116-154); there
 * the library's threads pack x|y of every point (x|y|z for a launch with some z != 1) into pinned
 * staging -- half the PCIe bytes -- and check every t < p on the host; smaller MSMs upload the
 * scalars first (the bucket sort starts on them) and the points in 2^16-point pieces, packed the
 * same way per piece, each prepared as it lands.  The packing runs on a pool of
 * MSM_HOST_PACK_THREADS (default 8) threads per device context, created on first use and parked
 * between calls, plus three pinned staging buffers per context (up to 32 MiB each at 2^20).  The
 * caller keeps ownership of the arrays; they are not read after the call returns. */
int msm_compute(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                uint32_t out_xy_be[16]);

/* compute_msm with the reference's CPU/GPU co-compute (?cpuWorkRatio, submission.ts:94-154):
 * share = floor(cpu_work_ratio * n) points [0, share) run on the library's host Pippenger
 * (msm_compute_cpu's, cpu_threads threads, <= 0 as there, its own window) on a
 * thread of their own while points [share, n) run as msm_compute(opts) on the GPU(s); the two
 * results join with one EC add (point_add_affine, lib.rs:240-253).  cpu_work_ratio 0 (or a share
 * that floors to 0) is msm_compute; a share >= n is the reference's CPU-only branch.  Still a device
 * entry: MSM_ERR_NO_DEVICE without a gfx950.  A negative or NaN ratio gives MSM_ERR_INVALID_ARG.
 * The result equals msm_compute's for every ratio; on MI355X any share > ~0.1% delays it (the host
 * runs a 2^20 MSM ~800x slower than one GPU), so this exists for interface parity. */
int msm_compute_cocompute(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                          double cpu_work_ratio, int cpu_threads, uint32_t out_xy_be[16]);

/* Same with inputs already in device memory (device pointers, wire layout).  `hip_stream` may be
 * NULL or a hipStream_t: the library's streams then wait for the work enqueued on it so far (the
 * inputs it produces), and the call returns when the result is on the host.  With NULL the
 * caller must have completed the inputs' producers (e.g. torch.cuda.synchronize()).  The same
 * holds for every *_device entry below. */
int msm_compute_device(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, const msm_opts* opts,
                       void* hip_stream, uint32_t out_xy_be[16]);

/* Shard entry for multi-GPU / co-compute: the shard's MSM as a projective point
 * X|Y|T|Z (32 big-endian words, standard form) so shards join with one EC add each
 * (generalises the cpu/gpu co-compute join, submission.ts:116-154 + lib.rs:240-253). */
int msm_compute_device_partial(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n,
                               const msm_opts* opts, void* hip_stream, uint32_t out_xyzt_be[32]);
int msm_compute_partial(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, const msm_opts* opts,
                        uint32_t out_xyzt_be[32]);
/* Sum `count` projective partials and return the affine result. */
int msm_combine_partials(const uint32_t* partials_xyzt_be, size_t count, uint32_t out_xy_be[16]);
/* The multi-GPU join of a batch: partials [world][count][32] (as one all_gather over `world`
 * ranks returns them); result k = sum over ranks of partial [w][k], affine, [count][16].  One
 * field inversion for the whole batch (Montgomery's trick) instead of one per MSM. */
int msm_combine_partials_many(const uint32_t* partials_xyzt_be, size_t world, size_t count, uint32_t* out_xy_be);

/* Batch of `count` independent MSMs of equal size n, inputs contiguous ([count][n][32] points,
 * [count][n][8] scalars), all device-resident; results [count][16].  Prover-batch shape. */
int msm_compute_batch_device(const uint32_t* d_points_be, const uint32_t* d_scalars_be, size_t n, size_t count,
                             const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be);

/* `count` independent MSMs of n points each, inputs given by per-MSM device pointers; results
 * [count][16].  Pipelined: launches of 2-4 MSMs stay on the device while the host finishes earlier ones
 * (window Horner), so throughput exceeds 1 / latency.  With window_bits = 0 the window is tuned
 * for throughput, which below 2^20 points is narrower than msm_best_window's (same results).
 * msm_compute_batch_device is this with contiguous inputs. */
int msm_compute_many_device(const uint32_t* const* d_points_be, const uint32_t* const* d_scalars_be, size_t n,
                            size_t count, const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be);
/* Same, each result as a projective X|Y|T|Z partial ([count][32] words) for a later
 * msm_combine_partials: the pipelined shard entry of a multi-GPU batch. */
int msm_compute_many_device_partial(const uint32_t* const* d_points_be, const uint32_t* const* d_scalars_be,
                                    size_t n, size_t count, const msm_opts* opts, void* hip_stream,
                                    uint32_t* out_xyzt_be);

/* Prover batch: `count` independent MSMs over ONE base vector (d_points_be, [n][32]) with their own
 * scalar vectors d_scalars_be[b] ([n][8] each); results [count][16].  The base vector is prepared
 * once per call (k_prepare_points) and every MSM reads its records; otherwise as
 * msm_compute_many_device.  BASELINE configs[4] (64 x 2^18). */
int msm_compute_shared_device(const uint32_t* d_points_be, const uint32_t* const* d_scalars_be, size_t n,
                              size_t count, const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be);

/* Host-resident batches (the streaming API of SURVEY.md §8f2).  msm_compute_many: `count`
 * independent MSMs, per-MSM host arrays; msm_compute_shared: one host base vector, per-MSM host
 * scalar vectors.  Inputs are uploaded on a copy stream into the in-flight launch slots while the
 * other slots compute (the base vector of msm_compute_shared once, piece by piece, prepared as it
 * lands); msm_compute_many packs x|y of every point as msm_compute does (t checked on the host,
 * MSM_ERR_COORD_RANGE for t >= p).  Results [count][16].  Footprint: msm_compute_many's packing
 * keeps three pinned host buffers of one launch's points and scalars (nm * n * 128 B each: nm = 2
 * MSMs per launch up to 2^21 points, 4 up to 2^18, 8 up to 2^16 -- e.g. 3 x 256 MiB at 2^20) until
 * msm_shutdown; a launch needing more than 512 MiB per buffer (MSM_PIN_MAX_MB) uploads unpacked. */
int msm_compute_many(const uint32_t* const* points_be, const uint32_t* const* scalars_be, size_t n, size_t count,
                     const msm_opts* opts, uint32_t* out_xy_be);
int msm_compute_shared(const uint32_t* points_be, const uint32_t* const* scalars_be, size_t n, size_t count,
                       const msm_opts* opts, uint32_t* out_xy_be);

/* Resident prepared bases: a prover's base vector stays fixed while every call brings new scalars,
 * so the vector is prepared once into a handle and each MSM then uploads (host entries) or reads
 * (device entries) scalars only -- no point upload, no k_prepare_points.
 *
 * A handle lives on ONE device (opts->device at creation, -1 = the calling thread's current one)
 * and holds `levels` copies of the n 128-B prepared records there: level j is 2^(j S) P_i.  With
 * levels = k > 1 every MSM runs folded: scalar i is cut into k chunks of S bits (all 256 bits, the
 * wire scalar is not reduced), and the MSM of the k n (level, point) pairs runs over the lowest Wc
 * of the width's windows only -- 1/k of the bucket reduction, k times the entries per bucket
 * (DESIGN.md §9 gives S and Wc).  levels = 1 is the plain MSM on resident records.
 *
 * Creation runs the preparation once: MSM_ERR_COORD_RANGE and MSM_ERR_BAD_POINT are reported
 * there and nowhere later.  levels: 0 = auto (1 unless a measured size says otherwise), else 1..8;
 * levels * n must stay below 2^30 and inside the launch plan's entry limit (MSM_ERR_INVALID_ARG);
 * MSM_ERR_OOM when the records do not fit; a failed creation leaves nothing allocated and *out
 * null.  opts->window_bits at creation fixes the window width of a levels > 1 handle (0 = the
 * library's choice for the folded problem).  Results of a levels > 1 handle are specified for points
 * on the curve only (the shifted levels are multiples computed with the curve's doubling law).
 * MSM_FLAG_DEVICES and MSM_FLAG_WINDOWS give MSM_ERR_INVALID_ARG at creation and at compute.
 *
 * Compute: opts may set run_length, MSM_FLAG_SERIAL and device (-1 or the handle's own); with
 * levels > 1 window_bits must be 0 or the handle's width, with levels = 1 any width is accepted
 * (the records do not depend on it).  The scalar vectors hold the handle's n scalars each (the
 * msm_bases_compute_subset* entries below take shorter and indexed ones); n = 0
 * gives the identity and count = 0 returns at once, as in the entries above.  The `many` entries
 * are pipelined as msm_compute_shared_device is.  Calls on one handle may run concurrently from
 * several threads (they serialise on the device, as every entry does).
 *
 * Lifetime: msm_bases_destroy frees the records; msm_shutdown frees those of every live handle.
 * A handle used after either returns MSM_ERR_INVALID_ARG (handles are registry tokens, never
 * dereferenced). */
typedef struct msm_bases msm_bases;
typedef struct msm_bases_info_t {
  uint64_t n;           /* points of the base vector                                   */
  uint32_t levels;      /* copies held (1 = unfolded)                                  */
  uint32_t window_bits; /* levels > 1: the window width the levels were shifted for    */
  uint32_t chunk_bits;  /* levels > 1: S, bits per scalar chunk; else 0                */
  uint32_t windows;     /* levels > 1: Wc, windows a folded MSM runs; else 0           */
  int32_t device;       /* HIP ordinal the records live on                             */
  uint32_t reserved;    /* 0 */
  uint64_t bytes;       /* device memory of the records: levels * n * 128              */
} msm_bases_info_t;
int msm_bases_create(const uint32_t* points_be, size_t n, const msm_opts* opts, uint32_t levels, msm_bases** out);
int msm_bases_create_device(const uint32_t* d_points_be, size_t n, const msm_opts* opts, uint32_t levels,
                            void* hip_stream, msm_bases** out);

/* Compressed points: an Aleo group element is its x-coordinate, so a base vector may arrive as x
 * alone -- 8 x uint32 per point, big-endian word order as every field element here -- and y is
 * recovered on the device (k_decompress_x: one inversion, a Tonelli-Shanks square root over the
 * 2^47-part of Fq*, p - 1 = 2^47 q).  y^2 = (a x^2 - 1) / (d x^2 - 1); the denominator is never 0.
 *
 *   MSM_POINTS_X_SUBGROUP  the eight words are x < p.  y is THE root whose point lies in the
 *       prime-order subgroup, [r](x, y) = O (at most one does: (x, -y) = -(x, y) + (0, -1)).  x = 0
 *       is the identity (0, 1).  A non-square y^2, or an x neither of whose points is in the
 *       subgroup, is MSM_ERR_BAD_POINT.  This differs from the reference's getPointFromX
 *       (FieldMath.ts:31-55), which returns -y without a check when [r](x, y) != O: it hands back a
 *       point outside the subgroup where this library reports an error.
 *   MSM_POINTS_X_YSIGN     bit 255 (the top bit of word 0) is a sign flag, bits 253 and 254 must be
 *       zero, the low 253 bits are x < p (MSM_ERR_COORD_RANGE otherwise).  y is the root with
 *       (y > p - y) == flag, compared on canonical integers.  No subgroup test: every curve point is
 *       representable, torsion points included ((0, flag 1) is the order-2 point (0, p - 1)).
 *       y = 0 with the flag set is MSM_ERR_BAD_POINT (non-canonical), as is a non-square y^2.
 *
 * msm_decompress_points* write wire records (x | y | t = x y | z = 1, 32 words each), which every
 * msm_compute* entry reads as they are; a point in error is written as the identity.
 * msm_bases_create_compressed* make the handle msm_bases_create* makes from the same points (the
 * decompressed x|y goes through the same preparation), from a 32-byte-per-point upload; everything
 * said of msm_bases_create* above holds, and the handle's info and compute entries do not know the
 * difference.  Rules: an unknown form, a scalar flag, MSM_FLAG_DEVICES or MSM_FLAG_WINDOWS on opts
 * give MSM_ERR_INVALID_ARG; device pointers must be 16-byte aligned (MSM_ERR_INVALID_ARG, decided
 * from the pointer value before anything is enqueued); MSM_ERR_COORD_RANGE takes precedence over
 * MSM_ERR_BAD_POINT (neither says which point); n = 0 works.  opts may set device (and, for a
 * creation, window_bits).  The device entries are ordered after the work queued on hip_stream and
 * return when the result is complete.
 *
 * msm_compress_points is the host-side inverse for affine points (x | y, 16 words each, both < p,
 * MSM_ERR_COORD_RANGE otherwise): X_SUBGROUP writes x, X_YSIGN x with the flag of y.  It tests
 * neither the curve equation nor subgroup membership. */
#define MSM_POINTS_X_SUBGROUP 1u
#define MSM_POINTS_X_YSIGN 2u
int msm_decompress_points(const uint32_t* xs_be, size_t n, uint32_t form, const msm_opts* opts,
                          uint32_t* points_be /* [n][32] wire records */);
int msm_decompress_points_device(const uint32_t* d_xs_be, size_t n, uint32_t form, const msm_opts* opts,
                                 void* hip_stream, uint32_t* d_points_be);
int msm_bases_create_compressed(const uint32_t* xs_be, size_t n, uint32_t form, const msm_opts* opts,
                                uint32_t levels, msm_bases** out);
int msm_bases_create_compressed_device(const uint32_t* d_xs_be, size_t n, uint32_t form, const msm_opts* opts,
                                       uint32_t levels, void* hip_stream, msm_bases** out);
int msm_compress_points(const uint32_t* xy_be /* [n][16] affine */, size_t n, uint32_t form,
                        uint32_t* xs_be); /* host only; does not test subgroup membership */

int msm_bases_destroy(msm_bases* bases);
int msm_bases_info(const msm_bases* bases, msm_bases_info_t* out);
int msm_bases_compute(const msm_bases* bases, const uint32_t* scalars_be, const msm_opts* opts,
                      uint32_t out_xy_be[16]);
int msm_bases_compute_device(const msm_bases* bases, const uint32_t* d_scalars_be, const msm_opts* opts,
                             void* hip_stream, uint32_t out_xy_be[16]);
int msm_bases_compute_many(const msm_bases* bases, const uint32_t* const* scalars_be, size_t count,
                           const msm_opts* opts, uint32_t* out_xy_be);
int msm_bases_compute_many_device(const msm_bases* bases, const uint32_t* const* d_scalars_be, size_t count,
                                  const msm_opts* opts, void* hip_stream, uint32_t* out_xy_be);

/* MSMs over a SUBSET of a handle's bases: one handle sized for a prover's largest polynomial serves
 * its shorter ones (a prefix, a slice) and its sparse ones (an index list) without zero-padded
 * scalar vectors.  Everything is sized by m -- the upload, the recode, the sort, the workspace and
 * the launch plan; only the record gather reaches into the handle's n records.
 *
 *   range form   (indices == NULL): result b = sum_i scalars[b][i] * P_(first + i),  i < m
 *   indexed form (indices != NULL): result b = sum_i scalars[b][i] * P_(indices[b][i])
 *
 * Each scalar vector holds m scalars (the full 256-bit wire integers, as everywhere).  The single
 * entries use indices[0]; in the `many` entries every MSM shares m (and `first`), and in indexed
 * form MSM b has its own index vector indices[b] (the pointers may repeat).  Indices may repeat
 * inside a vector, so m may exceed n.  m = 0 gives the identity, count = 0 returns at once.
 *
 * Limits as at creation: levels * m < 2^30 and inside the launch plan's entry limit; the range
 * form needs first + m <= n and the indexed form first == 0 (MSM_ERR_INVALID_ARG).  The opts rules
 * are msm_bases_compute's, and so are the results for a stale handle or null arguments.
 *
 * An index >= n gives MSM_ERR_INVALID_ARG.  The host entries check every index of every vector
 * before anything is uploaded or enqueued.  The device entries check on the device: the kernel that
 * reads the caller's indices replaces such an index by 0, so it never becomes an out-of-range read,
 * the launch runs to its end, and the entry then returns the error (its results are unspecified).
 *
 * The range [0, m) of a levels = 1 handle runs exactly as a handle of those m points does. */
typedef struct msm_subset_t {
  uint64_t first;                 /* range form: bases [first, first + m)                        */
  uint64_t m;                     /* terms per MSM                                               */
  const uint32_t* const* indices; /* NULL: range form.  Else indices[b] = the m base indices of
                                     MSM b (each < n; host arrays for the host entries, device
                                     pointers for the *_device entries); `first` must be 0       */
} msm_subset_t;
int msm_bases_compute_subset(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* scalars_be,
                             const msm_opts* opts, uint32_t out_xy_be[16]);
int msm_bases_compute_subset_device(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* d_scalars_be,
                                    const msm_opts* opts, void* hip_stream, uint32_t out_xy_be[16]);
int msm_bases_compute_subset_many(const msm_bases* bases, const msm_subset_t* subset,
                                  const uint32_t* const* scalars_be, size_t count, const msm_opts* opts,
                                  uint32_t* out_xy_be);
int msm_bases_compute_subset_many_device(const msm_bases* bases, const msm_subset_t* subset,
                                         const uint32_t* const* d_scalars_be, size_t count, const msm_opts* opts,
                                         void* hip_stream, uint32_t* out_xy_be);

/* Per-point scalar multiples of a handle's bases: Q_i = s_i * P_i, m points out where every entry
 * above ends in one (ark-ec's batch_mul beside its VariableBaseMSM).  A commitment key is updated or
 * blinded (P_i <- tau^i P_i, rho_i P_i), a folding argument halves its generators (x * G_(i+m)), many
 * keys are derived from one base (s_i * G: an index vector of zeros) -- on the device, from the resident
 * records, with one ladder per point (k_scale_points: fixed 2-bit windows over {P, 2P, 3P}, no
 * data-dependent branch, one inversion per point; DESIGN.md §9 has the measured cost).
 *
 *   subset == NULL            Q_i = scalars[i] * P_i,               i < n (m = n)
 *   range form                Q_i = scalars[i] * P_(first + i),     i < m
 *   indexed form              Q_i = scalars[i] * P_(indices[0][i]), i < m
 *
 * The subset is msm_bases_compute_subset's (first + m <= n; indexed: first == 0, each index < n,
 * repeats allowed, so m may exceed n; m < 2^30).  A handle of levels > 1 is read at level 0.
 *
 * Scalars: 8 big-endian words each, or ceil(b / 32) with MSM_FLAG_SCALAR_BITS and scalar_bits = b in
 * 1..256 (MSM_ERR_INVALID_ARG outside).  The scalar is the integer it is and is not reduced mod r, so
 * the result is also defined for the curve's torsion points; the ladder's length follows b, and a
 * 64-bit scalar costs a quarter of a 256-bit one.  Only these word formats: MSM_FLAG_SCALAR_TYPE and
 * MSM_FLAG_SCALAR_FIELD (native and wide scalars), MSM_FLAG_DEVICES, MSM_FLAG_WINDOWS and
 * MSM_FLAG_HALF_WINDOWS give MSM_ERR_INVALID_ARG before any device work.  opts->device is -1 or the
 * handle's own; run_length and MSM_FLAG_SERIAL are ignored.
 *
 * msm_bases_scale* write m wire records x | y | t = x y | z = 1, every coordinate canonical (< p);
 * s = 0, and any multiple that is the identity, gives (0, 1, 0, 1).  Scaling by ones at scalar_bits = 1
 * reads a handle's own points back -- those of a handle made from x-coordinates included.
 * msm_bases_scale_create* keep the m points as a new handle, without their leaving the device: its
 * level 0 is bit-identical to what msm_bases_create makes from the records msm_bases_scale returns;
 * `levels` and opts->window_bits mean what they mean there, and so do the limits and the errors of a
 * creation.  A failed creation leaves *out null and nothing allocated.  Results are specified for
 * on-curve bases.  m = 0: the scale entries return MSM_OK and write nothing, the create entries
 * return an empty handle.
 *
 * A scalar bit at or above b, or an index >= n, gives MSM_ERR_INVALID_ARG: from the host entries
 * before anything is uploaded or enqueued; from the device entries after the launch, which masks the
 * bit or reads base 0 instead, runs to its end and never reads out of range (the output is then
 * unspecified, a creation leaves nothing allocated, and the source handle stays usable).
 * Device pointers: d_points_be and 8-word scalars 16-byte aligned, narrow scalars and indices 4-byte
 * aligned (MSM_ERR_INVALID_ARG, decided from the pointer value before anything is enqueued); output
 * and scalars must not overlap.  The device entries are ordered after the work queued on hip_stream
 * and return when the result is complete.  A stale handle or a null argument: MSM_ERR_INVALID_ARG. */
int msm_bases_scale(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* scalars_be,
                    const msm_opts* opts, uint32_t* points_be /* [m][32] wire records */);
int msm_bases_scale_device(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* d_scalars_be,
                           const msm_opts* opts, void* hip_stream, uint32_t* d_points_be);
int msm_bases_scale_create(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* scalars_be,
                           const msm_opts* opts, uint32_t levels, msm_bases** out);
int msm_bases_scale_create_device(const msm_bases* bases, const msm_subset_t* subset, const uint32_t* d_scalars_be,
                                  const msm_opts* opts, uint32_t levels, void* hip_stream, msm_bases** out);

/* Pairwise combinations of bases handles: R_i = a_i * A_i +- b_i * B_i, m points out -- the other half
 * of a folding step beside msm_bases_scale (G_i + x * G_(i+m), x^-1 * G_i + x * G_(i+m)), a key updated
 * by a delta (P_i + Q_i) or differenced against another (P_i - Q_i), on the device, from the resident
 * records of one handle or of two.  Three kernels serve the three forms (DESIGN.md §9 has the cost):
 *
 *   no scalars                R_i = A_i +- B_i                 one complete addition per point
 *   one side has scalars      R_i = a_i * A_i +- B_i, or       msm_bases_scale's ladder on that side,
 *                             R_i = A_i +- b_i * B_i           then one addition
 *   both sides have scalars   R_i = a_i * A_i +- b_i * B_i     one joint ladder over {A, B, A + B}: a
 *                                                              doubling and an addition per scalar bit
 *
 * and every form shares one inversion among eight outputs (k_fixed_normalise).
 *
 * The A_i are the m bases that `a` selects from `bases`, the B_i the m that `b` selects from b_bases
 * (NULL: from `bases` too); each subset is read as msm_bases_scale reads one (the range form, or
 * indices[0]; repeats allowed), its rules (msm_bases_compute_subset's) hold per side, and the two
 * sides may mix the forms.  a.m == b.m == m.  Both handles are read at level 0 and must be on the same
 * device (MSM_ERR_INVALID_ARG).
 *
 * Scalars: as msm_bases_scale's -- 8 big-endian words each, or ceil(b / 32) with MSM_FLAG_SCALAR_BITS
 * and scalar_bits = b in 1..256, one width for both sides; the integer it is, not reduced mod r.  A
 * NULL array means every scalar is 1.  With MSM_COMBINE_A_BROADCAST (_B_BROADCAST) the array holds one
 * scalar that every i uses.  MSM_COMBINE_SUB subtracts the B term.  An unknown flag bit, reserved != 0,
 * a.m != b.m, a broadcast flag on a NULL array, and the opts flags msm_bases_scale refuses give
 * MSM_ERR_INVALID_ARG before any device work.
 *
 * msm_bases_combine* write m wire records x | y | t = x y | z = 1, canonical, the identity as
 * (0, 1, 0, 1); msm_bases_combine_create* keep the points as a new handle whose level 0 is bit-identical
 * to what msm_bases_create makes from those records (`levels`, opts->window_bits, the limits and the
 * errors of a creation as there; a failed creation leaves *out null and nothing allocated).  m = 0: the
 * combine entries return MSM_OK and write nothing, the create entries return an empty handle.
 *
 * A scalar bit at or above b, or an index >= n of its side's handle, gives MSM_ERR_INVALID_ARG: from
 * the host entries before anything is uploaded or enqueued; from the device entries after the launch,
 * which masks the bit or reads base 0 instead, runs to its end and never reads out of range (the output
 * is then unspecified, a creation leaves nothing allocated, and both source handles stay usable).
 * Device pointers: as msm_bases_scale's, for both scalar arrays and both index arrays -- d_points_be and
 * 8-word scalars 16-byte aligned, narrow scalars and indices 4-byte aligned; the output must overlap
 * none of them.  The device entries are ordered after the work queued on hip_stream and return when the
 * result is complete.  A stale handle or a null argument: MSM_ERR_INVALID_ARG. */
#define MSM_COMBINE_SUB          1u  /* R_i = a_i A_i - b_i B_i                               */
#define MSM_COMBINE_A_BROADCAST  2u  /* a_scalars holds ONE scalar, used for every i          */
#define MSM_COMBINE_B_BROADCAST  4u  /* likewise b_scalars                                    */
typedef struct msm_combine_t {
  const msm_bases* b_bases;   /* NULL: the B_i come from the same handle as the A_i          */
  msm_subset_t a, b;          /* the m bases A_i and B_i, each as msm_bases_scale reads a subset
                                 (range, or indices[0]); a.m == b.m == m                     */
  const uint32_t* a_scalars;  /* NULL: a_i = 1.  Else [m][sw] (or [sw] with _A_BROADCAST)     */
  const uint32_t* b_scalars;  /* NULL: b_i = 1.  Likewise                                    */
  uint32_t flags, reserved;   /* reserved = 0                                                */
} msm_combine_t;
int msm_bases_combine(const msm_bases* bases, const msm_combine_t* combine, const msm_opts* opts,
                      uint32_t* points_be /* [m][32] wire records */);
int msm_bases_combine_device(const msm_bases* bases, const msm_combine_t* combine, const msm_opts* opts,
                             void* hip_stream, uint32_t* d_points_be);
int msm_bases_combine_create(const msm_bases* bases, const msm_combine_t* combine, const msm_opts* opts,
                             uint32_t levels, msm_bases** out);
int msm_bases_combine_create_device(const msm_bases* bases, const msm_combine_t* combine, const msm_opts* opts,
                                    uint32_t levels, void* hip_stream, msm_bases** out);

/* Fixed-base tables: Q_i = sum_(j<k) s_ij * B_j for m rows of scalars over the same k bases (ark-ec's
 * FixedBase::msm / batch_mul on a generator, beside the two above): powers-of-tau and SRS generation
 * ([tau^i] G), batches of public keys or nonces (k_i * G), of Pedersen commitments (v_i * G + r_i * H),
 * the s * G legs of a folding step.  msm_bases_scale with an all-zero index vector computes the k = 1
 * case with a whole ladder per output; a table turns an output into one mixed addition per window and
 * base with no doubling, and one inversion shared by eight outputs (k_fixed_eval, k_fixed_normalise;
 * DESIGN.md §9 has the measured cost).
 *
 * msm_fixed_create builds the table of k bases, 1 <= k <= 8, taken from level 0 of a handle with a
 * msm_subset_t as msm_bases_scale reads it: NULL (all n bases, so n <= 8), the range
 * [first, first + m), or indices[0][0..m) (host array, first == 0, repeats allowed); k = m.  A handle
 * made from x-coordinates, or from points with z != 1, serves as any other.  window_bits = w is 2..16,
 * or 0 for the library's choice (12); scalar_bits = b is 1..256, or 0 for 256: the widest scalar the
 * table serves.  The table holds, for every base and every window win < W = ceil((b + 1) / w), the
 * multiples d * 2^(w win) * B_j, d = 1 .. 2^(w-1), as prepared records -- entry (j, win, d) at
 * (j W + win) 2^(w-1) + d - 1, exactly the records msm_bases_create makes of those affine points --
 * k W 2^(w-1) 128 bytes in all (5.5 MiB per base at w = 12, b = 256; 528 KiB at w = 8).  The build
 * stages the points in the device context's workspace at half the table's size, which the context
 * keeps until msm_shutdown.  A table above 256 MiB, k outside 1..8, w or b outside their ranges:
 * MSM_ERR_INVALID_ARG before any allocation.  opts: device -1 or
 * the handle's own; MSM_FLAG_DEVICES, _WINDOWS, _HALF_WINDOWS, _SCALAR_BITS, _SCALAR_TYPE and
 * _SCALAR_FIELD give MSM_ERR_INVALID_ARG; NULL is fine.  The table owns its records: the source handle
 * may be destroyed at once.  msm_fixed_destroy frees a table, msm_shutdown every live one; a table is a
 * registry token as a handle is, and a stale one gives MSM_ERR_INVALID_ARG.  A failed creation leaves
 * *out null and nothing allocated.
 *
 * Scalars: scalars_be[(i k + j) sw ..] is s_ij, sw = 8 big-endian words, or ceil(b' / 32) with
 * MSM_FLAG_SCALAR_BITS and scalar_bits = b' in 1..b (a call wider than its table: MSM_ERR_INVALID_ARG).
 * The scalar is the integer it is and is not reduced mod r.  An 8-word call on a table of b < 256 is
 * read at the table's width.  The cost follows the call's width: ceil((b' + 1) / w) additions per
 * scalar.  MSM_FLAG_SCALAR_TYPE, _SCALAR_FIELD, _DEVICES, _WINDOWS and _HALF_WINDOWS give
 * MSM_ERR_INVALID_ARG before any device work; opts->device is -1 or the table's own; m < 2^30.
 *
 * msm_fixed_mul* write m wire records x | y | t = x y | z = 1, word for word what msm_bases_scale
 * writes for the same point (the identity: (0, 1, 0, 1)).  msm_fixed_mul_create* keep the m points as
 * a new msm_bases handle, without their leaving the device: its level 0 is bit-identical to what
 * msm_bases_create makes from the records msm_fixed_mul returns; `levels` and opts->window_bits mean
 * what they mean there, and so do the limits and the errors of a creation.  m = 0: the mul entries
 * return MSM_OK and write nothing, the create entries return an empty handle.  Results are specified
 * for on-curve bases.
 *
 * A scalar bit at or above the call's width gives MSM_ERR_INVALID_ARG: from the host entries before
 * anything is uploaded or enqueued; from the device entries after the launch, which masks the bit and
 * runs to its end (the output is then unspecified, a creation leaves nothing allocated, and the table
 * stays usable).  Device pointers: d_points_be and 8-word scalars 16-byte aligned, narrow scalars
 * 4-byte aligned (MSM_ERR_INVALID_ARG, decided from the pointer value before anything is enqueued);
 * output and scalars must not overlap.  The device entries are ordered after the work queued on
 * hip_stream and return when the result is complete.  A null argument: MSM_ERR_INVALID_ARG. */
typedef struct msm_fixed msm_fixed;
typedef struct msm_fixed_info_t {
  uint32_t bases;       /* k                                                            */
  uint32_t window_bits; /* w                                                            */
  uint32_t scalar_bits; /* b: the widest scalar served                                  */
  uint32_t windows;     /* W = ceil((b + 1) / w), windows per base                      */
  uint64_t records;     /* k * W * 2^(w-1)                                              */
  uint64_t bytes;       /* device memory of the records: records * 128                  */
  int32_t device;       /* HIP ordinal the records live on                              */
  uint32_t reserved;    /* 0 */
} msm_fixed_info_t;
int msm_fixed_create(const msm_bases* bases, const msm_subset_t* subset, uint32_t window_bits, uint32_t scalar_bits,
                     const msm_opts* opts, msm_fixed** out);
/* The same table over up to MSM_FIXED_VECTOR_MAX_BASES bases, for many rows over the same few hundred or
 * few thousand generators: the row commitments of a matrix (Hyrax, Dory), batches of Pedersen vector
 * commitments, the L and R terms of an inner-product argument's short rounds.  msm_fixed_create_vector
 * returns an ordinary table: the subset, the record layout, the scalars' layout [m][k][sw], the widths,
 * the errors, the 256 MiB limit and the lifetime are msm_fixed_create's, and msm_fixed_destroy,
 * msm_fixed_info (`bases` = k) and the four msm_fixed_mul* entries serve it with the meanings above.  k
 * is 1 .. 4096 (subset == NULL: all n bases, so n <= 4096).  window_bits = 0 picks the widest w in
 * 2..12 whose table fits the 256 MiB limit: in the sweep of DESIGN.md §9 a call's time followed its
 * window count ceil((b + 1) / w) at every shape, whatever the table's size.  For b = 256 that is w = 12
 * up to k = 46, 9 at k = 256, 6 at k = 1024 and 3 at k = 4096 (tables of up to 256 MiB: pass window_bits
 * for a smaller one).  For k <= 8 the records are those msm_fixed_create makes with the same w and b.
 * A table of k <= 8 is evaluated as above whichever creator made it; one of k > 8 cuts every row into
 * parts of up to 8 bases, sums each part in a lane of its own and adds a row's parts with the complete
 * addition (k_vector_eval, k_vector_fold), in slabs of rows so that the partial sums stay within
 * 256 MiB of the device context's workspace.  m * (parts per row) >= 2^30: MSM_ERR_INVALID_ARG. */
#define MSM_FIXED_VECTOR_MAX_BASES 4096
int msm_fixed_create_vector(const msm_bases* bases, const msm_subset_t* subset, uint32_t window_bits,
                            uint32_t scalar_bits, const msm_opts* opts, msm_fixed** out);
int msm_fixed_destroy(msm_fixed* table);
int msm_fixed_info(const msm_fixed* table, msm_fixed_info_t* out);
int msm_fixed_mul(const msm_fixed* table, const uint32_t* scalars_be /* [m][k][sw] */, size_t m, const msm_opts* opts,
                  uint32_t* points_be /* [m][32] wire records */);
int msm_fixed_mul_device(const msm_fixed* table, const uint32_t* d_scalars_be, size_t m, const msm_opts* opts,
                         void* hip_stream, uint32_t* d_points_be);
int msm_fixed_mul_create(const msm_fixed* table, const uint32_t* scalars_be, size_t m, const msm_opts* opts,
                         uint32_t levels, msm_bases** out);
int msm_fixed_mul_create_device(const msm_fixed* table, const uint32_t* d_scalars_be, size_t m, const msm_opts* opts,
                                uint32_t levels, void* hip_stream, msm_bases** out);

/* Scalar-field vectors: arithmetic mod r -- the order of the curve's prime subgroup, the Fr of
 * ark-ed-on-bls12-377 -- on vectors of 32-byte elements: the scalar side of what the point entries above
 * do.  A witness folded between the rounds of an inner-product argument (a'_i = x a_i + x^-1 a_(i+m)),
 * Hadamard products, sums, differences and scalings, the powers tau^i of an SRS, inner products <a, b>,
 * and the conversion of arkworks Fr memory into the wire scalars every *_device entry reads, without the
 * vectors leaving the device.  Arithmetic mod r on scalars means something only for bases in the
 * prime-order subgroup (the curve has cofactor 4): s and s + r move a point outside it differently.
 *
 * Element forms, 32 bytes each:
 *   MSM_FR_WIRE   8 u32 words, most significant first: the scalar format of every entry above.  On input
 *                 any integer < 2^256, meaning its residue mod r; on output canonical (< r).
 *   MSM_FR_MONT   the 32 bytes of MSM_FIELD_FR_MONT (a 2^256 mod r, four little-endian u64 limbs).  On
 *                 input a >= r is an error by that type's rule: MSM_ERR_INVALID_ARG from the host entries
 *                 before anything is uploaded, from the device entries after the launch, which runs to its
 *                 end and reads nothing out of range (the results are then unspecified).  On output
 *                 canonical.
 * Every entry computes exactly; the cost is word Montgomery products (DESIGN.md §9 has the counts and the
 * measured times): converting between the forms is folded into the products an operation makes anyway.
 *
 * msm_fr_combine*: out_i = x_i * a_i +- y_i * b_i mod r for i < m.  `a` is required; b NULL: no second
 * term (y or MSM_FR_SUB without b: MSM_ERR_INVALID_ARG).  x and y are each NULL (the multiplier 1), one
 * element used for every i (MSM_FR_X_BROADCAST / MSM_FR_Y_BROADCAST) or m elements.  in_form is the form
 * of a, b, x and y, out_form that of out.  So: a fold is a = the low half, b = the high half, both
 * multipliers broadcast; a Hadamard product x per element and no b; a sum or difference a and b alone; a
 * scaling a and a broadcast x; and `a` alone converts between the forms (and reduces wire integers mod r).
 * `out` may be exactly `a` or exactly `b` (an in-place fold); any other overlap of the output with an
 * operand is MSM_ERR_INVALID_ARG from the device entries, decided from the pointer values.  An unknown
 * flag bit or form, reserved != 0 and a broadcast flag on a NULL operand give MSM_ERR_INVALID_ARG before
 * any device work.
 *
 * msm_fr_powers*: out_i = c * g^i mod r for i < n (0^0 = 1).  g and c are host arrays of 8 wire words in
 * both entries, any integers < 2^256; c NULL means 1.  A lane reaches its first power by square-and-multiply
 * and steps from there, so no chain of products is longer than about 2 log2(n / 16) + 17.
 *
 * msm_fr_dot*: sum_i a_i * b_i mod r, or sum_i a_i with b NULL, over n elements in in_form: one element
 * in out_form, written to the host array out[8] by both entries.  Two kernels: per-lane sums reduced per
 * workgroup, then one workgroup over those partial sums; no atomics, and the result does not depend on the
 * order since it is exact.
 *
 * Common rules.  m = 0 or n = 0 returns MSM_OK and touches nothing (msm_fr_dot leaves out as it is); m
 * and n are below 2^32.  opts carries the device only (NULL is fine): MSM_FLAG_SCALAR_BITS, _SCALAR_TYPE,
 * _SCALAR_FIELD, _DEVICES, _WINDOWS and _HALF_WINDOWS give MSM_ERR_INVALID_ARG.  Device vectors must be
 * 16-byte aligned, as every row of an [n, 8] int32 tensor is (MSM_ERR_INVALID_ARG, decided from the
 * pointer value before anything is enqueued).  The device entries are ordered after the work queued on
 * hip_stream and return when the result is complete; the host entries stage their vectors through the
 * device context's workspace.  A null required argument: MSM_ERR_INVALID_ARG. */
#define MSM_FR_WIRE 0u
#define MSM_FR_MONT 1u
#define MSM_FR_SUB          1u  /* out_i = x_i a_i - y_i b_i                          */
#define MSM_FR_X_BROADCAST  2u  /* x holds ONE element, used for every i             */
#define MSM_FR_Y_BROADCAST  4u  /* likewise y                                        */
typedef struct msm_fr_combine_t {
  const uint32_t* a;          /* [m][8], required                                            */
  const uint32_t* b;          /* NULL: no second term.  Else [m][8]                          */
  const uint32_t* x;          /* NULL: x_i = 1.  Else [m][8] (or [8] with _X_BROADCAST)       */
  const uint32_t* y;          /* NULL: y_i = 1.  Likewise                                    */
  uint32_t flags;             /* MSM_FR_SUB | MSM_FR_X_BROADCAST | MSM_FR_Y_BROADCAST         */
  uint32_t in_form, out_form; /* MSM_FR_WIRE or MSM_FR_MONT                                  */
  uint32_t reserved;          /* 0                                                           */
} msm_fr_combine_t;
int msm_fr_combine(const msm_fr_combine_t* combine, size_t m, const msm_opts* opts, uint32_t* out /* [m][8] */);
int msm_fr_combine_device(const msm_fr_combine_t* combine, size_t m, const msm_opts* opts, void* hip_stream,
                          uint32_t* d_out);
int msm_fr_powers(const uint32_t g_be[8], const uint32_t* c_be /* [8], or NULL: 1 */, size_t n, uint32_t out_form,
                  const msm_opts* opts, uint32_t* out /* [n][8] */);
int msm_fr_powers_device(const uint32_t g_be[8], const uint32_t* c_be, size_t n, uint32_t out_form, const msm_opts* opts,
                         void* hip_stream, uint32_t* d_out);
int msm_fr_dot(const uint32_t* a, const uint32_t* b /* NULL: sum of a */, size_t n, uint32_t in_form, uint32_t out_form,
               const msm_opts* opts, uint32_t out[8]);
int msm_fr_dot_device(const uint32_t* d_a, const uint32_t* d_b, size_t n, uint32_t in_form, uint32_t out_form,
                      const msm_opts* opts, void* hip_stream, uint32_t out[8]);

/* Scalar-field vectors, second set: what a prover or verifier still did on the host with an Fr column --
 * batch inverses (arkworks' batch_inversion_and_mul: the x^-1 of every folding round, the denominators of
 * a permutation or lookup argument, Lagrange and barycentric weights), running products and sums (the grand
 * product z_0 = 1, z_(i+1) = z_i f_i / g_i of a permutation argument, the running sums of a log-derivative
 * lookup) and tensor products of k pairs (the verifier's s_i = prod_j x_j^(+-1) after k folds, the
 * eq(r, .) table prod_j (r_j or 1 - r_j) that weights a vector table's row commitments; msm_fr_powers is
 * the pairs (1, g^(2^j))).  The element forms, the common rules above and their error codes hold for
 * every entry here: opts carries the device only, device vectors are 16-byte aligned, m < 2^32, m = 0
 * returns MSM_OK and touches nothing, a Montgomery input >= r is refused by the host entries before
 * anything is uploaded and by the device entries after the launch, results are complete on return and
 * canonical.  `c` is a host array of 8 wire words in both entries of a pair, any integer < 2^256, NULL
 * meaning 1, as msm_fr_powers' c.  DESIGN.md §9 has the products per element and the measured times.
 *
 * msm_fr_inverse*: out_i = c * a_i^-1 mod r for i < m, and out_i = 0 where a_i = 0 mod r (arkworks'
 * convention: zeros stay zeros and change nothing else; a wire input that is a non-zero multiple of r is
 * such a zero).  `out` may be exactly `a`; any other overlap is MSM_ERR_INVALID_ARG from the device entry,
 * decided from the pointer values.  Montgomery's trick per tile of 2048 elements: the elements of a tile
 * are multiplied together (a zero as 1), ONE inversion per tile -- t^(r-2) by a fixed 4-bit window over the
 * constant exponent, 249 squarings and 72 products, no branch on the data -- and a walk back: three
 * products per element, and c and the output's form folded into the tile's inverse.
 *
 * msm_fr_scan*: the inclusive running product out_i = c * prod_(j<=i) a_j, or with MSM_FR_SCAN_SUM the
 * running sum out_i = sum_(j<=i) a_j (c must then be NULL: MSM_ERR_INVALID_ARG).  MSM_FR_SCAN_EXCLUSIVE
 * takes j < i instead: out_0 = c (1 if NULL) for a product, 0 for a sum.  An unknown flag bit is
 * MSM_ERR_INVALID_ARG.  `out` may be exactly `a`, as above.  Three launches -- every span of the vector
 * folded to one total (at most 1024 spans, each a whole number of tiles), one workgroup turning the totals
 * into carries, every span scanned again from its carry -- and NO waiting between workgroups inside a
 * kernel: no look-back, no flag to spin on, no grid barrier, so nothing depends on which workgroups are
 * resident.  Three operations per element.
 *
 * msm_fr_tensor*: out_i = c * prod_(j<k) (bit_j(i) ? hi_j : lo_j) mod r for i < 2^k, bit 0 the least
 * significant, 0 <= k <= MSM_FR_TENSOR_MAX_K (more: MSM_ERR_INVALID_ARG; k = 0 gives the one element c).
 * lo and hi are host arrays [k][8] of wire words in both entries, any integers < 2^256 (NULL with k > 0:
 * MSM_ERR_INVALID_ARG); out holds 2^k elements in out_form.  A lane multiplies out the low k - 4 bits and
 * steps through the 16 products of the top four, which the host prepares: k + 12 products in a chain at
 * most, one product per element stored. */
#define MSM_FR_SCAN_SUM       1u  /* running sum instead of running product         */
#define MSM_FR_SCAN_EXCLUSIVE 2u  /* out_i over j < i instead of j <= i             */
#define MSM_FR_TENSOR_MAX_K 31u
int msm_fr_inverse(const uint32_t* a, const uint32_t* c_be /* [8], or NULL: 1 */, size_t m, uint32_t in_form,
                   uint32_t out_form, const msm_opts* opts, uint32_t* out /* [m][8] */);
int msm_fr_inverse_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t in_form, uint32_t out_form,
                          const msm_opts* opts, void* hip_stream, uint32_t* d_out);
int msm_fr_scan(const uint32_t* a, const uint32_t* c_be /* [8], or NULL: 1; NULL for a sum */, size_t m, uint32_t flags,
                uint32_t in_form, uint32_t out_form, const msm_opts* opts, uint32_t* out /* [m][8] */);
int msm_fr_scan_device(const uint32_t* d_a, const uint32_t* c_be, size_t m, uint32_t flags, uint32_t in_form,
                       uint32_t out_form, const msm_opts* opts, void* hip_stream, uint32_t* d_out);
int msm_fr_tensor(const uint32_t* lo_be /* [k][8] */, const uint32_t* hi_be /* [k][8] */, uint32_t k,
                  const uint32_t* c_be /* [8], or NULL: 1 */, uint32_t out_form, const msm_opts* opts,
                  uint32_t* out /* [2^k][8] */);
int msm_fr_tensor_device(const uint32_t* lo_be, const uint32_t* hi_be, uint32_t k, const uint32_t* c_be, uint32_t out_form,
                         const msm_opts* opts, void* hip_stream, uint32_t* d_out);

/* The reference's CPU-only path (cpuWorkRatio = 1: submission.ts:96-115 -> msm_end_to_end,
 * lib.rs:24-44, 106-121) as the library's own multithreaded host Pippenger: signed c-bit digits,
 * 7M mixed adds into per-thread bucket tables.  window_bits 0 = auto, n_threads <= 0 = all
 * hardware threads the process may run (capped by a cgroup CPU quota).  An explicit entry, never a fallback for the GPU entries. */
int msm_compute_cpu(const uint32_t* points_be, const uint32_t* scalars_be, size_t n, uint32_t window_bits,
                    int n_threads, uint32_t out_xy_be[16]);

/* point_add_affine (lib.rs:240-253): affine a + b -> affine, 16 words each. */
int msm_point_add_affine(const uint32_t a_xy_be[16], const uint32_t b_xy_be[16], uint32_t out_xy_be[16]);

/* split_dynamic (lib.rs:196-202, msm-macro lib.rs:73-177): the reference's own unsigned digit
 * split, out[w*n + i] = c-bit window w of scalar i with w = 0 the MOST significant window,
 * n_windows = ceil(256 / c).  Host-side; kept for interface parity and tests. */
int msm_split(uint32_t window_bits, const uint32_t* scalars_be, size_t n, uint32_t* out);
uint32_t msm_split_windows(uint32_t window_bits);

/* Synthetic-input utilities (the benchmark page's generators, src/ui/AllBenchmarks.tsx:107-140 and
 * src/reference/webgpu/utils.ts:81-100), host-side and multithreaded:
 *   points_be[i] = (k0 + i*step) * G for the affine base G (16 BE words), wire layout, z = 1;
 *   scalars_be[i] = 4 xorshift64(13,7,17) words (first = most significant) reduced mod p. */
int msm_gen_points(const uint32_t g_xy_be[16], uint64_t k0, uint64_t step, size_t n, uint32_t* points_be);
int msm_gen_scalars(uint64_t seed, size_t n, uint32_t* scalars_be);

/* Profiling.  enable = 0: off; 1: hipEvents between every phase (launches go eagerly, no graph
 * replay); 2: k_accumulate's duration and the device total of every launch (the production path:
 * k_accumulate always runs between two events).  msm_last_profile reports the calling thread's
 * device. */
int msm_set_profiling(int enable);
int msm_last_profile(msm_profile_t* out);

#ifdef __cplusplus
}
#endif

#endif /* MSM_MI355X_H */
