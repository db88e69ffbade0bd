// compute_msm — drop-in for the reference's public entry point
// (src/submission/submission.ts:25-157), routed through the N-API addon (addon.cc) into
// libmsm's HIP kernels on MI355X.  Same signature and result:
//
//   compute_msm(baseAffinePoints: BigIntPoint[] | U32ArrayPoint[],
//               scalars: bigint[] | Uint32Array[]) => Promise<{ x: bigint, y: bigint }>
//
// Also accepted (an extension, and the fast form): flat wire buffers, a Uint32Array of n x 32
// point words and one of n x 8 scalar words -- the layout flattenU32 builds -- which skips the JS
// marshalling of n point objects (at 2^20 that marshalling is ~25x the MSM itself).  Flat arrays
// over a SharedArrayBuffer (as the reference allocates them, submission.ts:35-39) are read in
// place; over a plain ArrayBuffer the addon copies them first (they could be detached meanwhile).
//
// The browser-only knobs (?windowSize=, submission.ts:29-33) become an optional third
// argument { windowSize } or the MSM_WINDOW_SIZE environment variable.  { devices: [0, 1, ...] }
// shards the MSM over those gfx950 devices inside this one call (one host thread and PCIe link
// each, partials joined with one EC add each) -- the multi-device form of the reference's
// CPU/GPU split.  { cpuWorkRatio } (or MSM_CPU_WORK_RATIO) is that split itself (?cpuWorkRatio,
// submission.ts:94-154): the first floor(ratio n) points on libmsm's host Pippenger beside the GPU
// share, joined with one EC add (msm_compute_cocompute).  Same result for every ratio; on MI355X
// any share above ~0.1% only delays it (the host is ~800x slower than one GPU).
// There is no WebGPU/WGSL/CPU fallback: without the addon or a gfx950 device this rejects.
import { createRequire } from "module";
import fs from "fs";

const require = createRequire(import.meta.url);
const addon = require("./msm_napi.node");

export const nUint32PerScalar = 8; // consts.ts:1
export const nUint32PerPoint = 4 * nUint32PerScalar; // consts.ts:3

// getBestWindowSize (submission.ts:18-23), tuned for libmsm's signed-digit pipeline.
export function getBestWindowSize(n) {
  return addon.bestWindowSize(n);
}

function windowFrom(options) {
  if (options && options.windowSize) return options.windowSize | 0;
  const env = typeof process !== "undefined" && process.env ? process.env.MSM_WINDOW_SIZE : undefined;
  return env ? parseInt(env, 10) : 0;
}

// u32ArrayToBigInts (submission.ts:159-175): 8 big-endian words per value.
export function u32ArrayToBigInts(u32Array) {
  const out = [];
  for (let i = 0; i < u32Array.length; i += 8) {
    let v = 0n;
    for (let j = 0; j < 8 && i + j < u32Array.length; j++) v = (v << 32n) | BigInt(u32Array[i + j]);
    out.push(v);
  }
  return out;
}

// U32ArrayPoint[] / Uint32Array[] -> flat wire buffers (submission.ts:75-86 layout x|y|t|z).
// Element-wise copies: on Node 12 a per-coordinate TypedArray.set() costs more than the 8 word
// copies it replaces (2^20 points: ~15-30% faster flatten, measured locally).
// Exported for tools/node_e2e.mjs, which times this JS marshalling share of compute_msm.
// The buffers live on SharedArrayBuffers (as in submission.ts:35-39), so the addon reads them in
// place.
export function flattenU32(points, scalars) {
  const n = Math.min(points.length, scalars.length);
  const pb = new Uint32Array(new SharedArrayBuffer(n * nUint32PerPoint * 4));
  const sb = new Uint32Array(new SharedArrayBuffer(n * nUint32PerScalar * 4));
  flattenInto(points, scalars, n, pb, sb);
  return [pb, sb];
}

// Staging buffers of compute_msm's object inputs, kept between calls: the first touch of fresh
// SharedArrayBuffer pages costs ~50 ms per 160 MiB (2^20 points) in page faults, more than the
// word copies.  A call takes a free pair (or makes one) and gives it back when its promise settles,
// so concurrent calls never share one; at most two pairs of up to 2^21 points are kept.
const stagingFree = [];
function takeStaging(n) {
  for (let i = 0; i < stagingFree.length; i++) if (stagingFree[i].cap >= n) return stagingFree.splice(i, 1)[0];
  return { cap: n, pb: new Uint32Array(new SharedArrayBuffer(n * nUint32PerPoint * 4)),
           sb: new Uint32Array(new SharedArrayBuffer(n * nUint32PerScalar * 4)) };
}
function giveStaging(st) {
  if (st.cap <= 1 << 21 && stagingFree.length < 2) stagingFree.push(st);
}
// Exported for tools/node_e2e.mjs: compute_msm's marshalling of object inputs into reused staging.
export function flattenStaged(points, scalars) {
  const n = Math.min(points.length, scalars.length);
  const st = takeStaging(n);
  flattenInto(points, scalars, n, st.pb, st.sb);
  return { st, pb: st.pb.subarray(0, n * nUint32PerPoint), sb: st.sb.subarray(0, n * nUint32PerScalar) };
}
export const releaseStaged = (staged) => giveStaging(staged.st);

function flattenInto(points, scalars, n, pb, sb) {
  for (let i = 0; i < n; i++) {
    const p = points[i];
    const o = i * 32;
    const x = p.x, y = p.y, t = p.t, z = p.z, s = scalars[i];
    pb[o] = x[0]; pb[o + 1] = x[1]; pb[o + 2] = x[2]; pb[o + 3] = x[3];
    pb[o + 4] = x[4]; pb[o + 5] = x[5]; pb[o + 6] = x[6]; pb[o + 7] = x[7];
    pb[o + 8] = y[0]; pb[o + 9] = y[1]; pb[o + 10] = y[2]; pb[o + 11] = y[3];
    pb[o + 12] = y[4]; pb[o + 13] = y[5]; pb[o + 14] = y[6]; pb[o + 15] = y[7];
    pb[o + 16] = t[0]; pb[o + 17] = t[1]; pb[o + 18] = t[2]; pb[o + 19] = t[3];
    pb[o + 20] = t[4]; pb[o + 21] = t[5]; pb[o + 22] = t[6]; pb[o + 23] = t[7];
    pb[o + 24] = z[0]; pb[o + 25] = z[1]; pb[o + 26] = z[2]; pb[o + 27] = z[3];
    pb[o + 28] = z[4]; pb[o + 29] = z[5]; pb[o + 30] = z[6]; pb[o + 31] = z[7];
    const q = i * 8;
    sb[q] = s[0]; sb[q + 1] = s[1]; sb[q + 2] = s[2]; sb[q + 3] = s[3];
    sb[q + 4] = s[4]; sb[q + 5] = s[5]; sb[q + 6] = s[6]; sb[q + 7] = s[7];
  }
}

function ratioFrom(options) {
  if (options && options.cpuWorkRatio !== undefined && options.cpuWorkRatio !== null) return Number(options.cpuWorkRatio);
  const env = typeof process !== "undefined" && process.env ? process.env.MSM_CPU_WORK_RATIO : undefined;
  return env ? parseFloat(env) : 0;
}

function devicesFrom(options) {
  if (!options || options.devices === undefined || options.devices === null) return undefined;
  if (!Array.isArray(options.devices)) throw new TypeError("options.devices must be an array of device ordinals");
  return options.devices;
}

export const compute_msm = async (baseAffinePoints, scalars, options) => {
  const windowSize = windowFrom(options);
  const devices = devicesFrom(options);
  const cpuWorkRatio = ratioFrom(options);
  if (baseAffinePoints instanceof Uint32Array && scalars instanceof Uint32Array) {
    // already flat wire buffers (x|y|t|z BE words per point, BE words per scalar): no marshalling
    const n = Math.min(Math.floor(baseAffinePoints.length / nUint32PerPoint), Math.floor(scalars.length / nUint32PerScalar));
    const result = await addon.computeMsmU32(baseAffinePoints.subarray(0, n * nUint32PerPoint),
                                             scalars.subarray(0, n * nUint32PerScalar), windowSize, devices, cpuWorkRatio);
    const [x, y] = u32ArrayToBigInts(result);
    return { x, y };
  }
  const hasBigInt =
    (baseAffinePoints.length > 0 && typeof baseAffinePoints[0].x === "bigint") ||
    (scalars.length > 0 && typeof scalars[0] === "bigint");
  let result;
  if (hasBigInt) {
    // native marshalling (napi_get_value_bigint_words) replaces convert_worker.ts
    const pts = typeof baseAffinePoints[0].x === "bigint" ? baseAffinePoints : baseAffinePoints.map(toBigIntPoint);
    const sc = typeof scalars[0] === "bigint" ? scalars : scalars.map((s) => u32ArrayToBigInts(s)[0]);
    result = await addon.computeMsmBigInt(pts, sc, windowSize, devices, cpuWorkRatio);
  } else {
    const staged = flattenStaged(baseAffinePoints, scalars);
    try {
      result = await addon.computeMsmU32(staged.pb, staged.sb, windowSize, devices, cpuWorkRatio);
    } finally {
      giveStaging(staged.st);
    }
  }
  const [x, y] = u32ArrayToBigInts(result);
  return { x, y };
};

// ---- resident prepared bases (msm_bases_*, include/msm.h) -----------------------------------------
// A prover's base vector is prepared once and kept on the GPU; every MSM then brings scalars only:
//
//   const bases = prepare_bases(baseAffinePoints, { levels });   // -> handle
//   const { x, y } = await compute_msm_prepared(bases, scalars); // any number of times
//   release_bases(bases);
//
// The inputs take the forms compute_msm takes (BigIntPoint[] / U32ArrayPoint[] / a flat Uint32Array of
// n x 32 words; bigint[] / Uint32Array[] / a flat Uint32Array of n x 8 words).  levels > 1 also keeps
// shifted copies of the base (folded MSMs, 0 or absent = the library's choice); a coordinate >= p
// or a z = 0 point throws here, never from compute_msm_prepared.  A handle that is never released
// is freed when the addon's environment is torn down.
function wordsOf(v, out, at) {
  let b = BigInt(v);
  if (b < 0n || b >> 256n) throw new RangeError("value must be a bigint in [0, 2^256)");
  for (let i = 7; i >= 0; i--) {
    out[at + i] = Number(b & 0xffffffffn);
    b >>= 32n;
  }
}

function pointWords(points) {
  if (points instanceof Uint32Array) return points.subarray(0, Math.floor(points.length / nUint32PerPoint) * nUint32PerPoint);
  const pb = new Uint32Array(points.length * nUint32PerPoint);
  points.forEach((p, i) =>
    ["x", "y", "t", "z"].forEach((k, j) => {
      if (typeof p[k] === "bigint") wordsOf(p[k], pb, 32 * i + 8 * j);
      else pb.set(p[k].subarray(0, 8), 32 * i + 8 * j);
    }));
  return pb;
}

// (`bits`: narrow scalars of ceil(bits / 32) words each; a bigint at or above 2^bits throws)
function scalarWords(scalars, bits) {
  if (scalars instanceof Uint32Array) return scalars;
  if (bits === undefined) {
    const sb = new Uint32Array(scalars.length * nUint32PerScalar);
    scalars.forEach((s, i) => {
      if (typeof s === "bigint") wordsOf(s, sb, 8 * i);
      else sb.set(s.subarray(0, 8), 8 * i);
    });
    return sb;
  }
  const words = Math.ceil(bits / 32);
  const sb = new Uint32Array(scalars.length * words);
  scalars.forEach((s, i) => {
    if (typeof s !== "bigint") {
      sb.set(s.subarray(0, words), words * i);
      return;
    }
    let b = s;
    if (b < 0n || b >> BigInt(bits)) throw new RangeError(`scalar must be a bigint in [0, 2^${bits})`);
    for (let k = words - 1; k >= 0; k--) {
      sb[words * i + k] = Number(b & 0xffffffffn);
      b >>= 32n;
    }
  });
  return sb;
}

// Compressed points (include/msm.h MSM_POINTS_X_*): { form: "x" } takes Aleo's form, x alone -- a
// bigint[] or a flat Uint32Array of n x 8 big-endian words -- and y is the root whose point lies in the
// prime-order subgroup (what the reference's getPointFromX computes on the host, here on the GPU and
// with an error, not -y, when neither root does).  { form: "x_ysign" } takes x with y's sign: a flat
// array carries the flag in bit 255 of each x; for bigints { signs } (an array of booleans, true for
// y > p - y) gives it and it is set here.  An x of no such point throws with the library's code
// (-4, or -3 for an x out of range).
const POINT_FORMS = { x: 1, x_ysign: 2 };
function xWords(xs, form, signs) {
  if (xs instanceof Uint32Array) {
    if (signs !== undefined) throw new TypeError("options.signs: only with bigint x-coordinates");
    return xs.subarray(0, Math.floor(xs.length / 8) * 8);
  }
  if (signs !== undefined && (form !== "x_ysign" || signs.length !== xs.length))
    throw new TypeError('options.signs: one boolean per point, with form "x_ysign"');
  const out = new Uint32Array(xs.length * 8);
  xs.forEach((x, i) => {
    wordsOf(x, out, 8 * i);
    if (signs !== undefined) {
      if (out[8 * i] >>> 31) throw new RangeError("x does not leave bit 255 free for the sign");
      if (signs[i]) out[8 * i] = (out[8 * i] | 0x80000000) >>> 0;
    }
  });
  return out;
}
function formCode(form) {
  if (!Object.prototype.hasOwnProperty.call(POINT_FORMS, form))
    throw new TypeError("options.form: one of " + Object.keys(POINT_FORMS).join(", "));
  return POINT_FORMS[form];
}

export function prepare_bases(baseAffinePoints, options) {
  const levels = options && options.levels ? options.levels | 0 : 0;
  if (options && options.form !== undefined && options.form !== null)
    return addon.prepareBases(xWords(baseAffinePoints, options.form, options.signs), levels, windowFrom(options),
                              formCode(options.form));
  return addon.prepareBases(pointWords(baseAffinePoints), levels, windowFrom(options));
}

// Compressed points -> a flat Uint32Array of n x 32 wire words (x|y|t|z, z = 1), which compute_msm
// takes as it is.  Synchronous, as prepare_bases is.
export function decompress_points(xs, options) {
  const form = options && options.form !== undefined ? options.form : "x";
  return addon.decompressPoints(xWords(xs, form, options ? options.signs : undefined), formCode(form));
}

// With a third argument the MSM runs over a subset of the handle's bases, and `scalars` gives its
// length m (msm_bases_compute_subset): { first } the range [first, first + m), { indices } (a
// Uint32Array of m base indices, repeats allowed) the bases indices[i].  An index >= handle.n, or a
// range past the end, rejects.  Without it the call is what it always was: all n bases.
// { scalarBits: b } (1..256, alone or beside either) declares narrow scalars (msm_opts
// MSM_FLAG_SCALAR_BITS): a flat Uint32Array then holds ceil(b / 32) big-endian words per scalar,
// bigints are packed to that many words (one at or above 2^b rejects), and the MSM runs the windows
// of a b-bit scalar only -- 5 instead of 17 for 64-bit limbs.
// { scalarType } (beside any of them) declares native integer scalars (msm_opts_typed,
// MSM_FLAG_SCALAR_TYPE): `scalars` is then the typed array of that type as it is, negative values
// included -- "i8" Int8Array, "u8" Uint8Array, "i16" / "u16", "i32" / "u32", "i64" BigInt64Array,
// "u64" BigUint64Array, and "bit" a Uint8Array bitmap (scalar i is bit i & 7 of byte i >> 3) whose term
// count is { m }, else indices.length, the handle's n, or 8 per byte.  Another class throws TypeError.
// scalarBits = b then bounds the magnitude, |v| < 2^b with b up to the element's width.
// The wide names (msm_opts_typed.scalar_field, MSM_FLAG_SCALAR_FIELD) -- "u128", "i128" (two's
// complement), "u256" and "fr_mont" (an arkworks Fr of ark-ed-on-bls12-377 as it lies in memory:
// Montgomery form) -- take little-endian elements of 16 / 32 bytes as a BigUint64Array, Uint32Array or
// Uint8Array that holds exactly the call's terms; another length rejects.
const WIDE_BYTES = { u128: 16, i128: 16, u256: 32, fr_mont: 32 };
const NATIVE_CLASS = {
  bit: Uint8Array, u8: Uint8Array, i8: Int8Array, u16: Uint16Array, i16: Int16Array, u32: Uint32Array, i32: Int32Array,
  u64: BigUint64Array, i64: BigInt64Array,
};
export const compute_msm_prepared = async (handle, scalars, subset) => {
  if (!handle || typeof handle.id !== "number") throw new TypeError("compute_msm_prepared(handle, scalars): not a handle");
  if (subset !== undefined && subset !== null) {
    const { first, indices, scalarBits, scalarType, m } = subset;
    if (scalarBits !== undefined && !(Number.isInteger(scalarBits) && scalarBits >= 1 && scalarBits <= 256))
      throw new RangeError("subset.scalarBits: an integer in 1..256");
    if (indices !== undefined && !(indices instanceof Uint32Array)) throw new TypeError("subset.indices: a Uint32Array");
    if (first !== undefined && !(Number.isSafeInteger(first) && first >= 0)) throw new RangeError("subset.first: a non-negative integer");
    if (scalarType !== undefined) {
      const cls = NATIVE_CLASS[scalarType], wide = WIDE_BYTES[scalarType];
      if (!cls && !wide)
        throw new TypeError("subset.scalarType: one of " + Object.keys(NATIVE_CLASS).concat(Object.keys(WIDE_BYTES)).join(", "));
      if (cls && !(scalars instanceof cls)) throw new TypeError(`subset.scalarType ${scalarType}: scalars must be a ${cls.name}`);
      if (wide) {
        if (!(scalars instanceof BigUint64Array || scalars instanceof Uint32Array || scalars instanceof Uint8Array))
          throw new TypeError(`subset.scalarType ${scalarType}: scalars must be a BigUint64Array, Uint32Array or Uint8Array`);
        if (scalars.byteLength % wide) throw new RangeError(`subset.scalarType ${scalarType}: ${wide} bytes per scalar`);
      }
      if (m !== undefined && !(Number.isSafeInteger(m) && m >= 0)) throw new RangeError("subset.m: a non-negative integer");
      // (an options object is a subset call, as above: the prefix of as many bases as scalars)
      const result = await addon.computeMsmPrepared(handle.id, scalars, first === undefined ? 0 : first, indices,
                                                    scalarBits, scalarType, m);
      const [x, y] = u32ArrayToBigInts(result);
      return { x, y };
    }
    // an empty options object is still a subset call: the prefix of as many bases as scalars
    const result = await addon.computeMsmPrepared(handle.id, scalarWords(scalars, scalarBits),
                                                  first === undefined ? 0 : first, indices, scalarBits);
    const [x, y] = u32ArrayToBigInts(result);
    return { x, y };
  }
  const result = await addon.computeMsmPrepared(handle.id, scalarWords(scalars));
  const [x, y] = u32ArrayToBigInts(result);
  return { x, y };
};

// The per-point multiples s_i * P_i of a handle's bases (msm_bases_scale*): a flat Uint32Array of
// m x 32 wire words (x|y|t|z, z = 1), m = the number of scalars, over all the bases, the range
// { first } or the bases { indices } (repeats allowed: zeros give s_i * P_0).  Scalars are bigint[] or
// Uint32Array as in compute_msm_prepared, narrow with { scalarBits }; the integer is not reduced mod
// r.  { asBases: true } keeps the points on the GPU and returns a new handle instead ({ levels,
// windowSize } as in prepare_bases), which compute_msm_prepared and release_bases accept.
// Synchronous, as prepare_bases is.
export function scale_bases_prepared(handle, scalars, options) {
  if (!handle || typeof handle.id !== "number") throw new TypeError("scale_bases_prepared(handle, scalars): not a handle");
  const { first, indices, scalarBits, asBases, levels } = options || {};
  if (scalarBits !== undefined && !(Number.isInteger(scalarBits) && scalarBits >= 1 && scalarBits <= 256))
    throw new RangeError("options.scalarBits: an integer in 1..256");
  if (indices !== undefined && !(indices instanceof Uint32Array)) throw new TypeError("options.indices: a Uint32Array");
  if (first !== undefined && !(Number.isSafeInteger(first) && first >= 0)) throw new RangeError("options.first: a non-negative integer");
  return addon.scaleBases(handle.id, scalarWords(scalars, scalarBits), first === undefined ? 0 : first, indices, scalarBits,
                          !!asBases, levels ? levels | 0 : 0, windowFrom(options));
}

// The pairwise combinations a_i * A_i +- b_i * B_i of two subsets of a handle's bases (msm_bases_combine*):
// the A_i are the handle's bases from { aFirst } or { aIndices }, the B_i those of { other } (another
// handle; default the same one) from { bFirst } or { bIndices }.  { a } and { b }: absent (the scalar 1), one
// bigint (the same scalar for every i), or m scalars as scale_bases_prepared takes them, narrow with
// { scalarBits }; the integer is not reduced mod r.  { sub: true } subtracts the B term.  { m } is the
// number of points -- default the number of per-point scalars or indices, else what both ranges hold.
// A flat Uint32Array of m x 32 wire words, or with { keep: true } a new handle ({ levels, windowSize } as
// in prepare_bases).  Synchronous, as prepare_bases is.
export function combine_bases_prepared(handle, options) {
  if (!handle || typeof handle.id !== "number") throw new TypeError("combine_bases_prepared(handle, options): not a handle");
  const { other, a, b, aFirst, bFirst, aIndices, bIndices, sub, scalarBits, keep, levels } = options || {};
  let { m } = options || {};
  if (other !== undefined && (!other || typeof other.id !== "number")) throw new TypeError("options.other: not a handle");
  if (scalarBits !== undefined && !(Number.isInteger(scalarBits) && scalarBits >= 1 && scalarBits <= 256))
    throw new RangeError("options.scalarBits: an integer in 1..256");
  for (const [name, v] of [["aIndices", aIndices], ["bIndices", bIndices]])
    if (v !== undefined && !(v instanceof Uint32Array)) throw new TypeError(`options.${name}: a Uint32Array`);
  for (const [name, v] of [["aFirst", aFirst], ["bFirst", bFirst], ["m", m]])
    if (v !== undefined && !(Number.isSafeInteger(v) && v >= 0)) throw new RangeError(`options.${name}: a non-negative integer`);
  const words = scalarBits === undefined ? 8 : Math.ceil(scalarBits / 32);
  let flags = sub ? 1 : 0;
  const side = (v, flag) => {
    if (v === undefined || v === null) return undefined;
    if (typeof v === "bigint") {
      flags |= flag;
      return scalarWords([v], scalarBits);
    }
    const w = scalarWords(v, scalarBits);
    if (m === undefined) m = w.length / words;
    return w;
  };
  const aw = side(a, 2), bw = side(b, 4);
  if (m === undefined) {
    if (aIndices) m = aIndices.length;
    else if (bIndices) m = bIndices.length;
    else m = Math.max(0, Math.min(handle.n - (aFirst || 0), (other || handle).n - (bFirst || 0)));
  }
  return addon.combineBases(handle.id, other ? other.id : undefined, aw, bw, aFirst || 0, bFirst || 0, aIndices, bIndices, m,
                            flags, scalarBits, !!keep, levels ? levels | 0 : 0, windowFrom(options));
}

// Fixed-base tables (msm_fixed_*): prepare_fixed_base builds the windowed table of k <= 8 of a handle's
// bases -- all of them, the range { first, count } or the bases { indices } (repeats allowed) -- with
// { windowBits } (2..16, default the library's 12) and { scalarBits } (the widest scalar served, default
// 256).  fixed_base_mul then computes sum_j s_ij * B_j for m rows of k scalars, row after row in
// `scalars` (bigint[] or Uint32Array as in scale_bases_prepared, narrow with { scalarBits } no wider
// than the table's; the integer is not reduced mod r): a flat Uint32Array of m x 32 wire words, or
// with { asBases: true } a new handle ({ levels, windowSize } as in prepare_bases).  The table keeps
// its own records, so the handle may be released at once; release_fixed_base frees the table.
// Synchronous, as prepare_bases is.
export function prepare_fixed_base(handle, options) {
  return prepareTable("prepare_fixed_base", handle, options, false);
}

// The same table over up to 4096 bases (msm_fixed_create_vector), for many rows over the same
// generators: row commitments of a matrix, batches of Pedersen vector commitments.  { windowBits }
// defaults to the widest window that keeps the table within 64 MiB.  fixed_base_mul and
// release_fixed_base take the table it returns.
export function prepare_vector_base(handle, options) {
  return prepareTable("prepare_vector_base", handle, options, true);
}

function prepareTable(name, handle, options, vector) {
  if (!handle || typeof handle.id !== "number") throw new TypeError(`${name}(handle): not a handle`);
  const { first, count, indices, windowBits, scalarBits } = options || {};
  if (indices !== undefined && !(indices instanceof Uint32Array)) throw new TypeError("options.indices: a Uint32Array");
  for (const [name, v] of [["first", first], ["count", count], ["windowBits", windowBits], ["scalarBits", scalarBits]])
    if (v !== undefined && !(Number.isSafeInteger(v) && v >= 0)) throw new RangeError(`options.${name}: a non-negative integer`);
  return addon.prepareFixedBase(handle.id, first, count, indices, windowBits, scalarBits, vector);
}

export function fixed_base_mul(table, scalars, options) {
  if (!table || typeof table.id !== "number")
    throw new TypeError("fixed_base_mul(table, scalars): not a table");
  const { scalarBits, asBases, levels } = options || {};
  if (scalarBits !== undefined && !(Number.isInteger(scalarBits) && scalarBits >= 1 && scalarBits <= 256))
    throw new RangeError("options.scalarBits: an integer in 1..256");
  return addon.fixedBaseMul(table.id, scalarWords(scalars, scalarBits), scalarBits, !!asBases,
                            levels ? levels | 0 : 0, windowFrom(options));
}

export function release_fixed_base(table) {
  if (!table || typeof table.id !== "number") throw new TypeError("release_fixed_base(table): not a table");
  return addon.releaseFixedBase(table.id);
}

export function release_bases(handle) {
  if (!handle || typeof handle.id !== "number") throw new TypeError("release_bases(handle): not a handle");
  return addon.releaseBases(handle.id);
}

function toBigIntPoint(p) {
  return {
    x: u32ArrayToBigInts(p.x)[0],
    y: u32ArrayToBigInts(p.y)[0],
    t: u32ArrayToBigInts(p.t)[0],
    z: u32ArrayToBigInts(p.z)[0],
  };
}

// Reference helper entry points (lib.rs:196-253), exposed for parity with the wasm module.
export const split_dynamic = (windowSize, scalarsU32) => addon.split(windowSize, scalarsU32);
export const point_add_affine = (a16, b16) => addon.pointAddAffine(a16, b16);
export const init = () => addon.init();
export const deviceCount = () => addon.deviceCount();
export const deviceOrdinals = () => addon.deviceOrdinals();

// loadTestCase (src/test-data/testCases.ts:34-52): JSON-lines points whose string fields are
// BigInts, and one decimal scalar per line.  Paths instead of fetch() URLs (Node, not a browser).
export const loadTestCase = async (pointsPath, scalarsPath) => {
  const pointsText = await fs.promises.readFile(pointsPath, "utf8");
  if (pointsText.startsWith("version https://git-lfs.github.com/spec/v1"))
    throw new Error(`${pointsPath} is a Git-LFS pointer stub, not the test data`);
  const baseAffinePoints = pointsText
    .trim()
    .split("\n")
    .filter((l) => l.length)
    .map((line) => JSON.parse(line, (key, value) => (typeof value === "string" ? BigInt(value) : value)));
  const scalarsText = await fs.promises.readFile(scalarsPath, "utf8");
  const scalars = scalarsText
    .trim()
    .split("\n")
    .filter((l) => l.length)
    .map((line) => BigInt(line));
  return { baseAffinePoints, scalars };
};

// Expected results of the reference's 2^16..2^20 cases (testCases.ts:11-32).
export const expectedPowersResult = {
  16: { x: 4490298471131273381350715833932091894064554978284853693957586604825823442429n, y: 207233051598812890797414182362695316831408959017076683749810755208551572458n },
  17: { x: 405755281347735151880827575059343698498813029460786026451708154294960743560n, y: 7112985356832152643523650125935205310677117771129806490701829425450717492869n },
  18: { x: 4020134989704514076121556080357844499902614818105934254331815581426895427831n, y: 2694327822589008080344499645494473764166611881342421427746308662023437975766n },
  19: { x: 3856727778963570638772781884183843350150969534777451295534564482755471873113n, y: 1398750101296346671684024297455637342909036274728274942667983346895370713922n },
  20: { x: 5201851187583570844529445080011852189038251929148722905178398320328749074909n, y: 3586360219804356686204324370397321114669962278596135149389460948678051407803n },
};
