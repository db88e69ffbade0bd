// Type surface of submission.mjs — identical to the reference's (src/reference/types.ts:1-13,
// src/submission/submission.ts:25-28).
export type BigIntPoint = { x: bigint; y: bigint; t: bigint; z: bigint };
export type U32ArrayPoint = { x: Uint32Array; y: Uint32Array; t: Uint32Array; z: Uint32Array };

// Extensions: flat wire buffers (n x 32 / n x 8 BE words: the fast form, no per-point
// marshalling) and options { windowSize, devices, cpuWorkRatio } (devices: gfx950 HIP ordinals to
// shard over; cpuWorkRatio: the reference's CPU/GPU split, submission.ts:94-154).
export declare const compute_msm: (
  baseAffinePoints: BigIntPoint[] | U32ArrayPoint[] | Uint32Array,
  scalars: bigint[] | Uint32Array[] | Uint32Array,
  options?: { windowSize?: number; devices?: number[]; cpuWorkRatio?: number }
) => Promise<{ x: bigint; y: bigint }>;
export declare function flattenU32(points: U32ArrayPoint[], scalars: Uint32Array[]): [Uint32Array, Uint32Array];

// Resident prepared bases: the base vector prepared once and kept on the GPU, then scalars only.
// levels > 1 keeps shifted copies too (folded MSMs); absent or 0 = the library's choice.
export type BasesHandle = { id: number; n: number; levels: number; windowSize: number; bytes: number };
export declare function prepare_bases(
  baseAffinePoints: BigIntPoint[] | U32ArrayPoint[] | Uint32Array,
  options?: { levels?: number; windowSize?: number }
): BasesHandle;
// Compressed points: `form` "x" is Aleo's form, the x-coordinate alone (y: the root whose point lies in
// the prime-order subgroup); "x_ysign" is x with y's sign (y > p - y) in bit 255 -- carried by a flat
// Uint32Array of n x 8 big-endian words, or given as `signs` beside bigint x-coordinates.  y is
// recovered on the GPU; an x of no such point throws with the library's code ("-4"; "-3" out of range).
export type PointForm = "x" | "x_ysign";
export declare function prepare_bases(
  xs: bigint[] | Uint32Array,
  options: { form: PointForm; signs?: boolean[]; levels?: number; windowSize?: number }
): BasesHandle;
// The same points as a flat Uint32Array of n x 32 wire words (x|y|t|z, z = 1), as compute_msm takes them.
export declare function decompress_points(
  xs: bigint[] | Uint32Array,
  options?: { form?: PointForm; signs?: boolean[] }
): Uint32Array;
// With `subset` the MSM runs over a subset of the handle's bases and `scalars` gives its length m:
// the range [first, first + m), or the bases indices[0..m) (each < handle.n, repeats allowed;
// `first` must then be absent or 0).  An index or a range outside the handle rejects.
// `scalarBits` = b (1..256), alone or beside either: narrow scalars -- a flat Uint32Array holds
// ceil(b / 32) big-endian words per scalar, bigints are packed to that many words (one at or above
// 2^b rejects) -- and the MSM runs the windows of a b-bit scalar only.
// `scalarType`: native integer scalars -- `scalars` is the typed array of that type as it is, negative
// values included (Int8Array for "i8", Uint8Array for "u8" and for a "bit" bitmap, .. BigInt64Array for
// "i64", BigUint64Array for "u64"; another class throws TypeError); scalarBits then bounds the
// magnitude (|v| < 2^b, b up to the element's width) and `m` counts a bitmap's terms.
// The wide names take little-endian elements of 16 bytes ("u128"; "i128", two's complement) or 32 bytes
// ("u256"; "fr_mont", an ark-ed-on-bls12-377 Fr as it lies in memory, Montgomery form) as a
// BigUint64Array, Uint32Array or Uint8Array that holds exactly the call's terms.
export type ScalarType =
  | "bit" | "u8" | "i8" | "u16" | "i16" | "u32" | "i32" | "u64" | "i64" | "u128" | "i128" | "u256" | "fr_mont";
export type NativeScalars =
  | Uint8Array | Int8Array | Uint16Array | Int16Array | Uint32Array | Int32Array | BigUint64Array | BigInt64Array;
export type BasesSubset = {
  first?: number; indices?: Uint32Array; scalarBits?: number; scalarType?: ScalarType; m?: number;
};
export declare const compute_msm_prepared: (
  handle: BasesHandle,
  scalars: bigint[] | Uint32Array[] | Uint32Array | NativeScalars,
  subset?: BasesSubset
) => Promise<{ x: bigint; y: bigint }>;
// Per-point multiples s_i * P_i of a handle's bases (all of them, the range from `first`, or bases
// indices[i]): m x 32 wire words, or with asBases a new handle of those points.  Synchronous.
export type ScaleOptions = { first?: number; indices?: Uint32Array; scalarBits?: number; levels?: number; windowSize?: number };
export declare function scale_bases_prepared(
  handle: BasesHandle,
  scalars: bigint[] | Uint32Array[] | Uint32Array,
  options?: ScaleOptions & { asBases?: false }
): Uint32Array;
export declare function scale_bases_prepared(
  handle: BasesHandle,
  scalars: bigint[] | Uint32Array[] | Uint32Array,
  options: ScaleOptions & { asBases: true }
): BasesHandle;
// Pairwise combinations a_i * A_i +- b_i * B_i of two subsets of a handle's bases, or of two handles':
// m x 32 wire words, or with keep a new handle of those points.  a / b: absent (1), one bigint (broadcast)
// or m scalars.  Synchronous.
export type CombineOptions = {
  other?: BasesHandle; a?: bigint | bigint[] | Uint32Array[] | Uint32Array; b?: bigint | bigint[] | Uint32Array[] | Uint32Array;
  aFirst?: number; bFirst?: number; aIndices?: Uint32Array; bIndices?: Uint32Array; m?: number; sub?: boolean;
  scalarBits?: number; levels?: number; windowSize?: number;
};
export declare function combine_bases_prepared(handle: BasesHandle, options?: CombineOptions & { keep?: false }): Uint32Array;
export declare function combine_bases_prepared(handle: BasesHandle, options: CombineOptions & { keep: true }): BasesHandle;
// Fixed-base tables: the windowed table of k <= 8 of a handle's bases (all, the range from `first` of
// `count`, or bases indices[j]), then sum_j s_ij * B_j for m rows of k scalars (row after row): m x 32
// wire words, or with asBases a new handle of those points.  Synchronous.
export type FixedBaseTable = {
  id: number; bases: number; windowBits: number; scalarBits: number; windows: number; records: number; bytes: number;
};
export declare function prepare_fixed_base(
  handle: BasesHandle,
  options?: { first?: number; count?: number; indices?: Uint32Array; windowBits?: number; scalarBits?: number }
): FixedBaseTable;
// The same over up to 4096 bases; fixed_base_mul and release_fixed_base take the table.
export declare function prepare_vector_base(
  handle: BasesHandle,
  options?: { first?: number; count?: number; indices?: Uint32Array; windowBits?: number; scalarBits?: number }
): FixedBaseTable;
export type FixedMulOptions = { scalarBits?: number; levels?: number; windowSize?: number };
export declare function fixed_base_mul(
  table: FixedBaseTable,
  scalars: bigint[] | Uint32Array[] | Uint32Array,
  options?: FixedMulOptions & { asBases?: false }
): Uint32Array;
export declare function fixed_base_mul(
  table: FixedBaseTable,
  scalars: bigint[] | Uint32Array[] | Uint32Array,
  options: FixedMulOptions & { asBases: true }
): BasesHandle;
export declare function release_fixed_base(table: FixedBaseTable): number;
export declare function release_bases(handle: BasesHandle): number;

export declare function getBestWindowSize(n: number): number;
export declare function u32ArrayToBigInts(u32Array: Uint32Array): bigint[];
export declare const split_dynamic: (windowSize: number, scalars: Uint32Array) => Uint32Array;
export declare const point_add_affine: (a: Uint32Array, b: Uint32Array) => Uint32Array;
export declare const init: () => number;
export declare const deviceCount: () => number;
export declare const deviceOrdinals: () => number[];
export declare const nUint32PerScalar: 8;
export declare const nUint32PerPoint: 32;
export declare const loadTestCase: (
  pointsPath: string,
  scalarsPath: string
) => Promise<{ baseAffinePoints: BigIntPoint[]; scalars: bigint[] }>;
export declare const expectedPowersResult: Record<16 | 17 | 18 | 19 | 20, { x: bigint; y: bigint }>;
