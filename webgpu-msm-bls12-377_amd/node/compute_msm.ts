/**
 * compute_msm for src/submission: drop-in replacement of the WebGPU implementation
 * (/root/reference/src/submission/submission.ts:85-327).  Copy this file over
 * src/submission/submission.ts (or re-export compute_msm from it): the harness callers
 * (src/ui/AllBenchmarks.tsx:149-158, src/ui/Benchmark.tsx:32,
 * src/submission/miscellaneous/full_benchmarks.ts:62,99) need no change.
 *
 * The five WebGPU stage drivers and the BigInt CPU tail are replaced by one call into the
 * N-API shim (msm377_napi.node) over the C ABI in include/msm377.h; see INTEGRATION.md.
 */
import { BigIntPoint, U32ArrayPoint } from "../reference/types";

/** msm377_check_report: a point is counted once, in the first class it fails. */
export interface CheckReport {
  checked: bigint;
  noncanonical: bigint;
  off_curve: bigint;
  outside_subgroup: bigint;
  first_bad: bigint | null; // lowest failing index
  first_bad_reason: number; // the CHECK_* bit that point failed; 0 if none
}
export const CHECK_CANONICAL = 1, CHECK_CURVE = 2, CHECK_SUBGROUP = 4, CHECK_ALL = 7;

// eslint-disable-next-line @typescript-eslint/no-var-requires
const addon: {
  computeMsm(points: Buffer, scalars: Buffer): Promise<Buffer>;
  computeMsmSync(points: Buffer, scalars: Buffer): Buffer;
  computeEdMsmSync(points: Buffer, scalars: Buffer): Buffer;
  setBasesSync(points: Buffer): void;
  fixedBaseMsmSync(scalars: Buffer): Buffer;
  checkPointsSync(points: Buffer, flags?: number): CheckReport;
  version(): string;
} = require("./msm377/build/msm377_napi.node");

const leBufferToBigInt = (buf: Buffer): bigint =>
  BigInt("0x" + Buffer.from(buf).reverse().toString("hex"));

const bigIntToBufferLE = (v: bigint, bytes: number): Buffer =>
  Buffer.from(v.toString(16).padStart(bytes * 2, "0"), "hex").reverse();

// Most-significant-first u32 words: src/reference/webgpu/utils.ts:49-61
const u32WordsToBigInt = (words: Uint32Array): bigint => {
  let v = BigInt(0);
  for (const w of words) v = (v << BigInt(32)) | BigInt(w >>> 0);
  return v;
};

const toBigInt = (v: bigint | Uint32Array): bigint =>
  typeof v === "bigint" ? v : u32WordsToBigInt(v);

export const pointsToBuffer = (
  baseAffinePoints: BigIntPoint[] | U32ArrayPoint[] | Buffer,
): Buffer => {
  if (Buffer.isBuffer(baseAffinePoints)) return baseAffinePoints;
  const parts: Buffer[] = [];
  for (const pt of baseAffinePoints as (BigIntPoint | U32ArrayPoint)[]) {
    parts.push(bigIntToBufferLE(toBigInt(pt.x), 48));
    parts.push(bigIntToBufferLE(toBigInt(pt.y), 48));
  }
  return Buffer.concat(parts);
};

export const scalarsToBuffer = (
  scalars: bigint[] | Uint32Array[] | Buffer,
): Buffer => {
  if (Buffer.isBuffer(scalars)) return scalars;
  return Buffer.concat(
    (scalars as (bigint | Uint32Array)[]).map((s) => bigIntToBufferLE(toBigInt(s), 32)),
  );
};

// Declared scalar width (msm377_g1_msm_short): every scalar is below 2^scalarBits; a scalars Buffer holds scalarBytes
// (4, 8, 16 or 32; default 32) little-endian bytes per scalar.
export interface ShortScalars {
  scalarBytes?: 4 | 8 | 16 | 32;
  scalarBits: number;
  log_result?: boolean;
}

// The callers' native forms of the two Buffers (msm377_ctx_set_input_format): Montgomery coordinates, 104-byte records
// with an infinity flag, Montgomery scalars.  Full-width scalars only; the result stays {x, y} in plain bigints.
export interface NativeForms {
  pointForm?: 'wire' | 'mont' | 'mont_flag';
  scalarForm?: 'wire' | 'mont';
  log_result?: boolean;
}
const POINT_FORMS = { wire: 0, mont: 1, mont_flag: 2 };
const SCALAR_FORMS = { wire: 0, mont: 1 };

// Third argument: log_result as in the reference, a ShortScalars object or a NativeForms object; without one the call
// is the reference's.
export const compute_msm = async (
  baseAffinePoints: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  scalars: bigint[] | Uint32Array[] | Buffer,
  log_result: boolean | ShortScalars | NativeForms = true,
  force_recompile = false,
): Promise<{ x: bigint; y: bigint }> => {
  void force_recompile; // kernels are compiled ahead of time for gfx950
  if (log_result !== null && typeof log_result === 'object' && ('pointForm' in log_result || 'scalarForm' in log_result)) {
    const { pointForm = 'wire', scalarForm = 'wire', log_result: log = false } = log_result as NativeForms;
    if (!(pointForm in POINT_FORMS) || !(scalarForm in SCALAR_FORMS)) {
      throw new RangeError('pointForm: wire | mont | mont_flag; scalarForm: wire | mont');
    }
    if ('scalarBits' in log_result) throw new RangeError('native input forms take full-width scalars (no scalarBits)');
    if (!Buffer.isBuffer(baseAffinePoints) || !Buffer.isBuffer(scalars)) throw new TypeError('native input forms are Buffers');
    if (scalars.length === 0) {
      return { x: BigInt(0), y: BigInt(1) };
    }
    const o: Buffer = addon.computeMsmNativeSync(baseAffinePoints, scalars, POINT_FORMS[pointForm], SCALAR_FORMS[scalarForm]);
    const rn = { x: leBufferToBigInt(o.subarray(0, 48) as Buffer), y: leBufferToBigInt(o.subarray(48, 96) as Buffer) };
    if (log) {
      console.log(rn);
    }
    return rn;
  }
  if (log_result !== null && typeof log_result === 'object') {
    const { scalarBytes = 32, scalarBits, log_result: log = false } = log_result as ShortScalars;
    const sBuf = Buffer.isBuffer(scalars)
      ? scalars
      : Buffer.concat((scalars as (bigint | Uint32Array)[]).map((s) => bigIntToBufferLE(toBigInt(s), scalarBytes)));
    if (sBuf.length === 0) {
      return { x: BigInt(0), y: BigInt(1) };
    }
    const o: Buffer = addon.computeMsmShortSync(pointsToBuffer(baseAffinePoints), sBuf, scalarBytes, scalarBits);
    const rs = { x: leBufferToBigInt(o.subarray(0, 48) as Buffer), y: leBufferToBigInt(o.subarray(48, 96) as Buffer) };
    if (log) {
      console.log(rs);
    }
    return rs;
  }
  const scalarsBuf = scalarsToBuffer(scalars);
  const input_size = scalarsBuf.length / 32;

  if (input_size === 0) {
    return { x: BigInt(0), y: BigInt(1) };
  }

  const pointsBuf = pointsToBuffer(baseAffinePoints);
  const out = await addon.computeMsm(pointsBuf, scalarsBuf);
  const r = {
    x: leBufferToBigInt(out.subarray(0, 48) as Buffer),
    y: leBufferToBigInt(out.subarray(48, 96) as Buffer),
  };
  if (log_result) {
    console.log(r);
  }
  return r;
};

// The Edwards-BLS12 twin (BASELINE.json config 3; the reference's orphaned Edwards shaders,
// src/submission/miscellaneous/wgsl/add_points_any_a.template.wgsl:24-71): 64-byte points x || y, 32-byte
// little-endian each (README.md:299-301); the neutral element is (0, 1).
export const compute_msm_edwards = (points: Buffer, scalars: Buffer): { x: bigint; y: bigint } => {
  if (scalars.length === 0) {
    return { x: BigInt(0), y: BigInt(1) };
  }
  const out: Buffer = addon.computeEdMsmSync(points, scalars);
  return { x: leBufferToBigInt(out.subarray(0, 32) as Buffer), y: leBufferToBigInt(out.subarray(32, 64) as Buffer) };
};

// Fixed-base batches (BASELINE.json config 5): convert and keep a base set in HBM once, then any number of MSMs of
// n <= its size against it (msm377_g1_set_bases / msm377_g1_msm_fixed_base).
export const set_bases = (baseAffinePoints: BigIntPoint[] | U32ArrayPoint[] | Buffer): void => {
  addon.setBasesSync(pointsToBuffer(baseAffinePoints));
};

export const compute_msm_fixed_base = (scalars: bigint[] | Uint32Array[] | Buffer): { x: bigint; y: bigint } => {
  const scalarsBuf = scalarsToBuffer(scalars);
  if (scalarsBuf.length === 0) {
    return { x: BigInt(0), y: BigInt(1) };
  }
  const out: Buffer = addon.fixedBaseMsmSync(scalarsBuf);
  return { x: leBufferToBigInt(out.subarray(0, 48) as Buffer), y: leBufferToBigInt(out.subarray(48, 96) as Buffer) };
};

// Input validation (msm377_g1_check_points): compute_msm trusts its input; call this on freshly loaded points first.
export const check_points = (points: BigIntPoint[] | U32ArrayPoint[] | Buffer, flags: number = CHECK_ALL): CheckReport =>
  addon.checkPointsSync(pointsToBuffer(points), flags);

// Fixed-base batch multiplication (msm377_g1_batch_mul): out[i] = [s_i]B for ONE base B and n scalars, every output its own
// point.  `points`: n records -- 96-byte wire (outForm 'wire', default) or 104-byte 'mont_flag'; `infinity`: one byte per
// output, 1 for the identity.  Any curve point is a legal base and any 32-byte value a legal scalar.
const BATCH_MUL_FORMS = { wire: 0, mont_flag: 2 } as const;
export const batch_mul = (
  base: BigIntPoint | U32ArrayPoint | Buffer,
  scalars: bigint[] | Uint32Array[] | Buffer,
  { outForm = 'wire' }: { outForm?: keyof typeof BATCH_MUL_FORMS } = {},
): { points: Buffer; infinity: Buffer } => {
  if (!(outForm in BATCH_MUL_FORMS)) {
    throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  }
  const baseBuf = Buffer.isBuffer(base) ? base : pointsToBuffer([base] as BigIntPoint[] | U32ArrayPoint[]);
  return addon.batchMulSync(baseBuf, scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm]);
};

// Variable-base batch multiplication (msm377_g1_batch_mul_var): out[i] = [s_i]P_i, every output its own point.  `scalars`: one
// per point, or ONE scalar (a 32-byte Buffer, a one-element array) for all points.  Returns what batch_mul returns.
export const batch_mul_var = (
  points: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  scalars: bigint[] | Uint32Array[] | Buffer,
  { outForm = 'wire' }: { outForm?: keyof typeof BATCH_MUL_FORMS } = {},
): { points: Buffer; infinity: Buffer } => {
  if (!(outForm in BATCH_MUL_FORMS)) {
    throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  }
  return addon.batchMulVarSync(pointsToBuffer(points), scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm]);
};

// Pairwise linear combination (msm377_g1_batch_lincomb2): out[i] = [a_i]P_i + [b_i]Q_i, every output its own point.  `a`, `b`:
// each one scalar per pair, or ONE scalar (a 32-byte Buffer, a one-element array) for all pairs.  Returns what batch_mul
// returns.
export const batch_lincomb2 = (
  p: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  q: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  a: bigint[] | Uint32Array[] | Buffer,
  b: bigint[] | Uint32Array[] | Buffer,
  { outForm = 'wire' }: { outForm?: keyof typeof BATCH_MUL_FORMS } = {},
): { points: Buffer; infinity: Buffer } => {
  if (!(outForm in BATCH_MUL_FORMS)) {
    throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  }
  return addon.batchLincomb2Sync(pointsToBuffer(p), pointsToBuffer(q), scalarsToBuffer(a), scalarsToBuffer(b), BATCH_MUL_FORMS[outForm]);
};

// Multi-base batch multiplication (msm377_g1_batch_mul_multi): out[i] = sum_j [s_ij]B_j over k <= 16 fixed bases, every output
// its own point.  `scalars`: the k x n matrix as one flat list or Buffer, layout 'rows' (default: the k scalars of an output
// side by side) or 'columns' (the n scalars of a base side by side).  Returns what batch_mul returns.
const BATCH_MUL_LAYOUTS = { rows: 0, columns: 1 } as const;
export const batch_mul_multi = (
  bases: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  scalars: bigint[] | Uint32Array[] | Buffer,
  { outForm = 'wire', layout = 'rows' }: { outForm?: keyof typeof BATCH_MUL_FORMS; layout?: keyof typeof BATCH_MUL_LAYOUTS } = {},
): { points: Buffer; infinity: Buffer } => {
  if (!(outForm in BATCH_MUL_FORMS)) {
    throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  }
  if (!(layout in BATCH_MUL_LAYOUTS)) {
    throw new RangeError('layout: rows | columns');
  }
  return addon.batchMulMultiSync(pointsToBuffer(bases), scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm], BATCH_MUL_LAYOUTS[layout]);
};

// Edwards-BLS12 batch multiplication (msm377_ed_batch_mul_multi): out[i] = sum_j [s_ij]B_j over k <= 16 fixed bases of the
// Edwards curve, every output its own 64-byte wire point x || y (the identity is (0, 1)).  `bases`: a Buffer of 64-byte wire
// records; `scalars`: the k x n matrix as one flat list or Buffer in layout 'rows' (default) or 'columns'.  ed_batch_mul is
// the k = 1 call.
export const ed_batch_mul_multi = (
  bases: Buffer,
  scalars: bigint[] | Uint32Array[] | Buffer,
  { layout = 'rows' }: { layout?: keyof typeof BATCH_MUL_LAYOUTS } = {},
): Buffer => {
  if (!(layout in BATCH_MUL_LAYOUTS)) {
    throw new RangeError('layout: rows | columns');
  }
  return addon.edBatchMulMultiSync(bases, scalarsToBuffer(scalars), BATCH_MUL_LAYOUTS[layout]);
};

export const ed_batch_mul = (base: Buffer, scalars: bigint[] | Uint32Array[] | Buffer): Buffer => ed_batch_mul_multi(base, scalars);

// Edwards-BLS12 variable-base batch multiplication (msm377_ed_batch_mul_var): out[i] = [s_i]P_i, every output its own 64-byte
// wire point.  `points`: a Buffer of 64-byte wire records; `scalars`: one per point, or ONE scalar (a 32-byte Buffer, a
// one-element array) for all points.  Every curve point is a legal input; a point off the curve throws, and the text names
// its index.
export const ed_batch_mul_var = (points: Buffer, scalars: bigint[] | Uint32Array[] | Buffer): Buffer =>
  addon.edBatchMulVarSync(points, scalarsToBuffer(scalars));

// Edwards-BLS12 pairwise linear combination (msm377_ed_batch_lincomb2): out[i] = [a_i]P_i + [b_i]Q_i, every output its own
// 64-byte wire point.  `p`, `q`: Buffers of 64-byte wire records; `a`, `b`: scalars.  n is the largest element count; an
// argument of exactly ONE element with n > 1 stands for all pairs.  Every curve point is a legal input; a point off the
// curve throws, and the text names its array and index.
export const ed_batch_lincomb2 = (p: Buffer, q: Buffer, a: bigint[] | Uint32Array[] | Buffer, b: bigint[] | Uint32Array[] | Buffer): Buffer =>
  addon.edBatchLincomb2Sync(p, q, scalarsToBuffer(a), scalarsToBuffer(b));

// Edwards-BLS12 k-term linear combination (msm377_ed_batch_lincomb): out[i] = sum_j [s_ij]P_ij, 1 to 8 terms, every output
// its own 64-byte wire point.  `terms`: one {points, scalars} per term -- a Buffer of 64-byte wire records and the scalars.
// n is the largest element count; an argument of exactly ONE element with n > 1 stands for all outputs.  Every curve point
// is a legal input; a point off the curve throws, and the text names its index and its term.
export const ed_batch_lincomb = (terms: { points: Buffer; scalars: bigint[] | Uint32Array[] | Buffer }[]): Buffer =>
  addon.edBatchLincombSync(
    terms.map((t) => t.points),
    terms.map((t) => scalarsToBuffer(t.scalars)),
  );

// Row commitments (msm377_g1_set_generators / msm377_g1_commit_rows): out[i] = sum_j [s_ij]G_j over a RESIDENT set of up to
// 4 096 generators.  set_generators builds and keeps the window tables (windowBits 0 = 8, 8, or 16 for up to 64
// generators; an empty list drops the set); commit_rows runs over the first k generators, `scalars` the k x n matrix as one
// flat list or Buffer in layout 'rows' (default) or 'columns'.  Returns what batch_mul returns.
export const set_generators = (gens: BigIntPoint[] | U32ArrayPoint[] | Buffer, { windowBits = 0 }: { windowBits?: number } = {}): void => {
  addon.setGeneratorsSync(pointsToBuffer(gens), windowBits);
};

export const commit_rows = (
  scalars: bigint[] | Uint32Array[] | Buffer,
  k: number,
  { outForm = 'wire', layout = 'rows' }: { outForm?: keyof typeof BATCH_MUL_FORMS; layout?: keyof typeof BATCH_MUL_LAYOUTS } = {},
): { points: Buffer; infinity: Buffer } => {
  if (!(outForm in BATCH_MUL_FORMS)) {
    throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  }
  if (!(layout in BATCH_MUL_LAYOUTS)) {
    throw new RangeError('layout: rows | columns');
  }
  return addon.commitRowsSync(scalarsToBuffer(scalars), k, BATCH_MUL_FORMS[outForm], BATCH_MUL_LAYOUTS[layout]);
};

// Edwards-BLS12 row commitments (msm377_ed_set_generators / msm377_ed_commit_rows): out[i] = sum_j [s_ij]G_j over a RESIDENT
// set of up to 4 096 Edwards-BLS12 generators, independent of the G1 set.  ed_set_generators builds and keeps the window
// tables (`gens`: a Buffer of 64-byte wire records; windowBits 0 = 8, 8, or 16 for up to 64 generators; an empty Buffer
// drops the set; a generator off the curve throws, and the text names its index); ed_commit_rows runs over the first k
// generators, `scalars` the k x n matrix as one flat list or Buffer in layout 'rows' (default) or 'columns', and returns n
// 64-byte wire records (the identity is (0, 1)).
export const ed_set_generators = (gens: Buffer, { windowBits = 0 }: { windowBits?: number } = {}): void => {
  addon.edSetGeneratorsSync(gens, windowBits);
};

export const ed_commit_rows = (
  scalars: bigint[] | Uint32Array[] | Buffer,
  k: number,
  { layout = 'rows' }: { layout?: keyof typeof BATCH_MUL_LAYOUTS } = {},
): Buffer => {
  if (!(layout in BATCH_MUL_LAYOUTS)) {
    throw new RangeError('layout: rows | columns');
  }
  return addon.edCommitRowsSync(scalarsToBuffer(scalars), k, BATCH_MUL_LAYOUTS[layout]);
};
