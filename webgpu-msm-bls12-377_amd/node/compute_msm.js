'use strict';
// compute_msm for node (CommonJS twin of compute_msm.ts; runs as-is on node >= 12).
// Same name, arguments and result as the reference entry point
//   /root/reference/src/submission/submission.ts:85-90
// with the WebGPU stage drivers replaced by one call into the N-API shim over
// include/msm377.h.  Input forms (submission.ts:86-87): Buffer (the only form the harness
// passes to this function, src/ui/AllBenchmarks.tsx:149-158), BigIntPoint[] / bigint[],
// U32ArrayPoint[] / Uint32Array[] (most-significant-first words,
// src/reference/webgpu/utils.ts:49-61).
const path = require('path');
const addon = require(path.join(__dirname, 'build', 'msm377_napi.node'));

const leBufferToBigInt = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));

const bigIntToBufferLE = (v, bytes) => {
  const hex = BigInt(v).toString(16).padStart(bytes * 2, '0');
  return Buffer.from(hex, 'hex').reverse();
};

const u32WordsToBigInt = (words) => {
  let v = BigInt(0);
  for (const w of words) v = (v << BigInt(32)) | BigInt(w >>> 0);
  return v;
};

const toBigInt = (v) => (typeof v === 'bigint' ? v : u32WordsToBigInt(v));

const pointsToBuffer = (baseAffinePoints) => {
  if (Buffer.isBuffer(baseAffinePoints)) return baseAffinePoints;
  const parts = [];
  for (const pt of baseAffinePoints) {
    parts.push(bigIntToBufferLE(toBigInt(pt.x), 48));
    parts.push(bigIntToBufferLE(toBigInt(pt.y), 48));
  }
  return Buffer.concat(parts);
};

const scalarsToBuffer = (scalars) => {
  if (Buffer.isBuffer(scalars)) return scalars;
  return Buffer.concat(Array.from(scalars, (s) => bigIntToBufferLE(toBigInt(s), 32)));
};

// Third argument: log_result as in the reference, or {scalarBytes, scalarBits, log_result?} -- the caller declares that
// every scalar is below 2^scalarBits; a scalars Buffer then holds scalarBytes (4, 8, 16 or 32; default 32) little-endian
// bytes per scalar and the engine runs floor(scalarBits / 16) + 1 windows instead of 16 (msm377_g1_msm_short).  Without
// it the call is the reference's.  {pointForm, scalarForm} next to them (or alone) name the callers' native forms of the
// Buffers -- pointForm 'wire' | 'mont' | 'mont_flag' (104-byte records with an infinity flag), scalarForm 'wire' | 'mont'
// (msm377_ctx_set_input_format; full-width scalars only).  The result stays {x, y} in plain bigints.
const POINT_FORMS = { wire: 0, mont: 1, mont_flag: 2 };
const SCALAR_FORMS = { wire: 0, mont: 1 };
const compute_msm = async (baseAffinePoints, scalars, log_result = true, force_recompile = false) => {
  void force_recompile; // kernels are compiled ahead of time for gfx950; nothing to recompile
  if (log_result !== null && typeof log_result === 'object' && (log_result.pointForm !== undefined || log_result.scalarForm !== undefined)) {
    const { pointForm = 'wire', scalarForm = 'wire', scalarBits, log_result: log = false } = log_result;
    if (!(pointForm in POINT_FORMS) || !(scalarForm in SCALAR_FORMS)) throw new RangeError('pointForm: wire | mont | mont_flag; scalarForm: wire | mont');
    if (scalarBits !== undefined) throw new RangeError('native input forms take full-width scalars (no scalarBits)');
    if (!Buffer.isBuffer(baseAffinePoints) || !Buffer.isBuffer(scalars)) throw new TypeError('native input forms are Buffers');
    if (scalars.length === 0) return { x: BigInt(0), y: BigInt(1) };
    const o = addon.computeMsmNativeSync(baseAffinePoints, scalars, POINT_FORMS[pointForm], SCALAR_FORMS[scalarForm]);
    const rn = { x: leBufferToBigInt(o.slice(0, 48)), y: leBufferToBigInt(o.slice(48, 96)) };
    if (log) console.log(rn);
    return rn;
  }
  if (log_result !== null && typeof log_result === 'object') {
    const { scalarBytes = 32, scalarBits, log_result: log = false } = log_result;
    const sBuf = Buffer.isBuffer(scalars) ? scalars : Buffer.concat(Array.from(scalars, (s) => bigIntToBufferLE(toBigInt(s), scalarBytes)));
    if (sBuf.length === 0) return { x: BigInt(0), y: BigInt(1) };
    const o = addon.computeMsmShortSync(pointsToBuffer(baseAffinePoints), sBuf, scalarBytes, scalarBits);
    const rs = { x: leBufferToBigInt(o.slice(0, 48)), y: leBufferToBigInt(o.slice(48, 96)) };
    if (log) console.log(rs);
    return rs;
  }
  const scalarsBuf = scalarsToBuffer(scalars);
  const input_size = scalarsBuf.length / 32;
  if (input_size === 0) {
    return { x: BigInt(0), y: BigInt(1) };
  }
  const pointsBuf = pointsToBuffer(baseAffinePoints);
  const out = await addon.computeMsm(pointsBuf, scalarsBuf);
  const r = { x: leBufferToBigInt(out.slice(0, 48)), y: leBufferToBigInt(out.slice(48, 96)) };
  if (log_result) {
    console.log(r);
  }
  return r;
};

// The Edwards-BLS12 twin (BASELINE.json config 3; the reference's orphaned Edwards shaders,
// /root/reference/src/submission/miscellaneous/wgsl/add_points_any_a.template.wgsl:24-71): 64-byte points x || y,
// 32-byte little-endian each (README.md:299-301); returns {x, y}, the neutral element as (0, 1).
const compute_msm_edwards = (points, scalars) => {
  if (scalars.length === 0) return { x: BigInt(0), y: BigInt(1) };
  const out = addon.computeEdMsmSync(points, scalars);
  return { x: leBufferToBigInt(out.slice(0, 32)), y: leBufferToBigInt(out.slice(32, 64)) };
};

// Fixed-base batches (BASELINE.json config 5): convert and keep a base set in HBM once, then any number of MSMs of
// n <= its size against it (msm377_g1_set_bases / msm377_g1_msm_fixed_base).
const set_bases = (baseAffinePoints) => addon.setBasesSync(pointsToBuffer(baseAffinePoints));
const compute_msm_fixed_base = (scalars) => {
  const scalarsBuf = scalarsToBuffer(scalars);
  if (scalarsBuf.length === 0) return { x: BigInt(0), y: BigInt(1) };
  const out = addon.fixedBaseMsmSync(scalarsBuf);
  return { x: leBufferToBigInt(out.slice(0, 48)), y: leBufferToBigInt(out.slice(48, 96)) };
};

// Input validation (msm377_g1_check_points): are the points canonical (1), on the curve (2), in the prime-order subgroup (4)?
// compute_msm trusts its input; call this on freshly loaded points first.  Returns the report: counters as bigints, first_bad
// the lowest failing index or null, first_bad_reason the CHECK_* bit that point failed (0 if none).
const CHECK_CANONICAL = 1, CHECK_CURVE = 2, CHECK_SUBGROUP = 4, CHECK_ALL = 7;
const check_points = (points, flags = CHECK_ALL) => addon.checkPointsSync(pointsToBuffer(points), flags);

// Fixed-base batch multiplication (msm377_g1_batch_mul): out[i] = [s_i]B for ONE base B ({x, y}, or a 96-byte Buffer) and n
// scalars, every output its own point.  Returns {points, infinity}: n records -- 96-byte wire (outForm 'wire', default) or
// 104-byte 'mont_flag' -- and one byte per output, 1 for the identity.  Any curve point is a legal base and any 32-byte
// value a legal scalar.
const BATCH_MUL_FORMS = { wire: 0, mont_flag: 2 };
const batch_mul = (base, scalars, { outForm = 'wire' } = {}) => {
  if (!(outForm in BATCH_MUL_FORMS)) throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  const baseBuf = Buffer.isBuffer(base) ? base : pointsToBuffer([base]);
  return addon.batchMulSync(baseBuf, scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm]);
};

// Variable-base batch multiplication (msm377_g1_batch_mul_var): out[i] = [s_i]P_i, every output its own point.  `points`: {x, y}
// points or a Buffer of 96-byte wire records; `scalars`: one per point, or ONE scalar (a 32-byte Buffer, a one-element array)
// for all points.  Returns {points, infinity} as batch_mul does.  Any curve point is a legal input.
const batch_mul_var = (points, scalars, { outForm = 'wire' } = {}) => {
  if (!(outForm in BATCH_MUL_FORMS)) throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  return addon.batchMulVarSync(pointsToBuffer(points), scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm]);
};

// Pairwise linear combination (msm377_g1_batch_lincomb2): out[i] = [a_i]P_i + [b_i]Q_i, every output its own point.  `p`, `q`:
// as many {x, y} points, or Buffers of 96-byte wire records; `a`, `b`: each one scalar per pair, or ONE scalar (a 32-byte
// Buffer, a one-element array) for all pairs.  Returns {points, infinity} as batch_mul does.  Any curve point is a legal
// input, and any relation between p[i] and q[i].
const batch_lincomb2 = (p, q, a, b, { outForm = 'wire' } = {}) => {
  if (!(outForm in BATCH_MUL_FORMS)) throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  return addon.batchLincomb2Sync(pointsToBuffer(p), pointsToBuffer(q), scalarsToBuffer(a), scalarsToBuffer(b), BATCH_MUL_FORMS[outForm]);
};

// Multi-base batch multiplication (msm377_g1_batch_mul_multi): out[i] = sum_j [s_ij]B_j over k <= 16 fixed bases, every output
// its own point (Pedersen commitments [m_i]G + [r_i]H).  `bases`: k {x, y} points, or a Buffer of 96-byte wire records;
// `scalars`: the k x n matrix as one flat list or Buffer -- layout 'rows' (default: the k scalars of an output side by side)
// or 'columns' (the n scalars of a base side by side).  Returns {points, infinity} as batch_mul does.  Any curve point is a
// legal base, and any relation between the bases.
const BATCH_MUL_LAYOUTS = { rows: 0, columns: 1 };
const batch_mul_multi = (bases, scalars, { outForm = 'wire', layout = 'rows' } = {}) => {
  if (!(outForm in BATCH_MUL_FORMS)) throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  if (!(layout in BATCH_MUL_LAYOUTS)) throw new RangeError('layout: rows | columns');
  return addon.batchMulMultiSync(pointsToBuffer(bases), scalarsToBuffer(scalars), BATCH_MUL_FORMS[outForm], BATCH_MUL_LAYOUTS[layout]);
};

// Edwards-BLS12 batch multiplication (msm377_ed_batch_mul_multi): out[i] = sum_j [s_ij]B_j over k <= 16 fixed bases of the
// Edwards curve, every output its own point (addresses [sk_i]G, commitments [m_i]G + [r_i]H).  `bases`: a Buffer of 64-byte
// wire records x || y; `scalars`: the k x n matrix as one flat list or Buffer in layout 'rows' (default) or 'columns'.
// Returns a Buffer of n 64-byte records; the identity is (0, 1).  Every curve point is a legal base; a base off the curve
// is refused.  ed_batch_mul is the k = 1 call.
const ed_batch_mul_multi = (bases, scalars, { layout = 'rows' } = {}) => {
  if (!(layout in BATCH_MUL_LAYOUTS)) throw new RangeError('layout: rows | columns');
  return addon.edBatchMulMultiSync(bases, scalarsToBuffer(scalars), BATCH_MUL_LAYOUTS[layout]);
};
const ed_batch_mul = (base, scalars) => ed_batch_mul_multi(base, scalars);

// Edwards-BLS12 variable-base batch multiplication (msm377_ed_batch_mul_var): out[i] = [s_i]P_i, every output its own point
// (record scanning [view_key] nonce_i, the ElGamal / ECDH halves [r_i]PK_i).  `points`: a Buffer of 64-byte wire records
// x || y; `scalars`: one per point, or ONE scalar (a 32-byte Buffer, a one-element array) for all points.  Returns a Buffer
// of n 64-byte records; the identity is (0, 1).  Every curve point is a legal input; a point off the curve throws, and the
// text names its index.
const ed_batch_mul_var = (points, scalars) => addon.edBatchMulVarSync(points, scalarsToBuffer(scalars));

// Edwards-BLS12 pairwise linear combination (msm377_ed_batch_lincomb2): out[i] = [a_i]P_i + [b_i]Q_i, every output its own
// point (Schnorr verification [s_i]G + [c_i]PK_i, ElGamal decryption and re-randomisation, plain P_i + Q_i).  `p`, `q`:
// Buffers of 64-byte wire records x || y; `a`, `b`: scalars (bigint[], Uint32Array[] or a Buffer of 32 bytes each).  n is
// the largest element count; an argument of exactly ONE element with n > 1 stands for all pairs.  Returns a Buffer of n
// 64-byte records; the identity is (0, 1).  Every curve point is a legal input; a point off the curve throws, and the text
// names its array and index.
const ed_batch_lincomb2 = (p, q, a, b) => addon.edBatchLincomb2Sync(p, q, scalarsToBuffer(a), scalarsToBuffer(b));

// Edwards-BLS12 k-term linear combination (msm377_ed_batch_lincomb): out[i] = sum_j [s_ij]P_ij, 1 to 8 terms, every output
// its own point (a Schnorr check as one sum [s_i]G - [c_i]PK_i - R_i, both halves of a DLEQ proof, ElGamal re-encryption).
// `terms`: one {points, scalars} per term -- a Buffer of 64-byte wire records x || y, and scalars (bigint[], Uint32Array[]
// or a Buffer of 32 bytes each).  n is the largest element count; an argument of exactly ONE element with n > 1 stands for
// all outputs.  Returns a Buffer of n 64-byte records; the identity is (0, 1).  Every curve point is a legal input; a point
// off the curve throws, and the text names its index and its term.
const ed_batch_lincomb = (terms) =>
  addon.edBatchLincombSync(
    terms.map((t) => t.points),
    terms.map((t) => scalarsToBuffer(t.scalars)),
  );

// Row commitments (msm377_g1_set_generators / msm377_g1_commit_rows): out[i] = sum_j [s_ij]G_j over a RESIDENT set of up to
// 4 096 generators (Pedersen vector commitments).  set_generators(gens, {windowBits}) builds and keeps the window tables --
// `gens`: {x, y} points or a Buffer of 96-byte wire records; windowBits 0 (= 8), 8, or 16 for up to 64 generators; an empty
// list drops the set.  commit_rows(scalars, k, {outForm, layout}) runs over the first k generators: `scalars` the k x n matrix
// as one flat list or Buffer, layout 'rows' (default) or 'columns'.  Returns {points, infinity} as batch_mul does.
const set_generators = (gens, { windowBits = 0 } = {}) => addon.setGeneratorsSync(pointsToBuffer(gens), windowBits);
const commit_rows = (scalars, k, { outForm = 'wire', layout = 'rows' } = {}) => {
  if (!(outForm in BATCH_MUL_FORMS)) throw new RangeError("outForm: wire | mont_flag (plain mont cannot say 'identity')");
  if (!(layout in BATCH_MUL_LAYOUTS)) throw new RangeError('layout: rows | columns');
  return addon.commitRowsSync(scalarsToBuffer(scalars), k, BATCH_MUL_FORMS[outForm], BATCH_MUL_LAYOUTS[layout]);
};

// Edwards-BLS12 row commitments (msm377_ed_set_generators / msm377_ed_commit_rows): out[i] = sum_j [s_ij]G_j over a RESIDENT
// set of up to 4 096 Edwards-BLS12 generators (Pedersen and BHP-style hashes, vector commitments), independent of the G1 set.
// ed_set_generators(gens, {windowBits}) builds and keeps the window tables -- `gens`: a Buffer of 64-byte wire records
// x || y; windowBits 0 (= 8), 8, or 16 for up to 64 generators; an empty Buffer drops the set; a generator off the curve
// throws, and the text names its index.  ed_commit_rows(scalars, k, {layout}) runs over the first k generators: `scalars`
// the k x n matrix as one flat list or Buffer, layout 'rows' (default) or 'columns'.  Returns a Buffer of n 64-byte records;
// the identity is (0, 1).
const ed_set_generators = (gens, { windowBits = 0 } = {}) => addon.edSetGeneratorsSync(gens, windowBits);
const ed_commit_rows = (scalars, k, { layout = 'rows' } = {}) => {
  if (!(layout in BATCH_MUL_LAYOUTS)) throw new RangeError('layout: rows | columns');
  return addon.edCommitRowsSync(scalarsToBuffer(scalars), k, BATCH_MUL_LAYOUTS[layout]);
};

module.exports = { batch_lincomb2, batch_mul, batch_mul_multi, ed_batch_mul, ed_batch_mul_multi, ed_batch_mul_var, ed_batch_lincomb2, ed_batch_lincomb, ed_commit_rows, ed_set_generators, commit_rows, set_generators, batch_mul_var, compute_msm, compute_msm_edwards, set_bases, compute_msm_fixed_base, check_points, CHECK_CANONICAL, CHECK_CURVE, CHECK_SUBGROUP, CHECK_ALL, pointsToBuffer, scalarsToBuffer, version: addon.version };
