'use strict';
// Test driver: node run_ed_batch_mul_var.js <case.bin> <n>
// The case file holds n x 64 bytes of Edwards-BLS12 wire points, then the n scalars (32 bytes each).
// Prints the records of ed_batch_mul_var as hex, from the Buffer form and (checked equal) from the bigint[] form of the
// scalars, the records under the FIRST scalar for all points (a 32-byte Buffer, checked equal to a one-element array), the
// length of the empty batch, and the text of the refusal of a point off the curve.
// Used by tests/test_ed_batch_mul_var_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { ed_batch_mul_var } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const bad = parseInt(process.argv[4], 10);
const points = blob.slice(0, 64 * n), scalars = blob.slice(64 * n, 96 * n);
const r = ed_batch_mul_var(points, scalars);
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const ks = Array.from({ length: n }, (_, i) => le(scalars.slice(32 * i, 32 * (i + 1))));
if (!r.equals(ed_batch_mul_var(points, ks))) throw new Error('bigint form disagrees with the Buffer form');
const one = ed_batch_mul_var(points, scalars.slice(0, 32));
if (!one.equals(ed_batch_mul_var(points, [ks[0]]))) throw new Error('one-element array disagrees with the 32-byte Buffer');
const empty = ed_batch_mul_var(Buffer.alloc(0), Buffer.alloc(0));
const off = Buffer.from(points);
off[64 * bad + 32] ^= 1;  // y of that point: off the curve
let refused = '';
try {
  ed_batch_mul_var(off, scalars);
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({ points: r.toString('hex'), one: one.toString('hex'), empty: empty.length, refused }));
