'use strict';
// Test driver: node run_batch_mul_var.js <case.bin> <n> <outForm>
// The case file holds n x 96 bytes of wire points, then n x 32 bytes of scalars.  Prints the records and the identity bytes
// of batch_mul_var as hex, from the Buffer form and (checked equal) from the {x, y} / bigint[] form, the same for the FIRST
// scalar alone applied to all points, the empty batch, and the text of the refusal of outForm 'mont'.  Used by
// tests/test_batch_mul_var_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { batch_mul_var } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const outForm = process.argv[4];
const points = blob.slice(0, 96 * n);
const scalars = blob.slice(96 * n, 128 * n);
const r = batch_mul_var(points, scalars, { outForm });
const le = (b) => BigInt('0x' + Buffer.from(b).reverse().toString('hex'));
const ps = [], ks = [];
for (let i = 0; i < n; i++) {
  ps.push({ x: le(points.slice(96 * i, 96 * i + 48)), y: le(points.slice(96 * i + 48, 96 * i + 96)) });
  ks.push(le(scalars.slice(32 * i, 32 * (i + 1))));
}
const r2 = batch_mul_var(ps, ks, { outForm });
if (!r.points.equals(r2.points) || !r.infinity.equals(r2.infinity)) throw new Error('bigint form disagrees with the Buffer form');
const one = batch_mul_var(points, scalars.slice(0, 32), { outForm });
const empty = batch_mul_var(Buffer.alloc(0), Buffer.alloc(0), { outForm });
let refused = '';
try {
  batch_mul_var(points, scalars, { outForm: 'mont' });
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({
  points: r.points.toString('hex'), infinity: r.infinity.toString('hex'), onePoints: one.points.toString('hex'), oneInfinity: one.infinity.toString('hex'),
  empty: empty.points.length + empty.infinity.length, refused,
}));
