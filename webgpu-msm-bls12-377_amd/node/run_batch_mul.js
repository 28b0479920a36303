'use strict';
// Test driver: node run_batch_mul.js <case.bin> <n> <outForm>
// The case file holds the base's 96 bytes, then n x 32 bytes of scalars.  Prints the records and the identity bytes of
// batch_mul as hex, from the Buffer form and (checked equal) from the {x, y} / bigint[] form, the empty batch, and the
// text of the refusal of outForm 'mont'.  Used by tests/test_batch_mul_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { batch_mul } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const outForm = process.argv[4];
const base = blob.slice(0, 96);
const scalars = blob.slice(96, 96 + 32 * n);
const r = batch_mul(base, scalars, { outForm });
const le = (b) => BigInt('0x' + Buffer.from(b).reverse().toString('hex'));
const ks = [];
for (let i = 0; i < n; i++) ks.push(le(scalars.slice(32 * i, 32 * (i + 1))));
const r2 = batch_mul({ x: le(base.slice(0, 48)), y: le(base.slice(48, 96)) }, ks, { outForm });
if (!r.points.equals(r2.points) || !r.infinity.equals(r2.infinity)) throw new Error('bigint form disagrees with the Buffer form');
const empty = batch_mul(base, Buffer.alloc(0), { outForm });
let refused = '';
try {
  batch_mul(base, scalars, { outForm: 'mont' });
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({ points: r.points.toString('hex'), infinity: r.infinity.toString('hex'), empty: empty.points.length + empty.infinity.length, refused }));
