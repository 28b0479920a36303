'use strict';
// Test driver: node run_batch_lincomb2.js <case.bin> <n> <outForm>
// The case file holds n x 96 bytes of wire points p, n x 96 bytes of q, then n x 32 bytes of scalars a and n x 32 bytes of b.
// Prints the records and the identity bytes of batch_lincomb2 as hex, from the Buffer form and (checked equal) from the
// {x, y} / bigint[] form, the same for the FIRST scalar of a alone applied to all pairs (stride 0 beside stride 32), the empty
// batch, and the text of the refusal of outForm 'mont'.  Used by tests/test_batch_lincomb2_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { batch_lincomb2 } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const outForm = process.argv[4];
const p = blob.slice(0, 96 * n), q = blob.slice(96 * n, 192 * n);
const a = blob.slice(192 * n, 224 * n), b = blob.slice(224 * n, 256 * n);
const r = batch_lincomb2(p, q, a, b, { outForm });
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const points = (buf) => Array.from({ length: n }, (_, i) => ({ x: le(buf.slice(96 * i, 96 * i + 48)), y: le(buf.slice(96 * i + 48, 96 * i + 96)) }));
const scalars = (buf) => Array.from({ length: n }, (_, i) => le(buf.slice(32 * i, 32 * (i + 1))));
const r2 = batch_lincomb2(points(p), points(q), scalars(a), scalars(b), { outForm });
if (!r.points.equals(r2.points) || !r.infinity.equals(r2.infinity)) throw new Error('bigint form disagrees with the Buffer form');
const one = batch_lincomb2(p, q, a.slice(0, 32), b, { outForm });
const empty = batch_lincomb2(Buffer.alloc(0), Buffer.alloc(0), Buffer.alloc(0), Buffer.alloc(0), { outForm });
let refused = '';
try {
  batch_lincomb2(p, q, a, b, { outForm: 'mont' });
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({
  points: r.points.toString('hex'), infinity: r.infinity.toString('hex'), onePoints: one.points.toString('hex'), oneInfinity: one.infinity.toString('hex'),
  empty: empty.points.length + empty.infinity.length, refused,
}));
