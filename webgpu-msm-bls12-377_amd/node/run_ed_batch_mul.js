'use strict';
// Test driver: node run_ed_batch_mul.js <case.bin> <n> <k>
// The case file holds k x 64 bytes of Edwards-BLS12 wire bases, then the k x n scalars row-major (32 bytes each).
// Prints the records of ed_batch_mul_multi as hex, from the Buffer form and (checked equal) from the bigint[] form of the
// scalars and from the column-major layout of the same matrix, the k = 1 convenience on the first column against
// ed_batch_mul_multi with one base, the length of the empty batch, and the text of the refusal of a base off the curve.
// Used by tests/test_ed_batch_mul_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { ed_batch_mul, ed_batch_mul_multi } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const k = parseInt(process.argv[4], 10);
const bases = blob.slice(0, 64 * k), rows = blob.slice(64 * k, 64 * k + 32 * k * n);
const r = ed_batch_mul_multi(bases, rows);
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const scalars = Array.from({ length: k * n }, (_, i) => le(rows.slice(32 * i, 32 * (i + 1))));
if (!r.equals(ed_batch_mul_multi(bases, scalars))) throw new Error('bigint form disagrees with the Buffer form');
const columns = Buffer.alloc(32 * k * n);
for (let i = 0; i < n; i++) for (let j = 0; j < k; j++) rows.copy(columns, 32 * (j * n + i), 32 * (i * k + j), 32 * (i * k + j + 1));
if (!r.equals(ed_batch_mul_multi(bases, columns, { layout: 'columns' }))) throw new Error('column-major layout disagrees with row-major');
const single = ed_batch_mul(bases.slice(0, 64), columns.slice(0, 32 * n));
if (!single.equals(ed_batch_mul_multi(bases.slice(0, 64), columns.slice(0, 32 * n)))) throw new Error('ed_batch_mul is not the k = 1 call');
const empty = ed_batch_mul_multi(bases, Buffer.alloc(0));
const bad = Buffer.from(bases);
bad[32] ^= 1;  // y of the first base: off the curve
let refused = '';
try {
  ed_batch_mul_multi(bad, rows);
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({ points: r.toString('hex'), single: single.toString('hex'), empty: empty.length, refused }));
