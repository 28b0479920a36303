'use strict';
// Test driver: node run_commit_rows.js <case.bin> <n> <k> <outForm>
// The case file holds k x 96 bytes of wire generators, then the k x n scalars row-major (32 bytes each).
// Sets the generators, prints the records and the identity bytes of commit_rows as hex, from the Buffer form and (checked
// equal) from the {x, y} / bigint[] form and from the column-major layout of the same matrix, the empty batch, the text of the
// refusal of outForm 'mont' and of a call after the set is dropped.  Used by tests/test_commit_rows_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { set_generators, commit_rows } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const k = parseInt(process.argv[4], 10);
const outForm = process.argv[5];
const gens = blob.slice(0, 96 * k), rows = blob.slice(96 * k, 96 * k + 32 * k * n);
set_generators(gens);
const r = commit_rows(rows, k, { outForm });
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const points = Array.from({ length: k }, (_, j) => ({ x: le(gens.slice(96 * j, 96 * j + 48)), y: le(gens.slice(96 * j + 48, 96 * j + 96)) }));
const scalars = Array.from({ length: k * n }, (_, i) => le(rows.slice(32 * i, 32 * (i + 1))));
set_generators(points, { windowBits: 8 });
const r2 = commit_rows(scalars, k, { outForm });
if (!r.points.equals(r2.points) || !r.infinity.equals(r2.infinity)) throw new Error('bigint form disagrees with the Buffer form');
const columns = Buffer.alloc(32 * k * n);
for (let i = 0; i < n; i++) for (let j = 0; j < k; j++) rows.copy(columns, 32 * (j * n + i), 32 * (i * k + j), 32 * (i * k + j + 1));
const r3 = commit_rows(columns, k, { outForm, layout: 'columns' });
if (!r.points.equals(r3.points) || !r.infinity.equals(r3.infinity)) throw new Error('column-major layout disagrees with row-major');
const empty = commit_rows(Buffer.alloc(0), k, { outForm });
let refused = '';
try {
  commit_rows(rows, k, { outForm: 'mont' });
} catch (e) {
  refused = String(e);
}
set_generators(Buffer.alloc(0));
let dropped = '';
try {
  commit_rows(rows, k, { outForm });
} catch (e) {
  dropped = String(e);
}
console.log(JSON.stringify({ points: r.points.toString('hex'), infinity: r.infinity.toString('hex'), empty: empty.points.length + empty.infinity.length, refused, dropped }));
