'use strict';
// Test driver: node run_ed_commit_rows.js <case.bin> <n> <k> <layout>
// The case file holds k x 64 bytes of Edwards-BLS12 wire generators, then the k x n scalars row-major (32 bytes each).
// Sets the generators, prints the records of ed_commit_rows in <layout> ('rows' | 'columns') as hex, from the Buffer form and
// (checked equal) from the bigint[] form of the scalars, and checks the other layout of the same matrix equal; then the
// length of the empty batch, the text of the refusal of a generator off the curve (which leaves no set: the call after it
// is refused too) and of a call after the set is dropped.  Used by tests/test_ed_commit_rows_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { ed_set_generators, ed_commit_rows } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const k = parseInt(process.argv[4], 10);
const layout = process.argv[5];
const gens = blob.slice(0, 64 * k), rows = blob.slice(64 * k, 64 * k + 32 * k * n);
const columns = Buffer.alloc(32 * k * n);
for (let i = 0; i < n; i++) for (let j = 0; j < k; j++) rows.copy(columns, 32 * (j * n + i), 32 * (i * k + j), 32 * (i * k + j + 1));
const matrix = { rows, columns };
const other = layout === 'rows' ? 'columns' : 'rows';
ed_set_generators(gens);
const r = ed_commit_rows(matrix[layout], k, { layout });
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const scalars = Array.from({ length: k * n }, (_, i) => le(matrix[layout].slice(32 * i, 32 * (i + 1))));
ed_set_generators(gens, { windowBits: 8 });
if (!r.equals(ed_commit_rows(scalars, k, { layout }))) throw new Error('bigint form disagrees with the Buffer form');
if (!r.equals(ed_commit_rows(matrix[other], k, { layout: other }))) throw new Error('the two layouts of one matrix disagree');
const empty = ed_commit_rows(Buffer.alloc(0), k, { layout });
const bad = Buffer.from(gens);
bad[64 * 2 + 32] ^= 1;  // y of generator 2: off the curve
let refused = '', after = '', dropped = '';
try {
  ed_set_generators(bad);
} catch (e) {
  refused = String(e);
}
try {
  ed_commit_rows(rows, k);
} catch (e) {
  after = String(e);
}
ed_set_generators(gens);
ed_set_generators(Buffer.alloc(0));
try {
  ed_commit_rows(rows, k);
} catch (e) {
  dropped = String(e);
}
console.log(JSON.stringify({ points: r.toString('hex'), empty: empty.length, refused, after, dropped }));
