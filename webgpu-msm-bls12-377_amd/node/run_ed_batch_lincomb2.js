'use strict';
// Test driver: node run_ed_batch_lincomb2.js <case.bin> <n> <bad>
// The case file holds n x 64 bytes of Edwards-BLS12 wire points p, n x 64 of q, then the n scalars a and the n scalars b
// (32 bytes each).
// Prints the records of ed_batch_lincomb2 as hex, from the Buffer form and (checked equal) from the bigint[] form of the
// scalars, the records with the FIRST point of p for all pairs (the Schnorr shape: a 64-byte Buffer), those with the first
// scalar of b for all pairs (a 32-byte Buffer, checked equal to a one-element array), the length of the empty batch, and the
// text of the refusal of a point of q off the curve.
// Used by tests/test_ed_batch_lincomb2_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { ed_batch_lincomb2 } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const n = parseInt(process.argv[3], 10);
const bad = parseInt(process.argv[4], 10);
const p = blob.slice(0, 64 * n), q = blob.slice(64 * n, 128 * n), a = blob.slice(128 * n, 160 * n), b = blob.slice(160 * n, 192 * n);
const r = ed_batch_lincomb2(p, q, a, b);
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const ints = (buf) => Array.from({ length: n }, (_, i) => le(buf.slice(32 * i, 32 * (i + 1))));
if (!r.equals(ed_batch_lincomb2(p, q, ints(a), ints(b)))) throw new Error('bigint form disagrees with the Buffer form');
const onePoint = ed_batch_lincomb2(p.slice(0, 64), q, a, b);
const oneScalar = ed_batch_lincomb2(p, q, a, b.slice(0, 32));
if (!oneScalar.equals(ed_batch_lincomb2(p, q, a, [ints(b)[0]]))) throw new Error('one-element array disagrees with the 32-byte Buffer');
const empty = ed_batch_lincomb2(Buffer.alloc(0), Buffer.alloc(0), Buffer.alloc(0), Buffer.alloc(0));
const off = Buffer.from(q);
off[64 * bad + 32] ^= 1;  // y of that point of q: off the curve
let refused = '';
try {
  ed_batch_lincomb2(p, off, a, b);
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({ points: r.toString('hex'), onePoint: onePoint.toString('hex'), oneScalar: oneScalar.toString('hex'), empty: empty.length, refused }));
