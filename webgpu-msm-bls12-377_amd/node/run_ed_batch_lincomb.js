'use strict';
// Test driver: node run_ed_batch_lincomb.js <case.bin> <n> <k> <badTerm> <bad>
// The case file holds, term after term, n x 64 bytes of Edwards-BLS12 wire points and then that term's n scalars (32 bytes
// each).
// Prints the records of ed_batch_lincomb as hex, from the Buffer form and (checked equal) from the bigint[] form of the
// scalars, the records with the FIRST point of term 0 and the first scalar of the last term for all outputs (the Schnorr
// check as one sum: a 64-byte and a 32-byte Buffer, checked equal to a one-element array), the length of the empty batch,
// and the text of the refusal of a point of term badTerm off the curve.
// Used by tests/test_ed_batch_lincomb_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { ed_batch_lincomb } = require(path.join(__dirname, 'compute_msm.js'));

const blob = fs.readFileSync(process.argv[2]);
const [n, k, badTerm, bad] = process.argv.slice(3, 7).map((v) => parseInt(v, 10));
const terms = Array.from({ length: k }, (_, t) => ({ points: blob.slice(96 * n * t, 96 * n * t + 64 * n), scalars: blob.slice(96 * n * t + 64 * n, 96 * n * (t + 1)) }));
const r = ed_batch_lincomb(terms);
const le = (buf) => BigInt('0x' + Buffer.from(buf).reverse().toString('hex'));
const ints = (buf) => Array.from({ length: buf.length / 32 }, (_, i) => le(buf.slice(32 * i, 32 * (i + 1))));
if (!r.equals(ed_batch_lincomb(terms.map((t) => ({ points: t.points, scalars: ints(t.scalars) }))))) throw new Error('bigint form disagrees with the Buffer form');
const ones = terms.map((t, j) => ({ points: j === 0 ? t.points.slice(0, 64) : t.points, scalars: j === k - 1 ? t.scalars.slice(0, 32) : t.scalars }));
const schnorr = ed_batch_lincomb(ones);
if (!schnorr.equals(ed_batch_lincomb(ones.map((t, j) => (j === k - 1 ? { points: t.points, scalars: ints(t.scalars) } : t))))) throw new Error('one-element array disagrees with the 32-byte Buffer');
const empty = ed_batch_lincomb([{ points: Buffer.alloc(0), scalars: Buffer.alloc(0) }]);
const off = Buffer.from(terms[badTerm].points);
off[64 * bad + 32] ^= 1;  // y of that point: off the curve
let refused = '';
try {
  ed_batch_lincomb(terms.map((t, j) => (j === badTerm ? { points: off, scalars: t.scalars } : t)));
} catch (e) {
  refused = String(e);
}
console.log(JSON.stringify({ points: r.toString('hex'), schnorr: schnorr.toString('hex'), empty: empty.length, refused }));
