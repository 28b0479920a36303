'use strict';
// Test driver: node run_short.js <case.bin> <n> <scalarBytes> <scalarBits>
// The case file holds n x 96 bytes of points, then n x scalarBytes bytes of compact scalars.  Prints the short call's
// result from the Buffer form and from the bigint[] form (decimal strings, src/ui/Benchmark.tsx:41-48).
const fs = require('fs');
const { compute_msm } = require('./compute_msm.js');

(async () => {
  const blob = fs.readFileSync(process.argv[2]);
  const n = parseInt(process.argv[3], 10);
  const scalarBytes = parseInt(process.argv[4], 10);
  const scalarBits = parseInt(process.argv[5], 10);
  const points = blob.slice(0, 96 * n);
  const scalars = blob.slice(96 * n, (96 + scalarBytes) * n);
  const r = await compute_msm(points, scalars, { scalarBytes, scalarBits });
  const le = (b) => BigInt('0x' + Buffer.from(b).reverse().toString('hex'));
  const ks = [];
  for (let i = 0; i < n; i++) ks.push(le(scalars.slice(scalarBytes * i, scalarBytes * (i + 1))));
  const r2 = await compute_msm(points, ks, { scalarBytes, scalarBits });
  if (r2.x !== r.x || r2.y !== r.y) throw new Error('bigint[] form disagrees with the Buffer form');
  const empty = await compute_msm(Buffer.alloc(0), Buffer.alloc(0), { scalarBytes, scalarBits });
  let refused = '';
  try {
    await compute_msm(points, scalars, { scalarBytes, scalarBits: scalarBits - 1 });  // the widest scalar has bit scalarBits - 1 set
  } catch (e) {
    refused = String(e);
  }
  console.log(JSON.stringify({ x: r.x.toString(), y: r.y.toString(), empty_x: empty.x.toString(), empty_y: empty.y.toString(), refused }));
})().catch((e) => {
  console.error(String(e));
  process.exit(1);
});
