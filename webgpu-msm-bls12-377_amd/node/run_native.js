'use strict';
// Test driver: node run_native.js <case.bin> <n> <pointForm> <scalarForm>
// The case file holds n points in pointForm (96 bytes each, 104 for mont_flag), then n x 32 bytes of scalars in
// scalarForm.  Prints the result of the native-form call (decimal strings, src/ui/Benchmark.tsx:41-48), the empty call,
// and the message of a call that names an unknown form.
const fs = require('fs');
const { compute_msm } = require('./compute_msm.js');

(async () => {
  const blob = fs.readFileSync(process.argv[2]);
  const n = parseInt(process.argv[3], 10);
  const pointForm = process.argv[4];
  const scalarForm = process.argv[5];
  const stride = pointForm === 'mont_flag' ? 104 : 96;
  const points = blob.slice(0, stride * n);
  const scalars = blob.slice(stride * n, (stride + 32) * n);
  const r = await compute_msm(points, scalars, { pointForm, scalarForm });
  const empty = await compute_msm(Buffer.alloc(0), Buffer.alloc(0), { pointForm, scalarForm });
  let refused = '';
  try {
    await compute_msm(points, scalars, { pointForm: 'affine', scalarForm });
  } catch (e) {
    refused = String(e);
  }
  console.log(JSON.stringify({ x: r.x.toString(), y: r.y.toString(), empty_x: empty.x.toString(), empty_y: empty.y.toString(), refused }));
})().catch((e) => {
  console.error(String(e));
  process.exit(1);
});
