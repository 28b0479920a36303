'use strict';
// node run_check.js <points file> <n> [flags]: check_points on the first n 96-byte records of the file, the report as one
// JSON line (bigints as decimal strings).  Used by tests/test_check_points_node_gpu.py.
const fs = require('fs');
const path = require('path');
const { check_points, CHECK_ALL } = require(path.join(__dirname, 'compute_msm.js'));

const [file, nArg, flagsArg] = process.argv.slice(2);
const n = Number(nArg);
const points = fs.readFileSync(file).subarray(0, 96 * n);
const rep = flagsArg === undefined ? check_points(points) : check_points(points, Number(flagsArg));
const empty = check_points(Buffer.alloc(0), CHECK_ALL);
const str = (r) => ({
  checked: r.checked.toString(), noncanonical: r.noncanonical.toString(), off_curve: r.off_curve.toString(),
  outside_subgroup: r.outside_subgroup.toString(), first_bad: r.first_bad === null ? null : r.first_bad.toString(),
  first_bad_reason: r.first_bad_reason, bigints: typeof r.checked === 'bigint' && (r.first_bad === null || typeof r.first_bad === 'bigint'),
});
console.log(JSON.stringify({ report: str(rep), empty: str(empty) }));
