"""Multi-base batch multiplication through the node binding: batch_mul_multi(bases, scalars, {outForm, layout}) through
compute_msm.js -> N-API shim -> msm377_g1_batch_mul_multi, n = 33, k = 2, one base outside the subgroup, both output forms
(the driver runs both layouts and both input forms and checks them equal), against tests/pyref.py.  GPU only; skipped
when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import batch_mul_multi_vectors as MV
import batch_mul_vectors as V
import pyref as R
import util

pytestmark = pytest.mark.gpu

NODE_DIR = os.path.join(util.ROOT, "webgpu-msm-bls12-377_amd", "node")


def node_or_skip():
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    assert os.path.exists(os.path.join(NODE_DIR, "build", "msm377_napi.node")), "build the addon first: make -C webgpu-msm-bls12-377_amd/node"
    return node


@pytest.fixture(scope="module")
def case():
    n = 33
    pts = (R.G, dict(V.bases())["G_plus_torsion"])  # the second base lies outside the subgroup
    rows = (MV.ZERO_ROWS + MV.many_rows(2, n, 0x90E2, bits=64))[:n]
    rows[5] = (V.EDGE[2], V.EDGE[3])  # one full-width row
    wire, flags, _ = MV.expected(pts, rows)
    assert flags[0] == 1 and flags[1] == 0  # (0, r) over a base outside the subgroup is not the identity
    return n, MV.bases_bytes(pts) + MV.pack(rows)[0], wire, flags


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_batch_mul_multi_through_node(tmp_path, case, out_form):
    node = node_or_skip()
    n, blob, wire, flags = case
    path = tmp_path / "batch_mul_multi.bin"
    path.write_bytes(blob)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_batch_mul_multi.js"), str(path), str(n), "2", out_form], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    exp = wire if out_form == "wire" else V.mont_flag_records(wire, flags)
    assert (bytes.fromhex(got["points"]), bytes.fromhex(got["infinity"])) == (exp, flags)
    assert got["empty"] == 0
    assert "outForm" in got["refused"], got["refused"]
