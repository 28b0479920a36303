"""Fixed-base batch multiplication through the node binding: batch_mul(base, scalars, {outForm}) through compute_msm.js
-> N-API shim -> msm377_g1_batch_mul, n = 33, both output forms, against pyref.  GPU only; skipped when the image has no
node."""
import json
import os
import shutil
import subprocess

import pytest

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


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_batch_mul_through_node(tmp_path, out_form):
    node = node_or_skip()
    n = 33
    scalars = (V.EDGE + V.random_scalars(0x90DE, n))[:n]
    base = R.add(R.G, dict(V.bases())["torsion"])  # a base outside the subgroup: nothing is reduced mod r
    case = tmp_path / "batch_mul.bin"
    case.write_bytes(V.base_bytes(base) + R.encode_scalars(scalars))
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_batch_mul.js"), str(case), str(n), out_form], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    wire, flags, _ = V.expected(base, scalars)
    assert bytes.fromhex(got["infinity"]) == flags
    assert bytes.fromhex(got["points"]) == (wire if out_form == "wire" else V.mont_flag_records(wire, flags))
    assert got["empty"] == 0
    assert "outForm" in got["refused"], got["refused"]
