"""Variable-base batch multiplication through the node binding: batch_mul_var(points, scalars, {outForm}) through
compute_msm.js -> N-API shim -> msm377_g1_batch_mul_var, n = 65, both output forms and the one-scalar form, against the
host twin (which tests/test_batch_mul_var_host.py pins to pyref).  GPU only; skipped when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm

pytestmark = pytest.mark.gpu

NODE_DIR = os.path.join(util.ROOT, "webgpu-msm-bls12-377_amd", "node")


def node_or_skip():
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    assert os.path.exists(os.path.join(NODE_DIR, "build", "msm377_napi.node")), "build the addon first: make -C webgpu-msm-bls12-377_amd/node"
    return node


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_batch_mul_var_through_node(tmp_path, out_form):
    node = node_or_skip()
    n = 65
    points = R.encode_points(list(VV.mixed_points(n, period=4)))  # exceptional points among subgroup points
    scalars = R.encode_scalars(([0x1D] + V.EDGE + V.random_scalars(0x90DF, n))[:n])
    case = tmp_path / "batch_mul_var.bin"
    case.write_bytes(points + scalars)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_batch_mul_var.js"), str(case), str(n), out_form], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert (bytes.fromhex(got["points"]), bytes.fromhex(got["infinity"])) == msm.batch_mul_var_host(points, scalars, out_form)
    assert (bytes.fromhex(got["onePoints"]), bytes.fromhex(got["oneInfinity"])) == msm.batch_mul_var_host(points, scalars[:32], out_form)
    assert got["empty"] == 0
    assert "outForm" in got["refused"], got["refused"]
