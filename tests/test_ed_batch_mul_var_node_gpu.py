"""Edwards-BLS12 variable-base batch multiplication through the node binding: ed_batch_mul_var(points, scalars) through
compute_msm.js -> N-API shim -> msm377_ed_batch_mul_var, n = 257 on every class of curve point (the driver runs both scalar
forms and the one-scalar form and checks them equal), against the Python path of the same library and the host twin; a
point off the curve surfaces as an exception that names its index.  GPU only; skipped when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import ed_batch_mul_var_vectors as VV
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


def test_ed_batch_mul_var_through_node(tmp_path, engine):
    node = node_or_skip()
    n, bad = 257, 130
    points, scalars = VV.case(n)
    assert not R.ed_on_curve((points[bad][0], points[bad][1] ^ 1))  # what the driver plants at `bad`
    pb, sb = VV.encode(points, scalars)
    exp = engine.ed_batch_mul_var(pb, sb)
    assert exp == msm.ed_batch_mul_var_host(pb, sb)
    path = tmp_path / "ed_batch_mul_var.bin"
    path.write_bytes(pb + sb)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_ed_batch_mul_var.js"), str(path), str(n), str(bad)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert bytes.fromhex(got["points"]) == exp
    assert bytes.fromhex(got["one"]) == engine.ed_batch_mul_var(pb, sb[:32])
    assert got["empty"] == 0
    assert "msm377_ed_batch_mul_var" in got["refused"] and "point %d is not on the curve" % bad in got["refused"], got["refused"]
