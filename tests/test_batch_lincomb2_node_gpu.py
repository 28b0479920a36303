"""Pairwise linear combination through the node binding: batch_lincomb2(p, q, a, b, {outForm}) through compute_msm.js ->
N-API shim -> msm377_g1_batch_lincomb2, n = 65, both output forms and a stride-0 case, against the host twin (which
tests/test_batch_lincomb2_host.py pins to pyref).  GPU only; skipped when the image has no node."""
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
def test_batch_lincomb2_through_node(tmp_path, out_form):
    node = node_or_skip()
    n = 65
    p = list(VV.mixed_points(n, period=4))  # exceptional points among subgroup points
    q = list(VV.mixed_points(n, seed=0x4B12EF, period=5))
    a = ([0x1D] + V.EDGE + V.random_scalars(0x90E0, n))[:n]
    b = (V.EDGE[::-1] + V.random_scalars(0x90E1, n))[:n]
    q[20], b[20] = p[20], a[20]          # Q = P with equal digits
    q[21], b[21] = R.neg(p[21]), a[21]   # Q = -P: the identity
    p, q, a, b = R.encode_points(p), R.encode_points(q), R.encode_scalars(a), R.encode_scalars(b)
    case = tmp_path / "batch_lincomb2.bin"
    case.write_bytes(p + q + a + b)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_batch_lincomb2.js"), str(case), str(n), out_form], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    exp = msm.batch_lincomb2_host(p, q, a, b, out_form)
    assert exp[1][21] == 1
    assert (bytes.fromhex(got["points"]), bytes.fromhex(got["infinity"])) == exp
    assert (bytes.fromhex(got["onePoints"]), bytes.fromhex(got["oneInfinity"])) == msm.batch_lincomb2_host(p, q, a[:32], b, out_form)
    assert got["empty"] == 0
    assert "outForm" in got["refused"], got["refused"]
