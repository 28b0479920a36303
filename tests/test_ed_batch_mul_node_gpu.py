"""Edwards-BLS12 batch multiplication through the node binding: ed_batch_mul_multi(bases, scalars, {layout}) through
compute_msm.js -> N-API shim -> msm377_ed_batch_mul_multi, n = 257, k = 2, one base outside the subgroup (the driver runs
both layouts, both scalar forms and the k = 1 convenience and checks them equal), against the Python path of the same
library and, at a probe set, tests/pyref.py.  GPU only; skipped when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import ed_batch_mul_vectors as EV
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


def test_ed_batch_mul_through_node(tmp_path, engine):
    node = node_or_skip()
    n = 257
    pts = (R.ED_G, dict(EV.bases())["P_plus_order4_a"])  # the second base lies outside the subgroup
    rows = EV.many_rows(2, n, 0x90E2ED)
    bases, buf = EV.bases_bytes(pts), EV.pack(rows)[0]
    exp = engine.ed_batch_mul_multi(bases, buf)
    probe = [0, 1, 2, 3, 64, 256]
    assert b"".join(exp[64 * i : 64 * i + 64] for i in probe) == EV.expected(pts, [rows[i] for i in probe])[0]
    path = tmp_path / "ed_batch_mul.bin"
    path.write_bytes(bases + buf)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_ed_batch_mul.js"), str(path), str(n), "2"], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert bytes.fromhex(got["points"]) == exp
    assert bytes.fromhex(got["single"]) == engine.ed_batch_mul(bases[:64], R.encode_scalars([row[0] for row in rows]))
    assert got["empty"] == 0
    assert "msm377_ed_batch_mul_multi" in got["refused"], got["refused"]
