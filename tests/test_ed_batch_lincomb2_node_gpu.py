"""Edwards-BLS12 pairwise linear combination through the node binding: ed_batch_lincomb2(p, q, a, b) through compute_msm.js
-> N-API shim -> msm377_ed_batch_lincomb2, n = 65 on every class of curve point and the first relations (the driver runs both
scalar forms, one stride-0 point and one stride-0 scalar), against the Python path of the same library and the host twin; a
point of q off the curve surfaces as an exception that names its array and index.  GPU only; skipped when the image has no
node."""
import json
import os
import shutil
import subprocess

import pytest

import ed_batch_lincomb2_vectors as LV
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


def test_ed_batch_lincomb2_through_node(tmp_path, engine):
    node = node_or_skip()
    n, bad = 65, 33
    ps, qs, as_, bs, _ = LV.case(n)
    assert not R.ed_on_curve((qs[bad][0], qs[bad][1] ^ 1))  # what the driver plants at `bad` of q
    pb, qb, ab, bb = LV.encode(ps, qs, as_, bs)
    exp = engine.ed_batch_lincomb2(pb, qb, ab, bb)
    assert exp == msm.ed_batch_lincomb2_host(pb, qb, ab, bb)
    path = tmp_path / "ed_batch_lincomb2.bin"
    path.write_bytes(pb + qb + ab + bb)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_ed_batch_lincomb2.js"), str(path), str(n), str(bad)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert bytes.fromhex(got["points"]) == exp
    assert bytes.fromhex(got["onePoint"]) == msm.ed_batch_lincomb2_host(pb[:64], qb, ab, bb)
    assert bytes.fromhex(got["oneScalar"]) == msm.ed_batch_lincomb2_host(pb, qb, ab, bb[:32])
    assert got["empty"] == 0
    assert "msm377_ed_batch_lincomb2" in got["refused"] and "point %d of q is not on the curve" % bad in got["refused"], got["refused"]
