"""Edwards-BLS12 k-term linear combination through the node binding: ed_batch_lincomb(terms) through compute_msm.js -> N-API
shim -> msm377_ed_batch_lincomb, n = 65 at k = 3 on every class of curve point and the first relations (the driver runs both
scalar forms and the Schnorr-as-one-sum shape: one stride-0 point, one stride-0 scalar), against the Python path of the same
library and the host twin; a point of term 1 off the curve surfaces as an exception that names its index and term.  GPU
only; skipped when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import ed_batch_lincomb_vectors as KV
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


def test_ed_batch_lincomb_through_node(tmp_path, engine):
    node = node_or_skip()
    n, k, bad_term, bad = 65, 3, 1, 33
    points, scalars, _ = KV.case(n, k)
    assert not R.ed_on_curve((points[bad_term][bad][0], points[bad_term][bad][1] ^ 1))  # what the driver plants there
    pb, sb = KV.encode(points, scalars)
    exp = engine.ed_batch_lincomb(pb, sb)
    assert exp == msm.ed_batch_lincomb_host(pb, sb)
    path = tmp_path / "ed_batch_lincomb.bin"
    path.write_bytes(b"".join(p + s for p, s in zip(pb, sb)))
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_ed_batch_lincomb.js"), str(path), str(n), str(k), str(bad_term), str(bad)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert bytes.fromhex(got["points"]) == exp
    assert bytes.fromhex(got["schnorr"]) == msm.ed_batch_lincomb_host([pb[0][:64], pb[1], pb[2]], [sb[0], sb[1], sb[2][:32]])
    assert got["empty"] == 0
    assert "msm377_ed_batch_lincomb" in got["refused"] and "point %d of term %d is not on the curve" % (bad, bad_term) in got["refused"], got["refused"]
