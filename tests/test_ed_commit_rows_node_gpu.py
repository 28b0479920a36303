"""Edwards-BLS12 row commitments through the node binding: ed_set_generators(gens) and ed_commit_rows(scalars, k, {layout})
through compute_msm.js -> N-API shim -> msm377_ed_set_generators / msm377_ed_commit_rows, k = 33 (three segments of 11),
n = 65, both layouts (the driver runs both input forms and checks the other layout equal).  The result equals the host
twin's bytes (tests/test_ed_commit_rows_host.py pins it to pyref) and the Python path's.  GPU only; skipped when the image
has no node."""
import json
import os
import shutil
import subprocess

import pytest

import ed_commit_rows_vectors as ECR
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


@pytest.fixture(scope="module")
def case():
    n, k = 65, 33
    _, gens = ECR.known_logs(k)
    rows = ECR.sliding_rows(ECR.mixed_buffer(n + k - 1, 0x90DE), n, k)
    rows[3] = tuple([0] * k)  # one identity output
    data = ECR.pack(rows)[0]
    wire = msm.ed_commit_rows_host(gens, data)
    assert wire[64 * 3 : 64 * 4] == ECR.IDENTITY_WIRE and wire[64 * 4 : 64 * 5] != ECR.IDENTITY_WIRE
    return n, k, gens, data, wire


@pytest.mark.parametrize("layout", ["rows", "columns"])
def test_ed_commit_rows_through_node(engine, tmp_path, case, layout):
    node = node_or_skip()
    n, k, gens, data, wire = case
    path = tmp_path / "ed_commit_rows.bin"
    path.write_bytes(gens + data)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_ed_commit_rows.js"), str(path), str(n), str(k), layout], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert bytes.fromhex(got["points"]) == wire
    assert got["empty"] == 0
    assert "point 2 of the generators is not on the curve" in got["refused"], got["refused"]
    assert "call sequence" in got["after"], got["after"]  # the failed set left none
    assert "call sequence" in got["dropped"], got["dropped"]
    try:  # the Python path: the same bytes
        engine.ed_set_generators(gens)
        assert engine.ed_commit_rows(data, k) == wire
    finally:
        engine.ed_set_generators(None)
