"""Row commitments through the node binding: set_generators(gens) and commit_rows(scalars, k, {outForm, layout}) through
compute_msm.js -> N-API shim -> msm377_g1_set_generators / msm377_g1_commit_rows, k = 33 (three segments of 11), n = 65,
both output forms (the driver runs both layouts and both input forms and checks them equal).  The result equals the
Python path's bytes and the known-logarithm closed form of tests/commit_rows_vectors.py.  GPU only; skipped when the image
has no node."""
import json
import os
import shutil
import subprocess

import pytest

import batch_mul_vectors as V
import commit_rows_vectors as CR
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
    n, k = 65, 33
    logs, gens = CR.known_logs(k)
    rows = CR.sliding_rows(CR.sliding_buffer(n, k, 0x90DE), n, k)
    rows[3] = tuple([0] * k)  # one identity output
    wire, flags = CR.closed_rows(logs, rows)
    assert flags[3] == 1 and flags[4] == 0
    return n, k, gens, CR.pack(rows)[0], wire, flags


@pytest.mark.parametrize("out_form", ["wire", "mont_flag"])
def test_commit_rows_through_node(engine, tmp_path, case, out_form):
    node = node_or_skip()
    n, k, gens, data, wire, flags = case
    path = tmp_path / "commit_rows.bin"
    path.write_bytes(gens + data)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_commit_rows.js"), str(path), str(n), str(k), out_form], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    exp = wire if out_form == "wire" else V.mont_flag_records(wire, flags)
    assert (bytes.fromhex(got["points"]), bytes.fromhex(got["infinity"])) == (exp, flags)
    assert got["empty"] == 0
    assert "outForm" in got["refused"], got["refused"]
    assert "call sequence" in got["dropped"], got["dropped"]
    try:  # the Python path: the same bytes
        engine.set_generators(gens)
        assert engine.commit_rows(data, k, out_form) == (exp, flags)
    finally:
        engine.set_generators(None)
