"""The short-scalar option of the node binding: compute_msm(points, scalars, {scalarBytes, scalarBits}) through
compute_msm.js -> N-API shim -> msm377_g1_msm_short, against the CPU oracle; and the two-argument call, unchanged, on a
golden vector.  GPU only; skipped when the image has no node."""
import json
import os
import random
import shutil
import subprocess

import pytest

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


def test_compute_msm_js_with_a_declared_width(oracle, tmp_path):
    node = node_or_skip()
    n, sb, bits = 1024, 8, 64
    rng = random.Random(0x40DE)
    ks = [rng.getrandbits(bits) for _ in range(n)]
    ks[:3] = [0, 1, (1 << bits) - 1]
    pts = util.oracle_gen_points(oracle, n, 0x377377377, 0x5CA1A5)
    case = tmp_path / "short_case.bin"
    case.write_bytes(pts + msm.encode_scalars(ks, sb))
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_short.js"), str(case), str(n), str(sb), str(bits)], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    ex, ey = R.decode_result(util.oracle_msm(oracle, pts, R.encode_scalars(ks)))
    assert got["x"] == str(ex) and got["y"] == str(ey)
    assert got["empty_x"] == "0" and got["empty_y"] == "1"
    assert "63 bits" in got["refused"], got["refused"]  # a width one bit too small is refused, and the message names it


def test_two_argument_call_is_unchanged(golden):
    node = node_or_skip()
    case = golden["g1_n1024_random"]
    proc = subprocess.run(
        [node, os.path.join(NODE_DIR, "run_golden.js"), os.path.join(util.GOLDEN_DIR, "g1_n1024_random.bin"), str(case["n"])],
        capture_output=True, text=True, timeout=300,
    )
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    ex, ey = R.decode_result(case["expected"])
    assert got["x"] == str(ex) and got["y"] == str(ey) and got["forms"] == 3
