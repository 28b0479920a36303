"""The native input forms through the node binding: compute_msm(points, scalars, {pointForm, scalarForm}) through
compute_msm.js -> N-API shim -> msm377_ctx_set_input_format + msm377_g1_msm, on a golden vector re-encoded by the Python
codecs and on a case with flagged points against pyref.  GPU only; skipped when the image has no node."""
import json
import os
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


def run_native(node, tmp_path, points: bytes, scalars: bytes, n: int, pform: str, sform: str):
    case = tmp_path / ("native_%s_%s.bin" % (pform, sform))
    case.write_bytes(points + scalars)
    proc = subprocess.run([node, os.path.join(NODE_DIR, "run_native.js"), str(case), str(n), pform, sform], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    return json.loads(proc.stdout.strip().splitlines()[-1])


def test_golden_vector_in_montgomery_form(golden, tmp_path):
    node = node_or_skip()
    case = golden["g1_n1024_random"]
    pts, ks = R.decode_points(case["points"]), R.decode_scalars(case["scalars"])
    got = run_native(node, tmp_path, msm.encode_points_native(pts, "mont"), msm.encode_scalars_native(ks, "mont"), case["n"], "mont", "mont")
    ex, ey = R.decode_result(case["expected"])
    assert got["x"] == str(ex) and got["y"] == str(ey)
    assert got["empty_x"] == "0" and got["empty_y"] == "1"
    assert "pointForm" in got["refused"], got["refused"]


def test_flagged_points_through_node(golden, tmp_path):
    node = node_or_skip()
    case = golden["g1_n48_repeats_and_negs"]
    n = case["n"]
    pts, ks = R.decode_points(case["points"]), R.decode_scalars(case["scalars"])
    flagged = {0, 5, 31, 32, 47}
    buf = bytearray(msm.encode_points_native(pts, "mont_flag"))
    for i in flagged:
        buf[104 * i : 104 * i + 96] = b"\xff" * 96
        buf[104 * i + 96] = 0xFF
    got = run_native(node, tmp_path, bytes(buf), msm.encode_scalars_native(ks, "mont"), n, "mont_flag", "mont")
    exp = R.msm_naive([p for i, p in enumerate(pts) if i not in flagged], [k for i, k in enumerate(ks) if i not in flagged])
    ex, ey = R.decode_result(R.encode_result(exp)) or (0, 1)
    assert got["x"] == str(ex) and got["y"] == str(ey)
