"""check_points through the reference-side host path: node -> compute_msm.js -> N-API shim -> msm377_g1_check_points, on
one golden set and one crafted set (a fresh node child per case).  GPU only; skipped when the image has no node."""
import json
import os
import shutil
import subprocess

import pytest

import check_vectors as V
import util

pytestmark = pytest.mark.gpu

NODE_DIR = os.path.join(util.ROOT, "webgpu-msm-bls12-377_amd", "node")


def run_check(path, n, flags=None):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    addon = os.path.join(NODE_DIR, "build", "msm377_napi.node")
    assert os.path.exists(addon), "build the addon first: make -C webgpu-msm-bls12-377_amd/node"
    argv = [node, os.path.join(NODE_DIR, "run_check.js"), str(path), str(n)] + ([str(flags)] if flags is not None else [])
    proc = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    got = json.loads(proc.stdout.strip().splitlines()[-1])
    assert got["empty"] == {"checked": "0", "noncanonical": "0", "off_curve": "0", "outside_subgroup": "0", "first_bad": None, "first_bad_reason": 0, "bigints": True}
    assert got["report"]["bigints"]
    return got["report"]


def test_check_points_js_golden(golden):
    name = "g1_n1024_random"
    rep = run_check(os.path.join(util.GOLDEN_DIR, name + ".bin"), golden[name]["n"])  # the file starts with the points
    assert (rep["checked"], rep["noncanonical"], rep["off_curve"], rep["outside_subgroup"], rep["first_bad"], rep["first_bad_reason"]) == ("1024", "0", "0", "0", None, 0)


@pytest.mark.parametrize("flags", [7, 3])
def test_check_points_js_crafted(tmp_path, flags):
    blob, verdicts = V.g1_crafted()
    path = tmp_path / "crafted.bin"
    path.write_bytes(blob)
    rep = run_check(path, len(verdicts), flags)
    n, nc, oc, og, first, reason = V.expected_report(verdicts, flags)
    assert first is not None
    assert (rep["checked"], rep["noncanonical"], rep["off_curve"], rep["outside_subgroup"], rep["first_bad"], rep["first_bad_reason"]) == (str(n), str(nc), str(oc), str(og), str(first), reason)
