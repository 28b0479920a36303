"""Edwards-BLS12 batch multiplication on the host (include/msm377.h "Edwards-BLS12 batch multiplication"): the host twin
csrc/ed_batch_mul_host.hpp, the 9-limb inverse csrc/fq_inverse.hpp and the recode csrc/batch_mul_recode.hpp.
tests/native/ed_batch_mul_host.cpp is compiled with g++ and the address / undefined-behaviour sanitizers against the
headers (a stand-alone program: nothing is loaded into python) and asked for whole runs; the library's
msm377_ed_batch_mul_multi_host runs the same header.  Expected values: tests/pyref.py alone (R.ed_mul for every term,
R.ed_add for the sums).  CPU only; the device call: tests/test_ed_batch_mul_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import ed_batch_mul_vectors as EV
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ed_batch_mul_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
LAYOUTS = ("rows", "columns", "padded")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "ed_batch_mul_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, bases: bytes, k, scalars: bytes, n, out_stride, base_stride):
    """(return code, records) of one run of the host twin inside the sanitized program.  The program itself checks that a
    refused call leaves its poisoned output untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIQQQQ", k, 0, n, out_stride, base_stride, len(scalars)) + bases + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    assert len(blob) == 4 + (0 if rc else 64 * n)
    return rc, blob[4:]


def run_rows(exe, tmp_path, points, rows, layout="rows"):
    buf, out_stride, base_stride = EV.pack(rows, layout)
    return run_program(exe, tmp_path, EV.bases_bytes(points), len(points), buf, len(rows), out_stride, base_stride)


def test_limits(exe):
    res = subprocess.run([exe, "limits"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == EV.MAX_BASES


# ---- the recode and the inverse: the device's own code, compiled for the host ----
def test_recode_identity(exe, tmp_path):
    """s = sum digit 2^(c w) + carry 2^(c W) on the edges, every window's extreme digits and the rippling carries."""
    scalars = EV.all_scalars() + EV.random_scalars(0x4EC0DE, 64)
    src = tmp_path / "scalars.bin"
    src.write_bytes(R.encode_scalars(scalars))
    res = subprocess.run([exe, "recode", str(src)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == len(scalars)
    assert 0 in scalars and EV.ORD - 1 in scalars and EV.ORD + 1 in scalars and 4 * EV.ORD in scalars and 2**255 in scalars and 2**256 - 1 in scalars


def test_nine_limb_inverse(exe):
    res = subprocess.run([exe, "inverse"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) >= 300


# ---- the host twin against pyref ----
@pytest.mark.parametrize("name", [name for name, _ in EV.bases()])
def test_every_base_class(exe, tmp_path, name):
    pt = dict(EV.bases())[name]
    rows = [(s,) for s in EV.single_scalars()]
    wire, pts = EV.expected((pt,), rows)
    assert run_rows(exe, tmp_path, (pt,), rows) == (0, wire)
    assert msm.ed_batch_mul_multi_host(EV.bases_bytes((pt,)), EV.pack(rows)[0]) == wire
    assert pts[0] == R.ED_ID and wire[:64] == EV.IDENTITY_WIRE  # scalar 0: (0, 1), an ordinary record


@pytest.mark.parametrize("name", [name for name, _ in EV.tuples()])
def test_every_relation_between_bases(exe, tmp_path, name):
    points = dict(EV.tuples())[name]
    rows = EV.relation_rows(len(points))
    wire, pts = EV.expected(points, rows)
    assert run_rows(exe, tmp_path, points, rows) == (0, wire)
    for layout in ("rows", "columns"):
        assert msm.ed_batch_mul_multi_host(EV.bases_bytes(points), EV.pack(rows, layout)[0], layout) == wire, layout


def test_identity_output_with_no_identity_term():
    """(0, 1) comes out for a sum that cancels although neither term is the identity, beside a neighbour that is not."""
    for name, i in (("G_negG", 0), ("G_mG", 2), ("order4_pair", 4)):
        points = dict(EV.tuples())[name]
        rows = EV.relation_rows(2)
        wire, pts = EV.expected(points, rows)
        assert pts[i] == R.ED_ID and pts[i + 1] != R.ED_ID, name
        assert all(R.ed_mul(b, s) != R.ED_ID for b, s in zip(points, rows[i])), name
        got = msm.ed_batch_mul_multi_host(EV.bases_bytes(points), EV.pack(rows)[0])
        assert got[64 * i : 64 * i + 64] == EV.IDENTITY_WIRE and got == wire


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(exe, tmp_path, layout):
    """Row-major, column-major and padded rows of the same matrix: the same bytes.  k = 3."""
    points = dict(EV.tuples())["G_mG_order4"]
    rows = EV.relation_rows(3)
    wire, _ = EV.expected(points, rows)
    assert run_rows(exe, tmp_path, points, rows, layout) == (0, wire)


# ---- arguments ----
def test_empty_batch(exe, tmp_path):
    two = EV.bases_bytes((R.ED_G, R.ED_G))
    assert msm.ed_batch_mul_multi_host(two, b"") == b""
    assert msm.ed_batch_mul_multi_host(two, b"", "columns") == b""
    lib = msm.load_library()
    assert lib.msm377_ed_batch_mul_multi_host(None, 2, None, 0, 64, 32, None) == 0
    assert lib.msm377_ed_batch_mul_multi_host(None, 0, None, 0, 64, 32, None) == EINVAL  # the shape is checked first
    assert run_program(exe, tmp_path, two, 2, b"", 0, 64, 32) == (0, b"")


def test_invalid_arguments_leave_the_output_untouched(exe, tmp_path):
    lib = msm.load_library()
    bases = EV.bases_bytes([R.ed_mul(R.ED_G, j + 1) for j in range(17)])
    scalars = R.encode_scalars(list(range(5, 5 + 2 * 17)))
    out = ctypes.create_string_buffer(b"\xa5" * 144, 144)

    def call(b, k, s, out_stride, base_stride, o):
        return lib.msm377_ed_batch_mul_multi_host(b, k, s, 2, out_stride, base_stride, o)

    o = ctypes.addressof(out)
    gx, gy = R.ED_G
    noncanonical = bases[:64] + R.ed_encode_points([(gx + R.Q, gy)])  # a coordinate of q or more at position 1
    noncanonical_y = bases[:64] + R.ed_encode_points([(gx, gy + R.Q)])
    off_curve = bases[:64] + R.ed_encode_points([(gx, gy ^ 1)])
    assert not R.ed_on_curve((gx, gy ^ 1))
    assert call(bases, 0, scalars, 64, 32, o) == EINVAL
    assert call(bases, 17, scalars, 32 * 17, 32, o) == EINVAL
    assert call(bases, 2, scalars, 0, 32, o) == EINVAL
    assert call(bases, 2, scalars, 64, 0, o) == EINVAL
    assert call(bases, 2, scalars, 48, 32, o) == EINVAL
    assert call(bases, 2, scalars, 64, 48, o) == EINVAL
    assert call(None, 2, scalars, 64, 32, o) == EINVAL
    assert call(bases, 2, None, 64, 32, o) == EINVAL
    assert call(bases, 2, scalars, 64, 32, None) == EINVAL
    assert call(noncanonical, 2, scalars, 64, 32, o) == EINVAL
    assert call(noncanonical_y, 2, scalars, 64, 32, o) == EINVAL
    assert call(off_curve, 2, scalars, 64, 32, o) == EINVAL
    assert out.raw == b"\xa5" * 144
    assert call(off_curve, 1, scalars, 64, 32, o) == 0  # position 1 is not part of a k = 1 call
    assert out.raw[:128] == R.ed_encode_points([R.ed_mul(R.ED_G, 5), R.ed_mul(R.ED_G, 7)]) and out.raw[128:] == b"\xa5" * 16
    ctypes.memset(out, 0xA5, 144)
    assert call(bases, 16, scalars, 32 * 16, 32, o) == 0  # the largest k
    exp = [R.ed_mul(R.ED_G, sum((j + 1) * (5 + 16 * i + j) for j in range(16))) for i in range(2)]
    assert out.raw[:128] == R.ed_encode_points(exp)
    # the same refusals inside the sanitized program, which checks its poisoned output itself
    two = bases[:128]
    assert run_program(exe, tmp_path, two, 0, scalars, 2, 64, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, bases, 17, scalars, 2, 32 * 17, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, two, 2, scalars, 2, 48, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, two, 2, scalars, 2, 64, 0)[0] == EINVAL
    assert run_program(exe, tmp_path, noncanonical, 2, scalars, 2, 64, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, off_curve, 2, scalars, 2, 64, 32)[0] == EINVAL
    with pytest.raises(ValueError):
        msm.ed_batch_mul_multi_host(bases, scalars)  # 17 bases
