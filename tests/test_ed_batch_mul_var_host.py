"""Edwards-BLS12 variable-base batch multiplication on the host (include/msm377.h "Edwards-BLS12 variable-base batch
multiplication"): the host twin csrc/ed_batch_mul_var_host.hpp, the lazy doubling csrc/te377.hpp TeLazy::dbl / dbl_nt and
the walk's recode csrc/batch_mul_var_recode.hpp.  tests/native/ed_lazy_dbl_host.cpp is compiled with g++ against the
headers -- once plain and once with the address / undefined-behaviour sanitizers, a stand-alone program both times:
nothing is loaded into python -- and asked for whole runs; the library's msm377_ed_batch_mul_var_host runs the same
header.  Expected values: tests/pyref.py (R.ed_mul) and the reference's own vectors (tests/ed_vectors.py).  CPU only; the
device call: tests/test_ed_batch_mul_var_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import ed_batch_mul_var_vectors as VV
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import CHECK_CANONICAL, CHECK_CURVE, EINVAL, EPOINT

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ed_lazy_dbl_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
N = 65  # the pyref case: a wave and one point, every special class, the first edge scalars


def build(name, *flags):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    cmd = ["g++", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


@pytest.fixture(scope="module")
def exe():
    return build("ed_lazy_dbl_host", "-O2")


@pytest.fixture(scope="module")
def exe_san():
    return build("ed_lazy_dbl_host_san", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")  # (-O1: a 45 s build)


def run_program(exe, tmp_path, points: bytes, scalars: bytes, n, stride):
    """(return code, records) of one run of the host twin inside the stand-alone program, which itself checks that a
    refused call leaves its poisoned output untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<QII", n, stride, 0) + points + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    assert len(blob) == 4 + (0 if rc else 64 * n)
    return rc, blob[4:]


@pytest.fixture(scope="module")
def pyref_case():
    points, scalars = VV.case(N)
    return points, scalars, VV.expected(points, scalars)


# ---- the lazy doubling and the recode: the device's own code, compiled for the host ----
def class_points():
    """The generator, every class of ed_curve_points.special_classes, and the points of the N-point case."""
    import random

    import ed_curve_points as EP

    classes, p, low = EP.special_classes(random.Random("ed lazy dbl"))
    return [R.ED_G] + classes + p + list(VV.case(N)[0][:24])


@pytest.mark.parametrize("which", ["exe", "exe_san"])
def test_lazy_doubling_equals_the_canonical_one(request, tmp_path, which):
    """TeLazy::dbl / dbl_nt == Ed::dbl / dbl_nt after canon, on random points, the identity, the torsion points, images at the
    upper end of the stored form, and along the walk's chain (dbl_nt^3, dbl, madd_affine) x 64."""
    prog = request.getfixturevalue(which)
    pts = class_points()
    assert R.ED_ID in pts and sum(1 for p in pts if p[0] == 0 or p[1] == 0) >= 4  # (0, 1), (0, -1), (+-i, 0)
    src = tmp_path / "points.bin"
    src.write_bytes(R.ed_encode_points(pts))
    res = subprocess.run([prog, "dbl", str(src)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == len(pts)


@pytest.mark.parametrize("which", ["exe", "exe_san"])
def test_lazy_doubling_at_the_bound_of_the_stored_form(request, which):
    """Every coordinate at q + q / 16 - 1 - r: the largest values tools/check_lazy_bounds.py admits as `stored`."""
    res = subprocess.run([request.getfixturevalue(which), "bound"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == 256


def test_digit_sum_identity(exe_san, tmp_path):
    """bmv_pack / bmv_next as this walk reuses them: s = sum d_w 16^w + carry 2^256 on the edge scalars."""
    scalars = VV.edge_scalars() + VV.random_scalars("recode", 64)
    src = tmp_path / "scalars.bin"
    src.write_bytes(R.encode_scalars(scalars))
    res = subprocess.run([exe_san, "recode", str(src)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == len(scalars)
    assert {VV.final_carry(s) for s in scalars} == {0, 1}
    assert all(VV.final_carry(s) == 1 for s in (VV.MASK256, VV.nibbles(9), 0xF << 252, 9 << 252))


# ---- the host twin against pyref and the reference's vectors ----
def test_twin_against_pyref(exe_san, tmp_path, pyref_case):
    points, scalars, wire = pyref_case
    pb, sb = VV.encode(points, scalars)
    assert msm.ed_batch_mul_var_host(pb, sb) == wire
    assert run_program(exe_san, tmp_path, pb, sb, N, 32) == (0, wire)
    assert VV.IDENTITY_WIRE in [wire[64 * i : 64 * i + 64] for i in range(N) if points[i] != R.ED_ID and scalars[i] != 0]  # O from a point that is not O


def test_every_edge_scalar_on_a_cofactor_point():
    """All of edge_scalars on P + T (T of order 4) and on the generator."""
    import random

    import ed_curve_points as EP

    classes, _, _ = EP.special_classes(random.Random("ed var edge"))
    edges = VV.edge_scalars()
    for pt in (classes[5], R.ED_G):
        pb, sb = VV.encode([pt] * len(edges), edges)
        assert msm.ed_batch_mul_var_host(pb, sb) == VV.expected([pt] * len(edges), edges)


def test_reference_vectors():
    """The reference's MULTIPLY and (x-only) GROUP_SCALAR_MUL vectors as one batch."""
    multiply, group = VV.reference_cases()
    points = [pt for pt, _, _ in multiply] + [R.ed_point_from_x(x) for x, _, _ in group]
    scalars = [k for _, k, _ in multiply] + [k for _, k, _ in group]
    out = msm.ed_batch_mul_var_host(*VV.encode(points, scalars))
    got = [(int.from_bytes(out[64 * i : 64 * i + 32], "little"), int.from_bytes(out[64 * i + 32 : 64 * i + 64], "little")) for i in range(len(points))]
    assert got[: len(multiply)] == [exp for _, _, exp in multiply]
    assert [g[0] for g in got[len(multiply) :]] == [xr for _, _, xr in group]


def test_one_scalar_for_all_equals_the_scalar_repeated(exe_san, tmp_path, pyref_case):
    points = pyref_case[0]
    pb = R.ed_encode_points(list(points))
    for s in (VV.MASK256, R.ED_SUBGROUP + 1, 0xD0E50F7AB1, 0):
        one = R.encode_scalars([s])
        exp = msm.ed_batch_mul_var_host(pb, one * N)
        assert msm.ed_batch_mul_var_host(pb, one) == exp, s
        assert run_program(exe_san, tmp_path, pb, one, N, 0) == (0, exp), s
    assert exp == VV.IDENTITY_WIRE * N  # the zero scalar


# ---- refusals ----
def test_points_off_the_curve_are_refused_with_the_lowest_index(exe_san, tmp_path, pyref_case):
    points, scalars, _ = pyref_case
    gx, gy = R.ED_G
    bad = VV.off_curve_point()
    sb = R.encode_scalars(list(scalars))
    cases = [
        ({0: bad}, 0, CHECK_CURVE),
        ({N // 2: bad}, N // 2, CHECK_CURVE),
        ({N - 1: bad}, N - 1, CHECK_CURVE),
        ({40: bad, 7: bad}, 7, CHECK_CURVE),
        ({9: (gx + R.Q, gy)}, 9, CHECK_CANONICAL),  # a coordinate of q or more (q + x fits 32 bytes)
        ({9: (gx, gy + R.Q), 3: bad}, 3, CHECK_CURVE),
        ({9: (gx, gy + R.Q), 30: bad}, 9, CHECK_CANONICAL),
    ]
    for planted, index, reason in cases:
        pts = list(points)
        for i, p in planted.items():
            pts[i] = p
        pb = R.ed_encode_points(pts)
        with pytest.raises(msm.MsmError) as err:
            msm.ed_batch_mul_var_host(pb, sb)
        assert err.value.code == EPOINT and err.value.index == index, planted
        rep = msm.ed_check_points_host(pb, CHECK_CANONICAL | CHECK_CURVE)
        assert (rep.first_bad, rep.first_bad_reason) == (index, reason)
        assert run_program(exe_san, tmp_path, pb, sb, N, 32)[0] == EPOINT  # ... with its poisoned output untouched


def test_arguments():
    lib = msm.load_library()
    pb, sb = VV.encode([R.ED_G, R.ed_mul(R.ED_G, 5)], [3, 4])
    out = ctypes.create_string_buffer(b"\xa5" * 144, 144)
    o = ctypes.addressof(out)
    call = lib.msm377_ed_batch_mul_var_host
    for stride in (1, 4, 16, 31, 33, 64):
        assert call(pb, sb, 2, stride, o) == EINVAL, stride
    assert call(None, sb, 2, 32, o) == EINVAL
    assert call(pb, None, 2, 32, o) == EINVAL
    assert call(pb, sb, 2, 32, None) == EINVAL
    assert call(None, None, 0, 16, None) == EINVAL  # the stride is checked first
    assert call(None, None, 0, 32, None) == 0 and call(None, None, 0, 0, None) == 0
    assert out.raw == b"\xa5" * 144
    assert call(pb, sb, 2, 32, o) == 0
    assert out.raw[:128] == R.ed_encode_points([R.ed_mul(R.ED_G, 3), R.ed_mul(R.ED_G, 20)]) and out.raw[128:] == b"\xa5" * 16
    assert msm.ed_batch_mul_var_host(b"", b"") == b""
    with pytest.raises(ValueError):
        msm.ed_batch_mul_var_host(pb, sb + sb)
    # in place: the outputs over the points
    buf = ctypes.create_string_buffer(pb, 128)
    assert call(buf, sb, 2, 32, ctypes.addressof(buf)) == 0
    assert buf.raw == out.raw[:128]
