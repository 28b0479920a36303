"""Multi-base batch multiplication on the host (include/msm377.h "multi-base batch multiplication"): the host twin
csrc/batch_mul_multi_host.hpp.  tests/native/batch_mul_multi_host.cpp is compiled with g++ and the address /
undefined-behaviour sanitizers against the headers (a stand-alone program: nothing is loaded into python) and asked for
whole runs; the library's msm377_g1_batch_mul_multi_host runs the same header.  Expected values: tests/pyref.py alone
(R.mul for every term, R.add for the sums).  CPU only; the device call: tests/test_batch_mul_multi_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import batch_mul_multi_vectors as MV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "batch_mul_multi_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER
LAYOUTS = ("rows", "columns", "padded")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "batch_mul_multi_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, bases: bytes, k, scalars: bytes, n, out_stride, base_stride, scalar_form=V.WIRE, out_form=V.WIRE):
    """(return code, records, flags) of one run of the host twin inside the sanitized program.  The program itself
    checks that a refused call leaves its poisoned outputs untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIIIQQQQ", scalar_form, out_form, k, 0, n, out_stride, base_stride, len(scalars)) + bases + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    stride = 104 if out_form == V.MONT_FLAG else 96
    if rc:
        assert len(blob) == 4
        return rc, b"", b""
    assert len(blob) == 4 + n * (stride + 1)
    return rc, blob[4 : 4 + n * stride], blob[4 + n * stride :]


def run_rows(exe, tmp_path, points, rows, layout="rows", scalar_form=V.WIRE, out_form=V.WIRE):
    buf, out_stride, base_stride = MV.pack(rows, layout)
    return run_program(exe, tmp_path, MV.bases_bytes(points), len(points), buf, len(rows), out_stride, base_stride, scalar_form, out_form)


def test_limits(exe):
    res = subprocess.run([exe, "limits"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert int(res.stdout) == MV.MAX_BASES


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """tuple name -> (points, rows, wire records, flags): computed once, read by every test below."""
    rows = MV.host_rows()
    return {name: (pts, rows) + MV.expected(pts, rows)[:2] for name, pts in MV.tuples()}


@pytest.mark.parametrize("name", [name for name, _ in MV.tuples()])
def test_two_bases_against_pyref(exe, tmp_path, reference, name):
    pts, rows, wire, flags = reference[name]
    rc, got, got_flags = run_rows(exe, tmp_path, pts, rows)
    assert rc == 0
    assert got_flags == flags, name
    assert got == wire, name
    rc, got, got_flags = run_rows(exe, tmp_path, pts, rows, out_form=V.MONT_FLAG)
    assert rc == 0
    assert got_flags == flags, name
    assert got == V.mont_flag_records(wire, flags), name
    assert bytes(got[104 * i + 96] for i in range(len(flags))) == flags  # the record's own flag byte


def test_sums_cancel_with_no_term_zero(reference):
    """The cancelling pairs do what they were chosen for: an identity output whose two terms are both finite, beside a
    neighbour that is not the identity."""
    first = len(MV.host_rows()) - 8 - len(MV.cancelling_rows())
    for name, t in (("G_mG", 0), ("G_negG", 2), ("G_G", 4)):
        pts, rows, _, flags = reference[name]
        for block in range(3):
            i = first + 6 * block + t
            assert flags[i] == 1 and flags[i + 1] == 0, (name, i)
            assert all(R.mul(b, s) is not None for b, s in zip(pts, rows[i])), (name, i)
    pts, rows, _, flags = reference["small3_small3"]
    i = first + 18
    assert flags[i : i + 5] == bytes([1, 1, 0, 1, 1]) and R.mul(pts[0], rows[i][0]) is not None


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(exe, tmp_path, reference, layout):
    """Row-major, column-major and padded rows of the same matrix: the same bytes."""
    pts, rows, wire, flags = reference["G_mG"]
    assert run_rows(exe, tmp_path, pts, rows, layout) == (0, wire, flags)
    pts, rows, wire, flags = reference["order2_GplusT"]
    assert run_rows(exe, tmp_path, pts, rows, layout, out_form=V.MONT_FLAG) == (0, V.mont_flag_records(wire, flags), flags)


@pytest.fixture(scope="module")
def wider():
    """k -> (points, rows, wire, flags) for k = 3 and k = 16: subgroup points, a small-order point, a point outside the
    subgroup and a repeated base among them."""
    b = dict(V.bases())
    three = (R.G, R.mul(R.G, MV.M), b["G_plus_torsion"])
    sixteen = tuple([R.mul(R.G, j + 1) for j in range(12)] + [b["small_3"], b["small_5"], b["torsion"], R.G])
    out = {}
    for pts, rows in ((three, MV.many_rows(3, 20, 0x3B45E5)), (sixteen, MV.many_rows(16, 7, 0x16B45E5))):
        rows = rows + [tuple([0] * len(pts)), tuple([r] * (len(pts) - 1) + [0])]
        out[len(pts)] = (pts, rows) + MV.expected(pts, rows)[:2]
    return out


@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_more_bases(exe, tmp_path, wider, k, layout):
    pts, rows, wire, flags = wider[k]
    assert run_rows(exe, tmp_path, pts, rows, layout) == (0, wire, flags)
    assert 1 in flags and 0 in flags


def test_one_base_is_the_single_base_twin(exe, tmp_path):
    scalars = V.host_scalars()
    for name in ("G", "small_3", "G_plus_torsion"):
        pt = dict(V.bases())[name]
        wire, flags, _ = V.expected(pt, scalars)
        rows = [(s,) for s in scalars]
        for out_form, fname in ((V.WIRE, "wire"), (V.MONT_FLAG, "mont_flag")):
            single = msm.batch_mul_host(V.base_bytes(pt), R.encode_scalars(scalars), fname)
            assert single == (wire if out_form == V.WIRE else V.mont_flag_records(wire, flags), flags)
            assert run_rows(exe, tmp_path, (pt,), rows, "rows", out_form=out_form) == (0,) + single, name
            assert run_rows(exe, tmp_path, (pt,), rows, "padded", out_form=out_form) == (0,) + single, name


def test_library_runs_the_same_twin(reference, wider):
    for name in ("G_mG", "small3_small3", "torsion_G"):
        pts, rows, wire, flags = reference[name]
        for layout in ("rows", "columns"):
            buf = MV.pack(rows, layout)[0]
            assert msm.batch_mul_multi_host(MV.bases_bytes(pts), buf, "wire", layout) == (wire, flags), (name, layout)
        assert msm.batch_mul_multi_host(MV.bases_bytes(pts), MV.pack(rows)[0], "mont_flag") == (V.mont_flag_records(wire, flags), flags), name
    pts, rows, wire, flags = wider[16]
    assert msm.batch_mul_multi_host(MV.bases_bytes(pts), MV.pack(rows, "columns")[0], layout="columns") == (wire, flags)


def test_montgomery_scalars(exe, tmp_path):
    """MSM377_SCALARS_MONT: a 32-byte value v means v 2^-256 mod r, fully reduced -- for EVERY v, also v >= r."""
    values = [0, 1, r - 1, r, r + 1, 2**256 - 1, 2**255] + V.random_scalars(0x5CA1A3, 17)
    rows = list(zip(values[:12], values[12:]))
    reduced = [tuple(v * pow(2**256, -1, r) % r for v in row) for row in rows]
    b = dict(V.bases())
    for pts in ((R.G, R.mul(R.G, MV.M)), (b["G_plus_torsion"], b["small_6"])):
        wire, flags, _ = MV.expected(pts, reduced)
        for layout in ("rows", "columns"):
            assert run_rows(exe, tmp_path, pts, rows, layout, scalar_form=V.MONT) == (0, wire, flags)
        assert run_rows(exe, tmp_path, pts, reduced) == (0, wire, flags)
    assert run_rows(exe, tmp_path, (R.G, R.G), rows, scalar_form=2)[0] == EINVAL  # no such scalar form


# ---- arguments ----
def test_empty_batch(exe, tmp_path):
    two = MV.bases_bytes((R.G, R.G))
    assert msm.batch_mul_multi_host(two, b"") == (b"", b"")
    assert msm.batch_mul_multi_host(two, b"", "mont_flag", "columns") == (b"", b"")
    lib = msm.load_library()
    assert lib.msm377_g1_batch_mul_multi_host(None, 2, None, 0, 64, 32, V.WIRE, None, None) == 0
    assert lib.msm377_g1_batch_mul_multi_host(None, 0, None, 0, 64, 32, V.WIRE, None, None) == EINVAL  # the shape is checked first
    assert run_program(exe, tmp_path, two, 2, b"", 0, 64, 32) == (0, b"", b"")


def test_invalid_arguments_leave_the_outputs_untouched(exe, tmp_path):
    lib = msm.load_library()
    bases = MV.bases_bytes([R.mul(R.G, j + 1) for j in range(17)])
    scalars = R.encode_scalars(list(range(5, 5 + 2 * 17)))
    out, inf = ctypes.create_string_buffer(b"\xa5" * 208), ctypes.create_string_buffer(b"\xa5" * 2)

    def call(b, k, s, out_stride, base_stride, form, o):
        return lib.msm377_g1_batch_mul_multi_host(b, k, s, 2, out_stride, base_stride, form, o, ctypes.addressof(inf))

    o = ctypes.addressof(out)
    assert call(bases, 0, scalars, 64, 32, V.WIRE, o) == EINVAL
    assert call(bases, 17, scalars, 32 * 17, 32, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 0, 32, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 64, 0, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 48, 32, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 64, 48, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 64, 32, V.MONT, o) == EINVAL  # plain mont cannot say "identity"
    assert call(bases, 2, scalars, 64, 32, 3, o) == EINVAL
    assert call(None, 2, scalars, 64, 32, V.WIRE, o) == EINVAL
    assert call(bases, 2, None, 64, 32, V.WIRE, o) == EINVAL
    assert call(bases, 2, scalars, 64, 32, V.WIRE, None) == EINVAL
    noncanonical = bases[:96] + (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little")  # at position 1
    assert call(noncanonical, 2, scalars, 64, 32, V.WIRE, o) == EINVAL
    assert call(noncanonical, 1, scalars, 64, 32, V.WIRE, o) == 0  # position 1 is not part of a k = 1 call
    assert out.raw[:96] == R.encode_result(R.mul(R.G, 5)) and out.raw[96:192] == R.encode_result(R.mul(R.G, 7)) and inf.raw[:2] == b"\0\0"
    ctypes.memset(out, 0xA5, 208)
    ctypes.memset(inf, 0xA5, 2)
    assert call(bases, 16, scalars, 32 * 16, 32, V.WIRE, o) == 0  # the largest k
    exp = [R.mul(R.G, sum((j + 1) * (5 + 16 * i + j) for j in range(16))) for i in range(2)]
    assert out.raw[:192] == b"".join(R.encode_result(p) for p in exp)
    # the same refusals inside the sanitized program, which checks its poisoned outputs itself
    two = bases[:192]
    assert run_program(exe, tmp_path, two, 0, scalars, 2, 64, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, bases, 17, scalars, 2, 32 * 17, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, two, 2, scalars, 2, 48, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, two, 2, scalars, 2, 64, 0)[0] == EINVAL
    assert run_program(exe, tmp_path, noncanonical, 2, scalars, 2, 64, 32)[0] == EINVAL
    assert run_program(exe, tmp_path, two, 2, scalars, 2, 64, 32, out_form=V.MONT)[0] == EINVAL
    with pytest.raises(msm.MsmError) as e:
        msm.batch_mul_multi_host(two, scalars[:128], "mont")
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        msm.batch_mul_multi_host(bases, scalars)  # 17 bases
