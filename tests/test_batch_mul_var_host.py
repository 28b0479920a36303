"""Variable-base batch multiplication on the host (include/msm377.h "variable-base batch multiplication"): the nibble
packing of csrc/batch_mul_var_recode.hpp -- what the hot kernel walks -- and the host twin csrc/batch_mul_var_host.hpp,
the yardstick of the device call.  tests/native/batch_mul_var_host.cpp is compiled with g++ and the address /
undefined-behaviour sanitizers against the headers (a stand-alone program: nothing is loaded into python); the
library's msm377_g1_batch_mul_var_host runs the same header.  Expected values: tests/pyref.py alone.  CPU only; the device
call: tests/test_batch_mul_var_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "batch_mul_var_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER
FORM_NAMES = {V.WIRE: "wire", V.MONT: "mont", V.MONT_FLAG: "mont_flag"}


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "batch_mul_var_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, points: bytes, scalars: bytes, point_form=V.WIRE, scalar_form=V.WIRE, out_form=V.WIRE, stride=32):
    """(return code, records, flags) of one run of the host twin inside the sanitized program."""
    n = len(points) // (104 if point_form == V.MONT_FLAG else 96)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIIIQ", point_form, scalar_form, out_form, stride, n) + points + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    out_stride = 104 if out_form == V.MONT_FLAG else 96
    if rc:
        assert len(blob) == 4
        return rc, b"", b""
    assert len(blob) == 4 + n * (out_stride + 1)
    return rc, blob[4 : 4 + n * out_stride], blob[4 + n * out_stride :]


# ---- the packed digits ----
def test_nibble_packing(exe):
    """Unpacked from the top, the packed array hands out bm_digit's digits and carry: sum d_w 16^w + carry 2^256 == s."""
    scalars = V.EDGE + V.pattern_scalars(4) + V.window_scalars(4) + V.random_scalars(0x9AC4ED, 64)
    res = subprocess.run([exe, "pack"] + ["%x" % s for s in scalars], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(scalars)
    for s, line in zip(scalars, lines):
        packed, plain = ([int(x) for x in part.split()] for part in line.split("|"))
        top_down, carry = packed[:-1], packed[-1]
        assert len(top_down) == 64 and carry in (0, 1), hex(s)
        digits = top_down[::-1]
        assert digits + [carry] == plain, hex(s)
        assert all(-7 <= d <= 8 for d in digits), (hex(s), digits)
        assert sum(d << (4 * w) for w, d in enumerate(digits)) + (carry << 256) == s, (hex(s), digits, carry)
    ripple = [int(x) for x in lines[len(V.EDGE) + 2].split("|")[0].split()]  # 0xff..f: -1 at the bottom, the carry out of the top
    assert ripple == [0] * 63 + [-1, 1]


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """name -> (point bytes, scalar bytes, wire records, flags): every base of V.bases() as the point of every output."""
    scalars = V.host_scalars()
    out = {}
    for name, pt in V.bases():
        wire, flags, _ = V.expected(pt, scalars)
        out[name] = (V.base_bytes(pt) * len(scalars), R.encode_scalars(scalars), wire, flags)
    return out


@pytest.mark.parametrize("name", [name for name, _ in V.bases()])
def test_host_twin_against_pyref(exe, tmp_path, reference, name):
    points, scalars, wire, flags = reference[name]
    rc, got, got_flags = run_program(exe, tmp_path, points, scalars)
    assert rc == 0
    assert got_flags == flags, name
    assert got == wire, name
    rc, got, got_flags = run_program(exe, tmp_path, points, scalars, out_form=V.MONT_FLAG)
    assert rc == 0
    assert got_flags == flags, name
    assert got == V.mont_flag_records(wire, flags), name
    assert 1 in flags  # every list holds identity outputs (scalar 0 at least)


def test_library_runs_the_same_twin(reference):
    for name in ("G", "small_3", "small_5", "G_plus_torsion"):
        points, scalars, wire, flags = reference[name]
        assert msm.batch_mul_var_host(points, scalars) == (wire, flags), name
        assert msm.batch_mul_var_host(points, scalars, "mont_flag") == (V.mont_flag_records(wire, flags), flags), name


@pytest.fixture(scope="module")
def mixed():
    """One array that interleaves the exceptional points with random subgroup points; scalars cycle the host list."""
    n = 61
    points = list(VV.mixed_points(n, period=3))
    pool = V.host_scalars()
    scalars = [pool[(5 * i + 1) % len(pool)] for i in range(n)]
    flagged = (0, 7, 30, n - 1)
    wire, flags = VV.expected(points, scalars)
    wire_f, flags_f = VV.expected(points, scalars, flagged)
    return points, scalars, flagged, (wire, flags), (wire_f, flags_f)


@pytest.mark.parametrize("point_form", [V.WIRE, V.MONT, V.MONT_FLAG])
@pytest.mark.parametrize("out_form", [V.WIRE, V.MONT_FLAG])
def test_mixed_array_in_every_form(exe, tmp_path, mixed, point_form, out_form):
    points, scalars, flagged, plain, with_flags = mixed
    if point_form == V.WIRE:
        buf, (wire, flags) = R.encode_points(points), plain
    elif point_form == V.MONT:
        buf, (wire, flags) = VV.mont_records(points), plain
    else:  # flagged records hold garbage coordinates: never interpreted
        buf, (wire, flags) = VV.mont_records(points, True, flagged), with_flags
        assert all(flags[i] == 1 for i in flagged)
    exp = wire if out_form == V.WIRE else V.mont_flag_records(wire, flags)
    sbuf = R.encode_scalars(scalars)
    rc, got, got_flags = run_program(exe, tmp_path, buf, sbuf, point_form, V.WIRE, out_form)
    assert rc == 0 and got_flags == flags
    assert got == exp
    assert msm.batch_mul_var_host(buf, sbuf, FORM_NAMES[out_form], FORM_NAMES[point_form]) == (exp, flags)


def test_montgomery_scalars(exe, tmp_path, mixed):
    """MSM377_SCALARS_MONT: a 32-byte value v means v 2^-256 mod r, fully reduced -- for EVERY v, also v >= r."""
    points = list(mixed[0])[:24]
    values = (VV.MONT_SCALAR_VALUES + V.random_scalars(0x5CA1A3, 24))[:24]
    wire, flags = VV.expected(points, VV.mont_scalars(values))
    buf = R.encode_points(points)
    rc, got, got_flags = run_program(exe, tmp_path, buf, R.encode_scalars(values), V.WIRE, V.MONT, V.WIRE)
    assert rc == 0 and (got, got_flags) == (wire, flags)
    assert msm.batch_mul_var_host(buf, R.encode_scalars(values), scalar_form="mont") == (wire, flags)
    assert msm.batch_mul_var_host(buf, R.encode_scalars(VV.mont_scalars(values))) == (wire, flags)


@pytest.mark.parametrize("scalar", [2**256 - 1, 0, 0xD0E5_0F7A_B1E5])
def test_one_scalar_for_all_points(exe, tmp_path, mixed, scalar):
    points = list(mixed[0])[:20]
    buf, sbuf = R.encode_points(points), R.encode_scalars([scalar])
    wire, flags = VV.expected(points, [scalar])
    rc, got, got_flags = run_program(exe, tmp_path, buf, sbuf, stride=0)
    assert rc == 0 and (got, got_flags) == (wire, flags)
    assert msm.batch_mul_var_host(buf, sbuf) == (wire, flags)  # 32 bytes for 20 points: stride 0
    assert msm.batch_mul_var_host(buf, sbuf * 20) == (wire, flags)


def test_order_three_point_is_not_the_identity():
    """(0, 1) is a point of order 3 AND the wire encoding of the identity: the flag array tells them apart."""
    recs, flags = msm.batch_mul_var_host(V.base_bytes((0, 1)) * 3, R.encode_scalars([0, 1, 3]))
    assert recs == V.IDENTITY_WIRE * 3 and flags == b"\x01\x00\x01"


# ---- arguments ----
def test_empty_batch():
    assert msm.batch_mul_var_host(b"", b"") == (b"", b"")
    assert msm.batch_mul_var_host(b"", b"", "mont_flag", "mont_flag", "mont") == (b"", b"")
    lib = msm.load_library()
    assert lib.msm377_g1_batch_mul_var_host(None, V.WIRE, None, V.WIRE, 0, 32, V.WIRE, None, None) == 0
    assert lib.msm377_g1_batch_mul_var_host(None, V.WIRE, None, V.WIRE, 0, 0, V.MONT_FLAG, None, None) == 0


def test_invalid_arguments_leave_the_outputs_untouched(exe, tmp_path):
    lib = msm.load_library()
    points, scalars = R.encode_points([R.G, R.FIXED_BASE]), R.encode_scalars([5, 6])
    out, inf = ctypes.create_string_buffer(b"\xa5" * 208), ctypes.create_string_buffer(b"\xa5" * 2)

    def call(p, pf, s, sf, n, stride, form, o):
        return lib.msm377_g1_batch_mul_var_host(p, pf, s, sf, n, stride, form, o, ctypes.addressof(inf))

    o = ctypes.addressof(out)
    assert call(points, V.WIRE, scalars, V.WIRE, 2, 32, V.WIRE, o) == 0  # the call these vary
    assert out.raw[:192] == R.encode_points([R.mul(R.G, 5), R.mul(R.FIXED_BASE, 6)])
    ctypes.memset(out, 0xA5, 208)
    ctypes.memset(inf, 0xA5, 2)
    assert call(points, V.WIRE, scalars, V.WIRE, 2, 32, V.MONT, o) == EINVAL  # plain mont cannot say "identity"
    assert call(points, V.WIRE, scalars, V.WIRE, 2, 32, 3, o) == EINVAL
    assert call(points, V.WIRE, scalars, V.WIRE, 0, 32, V.MONT, o) == EINVAL
    assert call(points, 3, scalars, V.WIRE, 2, 32, V.WIRE, o) == EINVAL
    assert call(points, V.WIRE, scalars, 2, 2, 32, V.WIRE, o) == EINVAL
    for stride in (1, 4, 16, 31, 33, 64, 0xFFFFFFFF):
        assert call(points, V.WIRE, scalars, V.WIRE, 2, stride, V.WIRE, o) == EINVAL, stride
    assert call(None, V.WIRE, scalars, V.WIRE, 2, 32, V.WIRE, o) == EINVAL
    assert call(points, V.WIRE, None, V.WIRE, 2, 32, V.WIRE, o) == EINVAL
    assert call(points, V.WIRE, scalars, V.WIRE, 2, 32, V.WIRE, None) == EINVAL
    assert out.raw[:208] == b"\xa5" * 208 and inf.raw[:2] == b"\xa5" * 2
    rc, _, _ = run_program(exe, tmp_path, points, scalars, stride=8)
    assert rc == EINVAL
    with pytest.raises(msm.MsmError) as e:
        msm.batch_mul_var_host(points, scalars, "mont")
    assert e.value.code == EINVAL
