"""Fixed-base batch multiplication on the host (include/msm377.h "fixed-base batch multiplication"): the signed window
recode of csrc/batch_mul_recode.hpp -- the one definition the kernel, the host twin and this test share -- and the host
twin csrc/batch_mul_host.hpp.  tests/native/batch_mul_host.cpp is compiled with g++ and the address / undefined-behaviour
sanitizers against the headers (a stand-alone program: nothing is loaded into python) and asked for recodes and whole
runs; the library's msm377_g1_batch_mul_host runs the same header.  Expected values: tests/pyref.py alone.  CPU only; the
device call: tests/test_batch_mul_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "batch_mul_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "batch_mul_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, base: bytes, scalars: bytes, scalar_form=V.WIRE, out_form=V.WIRE):
    """(return code, records, flags) of one run of the host twin inside the sanitized program."""
    n = len(scalars) // 32
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIQ", scalar_form, out_form, n) + base + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    stride = 104 if out_form == V.MONT_FLAG else 96
    if rc:
        assert len(blob) == 4
        return rc, b"", b""
    assert len(blob) == 4 + n * (stride + 1)
    return rc, blob[4 : 4 + n * stride], blob[4 + n * stride :]


# ---- recode ----
def test_widths(exe):
    res = subprocess.run([exe, "widths"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    host, narrow, wide, _ = (int(x) for x in res.stdout.split())
    assert host == V.HOST_WIDTH and (narrow, wide) == V.WIDTHS


@pytest.mark.parametrize("c", sorted({V.HOST_WIDTH, *V.WIDTHS, 5, 13}))  # 5 and 13 do not divide 256: a short top window
def test_recode(exe, c):
    scalars = V.EDGE + V.pattern_scalars(c) + V.random_scalars(0x2EC0DE + c, 64)
    res = subprocess.run([exe, "recode", str(c)] + ["%x" % s for s in scalars], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(scalars)
    W = (256 + c - 1) // c
    for s, line in zip(scalars, lines):
        vals = [int(x) for x in line.split()]
        digits, carry = vals[:-1], vals[-1]
        assert len(digits) == W and carry in (0, 1), (c, hex(s))
        assert all(abs(d) <= 1 << (c - 1) for d in digits), (c, hex(s), digits)
        assert all(d != -(1 << (c - 1)) for d in digits), (c, hex(s))  # +2^(c-1) is a digit, -2^(c-1) is not
        assert sum(d << (c * w) for w, d in enumerate(digits)) + (carry << (c * W)) == s, (c, hex(s), digits, carry)
    if 256 % c == 0:  # the ripple pattern: digit -1 at the bottom, zeros above it, the carry out of the top
        vals = [int(x) for x in lines[len(V.EDGE) + 2].split()]
        assert vals == [-1] + [0] * (W - 1) + [1]


# ---- the device's chunk inversion (csrc/fp_inverse.hpp), run on the CPU ----
def test_binary_euclid_inversion(exe):
    """a^-1 for the smallest and largest residues, powers of two around the limb and word boundaries (long runs of
    halvings), values that end the walk early and late, and 64 random residues."""
    values = [1, 2, 3, R.P - 1, R.P - 2, (R.P - 1) // 2, (R.P + 1) // 2, 2**376, 2**376 - 1, 2**29, 2**32 - 1, 2**348 + 1, R.GX, R.GY]
    values += [2**k for k in (28, 31, 32, 58, 64, 200, 375)]
    g = R.splitmix64(0x1AE3A)
    for _ in range(64):
        values.append(sum(next(g) << (64 * k) for k in range(6)) % R.P or 1)
    res = subprocess.run([exe, "inverse"] + ["%x" % v for v in values], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    got = [int(line, 16) for line in res.stdout.split()]
    assert got == [pow(v, -1, R.P) for v in values]


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """name -> (base bytes, scalar bytes, wire records, flags): computed once, read by every test below."""
    scalars = V.host_scalars()
    out = {}
    for name, pt in V.bases():
        wire, flags, _ = V.expected(pt, scalars)
        out[name] = (V.base_bytes(pt), R.encode_scalars(scalars), wire, flags)
    return out


@pytest.mark.parametrize("name", [name for name, _ in V.bases()])
def test_host_twin_against_pyref(exe, tmp_path, reference, name):
    base, scalars, wire, flags = reference[name]
    rc, got, got_flags = run_program(exe, tmp_path, base, scalars, V.WIRE, V.WIRE)
    assert rc == 0
    assert got_flags == flags, name
    assert got == wire, name
    rc, got, got_flags = run_program(exe, tmp_path, base, scalars, V.WIRE, V.MONT_FLAG)
    assert rc == 0
    assert got_flags == flags, name
    assert got == V.mont_flag_records(wire, flags), name
    assert bytes(got[104 * i + 96] for i in range(len(flags))) == flags  # the record's own flag byte
    assert 1 in flags  # every list holds identity outputs (scalar 0 at least)


def test_library_runs_the_same_twin(reference):
    for name in ("G", "small_3", "small_5", "G_plus_torsion"):
        base, scalars, wire, flags = reference[name]
        assert msm.batch_mul_host(base, scalars) == (wire, flags), name
        assert msm.batch_mul_host(base, scalars, "mont_flag") == (V.mont_flag_records(wire, flags), flags), name


def test_order_three_point_is_not_the_identity():
    """(0, 1) is a point of order 3 AND the wire encoding of the identity: the flag array tells them apart."""
    base = V.base_bytes((0, 1))
    scalars = [0, 1, 2, 3, 4, 6, r, r + 1, 2**256 - 1]
    recs, flags = msm.batch_mul_host(base, R.encode_scalars(scalars))
    for i, s in enumerate(scalars):
        pt = R.mul((0, 1), s)
        assert recs[96 * i : 96 * i + 96] == R.encode_result(pt), s
        assert flags[i] == (1 if pt is None else 0), s
    assert recs[96:192] == V.IDENTITY_WIRE and flags[1] == 0  # [1](0, 1): the identity's bytes, flag 0
    assert recs[0:96] == V.IDENTITY_WIRE and flags[0] == 1


# ---- arguments ----
def test_empty_batch():
    assert msm.batch_mul_host(V.base_bytes(R.G), b"") == (b"", b"")
    assert msm.batch_mul_host(V.base_bytes(R.G), b"", "mont_flag") == (b"", b"")
    lib = msm.load_library()
    assert lib.msm377_g1_batch_mul_host(None, None, 0, V.WIRE, None, None) == 0


def test_invalid_arguments_leave_the_outputs_untouched():
    lib = msm.load_library()
    base, scalars = V.base_bytes(R.G), R.encode_scalars([5, 6])
    out, inf = ctypes.create_string_buffer(b"\xa5" * 208), ctypes.create_string_buffer(b"\xa5" * 2)

    def call(b, s, n, form, o):
        return lib.msm377_g1_batch_mul_host(b, s, n, form, o, ctypes.addressof(inf))

    assert call(base, scalars, 2, V.MONT, ctypes.addressof(out)) == EINVAL  # plain mont cannot say "identity"
    assert call(base, scalars, 2, 3, ctypes.addressof(out)) == EINVAL
    assert call(base, scalars, 2, 0xFFFFFFFF, ctypes.addressof(out)) == EINVAL
    assert call(None, scalars, 2, V.WIRE, ctypes.addressof(out)) == EINVAL
    assert call(base, None, 2, V.WIRE, ctypes.addressof(out)) == EINVAL
    assert call(base, scalars, 2, V.WIRE, None) == EINVAL
    noncanonical = (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little")
    assert call(noncanonical, scalars, 2, V.WIRE, ctypes.addressof(out)) == EINVAL
    assert out.raw[:208] == b"\xa5" * 208 and inf.raw[:2] == b"\xa5" * 2
    with pytest.raises(msm.MsmError) as e:
        msm.batch_mul_host(base, scalars, "mont")
    assert e.value.code == EINVAL


def test_montgomery_scalars(exe, tmp_path):
    """MSM377_SCALARS_MONT: a 32-byte value v means v 2^-256 mod r, fully reduced -- for EVERY v, also v >= r."""
    values = [0, 1, r - 1, r, r + 1, 2**256 - 1, 2**255] + V.random_scalars(0x5CA1A2, 24)
    reduced = [v * pow(2**256, -1, r) % r for v in values]
    for name in ("G", "G_plus_torsion"):
        pt = dict(V.bases())[name]
        wire, flags, _ = V.expected(pt, reduced)
        rc, got, got_flags = run_program(exe, tmp_path, V.base_bytes(pt), R.encode_scalars(values), V.MONT, V.WIRE)
        assert rc == 0 and (got, got_flags) == (wire, flags), name
        rc, got, got_flags = run_program(exe, tmp_path, V.base_bytes(pt), R.encode_scalars(reduced), V.WIRE, V.WIRE)
        assert rc == 0 and (got, got_flags) == (wire, flags), name
    rc, _, _ = run_program(exe, tmp_path, V.base_bytes(R.G), R.encode_scalars(values), 2, V.WIRE)  # no such scalar form
    assert rc == EINVAL
