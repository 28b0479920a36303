"""Pairwise linear combination on the host (include/msm377.h "pairwise linear combination"): the host twin
csrc/batch_lincomb2_host.hpp, the yardstick of the device call.  tests/native/batch_lincomb2_host.cpp is compiled with g++
and the address / undefined-behaviour sanitizers against the headers (a stand-alone program: nothing is loaded into
python); the library's msm377_g1_batch_lincomb2_host runs the same header.  Expected values: tests/pyref.py alone.  CPU
only; the device call: tests/test_batch_lincomb2_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import batch_lincomb2_vectors as LV
import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "batch_lincomb2_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER
FORM_NAMES = {V.WIRE: "wire", V.MONT: "mont", V.MONT_FLAG: "mont_flag"}


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "batch_lincomb2_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, p: bytes, q: bytes, a: bytes, b: bytes, point_form=V.WIRE, scalar_form=V.WIRE, out_form=V.WIRE, a_stride=32, b_stride=32):
    """(return code, records, flags) of one run of the host twin inside the sanitized program."""
    n = len(p) // (104 if point_form == V.MONT_FLAG else 96)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIIIIIQ", point_form, scalar_form, out_form, a_stride, b_stride, 0, n) + p + q + a + b)
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


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """name -> (base bytes x n, G bytes x n, a bytes, b bytes, records of [a]B + [b]G, records of [a]G + [b]B): every base
    of V.bases() as P with Q = G, and the other way round."""
    pool = LV.host_scalars()
    n = len(pool)
    a, b = pool, [pool[7 * i % n] for i in range(n)]  # (0, 0) in front
    assert (a[1], a[5]) == (1, r - 1)
    b[1], b[5] = r - 1, 1  # for the base G: G + [r - 1]G = O, a general addition of opposite points
    g = [R.G] * n
    out = {}
    for name, pt in V.bases():
        out[name] = (V.base_bytes(pt) * n, V.base_bytes(R.G) * n, R.encode_scalars(a), R.encode_scalars(b), LV.expected([pt] * n, g, a, b), LV.expected(g, [pt] * n, a, b))
    return out


@pytest.mark.parametrize("name", [name for name, _ in V.bases()])
def test_host_twin_against_pyref(exe, tmp_path, reference, name):
    base, gen, a, b, as_p, as_q = reference[name]
    for p, q, (wire, flags) in ((base, gen, as_p), (gen, base, as_q)):
        rc, got, got_flags = run_program(exe, tmp_path, p, q, a, b)
        assert rc == 0
        assert got_flags == flags, name
        assert got == wire, name
        rc, got, got_flags = run_program(exe, tmp_path, p, q, a, b, out_form=V.MONT_FLAG)
        assert rc == 0
        assert got_flags == flags, name
        assert got == V.mont_flag_records(wire, flags), name
    assert 1 in as_p[1]  # a = b = 0 at least


def test_library_runs_the_same_twin(reference):
    for name in ("G", "small_3", "small_5", "G_plus_torsion"):
        base, gen, a, b, as_p, as_q = reference[name]
        assert msm.batch_lincomb2_host(base, gen, a, b) == as_p, name
        assert msm.batch_lincomb2_host(gen, base, a, b) == as_q, name
        assert msm.batch_lincomb2_host(base, gen, a, b, "mont_flag") == (V.mont_flag_records(*as_p), as_p[1]), name


@pytest.fixture(scope="module")
def mixed():
    """Two arrays that interleave the exceptional points with random subgroup points, with Q = P, Q = -P and a result of
    O among them; flagged P, flagged Q and both for the mont_flag form."""
    n = 61
    p = list(VV.mixed_points(n, period=3))
    q = list(VV.mixed_points(n, seed=0x4B12ED, period=4))
    pool = LV.host_scalars()
    a = [pool[(5 * i + 1) % len(pool)] for i in range(n)]
    b = [pool[(3 * i + 2) % len(pool)] for i in range(n)]
    q[5], b[5] = p[5], a[5]
    q[10], b[10] = R.neg(p[10]), a[10]
    q[11], a[11], b[11] = R.mul(p[11], 77), (-77 * 0xABCDEF) % r, 0xABCDEF
    assert p[11] not in (q[11], R.neg(q[11]))
    fp, fq = (0, 7, 30), (7, 31, n - 1)
    plain, with_flags = LV.expected(p, q, a, b), LV.expected(p, q, a, b, fp, fq)
    assert plain[1][10] == 1 and plain[1][11] == 1
    return p, q, a, b, fp, fq, plain, with_flags


@pytest.mark.parametrize("point_form", [V.WIRE, V.MONT, V.MONT_FLAG])
@pytest.mark.parametrize("out_form", [V.WIRE, V.MONT_FLAG])
def test_mixed_array_in_every_form(exe, tmp_path, mixed, point_form, out_form):
    p, q, a, b, fp, fq, plain, with_flags = mixed
    if point_form == V.WIRE:
        pb, qb, (wire, flags) = R.encode_points(p), R.encode_points(q), plain
    elif point_form == V.MONT:
        pb, qb, (wire, flags) = VV.mont_records(p), VV.mont_records(q), plain
    else:  # flagged records hold garbage coordinates: never interpreted
        pb, qb, (wire, flags) = VV.mont_records(p, True, fp), VV.mont_records(q, True, fq), with_flags
        assert flags[7] == 1  # both flagged
    exp = LV.out_records(wire, flags, out_form)
    ab, bb = R.encode_scalars(a), R.encode_scalars(b)
    rc, got, got_flags = run_program(exe, tmp_path, pb, qb, ab, bb, point_form, V.WIRE, out_form)
    assert rc == 0 and got_flags == flags
    assert got == exp
    assert msm.batch_lincomb2_host(pb, qb, ab, bb, FORM_NAMES[out_form], FORM_NAMES[point_form]) == (exp, flags)


def test_montgomery_scalars(exe, tmp_path, mixed):
    """MSM377_SCALARS_MONT: a 32-byte value v means v 2^-256 mod r, fully reduced -- for EVERY v, also v >= r; both scalars."""
    n = 20
    p, q = list(mixed[0])[:n], list(mixed[1])[:n]
    va = (VV.MONT_SCALAR_VALUES + V.random_scalars(0x5CA1A4, n))[:n]
    vb = (V.random_scalars(0x5CA1A5, n - 7) + VV.MONT_SCALAR_VALUES)[:n]
    exp = LV.expected(p, q, VV.mont_scalars(va), VV.mont_scalars(vb))
    pb, qb = R.encode_points(p), R.encode_points(q)
    rc, got, got_flags = run_program(exe, tmp_path, pb, qb, R.encode_scalars(va), R.encode_scalars(vb), V.WIRE, V.MONT, V.WIRE)
    assert rc == 0 and (got, got_flags) == exp
    assert msm.batch_lincomb2_host(pb, qb, R.encode_scalars(va), R.encode_scalars(vb), scalar_form="mont") == exp
    assert msm.batch_lincomb2_host(pb, qb, R.encode_scalars(VV.mont_scalars(va)), R.encode_scalars(VV.mont_scalars(vb))) == exp


@pytest.mark.parametrize("a_stride,b_stride", [(32, 32), (0, 32), (32, 0), (0, 0)])
def test_strides(exe, tmp_path, mixed, a_stride, b_stride):
    n = 20
    p, q = list(mixed[0])[:n], list(mixed[1])[:n]
    a = list(mixed[2])[:n] if a_stride else [2**256 - 1]
    b = list(mixed[3])[:n] if b_stride else [0xD0E5_0F7A_B1E5]
    exp = LV.expected(p, q, a, b)
    pb, qb, ab, bb = R.encode_points(p), R.encode_points(q), R.encode_scalars(a), R.encode_scalars(b)
    rc, got, got_flags = run_program(exe, tmp_path, pb, qb, ab, bb, a_stride=a_stride, b_stride=b_stride)
    assert rc == 0 and (got, got_flags) == exp
    assert msm.batch_lincomb2_host(pb, qb, ab, bb) == exp  # 32 bytes for 20 pairs: stride 0
    assert msm.batch_lincomb2_host(pb, qb, ab * (1 if a_stride else n), bb * (1 if b_stride else n)) == exp


def test_order_three_point_is_not_the_identity():
    """(0, 1) is a point of order 3 AND the wire encoding of the identity: the flag array tells them apart."""
    three, g = V.base_bytes((0, 1)), V.base_bytes(R.G)
    recs, flags = msm.batch_lincomb2_host(three * 3, g * 3, R.encode_scalars([1, 0, 3]), R.encode_scalars([0, 0, 0]))
    assert recs == V.IDENTITY_WIRE * 3 and flags == b"\x00\x01\x01"
    recs, flags = msm.batch_lincomb2_host(g, three, R.encode_scalars([0]), R.encode_scalars([1]), "mont_flag")
    assert recs == V.mont_flag_records(V.IDENTITY_WIRE, b"\x00") and flags == b"\x00"


# ---- arguments ----
def test_empty_batch():
    assert msm.batch_lincomb2_host(b"", b"", b"", b"") == (b"", b"")
    assert msm.batch_lincomb2_host(b"", b"", b"", b"", "mont_flag", "mont_flag", "mont") == (b"", b"")
    lib = msm.load_library()
    assert lib.msm377_g1_batch_lincomb2_host(None, None, V.WIRE, None, None, V.WIRE, 0, 32, 0, V.WIRE, None, None) == 0


def test_invalid_arguments_leave_the_outputs_untouched(exe, tmp_path):
    lib = msm.load_library()
    p, q = R.encode_points([R.G, R.FIXED_BASE]), R.encode_points([R.FIXED_BASE, R.G])
    a, b = R.encode_scalars([5, 6]), R.encode_scalars([7, 8])
    out, inf = ctypes.create_string_buffer(b"\xa5" * 208), ctypes.create_string_buffer(b"\xa5" * 2)
    o = ctypes.addressof(out)

    def call(p=p, q=q, pf=V.WIRE, a=a, b=b, sf=V.WIRE, n=2, sa=32, sb=32, form=V.WIRE, o=o):
        return lib.msm377_g1_batch_lincomb2_host(p, q, pf, a, b, sf, n, sa, sb, form, o, ctypes.addressof(inf))

    assert call() == 0  # the call these vary
    assert out.raw[:192] == R.encode_points([R.add(R.mul(R.G, 5), R.mul(R.FIXED_BASE, 7)), R.add(R.mul(R.FIXED_BASE, 6), R.mul(R.G, 8))])
    ctypes.memset(out, 0xA5, 208)
    ctypes.memset(inf, 0xA5, 2)
    assert call(form=V.MONT) == EINVAL  # plain mont cannot say "identity"
    assert call(form=3) == EINVAL
    assert call(n=0, form=V.MONT) == EINVAL
    assert call(pf=3) == EINVAL
    assert call(sf=2) == EINVAL
    for stride in (1, 4, 16, 31, 33, 64, 0xFFFFFFFF):
        assert call(sa=stride) == EINVAL, stride
        assert call(sb=stride) == EINVAL, stride
        assert call(sa=0, sb=stride) == EINVAL, stride
    for name in ("p", "q", "a", "b", "o"):
        assert call(**{name: None}) == EINVAL, name
    assert out.raw[:208] == b"\xa5" * 208 and inf.raw[:2] == b"\xa5" * 2
    rc, _, _ = run_program(exe, tmp_path, p, q, a, b, b_stride=8)
    assert rc == EINVAL
    with pytest.raises(msm.MsmError) as e:
        msm.batch_lincomb2_host(p, q, a, b, "mont")
    assert e.value.code == EINVAL
