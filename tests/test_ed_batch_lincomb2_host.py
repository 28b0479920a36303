"""Edwards-BLS12 pairwise linear combination on the host (include/msm377.h "Edwards-BLS12 pairwise linear combination"):
the host twin csrc/ed_batch_lincomb2_host.hpp.  tests/native/ed_batch_lincomb2_host.cpp is compiled with g++ against the
headers -- once plain and once with the address / undefined-behaviour sanitizers, a stand-alone program both times: nothing
is loaded into python -- and asked for whole runs; the library's msm377_ed_batch_lincomb2_host runs the same header.
Expected values: tests/pyref.py (R.ed_mul, R.ed_add, R.ed_neg) and the reference's own vectors (tests/ed_vectors.py).  CPU
only; the device call: tests/test_ed_batch_lincomb2_gpu.py."""
import ctypes
import itertools
import os
import struct
import subprocess

import pytest

import ed_batch_lincomb2_vectors as LV
import ed_batch_mul_var_vectors as VV
import ed_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ed_batch_lincomb2_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
N = 65  # the pyref case: a wave and one pair, every special class, three relations, the first edge scalars
N_REL = 256  # the smallest case that holds all eight relations


def build(name, *flags):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    cmd = ["g++", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


@pytest.fixture(scope="module")
def exe_san():
    return build("ed_batch_lincomb2_host_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run_program(exe, tmp_path, p, q, a, b, n, strides=(64, 64, 32, 32), place=0):
    """(return code, records) of one run of the host twin inside the stand-alone program, which itself checks that a
    refused call leaves its poisoned output untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<Q6I", n, *strides, place, 0) + p + q + a + b)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    assert len(blob) == 4 + (0 if rc else 64 * n)
    return rc, blob[4:]


@pytest.fixture(scope="module")
def pyref_case():
    ps, qs, as_, bs, relations = LV.case(N)
    return ps, qs, as_, bs, relations, LV.expected(ps, qs, as_, bs)


def relation_block():
    """The pairs at the relation lanes of the 256-pair case, all eight relations twice, with pyref's records."""
    ps, qs, as_, bs, relations = LV.case(N_REL)
    lanes = sorted(relations)
    rows = [(ps[i], qs[i], as_[i], bs[i]) for i in lanes]
    return [relations[i] for i in lanes], rows, b"".join(R.ed_encode_result(LV.combine(*r)) for r in rows)


# ---- the vectors themselves ----
def test_vectors_cover_what_they_claim():
    ps, qs, as_, bs, relations = LV.case(N_REL)
    assert sorted(set(relations.values())) == sorted(LV.RELATIONS)
    assert {(VV.final_carry(a), VV.final_carry(b)) for a, b in zip(as_, bs)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    top = lambda s: (s >> 252) & 15  # noqa: E731
    assert any(VV.final_carry(a) and b >> 252 == 0 for a, b in zip(as_, bs)) and any(VV.final_carry(b) and a >> 252 == 0 for a, b in zip(as_, bs)), top
    names, rows, wire = relation_block()
    for name, (p, q, a, b), k in zip(names, rows, range(len(rows))):
        out = wire[64 * k : 64 * k + 64]
        if name == "Q = [m]P, a + b m = 0":
            assert out == LV.IDENTITY_WIRE and R.ed_mul(p, a) != R.ED_ID and R.ed_mul(q, b) != R.ED_ID
        if name in ("Q = -P, a = b", "a = b = 0", "both the identity"):
            assert out == LV.IDENTITY_WIRE, name


# ---- the host twin against pyref and the reference's vectors ----
def test_twin_against_pyref(exe_san, tmp_path, pyref_case):
    ps, qs, as_, bs, _, wire = pyref_case
    enc = LV.encode(ps, qs, as_, bs)
    assert msm.ed_batch_lincomb2_host(*enc) == wire
    assert run_program(exe_san, tmp_path, *enc, N) == (0, wire)


def test_relations_block(exe_san, tmp_path):
    """All eight relations (Q = +-P, Q = [m]P with a sum of O, order 4 with P + T, both O, zero scalars) through the library
    and through the sanitized stand-alone program."""
    names, rows, wire = relation_block()
    enc = LV.encode(*zip(*rows))
    assert msm.ed_batch_lincomb2_host(*enc) == wire, names
    assert run_program(exe_san, tmp_path, *enc, len(rows)) == (0, wire)


def test_reference_vectors():
    """The reference's MULTIPLY vectors composed: each as one term with the other term's scalar 0 (on either side), and each
    pair of neighbours summed with R.ed_add."""
    mult = list(V.MULTIPLY)
    other = R.ed_mul(R.ED_G, 0xD00E)
    ps, qs, as_, bs, exp = [], [], [], [], []
    for pt, k, res in mult:
        ps += [pt, other]
        qs += [other, pt]
        as_ += [k, 0]
        bs += [0, k]
        exp += [res, res]
    for (pt1, k1, r1), (pt2, k2, r2) in zip(mult, mult[1:] + mult[:1]):
        ps.append(pt1), qs.append(pt2), as_.append(k1), bs.append(k2), exp.append(R.ed_add(r1, r2))
    out = msm.ed_batch_lincomb2_host(*LV.encode(ps, qs, as_, bs))
    assert out == b"".join(R.ed_encode_result(e) for e in exp)


def test_all_sixteen_stride_combinations(exe_san, tmp_path, pyref_case):
    """Every argument as ONE element for all pairs, in every combination, equals the per-pair form on expanded arrays; the
    stand-alone program holds a stride-0 array in an allocation of exactly one element."""
    ps, qs, as_, bs, _, _ = pyref_case
    n = 9
    full = LV.encode(ps[20 : 20 + n], qs[20 : 20 + n], [VV.MASK256] + list(as_[21 : 20 + n]), [R.ED_SUBGROUP + 1] + list(bs[21 : 20 + n]))
    sizes = (64, 64, 32, 32)
    lib = msm.load_library()
    for zero in itertools.product((False, True), repeat=4):
        args = [buf[:size] if z else buf for buf, size, z in zip(full, sizes, zero)]
        expanded = [LV.expand(buf, size, n) if z else buf for buf, size, z in zip(full, sizes, zero)]
        exp = msm.ed_batch_lincomb2_host(*expanded)
        strides = tuple(0 if z else size for size, z in zip(sizes, zero))
        out = ctypes.create_string_buffer(64 * n)
        assert lib.msm377_ed_batch_lincomb2_host(*args, n, *strides, ctypes.addressof(out)) == 0
        assert out.raw == exp, zero
        # the Python form: one element against n > 1 elements elsewhere (four single elements are ONE pair)
        assert msm.ed_batch_lincomb2_host(*args) == (exp[:64] if all(zero) else exp), zero
        if sum(zero) in (1, 4):
            assert run_program(exe_san, tmp_path, *args, n, strides) == (0, exp), zero
    assert exp == LV.expected([ps[20]] * n, [qs[20]] * n, [VV.MASK256] * n, [R.ED_SUBGROUP + 1] * n)  # all four: by pyref


# ---- refusals ----
def test_points_off_the_curve_are_refused_with_array_and_lowest_index(exe_san, tmp_path, pyref_case):
    ps, qs, as_, bs, _, _ = pyref_case
    gx, gy = R.ED_G
    bad, noncanon = LV.off_curve_point(), (gx + R.Q, gy)
    ab = LV.encode(ps, qs, as_, bs)[2:]
    cases = [
        ({7: bad}, {}, "p", 7, "not on the curve"),
        ({}, {N - 1: bad}, "q", N - 1, "not on the curve"),
        ({40: bad}, {7: bad}, "q", 7, "not on the curve"),  # both: the lower index
        ({7: bad}, {40: bad}, "p", 7, "not on the curve"),
        ({9: noncanon}, {9: bad}, "p", 9, "not below q"),  # equal indices: p
        ({}, {0: noncanon, 3: bad}, "q", 0, "not below q"),
    ]
    for in_p, in_q, array, index, text in cases:
        pp, qq = list(ps), list(qs)
        for i, pt in in_p.items():
            pp[i] = pt
        for i, pt in in_q.items():
            qq[i] = pt
        pb, qb = R.ed_encode_points(pp), R.ed_encode_points(qq)
        with pytest.raises(msm.MsmError) as err:
            msm.ed_batch_lincomb2_host(pb, qb, *ab)
        assert (err.value.code, err.value.array, err.value.index) == (EPOINT, array, index) and text in str(err.value), (in_p, in_q)
        assert run_program(exe_san, tmp_path, pb, qb, *ab, N)[0] == EPOINT  # ... with its poisoned output untouched
    # a stride-0 point: ONE record is checked, and it is index 0 of its array
    one_bad = R.ed_encode_points([bad])
    pb = R.ed_encode_points(list(ps))
    for args, array in (((one_bad, pb), "p"), ((pb, one_bad), "q")):
        with pytest.raises(msm.MsmError) as err:
            msm.ed_batch_lincomb2_host(*args, *ab)
        assert (err.value.code, err.value.array, err.value.index) == (EPOINT, array, 0)
    strides = (0, 64, 32, 32)
    assert run_program(exe_san, tmp_path, one_bad, pb, *ab, N, strides)[0] == EPOINT


# ---- in place ----
def test_in_place_and_fold_in_place(exe_san, tmp_path, pyref_case):
    ps, qs, as_, bs, _, wire = pyref_case
    pb, qb, ab, bb = LV.encode(ps, qs, as_, bs)
    assert run_program(exe_san, tmp_path, pb, qb, ab, bb, N, place=1) == (0, wire)  # out == p
    assert run_program(exe_san, tmp_path, pb, qb, ab, bb, N, place=2) == (0, wire)  # out == q
    assert run_program(exe_san, tmp_path, pb, qb, ab, bb, N, place=3) == (0, wire)  # p = G, q = G + N records, out = G
    lib = msm.load_library()
    g = ctypes.create_string_buffer(pb + qb, 128 * N)
    base = ctypes.addressof(g)
    assert lib.msm377_ed_batch_lincomb2_host(ctypes.c_char_p(base), ctypes.c_char_p(base + 64 * N), ab, bb, N, 64, 64, 32, 32, base) == 0
    assert g.raw == wire + qb
    same = ctypes.create_string_buffer(pb, 64 * N)  # p == q as the same pointer: [a + b]P
    out = ctypes.create_string_buffer(64 * N)
    assert lib.msm377_ed_batch_lincomb2_host(same, same, ab, bb, N, 64, 64, 32, 32, ctypes.addressof(out)) == 0
    assert out.raw == msm.ed_batch_lincomb2_host(pb, pb, ab, bb)
    assert out.raw[64 * 20 : 64 * 30] == b"".join(R.ed_encode_result(R.ed_mul(ps[i], as_[i] + bs[i])) for i in range(20, 30))


def test_arguments():
    lib = msm.load_library()
    pb, qb, ab, bb = LV.encode([R.ED_G, R.ed_mul(R.ED_G, 5)], [R.ed_mul(R.ED_G, 7), R.ED_G], [3, 4], [1, 2])
    exp = R.ed_encode_points([R.ed_mul(R.ED_G, 10), R.ed_mul(R.ED_G, 22)])
    out = ctypes.create_string_buffer(b"\xa5" * 144, 144)
    o = ctypes.addressof(out)
    call = lib.msm377_ed_batch_lincomb2_host
    good = (64, 64, 32, 32)
    for pos in range(4):
        for stride in (1, 4, 16, 31, 33, 96, 32 if pos < 2 else 64):
            strides = list(good)
            strides[pos] = stride
            assert call(pb, qb, ab, bb, 2, *strides, o) == EINVAL, (pos, stride)
    for hole in range(4):
        args = [pb, qb, ab, bb]
        args[hole] = None
        assert call(*args, 2, *good, o) == EINVAL, hole
    assert call(pb, qb, ab, bb, 2, *good, None) == EINVAL
    assert call(None, None, None, None, 0, 64, 64, 16, 32, None) == EINVAL  # the strides are checked first
    assert call(None, None, None, None, 0, *good, None) == 0 and call(None, None, None, None, 0, 0, 0, 0, 0, None) == 0  # n = 0
    one = ctypes.create_string_buffer(pb[:64], 64)  # the outputs over the ONE point of a stride-0 array
    assert call(one, qb, ab, bb, 2, 0, 64, 32, 32, ctypes.addressof(one)) == EINVAL
    assert call(pb, one, ab, bb, 2, 64, 0, 32, 32, ctypes.addressof(one)) == EINVAL
    assert one.raw == pb[:64] and out.raw == b"\xa5" * 144
    assert call(pb, qb, ab, bb, 2, *good, o) == 0
    assert out.raw[:128] == exp and out.raw[128:] == b"\xa5" * 16
    assert msm.ed_batch_lincomb2_host(b"", b"", b"", b"") == b""
    with pytest.raises(ValueError):
        msm.ed_batch_lincomb2_host(pb, qb, ab, bb + bb)
    with pytest.raises(ValueError):
        msm.ed_batch_lincomb2_host(pb + pb + pb, qb, ab, bb)  # 6 against 2: neither n nor one
