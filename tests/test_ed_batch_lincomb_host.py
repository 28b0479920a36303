"""Edwards-BLS12 k-term linear combination on the host (include/msm377.h "Edwards-BLS12 k-term linear combination"): the host
twin csrc/ed_batch_lincomb_host.hpp.  tests/native/ed_batch_lincomb_host.cpp is compiled with g++ against the headers -- once
plain and once with the address / undefined-behaviour sanitizers, a stand-alone program both times: nothing is loaded into
python -- and asked for whole runs; the library's msm377_ed_batch_lincomb_host runs the same header.  Expected values:
tests/pyref.py (R.ed_mul, R.ed_add, R.ed_neg) and the older twins for k = 1 and k = 2.  CPU only; the device call:
tests/test_ed_batch_lincomb_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import ed_batch_lincomb_vectors as KV
import ed_batch_mul_var_vectors as VV
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ed_batch_lincomb_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
N, K = 33, 3  # the pyref case: 99 terms in all
N_REL = 256  # the smallest case that holds the whole relations block


def build(name, *flags):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    cmd = ["g++", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


@pytest.fixture(scope="module")
def exe_plain():
    return build("ed_batch_lincomb_host_plain", "-O2")


@pytest.fixture(scope="module")
def exe_san():
    return build("ed_batch_lincomb_host_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def run_program(exe, tmp_path, points, scalars, n, strides=None, place=0):
    """(return code, records) of one run of the host twin inside the stand-alone program, which itself checks that a
    refused call leaves its poisoned output untouched (exit code 3 otherwise)."""
    k = len(points)
    strides = strides or [(64, 32)] * k
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    blob = struct.pack("<QII", n, k, place) + b"".join(struct.pack("<II", *s) for s in strides)
    src.write_bytes(blob + b"".join(p + s for p, s in zip(points, scalars)))
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    assert len(blob) == 4 + (0 if rc else 64 * n)
    return rc, blob[4:]


@pytest.fixture(scope="module")
def pyref_case():
    points, scalars, relations = KV.case(N, K)
    return points, scalars, relations, KV.expected(points, scalars)


def relation_block(k):
    """The outputs at the relation lanes of the 256-output case, the whole block, with pyref's records."""
    points, scalars, relations = KV.case(N_REL, k)
    lanes = sorted(relations)
    pts = [[p[i] for i in lanes] for p in points]
    scs = [[s[i] for i in lanes] for s in scalars]
    return [relations[i] for i in lanes], pts, scs, KV.expected(pts, scs)


def raw_terms(points, scalars, strides=None):
    """(C array of msm377_lincomb_term, the buffers it points into)."""
    strides = strides or [(64, 32)] * len(points)
    return E._lincomb_host_terms(points, scalars, strides)


# ---- the vectors themselves ----
def test_vectors_cover_what_they_claim():
    points, scalars, relations = KV.case(N_REL, K)
    assert sorted(relations.values()) == sorted(KV.relations(K)) and len(KV.relations(K)) == 6 + K
    assert {tuple(VV.final_carry(s[i]) for s in scalars) for i in range(N_REL)} >= {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)}
    names, pts, scs, wire = relation_block(K)
    for j, name in enumerate(names):
        out = wire[64 * j : 64 * j + 64]
        if name in KV.SUM_IS_IDENTITY:
            assert out == KV.IDENTITY_WIRE, name
        if name == "multiples of one base, scalars sum to 0":
            assert all(R.ed_mul(p[j], s[j]) != R.ED_ID for p, s in zip(pts, scs))  # O from terms none of which is O
        if name == "term j = -term 0, equal scalars":
            assert sum(p[j] == R.ed_neg(pts[0][j]) and s[j] == scs[0][j] for p, s in zip(pts[1:], scs[1:])) == 1
    for k in (1, 8):  # the block is whole at both ends of the range of k
        assert sorted(KV.case(N_REL, k)[2].values()) == sorted(KV.relations(k))


# ---- the host twin against pyref ----
def test_twin_against_pyref(exe_plain, exe_san, tmp_path, pyref_case):
    points, scalars, _, wire = pyref_case
    pb, sb = KV.encode(points, scalars)
    assert msm.ed_batch_lincomb_host(pb, sb) == wire
    assert run_program(exe_plain, tmp_path, pb, sb, N) == (0, wire)
    assert run_program(exe_san, tmp_path, pb, sb, N) == (0, wire)


def test_relations_block(exe_san, tmp_path):
    """The whole block (the same point k times, a cancelling pair, multiples of one base that sum to O, order 4 beside
    P + T, all O, zero scalars) through the library and through the sanitized stand-alone program."""
    names, pts, scs, wire = relation_block(K)
    pb, sb = KV.encode(pts, scs)
    assert msm.ed_batch_lincomb_host(pb, sb) == wire, names
    assert run_program(exe_san, tmp_path, pb, sb, len(names)) == (0, wire)


@pytest.mark.parametrize("k", [1, 2])
def test_one_and_two_terms_equal_the_older_twins(k):
    points, scalars, _ = KV.case(65, k)
    pb, sb = KV.encode(points, scalars)
    older = msm.ed_batch_mul_var_host(pb[0], sb[0]) if k == 1 else msm.ed_batch_lincomb2_host(pb[0], pb[1], sb[0], sb[1])
    assert msm.ed_batch_lincomb_host(pb, sb) == older


def test_stride_0_terms_equal_the_expanded_form(exe_san, tmp_path, pyref_case):
    """One term's point, scalar or both as ONE element for all outputs, and the Schnorr-as-one-sum shape (term 0 a stride-0
    point, term 2 a stride-0 scalar); the stand-alone program holds a stride-0 array in an allocation of exactly one element."""
    points, scalars, _, _ = pyref_case
    n = 9
    pb, sb = KV.encode([p[20 : 20 + n] for p in points], [s[20 : 20 + n] for s in scalars])
    sb[1] = R.encode_scalars([VV.MASK256]) + sb[1][32:]  # the ONE scalar of a stride-0 term: full width, a final carry
    lib = msm.load_library()
    patterns = [{(1, "p")}, {(1, "s")}, {(1, "p"), (1, "s")}, {(0, "p"), (2, "s")}, {(t, x) for t in range(K) for x in "ps"}]
    for zero in patterns:
        strides = [(0 if (t, "p") in zero else 64, 0 if (t, "s") in zero else 32) for t in range(K)]
        args_p = [b[:64] if (t, "p") in zero else b for t, b in enumerate(pb)]
        args_s = [b[:32] if (t, "s") in zero else b for t, b in enumerate(sb)]
        exp = msm.ed_batch_lincomb_host([KV.expand(b, 64, n) if len(b) == 64 else b for b in args_p], [KV.expand(b, 32, n) if len(b) == 32 else b for b in args_s])
        terms, keep = raw_terms(args_p, args_s, strides)
        out = ctypes.create_string_buffer(64 * n)
        assert lib.msm377_ed_batch_lincomb_host(terms, K, n, ctypes.addressof(out)) == 0
        assert out.raw == exp, zero
        assert msm.ed_batch_lincomb_host(args_p, args_s) == (exp[:64] if len(zero) == 2 * K else exp), zero  # all single: ONE output
        assert run_program(exe_san, tmp_path, args_p, args_s, n, strides) == (0, exp), zero
    assert exp == KV.expected([[p[20]] * n for p in points], [[scalars[0][20]] * n, [VV.MASK256] * n, [scalars[2][20]] * n])  # all: by pyref


# ---- refusals ----
def test_points_off_the_curve_are_refused_with_term_and_lowest_index(exe_san, tmp_path, pyref_case):
    points, scalars, _, _ = pyref_case
    gx, gy = R.ED_G
    bad, noncanon = KV.off_curve_point(), (gx + R.Q, gy)
    _, sb = KV.encode(points, scalars)
    cases = [
        ({(0, 7): bad}, 0, 7, "not on the curve"),
        ({(2, N - 1): bad}, 2, N - 1, "not on the curve"),
        ({(0, 20): bad, (1, 7): bad}, 1, 7, "not on the curve"),  # the lowest index, whatever the term
        ({(2, 9): bad, (1, 9): noncanon}, 1, 9, "not below q"),  # equal indices: the lowest term
        ({(2, 0): noncanon, (2, 3): bad, (0, 1): bad}, 2, 0, "not below q"),
    ]
    for plant, term, index, text in cases:
        pts = [list(p) for p in points]
        for (t, i), pt in plant.items():
            pts[t][i] = pt
        pb = [R.ed_encode_points(p) for p in pts]
        with pytest.raises(msm.MsmError) as err:
            msm.ed_batch_lincomb_host(pb, sb)
        assert (err.value.code, err.value.term, err.value.index, err.value.array) == (EPOINT, term, index, None) and text in str(err.value), plant
        assert run_program(exe_san, tmp_path, pb, sb, N)[0] == EPOINT  # ... with its poisoned output untouched
    # a stride-0 point: ONE record is checked, and it is index 0 of its term
    pb = [R.ed_encode_points(list(p)) for p in points]
    pb[1] = R.ed_encode_points([bad])
    with pytest.raises(msm.MsmError) as err:
        msm.ed_batch_lincomb_host(pb, sb)
    assert (err.value.code, err.value.term, err.value.index) == (EPOINT, 1, 0)
    assert run_program(exe_san, tmp_path, pb, sb, N, [(64, 32), (0, 32), (64, 32)])[0] == EPOINT


# ---- in place ----
def test_in_place_and_fold_in_place(exe_san, tmp_path, pyref_case):
    points, scalars, _, wire = pyref_case
    pb, sb = KV.encode(points, scalars)
    for t in range(K):
        assert run_program(exe_san, tmp_path, pb, sb, N, place=1 + t) == (0, wire), t  # out == term t's points
    assert run_program(exe_san, tmp_path, pb, sb, N, place=100) == (0, wire)  # term 0 = G, term 1 = G + N records, out = G
    lib = msm.load_library()
    g = ctypes.create_string_buffer(pb[0] + pb[1], 128 * N)
    base = ctypes.addressof(g)
    keep = [ctypes.create_string_buffer(b, len(b)) for b in sb + [pb[2]]]
    terms = E._lincomb_terms([(base, ctypes.addressof(keep[0]), 64, 32), (base + 64 * N, ctypes.addressof(keep[1]), 64, 32), (ctypes.addressof(keep[3]), ctypes.addressof(keep[2]), 64, 32)])
    assert lib.msm377_ed_batch_lincomb_host(terms, K, N, base) == 0
    assert g.raw == wire + pb[1]
    same = msm.ed_batch_lincomb_host([pb[0]] * K, sb)  # every term the same array: [s_0 + s_1 + s_2]P
    assert same[64 * 20 : 64 * 30] == b"".join(R.ed_encode_result(R.ed_mul(points[0][i], sum(s[i] for s in scalars))) for i in range(20, 30))


def test_arguments():
    lib = msm.load_library()
    call = lib.msm377_ed_batch_lincomb_host
    pb = [R.ed_encode_points([R.ED_G, R.ed_mul(R.ED_G, 5)]), R.ed_encode_points([R.ed_mul(R.ED_G, 7), R.ED_G]), R.ed_encode_points([R.ED_G, R.ED_G])]
    sb = [R.encode_scalars([3, 4]), R.encode_scalars([1, 2]), R.encode_scalars([6, 0])]
    exp = R.ed_encode_points([R.ed_mul(R.ED_G, 16), R.ed_mul(R.ED_G, 22)])
    out = ctypes.create_string_buffer(b"\xa5" * 144, 144)
    o = ctypes.addressof(out)
    terms, keep = raw_terms(pb, sb)
    nine, keep9 = raw_terms([pb[0]] * 9, [sb[0]] * 9)
    assert call(terms, 0, 2, o) == EINVAL and call(nine, 9, 2, o) == EINVAL and call(None, 3, 2, o) == EINVAL
    assert call(terms, 0, 0, o) == EINVAL and call(nine, 9, 0, o) == EINVAL and call(None, 3, 0, o) == EINVAL  # the shape is checked first
    for t in range(3):
        for which, strides in ((0, (1, 4, 16, 32, 63, 65, 96, 128)), (1, (1, 4, 16, 31, 33, 64))):
            for stride in strides:
                s = [[64, 32] for _ in range(3)]
                s[t][which] = stride
                bad, keep_bad = raw_terms(pb, sb, s)
                assert call(bad, 3, 2, o) == EINVAL and call(bad, 3, 0, o) == EINVAL, (t, which, stride)
    for t in range(3):
        for field in ("points", "scalars"):
            holed, keep_h = raw_terms(pb, sb)
            setattr(holed[t], field, None)
            assert call(holed, 3, 2, o) == EINVAL, (t, field)
            assert call(holed, 3, 0, o) == 0  # n = 0: whatever the pointers
    assert call(terms, 3, 2, None) == EINVAL
    assert call(terms, 3, 0, None) == 0
    one = ctypes.create_string_buffer(pb[1][:64], 64)  # the outputs over the ONE point of a stride-0 term
    over = E._lincomb_terms([(terms[0].points, terms[0].scalars, 64, 32), (ctypes.addressof(one), terms[1].scalars, 0, 32), (terms[2].points, terms[2].scalars, 64, 32)])
    assert call(over, 3, 2, ctypes.addressof(one)) == EINVAL
    assert one.raw == pb[1][:64] and out.raw == b"\xa5" * 144
    assert call(terms, 3, 2, o) == 0
    assert out.raw[:128] == exp and out.raw[128:] == b"\xa5" * 16
    assert msm.ed_batch_lincomb_host([b""], [b""]) == b""
    with pytest.raises(ValueError):
        msm.ed_batch_lincomb_host(pb, sb[:2])
    with pytest.raises(ValueError):
        msm.ed_batch_lincomb_host([pb[0] * 3, pb[1], pb[2]], sb)  # 6 against 2: neither n nor one
    with pytest.raises(msm.MsmError) as err:
        msm.ed_batch_lincomb_host([], [])
    assert err.value.code == EINVAL
    del keep, keep9
