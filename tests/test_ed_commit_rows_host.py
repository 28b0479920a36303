"""Edwards-BLS12 row commitments on the host (include/msm377.h "Edwards-BLS12 row commitments"): the host twin
csrc/ed_commit_rows_host.hpp.  tests/native/ed_commit_rows_host.cpp is compiled with g++ and the address /
undefined-behaviour sanitizers against the headers (a stand-alone program: nothing is loaded into python) and asked for
whole runs; the library's msm377_ed_commit_rows_host runs the same header.  Expected values: tests/pyref.py (R.ed_mul,
R.ed_add), and for k = 600 generators with known logarithms (tests/ed_commit_rows_vectors.py).  The buffers hold mostly
short scalars, so no case prices more than a few hundred full-width multiplications.  CPU only; the device call:
tests/test_ed_commit_rows_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import ed_commit_rows_vectors as ECR
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, EPOINT

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ed_commit_rows_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
KS = (1, 15, 16, 17, 33, 273)
ROWS = {1: 14, 15: 5, 16: 5, 17: 5, 33: 4, 273: 3}  # n per k
LAYOUTS = ("rows", "columns", "padded", "sliding")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "ed_commit_rows_host_san")
    cmd = ["g++", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, gens: bytes, k, scalars: bytes, n, out_stride, base_stride):
    """(return code, records) of one run of the host twin inside the sanitized program.  The program itself checks that a
    refused call leaves its poisoned output untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIQQQQ", k, len(gens) // 64, n, out_stride, base_stride, len(scalars)) + gens + scalars)
    res = subprocess.run([exe, "run", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr)
    blob = dst.read_bytes()
    rc = struct.unpack("<i", blob[:4])[0]
    assert len(blob) == 4 + (0 if rc else 64 * n)
    return rc, blob[4:]


def packed(buf, n, k, layout):
    """(bytes, out_stride, base_stride) of the sliding matrix row i = buf[i : i + k] in one of the four layouts."""
    if layout == "sliding":
        return ECR.sliding_bytes(buf), 32, 32
    return ECR.pack(ECR.sliding_rows(buf, n, k), layout)


def test_limits(exe):
    res = subprocess.run([exe, "limits"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert tuple(int(v) for v in res.stdout.split()) == (ECR.GEN_MAX, ECR.GEN_WIDE_MAX)


def test_vectors_cover_what_they_claim():
    gens, k = ECR.relation_generators(), ECR.REL_K
    assert ECR.plan(k)[0] == 18 and ECR.FOLD_GROUP == 16  # one full fold group and a group of two
    seg = lambda j: ECR.segment_of(j, k)  # noqa: E731
    assert seg(9) == seg(10) == seg(1) == 0 and seg(20) == 1 and seg(35) == 2 and seg(256) == 16 and seg(272) == 17
    assert gens[9] == R.ed_neg(gens[1]) and gens[20] == R.ed_neg(gens[0]) == gens[256] and gens[257] == gens[1] == gens[21]
    assert gens[3] == R.ED_ID and R.ed_add(gens[4], gens[4]) == R.ED_ID and gens[4] != R.ED_ID
    for t in (gens[5], gens[6]):
        assert R.ed_mul(t, 2) == gens[4] and R.ed_on_curve(t)
    assert gens[5] != gens[6] and all(R.ed_on_curve(g) for g in gens)
    assert R.ed_mul(gens[7], R.ED_SUBGROUP) != R.ED_ID  # P + T: outside the subgroup
    wire = ECR.relation_expected()  # (asserts which rows are the identity)
    rows = dict(ECR.relation_rows())
    only = [j for j, s in enumerate(rows["only_last"]) if s]
    assert only == [k - 1] and not any(rows["zero"])
    # a sum of O from GROUP sums that are not O, each of two partials
    row = rows["opposite_group_sums_of_two_partials"]
    group = [ECR.expected(gens, [tuple(s if (j >= 256) == hi else 0 for j, s in enumerate(row))]) for hi in (False, True)]
    assert ECR.IDENTITY_WIRE not in group and len(wire) == 64 * len(rows)


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """k -> (points, buffer, wire records): computed once by pyref, read by every test below.  The matrix is the sliding
    one, row i = buffer[i : i + k]."""
    out = {}
    for k in KS:
        pts = ECR.mixed_generators(k)
        buf = ECR.mixed_buffer(ROWS[k] + k - 1, 0xC0DE + k)
        out[k] = (pts, buf, ECR.expected(pts, ECR.sliding_rows(buf, ROWS[k], k)))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_against_pyref(exe, tmp_path, reference, k, layout):
    pts, buf, wire = reference[k]
    n = ROWS[k]
    data, out_stride, base_stride = packed(buf, n, k, layout)
    assert run_program(exe, tmp_path, R.ed_encode_points(list(pts)), k, data, n, out_stride, base_stride) == (0, wire)


def test_relations(exe, tmp_path):
    """The relations set (k = 273): every case the walk and the grouped fold of the device call must follow, here through
    the twin's general additions."""
    gens = R.ed_encode_points(list(ECR.relation_generators()))
    rows = [row for _, row in ECR.relation_rows()]
    wire = ECR.relation_expected()
    for layout in ("rows", "columns"):
        data, out_stride, base_stride = ECR.pack(rows, layout)
        assert run_program(exe, tmp_path, gens, ECR.REL_K, data, len(rows), out_stride, base_stride) == (0, wire), layout
        assert msm.ed_commit_rows_host(gens, data, layout) == wire, layout
    assert ECR.IDENTITY_WIRE in [wire[i : i + 64] for i in range(0, len(wire), 64)]


def test_library_runs_the_same_twin(exe, tmp_path, reference):
    for k in (1, 17, 33):
        pts, buf, wire = reference[k]
        gens = R.ed_encode_points(list(pts))
        rows = ECR.sliding_rows(buf, ROWS[k], k)
        for layout in ("rows", "columns"):
            assert msm.ed_commit_rows_host(gens, ECR.pack(rows, layout)[0], layout) == wire, (k, layout)
    # byte for byte the stand-alone program on a case of its own, sliding rows through the C ABI
    k, n = 33, 6
    logs, gens = ECR.known_logs(k)
    buf = ECR.mixed_buffer(n + k - 1, 0x5A3E)
    data = ECR.sliding_bytes(buf)
    out = ctypes.create_string_buffer(64 * n)
    assert msm.load_library().msm377_ed_commit_rows_host(gens, k, data, n, 32, 32, ctypes.addressof(out)) == 0
    assert run_program(exe, tmp_path, gens, k, data, n, 32, 32) == (0, out.raw)
    assert out.raw == ECR.closed_rows(logs, ECR.sliding_rows(buf, n, k))
    # k = 1 is the single-base twin
    assert msm.ed_commit_rows_host(ECR.G_WIRE, data) == msm.ed_batch_mul_multi_host(ECR.G_WIRE, data)


def test_600_generators_match_the_known_logarithms(exe, tmp_path):
    k, n = 600, 3
    logs, gens = ECR.known_logs(k)
    buf = ECR.mixed_buffer(n + k - 1, 0x600)
    exp = ECR.closed_rows(logs, ECR.sliding_rows(buf, n, k))
    assert run_program(exe, tmp_path, gens, k, ECR.sliding_bytes(buf), n, 32, 32) == (0, exp)
    data, _, _ = ECR.pack(ECR.sliding_rows(buf, n, k), "columns")
    assert msm.ed_commit_rows_host(gens, data, layout="columns") == exp
    assert ECR.IDENTITY_WIRE not in (exp[:64], exp[64:128], exp[128:])


# ---- refusals ----
def test_generators_off_the_curve_are_refused_with_the_lowest_index(exe, tmp_path):
    k, n = 20, 2
    pts = list(ECR.mixed_generators(k))
    scalars = R.encode_scalars(list(range(3, 3 + n * k)))
    gx, gy = R.ED_G
    bad, noncanon = ECR.off_curve_point(), (gx + R.Q, gy)
    for plant, index, text in (({7: bad}, 7, "not on the curve"), ({k - 1: noncanon}, k - 1, "not below q"), ({12: bad, 4: noncanon}, 4, "not below q"),
                               ({0: bad, 19: bad}, 0, "not on the curve"), ({9: noncanon, 10: bad}, 9, "not below q")):
        g = list(pts)
        for j, pt in plant.items():
            g[j] = pt
        gens = b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in g)
        with pytest.raises(msm.MsmError) as err:
            msm.ed_commit_rows_host(gens, scalars)
        assert (err.value.code, err.value.index) == (EPOINT, index) and text in str(err.value), plant
        assert run_program(exe, tmp_path, gens, k, scalars, n, 32 * k, 32)[0] == EPOINT  # ... with its poisoned output untouched
        if index:  # a call over the generators in front of the finding does not read it
            rows = [tuple(range(3 + i * index, 3 + (i + 1) * index)) for i in range(n)]
            assert msm.ed_commit_rows_host(gens[: 64 * index], scalars[: 32 * index * n]) == ECR.expected(pts[:index], rows)


def test_empty_batch(exe, tmp_path):
    two = R.ed_encode_points([R.ED_G, R.ED_G])
    assert msm.ed_commit_rows_host(two, b"") == b""
    lib = msm.load_library()
    assert lib.msm377_ed_commit_rows_host(None, 2, None, 0, 64, 32, None) == 0
    assert lib.msm377_ed_commit_rows_host(None, 0, None, 0, 64, 32, None) == EINVAL  # the shape is checked first
    assert lib.msm377_ed_commit_rows_host(None, 2, None, 0, 48, 32, None) == EINVAL
    assert run_program(exe, tmp_path, two, 2, b"", 0, 64, 32) == (0, b"")


def test_refusals_leave_the_outputs_untouched(exe, tmp_path):
    lib = msm.load_library()
    pts = [R.ed_mul(R.ED_G, j + 1) for j in range(3)]
    gens = R.ed_encode_points(pts)
    scalars = R.encode_scalars(list(range(5, 5 + 8)))
    out = ctypes.create_string_buffer(b"\xa5" * 144, 144)
    o = ctypes.addressof(out)

    def call(g, k, s, out_stride, base_stride, dst):
        return lib.msm377_ed_commit_rows_host(g, k, s, 2, out_stride, base_stride, dst)

    for k, os_, bs in ((0, 64, 32), (4097, 32, 32), (2, 0, 32), (2, 64, 0), (2, 48, 32), (2, 64, 48), (2, 16, 32), (2, 64, 33)):
        assert call(gens, k, scalars, os_, bs, o) == EINVAL, (k, os_, bs)
        # the same refusal inside the sanitized program, which checks its poisoned output itself
        assert run_program(exe, tmp_path, gens, k, scalars, 2, os_, bs)[0] == EINVAL, (k, os_, bs)
    assert call(None, 2, scalars, 64, 32, o) == EINVAL
    assert call(gens, 2, None, 64, 32, o) == EINVAL
    assert call(gens, 2, scalars, 64, 32, None) == EINVAL
    bad = gens[:64] + R.ed_encode_points([ECR.off_curve_point()])  # at position 1
    assert call(bad, 2, scalars, 64, 32, o) == EPOINT
    assert out.raw == b"\xa5" * 144
    assert call(bad, 1, scalars, 64, 32, o) == 0  # position 1 is not part of a k = 1 call
    assert out.raw[:128] == R.ed_encode_points([R.ed_mul(R.ED_G, 5), R.ed_mul(R.ED_G, 7)]) and out.raw[128:] == b"\xa5" * 16
    assert call(gens, 2, scalars, 64, 32, o) == 0
    assert out.raw[:128] == R.ed_encode_points([R.ed_mul(R.ED_G, 5 + 2 * 6), R.ed_mul(R.ED_G, 7 + 2 * 8)])
    with pytest.raises(ValueError):
        msm.ed_commit_rows_host(gens[:100], scalars)
    with pytest.raises(ValueError):
        msm.ed_commit_rows_host(gens, scalars)  # 8 scalars over 3 generators
