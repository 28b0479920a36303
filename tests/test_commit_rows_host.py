"""Row commitments on the host (include/msm377.h "row commitments"): the host twin csrc/commit_rows_host.hpp and the plan
csrc/commit_rows_plan.hpp.  tests/native/commit_rows_host.cpp is compiled with g++ and the address /
undefined-behaviour sanitizers against the headers (a stand-alone program: nothing is loaded into python) and asked for
whole runs; the library's msm377_g1_commit_rows_host runs the same header.  Expected values: tests/pyref.py, and for
k = 600 generators with known logarithms (tests/commit_rows_vectors.py).  No case prices more than about 2 000 terms.
CPU only; the device call: tests/test_commit_rows_gpu.py."""
import ctypes
import os
import struct
import subprocess

import pytest

import batch_mul_vectors as V
import commit_rows_vectors as CR
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "commit_rows_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
r = R.R_ORDER
KS = (1, 2, 16, 17, 33)
ROWS = {1: 12, 2: 10, 16: 5, 17: 5, 33: 4}  # n per k: n k muls of pyref per reference
LAYOUTS = ("rows", "columns", "padded", "sliding")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "commit_rows_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def run_program(exe, tmp_path, gens: bytes, k, scalars: bytes, n, out_stride, base_stride, scalar_form=V.WIRE, out_form=V.WIRE):
    """(return code, records, flags) of one run of the host twin inside the sanitized program.  The program itself
    checks that a refused call leaves its poisoned outputs untouched (exit code 3 otherwise)."""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<IIIIQQQQ", scalar_form, out_form, k, len(gens) // 96, n, out_stride, base_stride, len(scalars)) + gens + scalars)
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


def packed(buf, n, k, layout):
    """(bytes, out_stride, base_stride) of the sliding matrix row i = buf[i : i + k] in one of the four layouts."""
    if layout == "sliding":
        return CR.sliding_bytes(buf), 32, 32
    return CR.pack(CR.sliding_rows(buf, n, k), layout)


def test_limits(exe):
    res = subprocess.run([exe, "limits"], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert tuple(int(v) for v in res.stdout.split()) == (CR.GEN_MAX, CR.GEN_WIDE_MAX)


# ---- the plan ----
def test_plan_is_the_three_formulas(exe):
    """Every k in 1 .. 4 096 against ceil(k / 16), ceil(k / S), floor(2^20 / S) rounded down to the workgroup size; 0
    segments outside; every segment non-empty and the partial sums of a pass within the 2^20-point stash."""
    lib = msm.load_library()
    seg, bps, rows = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    for k in list(range(0, 4099)) + [2**16, 2**32 - 1]:
        lib.msm377_commit_rows_plan(k, ctypes.addressof(seg), ctypes.addressof(bps), ctypes.addressof(rows))
        got = (seg.value, bps.value, rows.value)
        assert got == CR.plan(k), k
        if 1 <= k <= 4096:
            assert (got[0] - 1) * got[1] < k <= got[0] * got[1] and got[1] <= 16 and got[2] % 256 == 0 and 0 < got[0] * got[2] <= 2**20, k
        else:
            assert got == (0, 0, 0), k
    assert CR.plan(4096) == (256, 16, 4096) and CR.plan(16) == (1, 16, 2**20) and CR.plan(17) == (2, 9, 2**19) and CR.plan(33)[:2] == (3, 11)
    assert msm.commit_rows_plan(4096) == (256, 16, 4096) and msm.commit_rows_plan(0) == (0, 0, 0)
    lib.msm377_commit_rows_plan(33, None, None, None)  # any pointer may be null
    for k in (0, 1, 16, 17, 33, 4096, 4097):  # the stand-alone program reads the same header
        res = subprocess.run([exe, "plan", str(k)], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and tuple(int(v) for v in res.stdout.split()) == CR.plan(k), k


# ---- the host twin against pyref ----
@pytest.fixture(scope="module")
def reference():
    """(k, scalar form) -> (points, buffer, wire records, flags): computed once by pyref, read by every test below.  The
    matrix is the sliding one, row i = buffer[i : i + k]; under the Montgomery form a value v means v 2^-256 mod r."""
    out = {}
    inv = pow(2**256, -1, r)
    for k in KS:
        pts = CR.mixed_generators(k)
        buf = CR.sliding_buffer(ROWS[k], k, 0xC0DE + k)
        for form in (V.WIRE, V.MONT):
            meant = buf if form == V.WIRE else [v * inv % r for v in buf]
            out[k, form] = (pts, buf) + CR.expected(pts, CR.sliding_rows(meant, ROWS[k], k))
    return out


@pytest.mark.parametrize("out_form", [V.WIRE, V.MONT_FLAG])
@pytest.mark.parametrize("scalar_form", [V.WIRE, V.MONT])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", KS)
def test_against_pyref(exe, tmp_path, reference, k, layout, scalar_form, out_form):
    pts, buf, wire, flags = reference[k, scalar_form]
    n = ROWS[k]
    data, out_stride, base_stride = packed(buf, n, k, layout)
    rc, got, got_flags = run_program(exe, tmp_path, R.encode_points(list(pts)), k, data, n, out_stride, base_stride, scalar_form, out_form)
    assert rc == 0
    assert got_flags == flags
    assert got == (wire if out_form == V.WIRE else V.mont_flag_records(wire, flags))


def test_relations(exe, tmp_path):
    """The relations set (k = 48): every case the fold of the device call must follow, here through the twin's general
    additions, in both output forms."""
    gens = R.encode_points(list(CR.relation_generators()))
    rows = [row for _, row in CR.relation_rows()]
    wire, flags = CR.relation_expected()
    data, out_stride, base_stride = CR.pack(rows)
    assert run_program(exe, tmp_path, gens, CR.REL_K, data, len(rows), out_stride, base_stride) == (0, wire, flags)
    assert run_program(exe, tmp_path, gens, CR.REL_K, data, len(rows), out_stride, base_stride, out_form=V.MONT_FLAG) == (0, V.mont_flag_records(wire, flags), flags)
    data, out_stride, base_stride = CR.pack(rows, "columns")
    assert run_program(exe, tmp_path, gens, CR.REL_K, data, len(rows), out_stride, base_stride) == (0, wire, flags)
    assert 1 in flags and 0 in flags


def test_library_runs_the_same_twin(exe, tmp_path, reference):
    for k in (2, 17, 33):
        for form, fname in ((V.WIRE, "wire"), (V.MONT, "mont")):
            pts, buf, wire, flags = reference[k, form]
            gens = R.encode_points(list(pts))
            rows = CR.sliding_rows(buf, ROWS[k], k)
            for layout in ("rows", "columns"):
                assert msm.commit_rows_host(gens, CR.pack(rows, layout)[0], "wire", layout, fname) == (wire, flags), (k, layout)
            assert msm.commit_rows_host(gens, CR.pack(rows)[0], "mont_flag", "rows", fname) == (V.mont_flag_records(wire, flags), flags)
    # byte for byte the stand-alone program on a case of its own, sliding rows through the C ABI
    k, n = 33, 6
    logs, gens = CR.known_logs(k)
    buf = CR.sliding_buffer(n, k, 0x5A3E)
    data = CR.sliding_bytes(buf)
    out, inf = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    rc = msm.load_library().msm377_g1_commit_rows_host(gens, k, data, V.WIRE, n, 32, 32, V.WIRE, ctypes.addressof(out), ctypes.addressof(inf))
    assert rc == 0
    assert run_program(exe, tmp_path, gens, k, data, n, 32, 32) == (0, out.raw, inf.raw)
    assert (out.raw, inf.raw) == CR.closed_rows(logs, CR.sliding_rows(buf, n, k))


def test_600_generators_match_the_known_logarithms(exe, tmp_path):
    k, n = 600, 3
    logs, gens = CR.known_logs(k)
    buf = CR.sliding_buffer(n, k, 0x600)
    exp = CR.closed_rows(logs, CR.sliding_rows(buf, n, k))
    assert run_program(exe, tmp_path, gens, k, CR.sliding_bytes(buf), n, 32, 32) == (0,) + exp
    data, out_stride, base_stride = CR.pack(CR.sliding_rows(buf, n, k), "columns")
    assert msm.commit_rows_host(gens, data, layout="columns") == exp
    assert exp[1] == b"\0\0\0"


# ---- arguments ----
def test_empty_batch(exe, tmp_path):
    two = R.encode_points([R.G, R.G])
    assert msm.commit_rows_host(two, b"") == (b"", b"")
    lib = msm.load_library()
    assert lib.msm377_g1_commit_rows_host(None, 2, None, V.WIRE, 0, 64, 32, V.WIRE, None, None) == 0
    assert lib.msm377_g1_commit_rows_host(None, 0, None, V.WIRE, 0, 64, 32, V.WIRE, None, None) == EINVAL  # the shape is checked first
    assert run_program(exe, tmp_path, two, 2, b"", 0, 64, 32) == (0, b"", b"")


def test_refusals_leave_the_outputs_untouched(exe, tmp_path):
    lib = msm.load_library()
    gens = R.encode_points([R.mul(R.G, j + 1) for j in range(3)])
    scalars = R.encode_scalars(list(range(5, 5 + 8)))
    out, inf = ctypes.create_string_buffer(b"\xa5" * 208), ctypes.create_string_buffer(b"\xa5" * 2)

    def call(g, k, s, scalar_form, out_stride, base_stride, form, o):
        return lib.msm377_g1_commit_rows_host(g, k, s, scalar_form, 2, out_stride, base_stride, form, o, ctypes.addressof(inf))

    o = ctypes.addressof(out)
    noncanonical = gens[:96] + (R.P).to_bytes(48, "little") + R.G[1].to_bytes(48, "little")  # at position 1
    refused = [
        (gens, 0, scalars, V.WIRE, 64, 32, V.WIRE),
        (gens, 4097, scalars, V.WIRE, 32, 32, V.WIRE),
        (gens, 2, scalars, V.WIRE, 0, 32, V.WIRE),
        (gens, 2, scalars, V.WIRE, 64, 0, V.WIRE),
        (gens, 2, scalars, V.WIRE, 48, 32, V.WIRE),
        (gens, 2, scalars, V.WIRE, 64, 48, V.WIRE),
        (noncanonical, 2, scalars, V.WIRE, 64, 32, V.WIRE),
        (gens, 2, scalars, V.WIRE, 64, 32, V.MONT),  # plain mont cannot say "identity"
        (gens, 2, scalars, V.WIRE, 64, 32, 3),
        (gens, 2, scalars, 2, 64, 32, V.WIRE),  # no such scalar form
    ]
    for g, k, s, sf, os_, bs, form in refused:
        assert call(g, k, s, sf, os_, bs, form, o) == EINVAL, (k, sf, os_, bs, form)
        # the same refusal inside the sanitized program, which checks its poisoned outputs itself
        assert run_program(exe, tmp_path, g, k, s, 2, os_, bs, sf, form)[0] == EINVAL, (k, sf, os_, bs, form)
    assert call(None, 2, scalars, V.WIRE, 64, 32, V.WIRE, o) == EINVAL
    assert call(gens, 2, None, V.WIRE, 64, 32, V.WIRE, o) == EINVAL
    assert call(gens, 2, scalars, V.WIRE, 64, 32, V.WIRE, None) == EINVAL
    assert out.raw[:208] == b"\xa5" * 208 and inf.raw[:2] == b"\xa5" * 2
    assert call(noncanonical, 1, scalars, V.WIRE, 64, 32, V.WIRE, o) == 0  # position 1 is not part of a k = 1 call
    assert out.raw[:192] == R.encode_result(R.mul(R.G, 5)) + R.encode_result(R.mul(R.G, 7)) and inf.raw[:2] == b"\0\0"
    with pytest.raises(msm.MsmError) as e:
        msm.commit_rows_host(gens[:192], scalars[:128], "mont")
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        msm.commit_rows_host(gens[:100], scalars)
